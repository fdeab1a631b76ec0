// instantiation unit of the fused decode mat-vec for KT_Q3_K (see gemv_dec_impl.h)
#include "gemv_dec_impl.h"
template int gemv_unit_launch<KT_Q3_K>(const GemvPlan &, const DecArgs &, hipStream_t);
