// instantiation unit of the fused decode mat-vec for KT_Q4_0 (see gemv_dec_impl.h)
#include "gemv_dec_impl.h"
template int gemv_unit_launch<KT_Q4_0>(const GemvPlan &, const DecArgs &, hipStream_t);
