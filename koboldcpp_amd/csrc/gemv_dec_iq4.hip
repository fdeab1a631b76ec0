// instantiation unit of the fused decode mat-vec for KT_IQ4_NL / KT_IQ4_XS (see gemv_dec_impl.h)
#include "gemv_dec_impl.h"
template int gemv_unit_launch<KT_IQ4_NL>(const GemvPlan &, const DecArgs &, hipStream_t);
template int gemv_unit_launch<KT_IQ4_XS>(const GemvPlan &, const DecArgs &, hipStream_t);
