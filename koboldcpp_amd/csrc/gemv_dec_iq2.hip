// instantiation unit of the fused decode mat-vec for KT_IQ2_XXS / KT_IQ2_XS / KT_IQ2_S (see gemv_dec_impl.h)
#include "gemv_dec_impl.h"
template int gemv_unit_launch<KT_IQ2_XXS>(const GemvPlan &, const DecArgs &, hipStream_t);
template int gemv_unit_launch<KT_IQ2_XS>(const GemvPlan &, const DecArgs &, hipStream_t);
template int gemv_unit_launch<KT_IQ2_S>(const GemvPlan &, const DecArgs &, hipStream_t);
