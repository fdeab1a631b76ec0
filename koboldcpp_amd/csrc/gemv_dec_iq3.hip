// instantiation unit of the fused decode mat-vec for KT_IQ3_XXS / KT_IQ3_S / KT_IQ1_S / KT_IQ1_M (see gemv_dec_impl.h)
#include "gemv_dec_impl.h"
template int gemv_unit_launch<KT_IQ3_XXS>(const GemvPlan &, const DecArgs &, hipStream_t);
template int gemv_unit_launch<KT_IQ3_S>(const GemvPlan &, const DecArgs &, hipStream_t);
template int gemv_unit_launch<KT_IQ1_S>(const GemvPlan &, const DecArgs &, hipStream_t);
template int gemv_unit_launch<KT_IQ1_M>(const GemvPlan &, const DecArgs &, hipStream_t);
