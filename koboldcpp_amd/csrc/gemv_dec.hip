// gemv_dec.hip -- C entry of the fused single-token mat-vec: shape, plan (gemv_plan.h), the kernel file's launcher.
#include "kcpp_internal.h"
#include "kcpp_common.h"

#include <cstdlib>

// the unit-per-lane launcher of p.type (gemv_dec_impl.h, one TU per type)
static int gemv_unit_launch_type(const GemvPlan &p, const DecArgs &a, hipStream_t s) {
    switch (p.type) {
#define KCPP_UNIT_T(T) case T: return gemv_unit_launch<T>(p, a, s);
    KCPP_UNIT_T(KT_Q4_K) KCPP_UNIT_T(KT_Q5_K) KCPP_UNIT_T(KT_Q6_K) KCPP_UNIT_T(KT_Q3_K) KCPP_UNIT_T(KT_Q2_K)
    KCPP_UNIT_T(KT_Q4_0) KCPP_UNIT_T(KT_Q5_0) KCPP_UNIT_T(KT_Q8_0) KCPP_UNIT_T(KT_IQ4_NL) KCPP_UNIT_T(KT_IQ4_XS)
    KCPP_UNIT_T(KT_IQ2_XXS) KCPP_UNIT_T(KT_IQ2_XS) KCPP_UNIT_T(KT_IQ2_S) KCPP_UNIT_T(KT_IQ3_XXS) KCPP_UNIT_T(KT_IQ3_S)
    KCPP_UNIT_T(KT_IQ1_S) KCPP_UNIT_T(KT_IQ1_M)
#undef KCPP_UNIT_T
    default: return GEMV_ERR_NO_INSTANCE;
    }
}

extern "C" int kcpp_gemv_dec(int type, const void *args, int mode, int pro, int rows_per_wave, void *stream) {
    const DecArgs &a = *(const DecArgs *)args;
    hipStream_t s = (hipStream_t)stream;
    GemvPlan p;
    if (gemv_plan(gemv_shape_of(type, a, mode, pro, rows_per_wave), GEMV_ENTRY_DEC, &p)) return p.rc;
    switch (p.kernel) {
    case GEMV_RS: return gemv_rs_launch(p, a, nullptr, s);
    case GEMV_Q4K: return gemv_q4k_launch(p, a, s);
    case GEMV_UNIT: return gemv_unit_launch_type(p, a, s);
    default: return GEMV_ERR_NO_INSTANCE;
    }
}

// what an entry runs for a call (gemv_plan.h GemvPlan; host only).  entry: GEMV_ENTRY_*; flags: GEMV_F_*.
// out = {rc, kernel, type, mode, pro, NI, IT, LPR, R, MC, PF, waves, XL, ROUTE, EX, block, nblk, lds_bytes}
extern "C" int kcpp_gemv_dec_plan(int entry, int type, int64_t K, int nseg, int64_t N0, int64_t N1, int64_t N2, int role0,
                                  int role1, int role2, int D, int mode, int pro, int rows_per_wave, int flags, int route_wt,
                                  int route_ne, int32_t out[18]) {
    const GemvShape s{type, K, nseg, {N0, N1, N2}, {role0, role1, role2}, D, mode, pro, rows_per_wave, flags, route_wt, route_ne};
    GemvPlan p;
    gemv_plan(s, entry, &p);
    const int32_t v[18] = {p.rc, p.kernel, p.type, p.mode, p.pro, p.NI, p.IT, p.LPR, p.R, p.MC, p.PF, p.waves, p.XL,
                           p.ROUTE, p.EX, p.block, (int32_t)p.nblk, (int32_t)p.lds_bytes};
    for (int i = 0; i < 18; ++i) out[i] = v[i];
    return p.rc;
}
// the combined launches' plans.  Mixed (kcpp_gemv_rs_qkv_mixed): out = {rc, NIA, NIB, MC, EX, block, nblk, lds_bytes}
extern "C" int kcpp_gemv_qkv_mixed_plan(int64_t K, int64_t N0, int64_t N1, int64_t N2, int role0, int role1, int role2, int D,
                                        int flags, int32_t out[8]) {
    const GemvShape s{KT_Q4_K_RS, K, 3, {N0, N1, N2}, {role0, role1, role2}, D, 2, 1, 2, flags, 0, 0};
    GemvMixedPlan m;
    gemv_qkv_mixed_plan(s, &m);
    const int32_t v[8] = {m.rc, m.NIA, m.NIB, m.MC, m.EX, m.block, (int32_t)m.nblk, (int32_t)m.lds_bytes};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return m.rc;
}
// the same for kcpp_gemv_rs_qkv_mixed_pro (pro 1 / 3): out = {rc, NIA, NIB, MC, EX, block, nblk, lds_bytes, PRO}
extern "C" int kcpp_gemv_qkv_mixed_plan_pro(int64_t K, int64_t N0, int64_t N1, int64_t N2, int role0, int role1, int role2, int D,
                                            int flags, int pro, int32_t out[9]) {
    const GemvShape s{KT_Q4_K_RS, K, 3, {N0, N1, N2}, {role0, role1, role2}, D, 2, pro, 2, flags, 0, 0};
    GemvMixedPlan m;
    gemv_qkv_mixed_plan(s, &m);
    const int32_t v[9] = {m.rc, m.NIA, m.NIB, m.MC, m.EX, m.block, (int32_t)m.nblk, (int32_t)m.lds_bytes, m.PRO};
    for (int i = 0; i < 9; ++i) out[i] = v[i];
    return m.rc;
}
// Dual (kcpp_gemv_qkv_dual; q of nseg_a segments Na in qtype, k|v of nseg_b segments Nb in Q8_0):
// out = {rc, nblk, lds_bytes, a.nblk, a.lds_bytes, a.NI, b.nblk, b.lds_bytes, b.IT}
extern "C" int kcpp_gemv_qkv_dual_plan(int qtype, int64_t Ka, int nseg_a, const int64_t *Na, int flags_a, int64_t Kb, int nseg_b,
                                       const int64_t *Nb, int flags_b, int32_t out[9]) {
    GemvShape sa{}, sb{};
    sa.type = qtype, sa.K = Ka, sa.nseg = nseg_a, sa.flags = flags_a;
    sb.K = Kb, sb.nseg = nseg_b, sb.flags = flags_b;
    for (int i = 0; i < 3; ++i) {
        sa.N[i] = i < nseg_a ? Na[i] : 0, sb.N[i] = i < nseg_b ? Nb[i] : 0;
        sa.role[i] = 0, sb.role[i] = i + 1;
    }
    GemvDualPlan d;
    gemv_qkv_dual_plan(sa, sb, &d);
    const int32_t v[9] = {d.rc, (int32_t)d.nblk, (int32_t)d.lds_bytes, (int32_t)d.a.nblk, (int32_t)d.a.lds_bytes, d.a.NI,
                          (int32_t)d.b.nblk, (int32_t)d.b.lds_bytes, d.b.IT};
    for (int i = 0; i < 9; ++i) out[i] = v[i];
    return d.rc;
}

extern "C" int64_t kcpp_gemv_dec_args_size(void) { return (int64_t)sizeof(DecArgs); }
