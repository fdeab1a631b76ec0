// gemv_rs.hip -- single-token mat-vec (decode) over the row-major decode layouts KT_Q4_K_RS / KT_Q5_K_RS / KT_Q6_K_RS.
//
// Why a layout of its own: in the ggml block order (block_q4_K, ggml-common.h:286: 16-B header + 128 B
// of nibbles, repeated) a lane that owns a 64-element unit reads three 16-B pieces at a 144-B stride,
// so every wave-wide load instruction touches ~18 cache lines for 1 KiB of data -- the address
// pattern alone capped a 66 MB gate|up read at 15 us against 11.3 us for a contiguous stream
// (tools/stream_probe.py).  The RS layouts keep each row's bytes together but split them into planes
// (kcpp_common.h):
//   Q4_K_RS row: [nsb][16] headers ++ [nsb][128] nibbles
//   Q5_K_RS row: [nsb][16] headers ++ [nsb][128] nibbles ++ [nsb][32] qh
//   Q6_K_RS row: [4 nsb][16] ql-lo ++ [4 nsb][16] ql-hi ++ [4 nsb][16] qh ++ [4 nsb][4] scales ++ [nsb] f16 d
// so lane l's data piece i is the 16 B at plane + 16 (l + 64 i): one wave load = 1 KiB contiguous.
//
// Work split: lane l owns the same piece positions of every row, so its Q8_K activation slices (from
// the LDS prologue: rms_norm * w -> Q8_K, quantize only, or a copy) live in registers for the whole
// launch; a wave owns R rows per group (x2 for gate|up), groups stride over a persistent grid, the
// next group's loads are in flight while the current one is reduced (PF), and the per-row results are
// parked per lane and stored once after the streaming loop (lean::store_group: residual, SiLU-GLU,
// RoPE + f16 K/V cache stores).
//
// Integer parts are exact (v_dot4_i32_i8 on the 4/6-bit weights and the Q8_K int8 activation, bsums
// for the min / -32 offsets) as in ggml_vec_dot_q4_K_q8_K / ggml_vec_dot_q6_K_q8_K
// (ggml-quants.c:7714, 8919); only the fp32 combination order differs (per 32/64 elements).
#include "gemv_lean.h"

#include <algorithm>
#include <cstdlib>

#ifdef KCPP_STAMPS
// phase stamps (tools/rs_stamps.py; instrumented A/B build only): per workgroup 8 words -- entry, activation
// ready, first group reduced, streaming done, results stored, (grid << 32 | block), K | mode << 24, rows
__device__ unsigned long long *g_rs_stamps;
__device__ unsigned g_rs_slot;
#define RS_STAMP(ph)                                                                                                  \
    if (threadIdx.x == 0 && st_) __hip_atomic_store(&st_[(ph)], __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED,   \
                                                     __HIP_MEMORY_SCOPE_AGENT);
extern "C" int kcpp_rs_set_stamps(void *p) {
    unsigned z = 0;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_rs_stamps), &p, sizeof p) != hipSuccess) return -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_rs_slot), &z, sizeof z) == hipSuccess ? 0 : -1;
}
#else
#define RS_STAMP(ph)
#endif

#include "gemv_rs.h"
#include "gemv_dec_impl.h"
using namespace rs;


// NI = pieces per lane per row (ceil(nsb * PIECES_PER_SB / 64)); R rows per group (x2 for gate|up);
// PRO 0: act copy, 1: rms_norm * w -> Q8_K, 2: quantize only, 3: LayerNorm * w -> Q8_K (the Command-R class: q|k|v,
// the 8-wave gate|up and the head only -- instances of their own, the PRO 1 / 2 ones are the code they were); MC = ceil(K / 4096) prologue chunks;
// PF: issue the next group's loads before reducing the current one.
// NWV waves per workgroup (4, or 8: one activation prologue shared by twice the waves)
// XL (long K: 70B ffn_down K = 28672, MoE n_ff > 14336): the lane's activation slices are read from the LDS image per
// piece instead of living in registers for the launch (NI up to 16 pieces per row would not fit beside the weights);
// NI is then a ceiling, pieces past the row are masked (their loads clamped to the row's last piece)
// ROUTE (MoE two-slot GLU, PRO 1, K <= 4096): the router runs in every workgroup on the prologue's normalised row
// (k_moe_route<WT, true>'s thread -> element map, fma order and wave / workgroup sums, so the ids and weights are
// bit-identical), then the expert weights are issued; one launch per layer less
// MODE 3 (MoE, both top-2 slots' down projections in one launch, NWV = 8, PRO 2): waves 0-3 stream expert eid's rows
// against slot 0's h (x), waves 4-7 the same rows of expert eid1 against slot 1's h (x + K); the halves meet in LDS and
// the row is ((w0 o0) + (w1 o1)) + res -- the two chained MODE 0 launches' result bit for bit
// EX (MODE 2, R = 2; the Qwen2 class): DecArgs.bias added to the products and, with rope_neox, the q / k groups are the
// NeoX rotation pairs (rows j and j + D/2 of a head: lean::ex_group_rows) -- separate instances, so the Llama launches
// (no bias, NORM pairs) run the instructions they ran before
template <int TYPE, int NI, int R, int MODE, int PRO, int MC, int PF, int NWV = 4, bool XL = false, bool ROUTE = false,
          bool EX = false>
__global__ void __launch_bounds__(64 * NWV) k_gemv_rs(const int kb_nblk, const DecArgs a) {
    static_assert(!EX || (MODE == 2 && R == 2), "EX: the q|k|v launch");
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    // the workgroup count as the first explicit argument, not gridDim.x.  Measured: growing DecArgs by bias[] /
    // rope_neox alone took the bench decode from 617 to 607 tok/s, and reading the count here instead brought it back
    // (profiles/qwen2_kernarg_ab.jsonl).  Supposed, not shown: the implicit arguments lie behind DecArgs, and a load
    // from them past byte 320 of the argument block is what costs the ~0.14 us per launch
    const int KB_BID = (int)blockIdx.x, KB_NBLK = kb_nblk;
    constexpr bool AUX = false;
    float *const aux0 = nullptr, *const aux1 = nullptr, *const aux2 = nullptr;
    uint16_t *const auxh = nullptr;
    const RopeP rp{};
    float *const auxrn = nullptr, *const auxyn = nullptr;
#include "gemv_rs_body.inc"
}
// the ggml plugin's fused nodes (AuxOut): the same body storing the intermediate nodes' tensors too -- MODE 0 the
// product before the residual, MODE 1 gate, silu(gate) and up beside the GLU product
template <int TYPE, int NI, int R, int MODE, int PRO, int MC, int PF, int NWV>
__global__ void __launch_bounds__(64 * NWV) k_gemv_rs_aux(const int kb_nblk, const DecArgs a, const AuxOut o) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int KB_BID = (int)blockIdx.x, KB_NBLK = kb_nblk;
    constexpr bool XL = false, ROUTE = false, AUX = true, EX = false;
    float *const aux0 = o.p0, *const aux1 = o.p1, *const aux2 = o.p2;
    uint16_t *const auxh = o.h0;
    const RopeP rp = o.rope;
    float *const auxrn = o.rn, *const auxyn = o.yn;
#include "gemv_rs_body.inc"
}

#ifndef Q_PF
#define Q_PF 0               // MODE 3 group prefetch and XL: the instance's compile-time probes (gemv_plan.h, mode 3)
#endif
#ifndef Q_XL
#define Q_XL false
#endif

namespace {
// The built instances of one (TYPE, NI, MC) class, registers-resident activation: (R, MODE, PRO, PF, NWV, ROUTE, EX),
// then the AUX kernel's (R, MODE, PRO, PF, NWV).  The plan (gemv_plan.h, GEMV_RS / GEMV_RS_AUX) chooses among them; the
// prefetching forms of the PF 0 shapes and the reverse are built and never chosen.
#define KCPP_RS_BY_PRO(X, PRO_)                                                                                       \
    X(1, 1, PRO_, 1, 4, false, false) X(1, 1, PRO_, 0, 4, false, false) X(2, 2, PRO_, 0, 4, false, false)              \
    X(2, 0, PRO_, 1, 4, false, false) X(2, 0, PRO_, 0, 4, false, false) X(1, 0, PRO_, 1, 4, false, false)              \
    X(1, 0, PRO_, 0, 4, false, false)
#define KCPP_RS_INSTANCES(X)                                                                                          \
    KCPP_RS_BY_PRO(X, 0) KCPP_RS_BY_PRO(X, 1) KCPP_RS_BY_PRO(X, 2)                                                     \
    X(1, 1, 1, 1, 8, false, false) X(1, 0, 2, 0, 8, false, false) X(2, 2, 1, 0, 4, false, true)                        \
    X(2, 2, 3, 0, 4, false, false) X(1, 1, 3, 1, 8, false, false) X(2, 0, 3, 0, 4, false, false)
#define KCPP_RS_AUX_INSTANCES(X) X(2, 0, 2, 0, 4) X(2, 0, 1, 0, 4) X(1, 0, 2, 0, 8) X(1, 1, 2, 1, 4) X(1, 1, 1, 1, 8)
// long K (XL, NI a ceiling, 8 waves, no prefetch): (R, MODE, PRO)
#define KCPP_RS_XL_INSTANCES(X) X(1, 0, 2) X(1, 0, 1) X(1, 0, 0) X(1, 1, 1) X(1, 1, 0) X(2, 2, 1)

template <int TYPE, int NI, int MC, bool XL>
const void *rs_instance(const GemvPlan &p) {
    const void *k = nullptr;
    if constexpr (XL) {
#define KCPP_RS_PICK(R_, MODE_, PRO_)                                                                                 \
    if (p.kernel == GEMV_RS && p.R == R_ && p.mode == MODE_ && p.pro == PRO_ && !p.PF && p.waves == 8 && !p.ROUTE && !p.EX) \
        k = (const void *)k_gemv_rs<TYPE, NI, R_, MODE_, PRO_, MC, 0, 8, true>;
        KCPP_RS_XL_INSTANCES(KCPP_RS_PICK)
#undef KCPP_RS_PICK
    } else {
#define KCPP_RS_PICK(R_, MODE_, PRO_, PF_, NWV_, ROUTE_, EX_)                                                         \
    if (p.kernel == GEMV_RS && p.R == R_ && p.mode == MODE_ && p.pro == PRO_ && p.PF == PF_ && p.waves == NWV_ &&     \
        p.ROUTE == ROUTE_ && p.EX == EX_)                                                                             \
        k = (const void *)k_gemv_rs<TYPE, NI, R_, MODE_, PRO_, MC, PF_, NWV_, false, ROUTE_, EX_>;
        KCPP_RS_INSTANCES(KCPP_RS_PICK)
        if constexpr (MC == 1) { KCPP_RS_PICK(1, 1, 1, 1, 8, true, false) }        // the routed two-slot GLU
#undef KCPP_RS_PICK
#define KCPP_RS_PICK(R_, MODE_, PRO_, PF_, NWV_)                                                                      \
    if (p.kernel == GEMV_RS_AUX && p.R == R_ && p.mode == MODE_ && p.pro == PRO_ && p.PF == PF_ && p.waves == NWV_)   \
        k = (const void *)k_gemv_rs_aux<TYPE, NI, R_, MODE_, PRO_, MC, PF_, NWV_>;
        KCPP_RS_AUX_INSTANCES(KCPP_RS_PICK)
#undef KCPP_RS_PICK
        // MODE 3 (both MoE slots' down projections): the Mixtral class, K 14336
        if constexpr (MC == 4 && NI == (TYPE == KT_Q6_K_RS ? 4 : 7))
            if (p.kernel == GEMV_RS && p.mode == 3 && p.R == 1 && p.pro == 2 && p.waves == 8)
                k = (const void *)k_gemv_rs<TYPE, NI, 1, 3, 2, 4, Q_PF, 8, Q_XL>;
    }
    return k;
}

// the (NI, MC, XL) classes built per type; rs_for_class calls f on the one the plan names (null: none)
template <int NI_, int MC_, bool XL_ = false>
struct RsClass { static constexpr int NI = NI_, MC = MC_; static constexpr bool XL = XL_; };
template <class F, class... C>
const void *rs_for_class(const GemvPlan &p, F &&f, C... c) {
    const void *k = nullptr;
    (void)((p.NI == C::NI && p.MC == C::MC && (bool)p.XL == C::XL ? (k = f(c), true) : false) || ...);
    return k;
}
template <int TYPE>
const void *rs_instance_of(const GemvPlan &p) {
    auto f = [&](auto c) { using C = decltype(c); return rs_instance<TYPE, C::NI, C::MC, C::XL>(p); };
    if constexpr (TYPE == KT_Q6_K_RS)
        return rs_for_class(p, f, RsClass<1, 1>{}, RsClass<2, 2>{}, RsClass<3, 3>{}, RsClass<4, 4>{}, RsClass<6, 6, true>{},
                            RsClass<8, 8, true>{});
    else if constexpr (TYPE == KT_Q5_K_RS)
        return rs_for_class(p, f, RsClass<1, 1>{}, RsClass<2, 1>{}, RsClass<3, 2>{}, RsClass<4, 2>{}, RsClass<5, 3>{}, RsClass<6, 3>{},
                            RsClass<7, 4>{}, RsClass<10, 5, true>{});
    else
        return rs_for_class(p, f, RsClass<1, 1>{}, RsClass<2, 1>{}, RsClass<3, 2>{}, RsClass<4, 2>{}, RsClass<5, 3>{}, RsClass<6, 3>{},
                            RsClass<7, 4>{}, RsClass<10, 5, true>{}, RsClass<12, 6, true>{}, RsClass<14, 7, true>{});
}
}  // namespace

int gemv_rs_launch(const GemvPlan &p, const DecArgs &a, const AuxOut *o, hipStream_t s) {
    const void *k = p.type == KT_Q4_K_RS   ? rs_instance_of<KT_Q4_K_RS>(p)
                    : p.type == KT_Q5_K_RS ? rs_instance_of<KT_Q5_K_RS>(p)
                    : p.type == KT_Q6_K_RS ? rs_instance_of<KT_Q6_K_RS>(p)
                                           : nullptr;
    if (p.kernel == GEMV_RS_AUX && !o) k = nullptr;
    int nblk = (int)p.nblk;                 // the kernels' first argument: see k_gemv_rs
    void *args[] = {&nblk, (void *)&a, (void *)o};
    return gemv_go(k, p.nblk, p.block, p.lds_bytes, args, s);
}

// ---------------------------------------------------------------- q|k (Q4_K_RS) + v (Q6_K_RS) in one launch
// The Q4_K_M "more bits" layers keep attn_v in Q6_K: instead of a second launch for its 1024 rows (a latency-bound
// kernel of its own: prologue, one group per wave, epilogue), segments 0 / 1 (q, k) run the Q4_K_RS path and
// segment 2 (v) the Q6_K_RS path of one grid over the same LDS activation (rms_norm -> Q8_K prologue, both types'
// vec_dot_type); groups are wave-uniform in type.  Mode 2 epilogue (RoPE + f16 q / K / V stores), R = 2.
// PRO: 1 = rms_norm, 3 = LayerNorm (lean::ActPro)
template <int NIA, int NIB, int MC, bool EX = false, int PRO = 1>
__global__ void __launch_bounds__(256) k_gemv_rs_qkv(const int kb_nblk, const DecArgs a) {   // kb_nblk: see k_gemv_rs
    using TA = RS<KT_Q4_K_RS>;
    using TB = RS<KT_Q6_K_RS>;
    constexpr int R = 2;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int K = (int)a.K, nsb = K / 256;
    const int RBA = nsb * TA::BYTES, RBB = nsb * TB::BYTES;
    const int npA = nsb * TA::PIECES_PER_SB, npB = nsb * TB::PIECES_PER_SB;
    const int N0 = (int)a.N[0], N1 = (int)a.N[1], N2 = (int)a.N[2];
    const int ngA = (N0 + N1) / R, ngroups = ngA + N2 / R;
    const int nw = kb_nblk * 4;
    const int wid = (int)blockIdx.x * 4 + wave;
    const typename TA::Lane lca = TA::lane_consts(lane);
    const typename TB::Lane lcb = TB::lane_consts(lane);
    auto group_rows = [&](int g, int &seg, int &row0) {
        if (g < ngA) {
            const int r = g * R;
            seg = r < N0 ? 0 : 1;
            row0 = seg == 0 ? r : r - N0;
        } else {
            seg = 2;
            row0 = (g - ngA) * R;
        }
    };
    struct BufA { typename TA::W w[NIA][R]; };
    struct BufB { typename TB::W w[NIB][R]; };
    auto issueA = [&](int g, BufA &b) {
        int seg, row0;
        group_rows(g, seg, row0);
        const uint8_t *W = seg == 0 ? a.W[0] : a.W[1];
        int rbase = row0, rstride = 1;      // EX: NeoX pairs in the q / k roles (lean::ex_group_rows)
        if constexpr (EX) lean::ex_group_rows(a, seg == 0 ? a.role[0] : a.role[1], row0, rbase, rstride);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int wrow = EX ? rbase + r * rstride : row0 + r;
#pragma unroll
            for (int i = 0; i < NIA; ++i) TA::load(W + (int64_t)wrow * RBA, nsb, min(lane + 64 * i, npA - 1), b.w[i][r]);
        }
    };
    auto issueB = [&](int g, BufB &b) {
        const int row0 = (g - ngA) * R;
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int i = 0; i < NIB; ++i) TB::load(a.W[2] + (int64_t)(row0 + r) * RBB, nsb, min(lane + 64 * i, npB - 1), b.w[i][r]);
    };
    BufA ba;
    BufB bb;
    const int g0 = min(wid, ngroups - 1);
    lean::ActPro<PRO, MC> pro;
    pro.load(a);
    if (g0 < ngA) issueA(g0, ba);
    else issueB(g0, bb);
    pro.compute(a, lds);
    typename TA::Act xa[NIA];
    typename TB::Act xb[NIB];
#pragma unroll
    for (int i = 0; i < NIA; ++i) TA::act(lds, K, min(TA::sb_of(lane, i), nsb - 1), lca, xa[i]);
#pragma unroll
    for (int i = 0; i < NIB; ++i) TB::act(lds, K, min(TB::sb_of(lane, i), nsb - 1), lcb, xb[i]);
    float slot[R] = {0.0f, 0.0f};
    int slot_g = -1;
    int k = 0;
    for (int g = wid; g < ngroups; g += nw, ++k) {
        float acc[R] = {0.0f, 0.0f};
        if (g < ngA) {
            if (k) issueA(g, ba);
#pragma unroll
            for (int i = 0; i < NIA; ++i) {
                const bool ok = (NIA * 64 == npA) || lane + 64 * i < npA;
#pragma unroll
                for (int r = 0; r < R; ++r) { const float p = TA::dot(ba.w[i][r], xa[i], lca); acc[r] += ok ? p : 0.0f; }
            }
        } else {
            if (k) issueB(g, bb);
#pragma unroll
            for (int i = 0; i < NIB; ++i) {
                const bool ok = (NIB * 64 == npB) || lane + 64 * i < npB;
#pragma unroll
                for (int r = 0; r < R; ++r) { const float p = TB::dot(bb.w[i][r], xb[i], lcb); acc[r] += ok ? p : 0.0f; }
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(wave_sum_f(acc[r]))));
        const bool mine = lane == k;
#pragma unroll
        for (int r = 0; r < R; ++r) slot[r] = mine ? acc[r] : slot[r];
        slot_g = mine ? g : slot_g;
    }
    if (slot_g < 0) return;
    int seg, row0;
    group_rows(slot_g, seg, row0);
    if constexpr (EX) lean::store_group_ex(a, seg, row0, slot);
    else lean::store_group<R, 2>(a, seg, row0, slot);
}

// q|k|v decode projection with q, k in Q4_K_RS and v in Q6_K_RS (segments 0, 1, 2): one launch.  -3 when not covered.
// pro: 1 = rms_norm prologue, 3 = LayerNorm (no bias / NeoX instance: -3)
extern "C" int kcpp_gemv_rs_qkv_mixed_pro(const void *args, int pro, void *stream) {
    const DecArgs &a = *(const DecArgs *)args;
    GemvMixedPlan m;
    if (gemv_qkv_mixed_plan(gemv_shape_of(KT_Q4_K_RS, a, 2, pro, 2), &m)) return m.rc;
    void (*k)(int, const DecArgs) = nullptr;
#define KCPP_QKVM(A_, B_, M_)                                                                                          \
    if (m.NIA == A_ && m.NIB == B_ && m.MC == M_)                                                                      \
        k = m.PRO == 3 ? k_gemv_rs_qkv<A_, B_, M_, false, 3> : (m.EX ? k_gemv_rs_qkv<A_, B_, M_, true> : k_gemv_rs_qkv<A_, B_, M_>);
    KCPP_QKVM(2, 1, 1)          // n_embd 4096 (Llama-3-8B)
    KCPP_QKVM(4, 2, 2)          // n_embd 8192 (Llama-3-70B)
    KCPP_QKVM(1, 1, 1)
#undef KCPP_QKVM
    int nblk = (int)m.nblk;
    void *ka[] = {&nblk, (void *)&a};
    return gemv_go((const void *)k, m.nblk, m.block, m.lds_bytes, ka, (hipStream_t)stream);
}
extern "C" int kcpp_gemv_rs_qkv_mixed(const void *args, void *stream) { return kcpp_gemv_rs_qkv_mixed_pro(args, 1, stream); }

// ---------------------------------------------------------------- q (RS layout) + k|v (Q8_0) in one launch
// Mixtral's Q5_K_M policy keeps attn_k / attn_v in Q8_0 (n_expert == 8) and attn_q in Q5_K, so its q|k|v decode step
// was two dependent launches of short latency-bound kernels.  Here one grid runs both unchanged: workgroups [0, nA) are
// the RS q launch (k_gemv_rs's body, mode 2: RoPE + f16 q), [nA, nA + nB) the Q8_0 k|v launch (k_gemv_dec's body,
// mode 2: RoPE of k + the f16 K / V cache stores), each with its own prologue (Q8_K / Q8_0 activation of the same
// normalised row) and its own grid size, so every row's arithmetic -- and result -- is the separate launches'.  The
// bodies are included textually (gemv_rs_body.inc, gemv_dec_body.inc) so that each reads its DecArgs kernel parameter
// directly (through a reference the parameter is copied to scratch memory and every load goes through it).
template <int TA, int NIA, int MCA, int ITB>
__global__ void __launch_bounds__(256) k_gemv_qkv_dual(const DecArgs a, const DecArgs b, int nA) {
    if ((int)blockIdx.x < nA) {
        constexpr int TYPE = TA, NI = NIA, R = 2, MODE = 2, PRO = 1, MC = MCA, PF = 0, NWV = 4;
        constexpr bool XL = false, ROUTE = false, AUX = false, EX = false;
        float *const aux0 = nullptr, *const aux1 = nullptr, *const aux2 = nullptr;
        uint16_t *const auxh = nullptr;
        const RopeP rp{};
        float *const auxrn = nullptr, *const auxyn = nullptr;
        extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
        const int KB_BID = (int)blockIdx.x, KB_NBLK = nA;
#include "gemv_rs_body.inc"
    } else {
        constexpr int TYPE = KT_Q8_0, R = 2, MODE = 2, PRO = 1, MC = 1, IT = ITB;
        extern __shared__ __attribute__((aligned(16))) uint8_t lds_act[];
        const int KB_BID = (int)blockIdx.x - nA, KB_NBLK = (int)gridDim.x - nA;
#define KB_ARGS b
#include "gemv_dec_body.inc"
#undef KB_ARGS
    }
}

// qa: the RS-layout segments (mode 2, rms_norm prologue), kv: Q8_0 segments (mode 2): the two halves of
// gemv_qkv_dual_plan.  -3 when the pair is not covered (the caller launches them separately).
extern "C" int kcpp_gemv_qkv_dual(const void *qargs, int qtype, const void *kvargs, void *stream) {
    const DecArgs &a = *(const DecArgs *)qargs;
    const DecArgs &b = *(const DecArgs *)kvargs;
    GemvDualPlan d;
    if (gemv_qkv_dual_plan(gemv_shape_of(qtype, a, 2, 1, 2), gemv_shape_of(KT_Q8_0, b, 2, 1, 2), &d)) return d.rc;
    void (*k)(const DecArgs, const DecArgs, int) = nullptr;
    if (d.b.IT == 2 && d.a.NI == 2 && qtype == KT_Q5_K_RS) k = k_gemv_qkv_dual<KT_Q5_K_RS, 2, 1, 2>;      // Mixtral: K 4096
    if (d.b.IT == 2 && d.a.NI == 2 && qtype == KT_Q4_K_RS) k = k_gemv_qkv_dual<KT_Q4_K_RS, 2, 1, 2>;
    if (d.b.IT == 2 && d.a.NI == 1 && qtype == KT_Q6_K_RS) k = k_gemv_qkv_dual<KT_Q6_K_RS, 1, 1, 2>;
    int nA = (int)d.a.nblk;
    void *ka[] = {(void *)&a, (void *)&b, &nA};
    return gemv_go((const void *)k, d.nblk, 256, d.lds_bytes, ka, (hipStream_t)stream);
}

// K coverage of the RS kernels (the runtime picks an RS layout only where this holds): gemv_plan.h gemv_rs_supported
extern "C" int kcpp_rs_supported(int type, int64_t K) { return gemv_rs_supported(type, K); }

// the plan restricted to the RS kernels; -3 = not covered
extern "C" int kcpp_gemv_rs(int type, const void *args, int mode, int pro, void *stream) {
    const DecArgs &a = *(const DecArgs *)args;
    GemvPlan p;
    if (gemv_plan(gemv_shape_of(type, a, mode, pro, 0), GEMV_ENTRY_RS, &p)) return p.rc;
    return gemv_rs_launch(p, a, nullptr, (hipStream_t)stream);
}

// the ggml plugin's fused nodes: the AUX instances, which also store the intermediate nodes' tensors (AuxOut); the
// prologue is the norm when DecArgs.nw is set (x = the norm's input, nw = the MUL's weight), else quantize only;
// -3 where no AUX instance covers the shape
extern "C" int kcpp_gemv_rs_aux(int type, const void *args, int mode, const AuxOut *aux, void *stream) {
    const DecArgs &a = *(const DecArgs *)args;
    GemvPlan p;
    if (gemv_plan(gemv_shape_of(type, a, mode, 0, 0, aux), GEMV_ENTRY_RS_AUX, &p)) return p.rc;
    return gemv_rs_launch(p, a, aux, (hipStream_t)stream);
}
