// gemm_common.h -- shared by the batched quantized GEMM's translation units (gemm.hip and one gemm_*.hip per kernel
// family): vector types, the exact f16 dequantization helpers, LDS-DMA, tile orders, and the host interface between
// the runner (gemm.hip gemm_run) and each family's launcher.
#pragma once
#include "kcpp_common.h"
#include "kcpp_internal.h"
#include "gemm_plan.h"

#include <algorithm>
#include <cstdlib>
#include <type_traits>

typedef _Float16 h2v __attribute__((ext_vector_type(2)));
typedef _Float16 h8v __attribute__((ext_vector_type(8)));
typedef float f16acc __attribute__((ext_vector_type(16)));

#define GB_M 128
#define GB_N 64
#define GB_K 256
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

#ifndef KCPP_GEMM_PROBE
#define KCPP_GEMM_PROBE 0       // timing probes only (tools/gemm_ab.py with a PROBE_DEFS build): 1 no loads in the
#endif                          // super-block loop, 2 no main-loop MFMAs, 3 no barrier, 4 no A staging, 5 no weight loads

// ---------------------------------------------------------------- dequant helpers
// v_perm_b32 byte selects: 4..7 = bytes of src0 (t), 0..3 = bytes of src1 (0x64 each):
// bytes (b0,0x64,b1,0x64) are the f16 halves 1024+b0, 1024+b1 (exact for b < 1024)
__device__ __forceinline__ h2v bias_lo(uint32_t t) { return __builtin_bit_cast(h2v, __builtin_amdgcn_perm(t, 0x64646464u, 0x00050004u)); }
__device__ __forceinline__ h2v bias_hi(uint32_t t) { return __builtin_bit_cast(h2v, __builtin_amdgcn_perm(t, 0x64646464u, 0x00070006u)); }

// (1024 + q) * s - (1024 + off) * s  ==  (q - off) * s   exactly (single rounding of an exact value)
__device__ __forceinline__ h2v scale2(h2v x, _Float16 s, _Float16 bias) {
    const h2v sv = {s, s};
    const h2v bv = {bias, bias};
    return __builtin_elementwise_fma(x, sv, bv);
}
// 8 weights (two dwords of bytes) -> fragment of 8 halves, (byte - off) * s
__device__ __forceinline__ h8v frag8(uint32_t t0, uint32_t t1, float s, float off) {
    const _Float16 sh = (_Float16)s;
    const _Float16 bh = (_Float16)(-(1024.0f + off) * s);
    const h2v a = scale2(bias_lo(t0), sh, bh), b = scale2(bias_hi(t0), sh, bh);
    const h2v c = scale2(bias_lo(t1), sh, bh), d = scale2(bias_hi(t1), sh, bh);
    h8v r;
    r[0] = a[0]; r[1] = a[1]; r[2] = b[0]; r[3] = b[1]; r[4] = c[0]; r[5] = c[1]; r[6] = d[0]; r[7] = d[1];
    return r;
}

// Q6_K variant: (byte - off) exactly first (small ints), then * s (exact: |8*(sc>>3)*(q-32)| <= 4096,
// a multiple of 8; |(sc&7)*(q-32)| <= 224).  A single fma would need a bias beyond the f16 range.
__device__ __forceinline__ h8v frag8_sub(uint32_t t0, uint32_t t1, float s, float off) {
    const h2v sv = {(_Float16)s, (_Float16)s};
    const h2v bv = {(_Float16)(-(1024.0f + off)), (_Float16)(-(1024.0f + off))};
    const h2v a = (bias_lo(t0) + bv) * sv, b = (bias_hi(t0) + bv) * sv;
    const h2v c = (bias_lo(t1) + bv) * sv, d = (bias_hi(t1) + bv) * sv;
    h8v r;
    r[0] = a[0]; r[1] = a[1]; r[2] = b[0]; r[3] = b[1]; r[4] = c[0]; r[5] = c[1]; r[6] = d[0]; r[7] = d[1];
    return r;
}

// get_scale_min_k4 (ggml-quants.c:1899) on the 12 scale bytes held in hdr.y/z/w (registers only)
__device__ __forceinline__ void k4_sm(const uint4 &hdr, int j, int &d, int &m) {
    auto b = [&](int k) -> int {
        const uint32_t w = k < 4 ? hdr.y : (k < 8 ? hdr.z : hdr.w);
        return (w >> (8 * (k & 3))) & 0xFF;
    };
    if (j < 4) { d = b(j) & 63; m = b(j + 4) & 63; }
    else { d = (b(j + 4) & 0xF) | ((b(j - 4) >> 6) << 4); m = (b(j + 4) >> 4) | ((b(j) >> 6) << 4); }
}

// get_scale_min_k4 for all 8 sub-blocks at once, four 6-bit values per dword: byte j of sc_lo / m_lo is
// sub-block j, byte j of sc_hi / m_hi sub-block 4 + j (scales bytes 0-3 = hdr.y, 4-7 = hdr.z, 8-11 = hdr.w)
__device__ __forceinline__ void k4_all(const uint4 &h, uint32_t &sc_lo, uint32_t &sc_hi, uint32_t &m_lo, uint32_t &m_hi) {
    sc_lo = h.y & 0x3F3F3F3Fu;
    m_lo = h.z & 0x3F3F3F3Fu;
    sc_hi = (h.w & 0x0F0F0F0Fu) | ((h.y >> 2) & 0x30303030u);
    m_hi = ((h.w >> 4) & 0x0F0F0F0Fu) | ((h.z >> 2) & 0x30303030u);
}

// fragment slot for element k (0..255) of weight row nl (0..63): (tile, step, lane); 16 B per slot
__device__ __forceinline__ int bslot(int nl, int k) {
    const int tile = nl >> 5, s = k >> 4, h = (k >> 3) & 1;
    return ((tile * 16 + s) * 64 + h * 32 + (nl & 31));
}

template <int TYPE> struct GemmTraits {
    static constexpr int NB = 1;            // B fragment planes (Q6_K: 2)
    static constexpr bool MINS = false;     // Q8_K bsum x mins term
    static constexpr bool SB = true;        // per-256 scaling (K-quants) vs per-32 (Q4_0/Q8_0)
};
template <> struct GemmTraits<KT_Q4_K> { static constexpr int NB = 1; static constexpr bool MINS = true; static constexpr bool SB = true; };
template <> struct GemmTraits<KT_Q5_K> { static constexpr int NB = 1; static constexpr bool MINS = true; static constexpr bool SB = true; };
template <> struct GemmTraits<KT_Q6_K> { static constexpr int NB = 2; static constexpr bool MINS = false; static constexpr bool SB = true; };
template <> struct GemmTraits<KT_Q3_K> { static constexpr int NB = 1; static constexpr bool MINS = false; static constexpr bool SB = true; };
template <> struct GemmTraits<KT_Q2_K> { static constexpr int NB = 1; static constexpr bool MINS = true; static constexpr bool SB = true; };
template <> struct GemmTraits<KT_Q4_0> { static constexpr int NB = 1; static constexpr bool MINS = false; static constexpr bool SB = false; };
template <> struct GemmTraits<KT_Q5_0> { static constexpr int NB = 1; static constexpr bool MINS = false; static constexpr bool SB = false; };
template <> struct GemmTraits<KT_Q8_0> { static constexpr int NB = 1; static constexpr bool MINS = false; static constexpr bool SB = false; };
template <> struct GemmTraits<KT_Q4_1> { static constexpr int NB = 1; static constexpr bool MINS = false; static constexpr bool SB = false; };
template <> struct GemmTraits<KT_Q5_1> { static constexpr int NB = 1; static constexpr bool MINS = false; static constexpr bool SB = false; };
template <> struct GemmTraits<KT_IQ4_NL> { static constexpr int NB = 1; static constexpr bool MINS = false; static constexpr bool SB = false; };
template <> struct GemmTraits<KT_IQ4_XS> { static constexpr int NB = 2; static constexpr bool MINS = false; static constexpr bool SB = true; };
// Q8_1-activation types: the per-block m_w * s_a term (block_q8_1.s)
template <int TYPE> constexpr bool kGemmM1 = TYPE == KT_Q4_1 || TYPE == KT_Q5_1;

__device__ __forceinline__ uint4 ldg16(const void *p) { return *(const uint4 *)p; }
__device__ __forceinline__ uint32_t u4c(const uint4 &v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w)); }

// 16 B global -> LDS per lane (LDS address = wave-uniform base + 16 * lane)
// LDS-DMA issued from inline asm: the compiler does not track these writes, so it inserts no vmcnt(0) in front of
// the LDS reads that follow (it cannot tell the ring stage being filled from the one being read, and a compiler-
// visible DMA would drain every prefetch at the first read); the kernel orders them itself (s_waitcnt + barrier).
// lds_base: wave-uniform LDS byte address; lane l writes lds_base + size * l.
__device__ __forceinline__ uint32_t lds_addr(const void *p) {
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)p;
}
__device__ __forceinline__ void dma16(const void *g, const void *lds_base) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(g),
                 "s"(__builtin_amdgcn_readfirstlane(lds_addr(lds_base))) : "memory", "m0");
}
__device__ __forceinline__ void dma4(const void *g, const void *lds_base) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off" ::"v"(g),
                 "s"(__builtin_amdgcn_readfirstlane(lds_addr(lds_base))) : "memory", "m0");
}

// XCD-aware tile order: blocks b and b + 8 share an XCD (dealt round-robin).  XCD x serves token tiles
// [G set, +G) (set = x % (MT / G)) against the row tiles of class x / (MT / G): the G token-tile workgroups of one
// row tile run back to back on one XCD, so its weights come from HBM once and from that XCD's L2 G - 1 times,
// while the XCD's L2 holds G token tiles of activations.  Falls back to plain order when the grid does not divide.
__device__ __forceinline__ void xcd_tile(int64_t id, int64_t nwg, int MT, int64_t ntn, int G, int64_t &mt, int64_t &nt) {
    const int nset = G > 0 && MT % G == 0 ? MT / G : 0;
    const int xper = nset > 0 && 8 % nset == 0 ? 8 / nset : 0;
    if (xper > 0 && nwg % 8 == 0 && ntn % xper == 0) {
        const int64_t x = id & 7, j = id >> 3;
        mt = (x % nset) * G + j % G;
        nt = (j / G) * xper + x / nset;
    } else {
        mt = id % MT;
        nt = id / MT;
    }
}

// swizzled 32-row LDS image of 16-byte chunks (the layout: gemm_q4v4.hip): slot of chunk c of row m
__device__ __forceinline__ int swz(int m, int c) { return 72 * (4 * (c >> 3) + (m >> 3)) + (m & 7) + 8 * (c & 7); }

// grouped layouts (MoE prefill): group e's gcnt[e] real rows sit at virtual rows [P_e, P_e + 128 ceil(n_e / 128)),
// P_e = the padded sizes before it; vrow -> (group, its virtual base, its real first row, its count)
__device__ __forceinline__ int grp_find(const int32_t *gcnt, int gne, int64_t v, int64_t &P, int64_t &r0, int64_t &n) {
    P = 0;
    r0 = 0;
    for (int e = 0; e < gne; ++e) {
        const int64_t c = gcnt[e], pe = (c + 127) / 128 * 128;
        if (v < P + pe) { n = c; return e; }
        P += pe;
        r0 += c;
    }
    n = 0;
    return -1;
}

// up to 3 weight segments back to back in the output columns (q|k|v); segment boundaries multiples of 128
struct Q80Segs {
    const uint8_t *W[3];
    int64_t N[3];
    int nseg;
};

// ---------------------------------------------------------------- host: runner <-> family launchers
// One launch of a family's kernel: matrix W -> Y (+ res).  The runner (gemm.hip gemm_run) fills the activation image,
// calls the launcher, then finishes split-K partials and the GLU product itself.
struct GemmArgs {
    int type;                                            // weight type (KT_*)
    const void *W;                                       // this launch's matrix (Q6P: its prefill image)
    const void *Wd;                                      // Q6P: the Q6_K_RS weights beside the image (row scales)
    float *Y;
    int64_t ldy;
    const float *res;
    int64_t ldr;
    const void *W2;                                      // V4 GLU: the up matrix, computed by the same launch
    float *Y2;                                           //   into Y2
    int64_t ldy2;
    int64_t K, N, M, Mp;
    const void *act;                                     // the quantized activation (V4 / Q6P read it as it is)
    void *af;                                            // the family's activation image (gemm.hip gemm_act_image)
    float *dy;
    void *bsf;
    const float *s81;                                    // V1 over Q8_1 activations: block_q8_1.s [M][K/32]
    float *part;                                         // split-K partials [KS][Mp][N]
    const int32_t *gcnt;                                 // grouped (MoE prefill): device row counts, groups, bytes
    int gne;                                             //   between the groups' matrices
    int64_t wstride;
    hipStream_t s;
};
// each returns 0, a KCPP_CHECK error, or -3 for a plan / type its kernels do not cover
int gemm_v1_launch(const GemmPlan &p, const GemmArgs &a);
int gemm_kq_launch(const GemmPlan &p, const GemmArgs &a);
int gemm_q4v3_launch(const GemmPlan &p, const GemmArgs &a);
int gemm_q6v3_launch(const GemmPlan &p, const GemmArgs &a);
int gemm_q4v4_launch(const GemmPlan &p, const GemmArgs &a);
int gemm_q6p_launch(const GemmPlan &p, const GemmArgs &a);
// Q8_0 at M <= 32, the whole operation: split-K partials of sg (and, mode 1, of W2) into part, then the ordered reduce
// (plain, + residual, silu(g) * u, or that quantized to Q8_0 into qout)
int gemm_q80s_run(Q80Segs sg, const void *W2, int64_t K, int64_t N, const void *act, int64_t M, float *Y, int64_t ldy,
                  const float *res, int64_t ldr, int mode, uint8_t *qout, float *part, hipStream_t s);
int gemm_q6p_build(const void *W, int64_t K, int64_t N, void *img, hipStream_t s);
