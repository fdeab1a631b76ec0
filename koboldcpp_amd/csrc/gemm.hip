// gemm.hip -- batched (prefill / ubatch) quantized mat-mul on CDNA4 matrix cores.
//
// Replaces the reference's batched paths -- mul_mat_q (ggml/src/ggml-cuda/mmq.cuh:2572-2905, DP4A
// on AMD, no MFMA) and the default ROCm "dequantize the whole weight to F16 + hipblasGemmEx with
// FP16 compute" path (ggml-cuda.cu:1186-1284) -- while computing exactly what the CPU vec_dot does
// (ggml-quants.c:3922,5519,7714,8282,8919): weights x CPU-quantized activations (Q8_K / Q8_0) as
// exact integer block dots, scaled per super-block (or per 32-block) in fp32.
//
// How the integer dot stays exact on f16 MFMA (v_mfma_f32_32x32x16_f16, fp32 accumulate):
//   * activations are int8 values -> exact in f16;
//   * the weight operand is the *integer* sub-block product sc*q (Q4_K <= 945, Q5_K <= 1953:
//     exact in f16), or for Q6_K sc*(q-32) split as 8*(sc>>3)*(q-32) + (sc&7)*(q-32), both
//     exact, accumulated into the same fp32 accumulator by two MFMAs;
//   * products are exact and partial sums stay < 2^24, so the fp32 accumulator holds the same
//     integer as the CPU's int32 `sumi`; Q4_K/Q5_K mins use a 16-deep MFMA over the Q8_K bsums.
// Dequantization to those f16 integers costs 2 VALU ops per pair of weights (v_perm_b32 builds
// 1024+q halves, v_pk_fma_f16 scales and removes the 1024 bias exactly).
//
// Tiling: workgroup = 4 waves = 128 tokens x 64 weight rows, K step 256.  The 64x256 weight tile
// is dequantized once per workgroup into LDS in MFMA-fragment order (ds_read_b128 per lane,
// conflict-free); each wave owns 32 tokens x 64 rows (two 32x32 MFMA tiles).
//
// Files: gemm_plan.h decides which kernel family runs a shape and with what geometry (host-only, testable without a
// GPU); this file runs the plan (gemm_run: activation image, launch, split-K finish, GLU) and holds the C entry
// points; each family's kernel and launcher sit in their own file (gemm_v1 / gemm_kq / gemm_q4v3 / gemm_q6v3 /
// gemm_q4v4 / gemm_q6p / gemm_q80s .hip); gemm_common.h is what they share.
#include "gemm_common.h"

// ================================================================ activation images, one per kernel family
// ---------------------------------------------------------------- activation -> f16 operand
// a16 [Mp][K] f16 (int8 values), dy [Mp][K/G] f32 (copied), bs16 [Mp][K/16] f16 (Q8_K bsums)
__global__ void k_act_to_f16(const uint8_t *__restrict__ act, int vt, int64_t K, int64_t M, int64_t Mp,
                             _Float16 *__restrict__ a16, float *__restrict__ dy, _Float16 *__restrict__ bs16) {
    const int64_t m = blockIdx.y;
    const int64_t G = vt == KT_Q8_K ? 256 : 32;
    const bool valid = m < M;
    const int8_t *qs = (const int8_t *)act + m * K;
    for (int64_t i = (int64_t)threadIdx.x * 4 + (int64_t)blockIdx.x * 1024; i < K && i < ((int64_t)blockIdx.x + 1) * 1024;
         i += (int64_t)blockDim.x * 4) {
        const int v = valid ? *(const int *)(qs + i) : 0;
        a16[m * K + i + 0] = (_Float16)(int8_t)(v & 0xFF);
        a16[m * K + i + 1] = (_Float16)(int8_t)((v >> 8) & 0xFF);
        a16[m * K + i + 2] = (_Float16)(int8_t)((v >> 16) & 0xFF);
        a16[m * K + i + 3] = (_Float16)(int8_t)((v >> 24) & 0xFF);
    }
    if (blockIdx.x == 0) {
        const float *d = (const float *)(act + M * K) + m * (K / G);
        for (int64_t i = threadIdx.x; i < K / G; i += blockDim.x) dy[m * (K / G) + i] = valid ? d[i] : 0.0f;
        if (vt == KT_Q8_K) {
            const int16_t *bs = (const int16_t *)(act + M * K + M * (K / 256) * 4) + m * (K / 16);
            for (int64_t i = threadIdx.x; i < K / 16; i += blockDim.x) bs16[m * (K / 16) + i] = valid ? (_Float16)bs[i] : (_Float16)0;
        }
    }
}

// A fragment order: af[(mt*(K/16) + s16)*64 + lane] = 8 halves of token 32mt + (lane&31),
// k = 16 s16 + 8 (lane>>5) .. +7.  bsf[(mt*(K/256) + sb)*64 + lane] = Q8_K bsums g = 8 (lane>>5)..+7.
__global__ void k_act_frag(const uint8_t *__restrict__ act, int64_t K, int64_t M, int64_t Mp, h8v *__restrict__ af,
                           float *__restrict__ dy, h8v *__restrict__ bsf) {
    const int64_t nA = Mp * K / 8, nS = (Mp / 32) * (K / 256) * 64, nD = Mp * (K / 256);
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int8_t *qs = (const int8_t *)act;
    const float *d = (const float *)(act + M * K);
    const int16_t *bs = (const int16_t *)(act + M * K + M * (K / 256) * 4);
    if (i < nA) {
        const int lane = (int)(i & 63);
        const int64_t s16 = (i >> 6) % (K / 16), mt = (i >> 6) / (K / 16);
        const int64_t m = 32 * mt + (lane & 31), k0 = 16 * s16 + 8 * (lane >> 5);
        uint2 v = make_uint2(0, 0);
        if (m < M) v = *(const uint2 *)(qs + m * K + k0);
        const uint32_t w[2] = {v.x, v.y};
        h8v r;
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = (_Float16)(int8_t)((w[e >> 2] >> (8 * (e & 3))) & 0xFF);
        af[i] = r;
    } else if (i < nA + nS) {
        const int64_t j = i - nA;
        const int lane = (int)(j & 63);
        const int64_t sb = (j >> 6) % (K / 256), mt = (j >> 6) / (K / 256);
        const int64_t m = 32 * mt + (lane & 31);
        h8v r;
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = m < M ? (_Float16)bs[m * (K / 16) + sb * 16 + 8 * (lane >> 5) + e] : (_Float16)0;
        bsf[j] = r;
    } else if (i < nA + nS + nD) {
        const int64_t j = i - nA - nS;
        const int64_t m = j / (K / 256);
        dy[j] = m < M ? d[j] : 0.0f;
    }
}

// k_act_frag3: af as k_act_frag with the permuted k order; dyT[sb][Mp] (transposed, so one super-block's
// 128 token scales are one contiguous 512 B LDS-DMA); bsf as k_act_frag.
__global__ void k_act_frag3(const uint8_t *__restrict__ act, int64_t K, int64_t M, int64_t Mp, h8v *__restrict__ af,
                            float *__restrict__ dyT, h8v *__restrict__ bsf) {
    const int64_t nA = Mp * K / 8, nS = (Mp / 32) * (K / 256) * 64, nD = Mp * (K / 256);
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int8_t *qs = (const int8_t *)act;
    const float *d = (const float *)(act + M * K);
    const int16_t *bs = (const int16_t *)(act + M * K + M * (K / 256) * 4);
    if (i < nA) {
        const int lane = (int)(i & 63), kg = lane >> 5;
        const int64_t s16 = (i >> 6) % (K / 16), mt = (i >> 6) / (K / 16);
        const int64_t m = 32 * mt + (lane & 31);
        const int p = (int)((s16 >> 2) & 3), st = (int)(s16 & 3);
        const int64_t k0 = 256 * (s16 >> 4) + 64 * p + 16 * kg + 4 * st;
        uint32_t lo = 0, hi = 0;
        if (m < M) {
            lo = *(const uint32_t *)(qs + m * K + k0);
            hi = *(const uint32_t *)(qs + m * K + k0 + 32);
        }
        h8v r;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            r[e] = (_Float16)(int8_t)((lo >> (8 * e)) & 0xFF);
            r[4 + e] = (_Float16)(int8_t)((hi >> (8 * e)) & 0xFF);
        }
        af[i] = r;
    } else if (i < nA + nS) {
        const int64_t j = i - nA;
        const int lane = (int)(j & 63);
        const int64_t sb = (j >> 6) % (K / 256), mt = (j >> 6) / (K / 256);
        const int64_t m = 32 * mt + (lane & 31);
        h8v r;
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = m < M ? (_Float16)bs[m * (K / 16) + sb * 16 + 8 * (lane >> 5) + e] : (_Float16)0;
        bsf[j] = r;
    } else if (i < nA + nS + nD) {
        const int64_t j = i - nA - nS;
        const int64_t sb = j / Mp, m = j % Mp;
        dyT[j] = m < M ? d[m * (K / 256) + sb] : 0.0f;
    }
}

// gcnt set: the image has Mp virtual rows of the grouped layout (grp_find), real rows from the M-row Q8_K act
__global__ void k_act_frag6(const uint8_t *__restrict__ act, int64_t K, int64_t M, int64_t Mp, h8v *__restrict__ af,
                            float *__restrict__ dyT, const int32_t *gcnt, int gne) {
    const int64_t nA = Mp * K / 8, nD = Mp * (K / 256);
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int8_t *qs = (const int8_t *)act;
    const float *d = (const float *)(act + M * K);
    auto real = [&](int64_t vm) -> int64_t {          // virtual row -> real row, or -1
        if (!gcnt) return vm < M ? vm : -1;
        int64_t P, r0, n;
        if (grp_find(gcnt, gne, vm, P, r0, n) < 0) return -1;
        return vm - P < n ? r0 + (vm - P) : -1;
    };
    if (i < nA) {
        const int lane = (int)(i & 63), kg = lane >> 5;
        const int64_t s16 = (i >> 6) % (K / 16), mt = (i >> 6) / (K / 16);
        const int64_t m = real(32 * mt + (lane & 31));
        const int u = (int)((s16 >> 2) & 3), g = (int)(s16 & 3);
        const int64_t k0 = 256 * (s16 >> 4) + 128 * (u >> 1) + 16 * (u & 1) + 32 * g + 8 * kg;
        uint2 v = make_uint2(0, 0);
        if (m >= 0) v = *(const uint2 *)(qs + m * K + k0);
        h8v r;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            r[e] = (_Float16)(int8_t)((v.x >> (8 * e)) & 0xFF);
            r[4 + e] = (_Float16)(int8_t)((v.y >> (8 * e)) & 0xFF);
        }
        af[i] = r;
    } else if (i < nA + nD) {
        const int64_t j = i - nA;
        const int64_t sb = j / Mp, m = real(j % Mp);
        dyT[j] = m >= 0 ? d[m * (K / 256) + sb] : 0.0f;
    }
}

// the image family `fam` reads (V4 / Q6P read the quantized activation itself); gcnt: k_act_frag6's grouped layout
static int gemm_act_image(int fam, const void *act, int vt, int64_t K, int64_t M, int64_t Mp, void *af, float *dy, void *bsf,
                          const int32_t *gcnt, int gne, hipStream_t s) {
    const int64_t nA = Mp * K / 8, nS = (Mp / 32) * (K / 256) * 64, nD = Mp * (K / 256);
    const auto blocks = [](int64_t nth) { return dim3((unsigned)((nth + 255) / 256)); };
    switch (fam) {
    case GEMM_V1:
        hipLaunchKernelGGL(k_act_to_f16, dim3((unsigned)((K + 1023) / 1024), (unsigned)Mp), dim3(256), 0, s,
                           (const uint8_t *)act, vt, K, M, Mp, (_Float16 *)af, dy, (_Float16 *)bsf);
        break;
    case GEMM_V2:
        hipLaunchKernelGGL(k_act_frag, blocks(nA + nS + nD), dim3(256), 0, s, (const uint8_t *)act, K, M, Mp, (h8v *)af, dy,
                           (h8v *)bsf);
        break;
    case GEMM_Q4V3:
        hipLaunchKernelGGL(k_act_frag3, blocks(nA + nS + nD), dim3(256), 0, s, (const uint8_t *)act, K, M, Mp, (h8v *)af, dy,
                           (h8v *)bsf);
        break;
    case GEMM_Q6V3:
        hipLaunchKernelGGL(k_act_frag6, blocks(nA + nD), dim3(256), 0, s, (const uint8_t *)act, K, M, Mp, (h8v *)af, dy, gcnt,
                           gne);
        break;
    default: return 0;
    }
    KCPP_CHECK(hipGetLastError());
    return 0;
}

// ================================================================ finishing kernels
// split-K partials [KS][Mp][N] summed in split order, then the residual (the unsplit kernel's tot + res)
__global__ void k_splitk_reduce(const float *__restrict__ part, int KS, int64_t M, int64_t Mp, int64_t N,
                                float *__restrict__ Y, int64_t ldy, const float *res, int64_t ldr) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * N) return;
    const int64_t t = i / N, n = i % N;
    float g = part[t * N + n];
    for (int k = 1; k < KS; ++k) g = __fadd_rn(g, part[((int64_t)k * Mp + t) * N + n]);
    Y[t * ldy + n] = res ? __fadd_rn(g, res[t * ldr + n]) : g;
}

__global__ void k_silu_mul_strided(float *__restrict__ y, int64_t ldy, const float *__restrict__ u, int64_t N, int64_t M) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * M) return;
    const int64_t m = i / N, n = i % N;
    const float g = y[m * ldy + n];
    y[m * ldy + n] = (g / (1.0f + expf(-g))) * u[i];
}

// kcpp_gemm_rms_norm / kcpp_gemm_q6p_rms_norm: the residual GEMM's split-K reduce also forms the next rms_norm's
// Q8_K activation (ops.hip k_rms_norm with partials; bit for bit the reduce followed by kcpp_rms_norm)
struct NormHook { const float *w; void *qout; float eps; bool used; };

static int splitk_finish(const GemmPlan &p, const GemmArgs &a, NormHook *hook) {
    if (hook && !hook->used && a.ldy == a.N &&
        kcpp_reduce_rms_norm(a.part, p.ks, a.Mp, a.res, a.ldr, a.Y, a.ldy, hook->w, hook->qout, a.N, a.M, hook->eps, a.s) == 0) {
        hook->used = true;
        return 0;
    }
    hipLaunchKernelGGL(k_splitk_reduce, dim3((unsigned)((a.M * a.N + 255) / 256)), dim3(256), 0, a.s, a.part, p.ks, a.M, a.Mp,
                       a.N, a.Y, a.ldy, a.res, a.ldr);
    KCPP_CHECK(hipGetLastError());
    return 0;
}

// ================================================================ the runner
static int gemm_launch(const GemmPlan &p, const GemmArgs &a) {
    switch (p.family) {
    case GEMM_V1: return gemm_v1_launch(p, a);
    case GEMM_V2: return gemm_kq_launch(p, a);
    case GEMM_Q4V3: return gemm_q4v3_launch(p, a);
    case GEMM_Q6V3: return gemm_q6v3_launch(p, a);
    case GEMM_V4: return gemm_q4v4_launch(p, a);
    case GEMM_Q6P: return gemm_q6p_launch(p, a);
    default: return -3;
    }
}

// a: the operation (W, Y, res; mode 1: up_W / up_Wd the up matrix, `up` [M][N] scratch for its product).  Activation
// image -> launch -> split-K finish (folding hook's rms_norm into the reduce when it can), and for GLU the up matrix
// the same way (V4: inside the first launch) and Y = silu(Y) * up.
static int gemm_run(const GemmPlan &p, GemmArgs a, int mode, const void *up_W, const void *up_Wd, float *up, NormHook *hook) {
    int rc = gemm_act_image(p.family, a.act, vec_dot_type(a.type), a.K, a.M, a.Mp, a.af, a.dy, a.bsf,
                            nullptr, 0, a.s);
    if (rc) return rc;
    const bool one_launch = p.family == GEMM_V4;
    float *const Y = a.Y;
    const int64_t ldy = a.ldy;
    if (mode == 1) a.res = nullptr;
    a.W2 = mode == 1 && one_launch ? up_W : nullptr;
    a.Y2 = up;
    a.ldy2 = a.N;
    const auto launch = [&]() -> int {
        const int r = gemm_launch(p, a);
        return r || p.ks == 1 ? r : splitk_finish(p, a, hook);
    };
    if ((rc = launch()) || mode != 1) return rc;
    if (!one_launch) {
        a.W = up_W;
        a.Wd = up_Wd;
        a.Y = up;
        a.ldy = a.N;
        a.ldr = 0;
        if ((rc = launch())) return rc;
    }
    hipLaunchKernelGGL(k_silu_mul_strided, dim3((unsigned)((a.N * a.M + 255) / 256)), dim3(256), 0, a.s, Y, ldy, up, a.N, a.M);
    KCPP_CHECK(hipGetLastError());
    return 0;
}

// workspace: activation image (a16, dy, bs16), the GLU up product [M][N], then the split-K partials
struct GemmWs { int64_t a16, dy, bs, up, part, bytes; };
static GemmWs ws_layout(int type, int64_t K, int64_t N, int64_t M) {
    const int64_t Mp = (M + GB_M - 1) / GB_M * GB_M;
    const int64_t G = (type == KT_Q4_0 || type == KT_Q5_0 || type == KT_Q8_0 || type == KT_Q4_1 || type == KT_Q5_1 ||
                       type == KT_IQ4_NL) ? 32 : 256;
    const auto al = [](int64_t b) { return (b + 255) & ~255LL; };
    GemmWs w;
    int64_t off = 0;
    w.a16 = off; off += al(Mp * K * 2);
    w.dy = off; off += al(Mp * (K / G) * 4);
    w.bs = off; off += al(Mp * (K / 16) * 2);
    w.up = off; off += al(M * N * 4);
    w.part = off;
    if (type == KT_Q8_0) off += 2 * (int64_t)gemm_ks_q80s(K, N) * 32 * N * 4;   // small-M split-K partials (g, u)
    off += (int64_t)gemm_ks_max(type, K, N) * Mp * N * 4;
    w.bytes = off;
    return w;
}

static int g_gemm_variant = 0;

static int gemm_impl(int type, const void *W, const void *W2, int64_t K, int64_t N, const void *act, int64_t M, float *Y,
                     int64_t ldy, const float *res, int64_t ldr, int mode, void *ws, void *stream, NormHook *hook) {
    if (type == KT_Q8_0_T) {          // the tile layout (gemm_q80t.hip): every M, activation KT_Q8_0_TA
        const void *Ws[1] = {W};
        const int64_t Ns[1] = {N};
        return kcpp_gemm_q80t(Ws, Ns, 1, W2, K, act, M, Y, ldy, res, ldr, mode, nullptr, ws, stream);
    }
    hipStream_t s = (hipStream_t)stream;
    if (K % GB_K) return -1;
    if (!ws) return -2;
    const GemmWs o = ws_layout(type, K, N, M);
    uint8_t *w8 = (uint8_t *)ws;
    const bool bs_aligned = ((uintptr_t)((const uint8_t *)act + M * K + M * (K / 256) * 4) & 15) == 0;
    const GemmPlan p = gemm_plan(type, K, N, M, mode, bs_aligned, gemm_force_of(g_gemm_variant));
    if (p.family == GEMM_COLS) {
        for (int64_t c0 = 0; c0 < M; c0 += p.tile) {
            const int rc = gemv_cols(type, W, W2, K, N, act, std::min<int64_t>(p.tile, M - c0), M, c0, Y, ldy, res, ldr, mode,
                                     stream);
            if (rc) return rc;
        }
        return 0;
    }
    if (p.family == GEMM_Q80S)
        return gemm_q80s_run({{(const uint8_t *)W, nullptr, nullptr}, {N, 0, 0}, 1}, W2, K, N, act, M, Y, ldy, res, ldr, mode,
                             nullptr, (float *)(w8 + o.part), s);
    const int vt = vec_dot_type(type);
    GemmArgs a = {};
    a.type = type;
    a.W = W; a.Y = Y; a.ldy = ldy; a.res = res; a.ldr = ldr;
    a.K = K; a.N = N; a.M = M; a.Mp = (M + GB_M - 1) / GB_M * GB_M;
    a.act = act;
    a.af = w8 + o.a16; a.dy = (float *)(w8 + o.dy); a.bsf = w8 + o.bs;
    a.s81 = vt == KT_Q8_1 ? act_view(vt, act, K, M, 0).s : nullptr;      // block_q8_1.s [M][K/32]
    a.part = (float *)(w8 + o.part);
    a.s = s;
    return gemm_run(p, a, mode, W2, nullptr, (float *)(w8 + o.up), hook);
}

extern "C" {

int kcpp_gemm_set_variant(int v) {
    const int old = g_gemm_variant;
    g_gemm_variant = v < 0 ? 0 : v;
    return old;
}

// the plan kcpp_gemm would run under the current variant (host-only; launches nothing):
// out = {family, layout, tile, waves, KS, XG, PF, workgroups} (gemm_plan.h GemmPlan)
int kcpp_gemm_plan(int type, int64_t K, int64_t N, int64_t M, int mode, int bs_aligned, int32_t out[8]) {
    if (!out || K <= 0 || N <= 0 || M <= 0 || K % GB_K || mode < 0 || mode > 1) return -1;
    if (type == KT_Q8_0_T || ks_block_bytes(type) == 0 || type == KT_F32 || type == KT_F16) return -3;
    const GemmPlan p = gemm_plan(type, K, N, M, mode, bs_aligned != 0, gemm_force_of(g_gemm_variant));
    const int32_t v[8] = {p.family, p.rs, p.tile, p.waves, p.ks, p.xg, p.pf, (int32_t)p.nwg};
    std::copy(v, v + 8, out);
    return 0;
}

int kcpp_gemm(int type, const void *W, const void *W2, int64_t K, int64_t N, const void *act, int64_t M, float *Y,
              int64_t ldy, const float *res, int64_t ldr, int mode, void *ws, void *stream) {
    return gemm_impl(type, W, W2, K, N, act, M, Y, ldy, res, ldr, mode, ws, stream, nullptr);
}

// q|k|v style: nseg <= 3 Q8_0 weights [K][N_i] whose outputs sit back to back in Y's columns, M <= 32,
// every N_i a multiple of 128; ws from kcpp_gemm_workspace_bytes(KT_Q8_0, K, sum N_i, M)
int kcpp_gemm_q80_segs(const void *const *W, const int64_t *N, int nseg, int64_t K, const void *act, int64_t M, float *Y,
                       int64_t ldy, void *ws, void *stream) {
    if (nseg < 1 || nseg > 3 || M < 1 || M > 32 || K % 32 || !ws) return -1;
    Q80Segs sg = {{nullptr, nullptr, nullptr}, {0, 0, 0}, nseg};
    int64_t Ntot = 0;
    for (int i = 0; i < nseg; ++i) {
        if (N[i] <= 0 || (N[i] % 128 && i + 1 < nseg)) return -1;
        sg.W[i] = (const uint8_t *)W[i];
        sg.N[i] = N[i];
        Ntot += N[i];
    }
    float *part = (float *)((uint8_t *)ws + ws_layout(KT_Q8_0, K, Ntot, M).part);
    return gemm_q80s_run(sg, nullptr, K, Ntot, act, M, Y, ldy, nullptr, 0, 0, nullptr, part, (hipStream_t)stream);
}

int kcpp_gemm_q80_glu_q80(const void *W, const void *W2, int64_t K, int64_t N, const void *act, int64_t M, void *qout,
                          void *ws, void *stream) {
    if (M < 1 || M > 32 || K % 32 || N % 32 || !ws || !qout) return -1;
    float *part = (float *)((uint8_t *)ws + ws_layout(KT_Q8_0, K, N, M).part);
    return gemm_q80s_run({{(const uint8_t *)W, nullptr, nullptr}, {N, 0, 0}, 1}, W2, K, N, act, M, nullptr, 0, nullptr, 0, 1,
                         (uint8_t *)qout, part, (hipStream_t)stream);
}

// Q6_K prefill image (k_q6p_build / k_gemm_q6p): N % 128 == 0, K % 256 == 0
int64_t kcpp_q6p_image_bytes(int64_t K, int64_t N) {
    if (K <= 0 || N <= 0 || K % 256 || N % 128) return 0;
    return N * K * 2;
}

int kcpp_q6p_build(const void *W, int64_t K, int64_t N, void *img, void *stream) {
    if (!W || !img || !kcpp_q6p_image_bytes(K, N)) return -1;
    return gemm_q6p_build(W, K, N, img, (hipStream_t)stream);
}

}  // extern "C"

// kcpp_gemm(KT_Q6_K_RS, ...) with the prefill image(s) beside the RS weights: the same results bit for bit (same
// K split rule, same epilogue order), int8 matrix cores.  M > 32; mode 0 (res optional) or 1 (silu(g) * u, W2 / img2);
// ws from kcpp_gemm_workspace_bytes(KT_Q6_K_RS, K, N, M).  Returns -3 for shapes the image does not cover.
static int gemm_q6p_impl(const void *img, const void *W, const void *img2, const void *W2, int64_t K, int64_t N,
                         const void *act, int64_t M, float *Y, int64_t ldy, const float *res, int64_t ldr, int mode, void *ws,
                         void *stream, NormHook *hook) {
    if (!img || !W || !act || !Y || !ws || M < 1 || (mode == 1 && (!img2 || !W2)) || mode < 0 || mode > 1) return -1;
    if (!kcpp_q6p_image_bytes(K, N)) return -3;
    const GemmWs o = ws_layout(KT_Q6_K_RS, K, N, M);
    static const int NWq = [] { const char *e = getenv("KCPP_Q6P_NW"); return e && atoi(e) == 4 ? 4 : 8; }();
    GemmArgs a = {};
    a.type = KT_Q6_K_RS;
    a.W = img; a.Wd = W; a.Y = Y; a.ldy = ldy; a.res = res; a.ldr = ldr;
    a.K = K; a.N = N; a.M = M; a.Mp = (M + 127) / 128 * 128;
    a.act = act;
    a.part = (float *)((uint8_t *)ws + o.part);
    a.s = (hipStream_t)stream;
    return gemm_run(gemm_plan_q6p(K, N, M, mode, NWq), a, mode, img2, W2, (float *)((uint8_t *)ws + o.up), hook);
}

// the GEMM (mode 0) followed by kcpp_rms_norm(Y, ldy, norm_w, -> q8k_out): when the GEMM splits K, its reduce forms the
// norm's Q8_K activation in the same launch (h.used); the results are those of the two calls bit for bit
static int norm_after(int rc, const NormHook &h, float *Y, int64_t ldy, int64_t N, int64_t M, void *stream) {
    if (rc || h.used) return rc;
    return kcpp_rms_norm(Y, ldy, h.w, nullptr, 0, h.qout, N, M, h.eps, stream);
}

extern "C" {

int kcpp_gemm_q6p(const void *img, const void *W, const void *img2, const void *W2, int64_t K, int64_t N, const void *act,
                  int64_t M, float *Y, int64_t ldy, const float *res, int64_t ldr, int mode, void *ws, void *stream) {
    return gemm_q6p_impl(img, W, img2, W2, K, N, act, M, Y, ldy, res, ldr, mode, ws, stream, nullptr);
}

int kcpp_gemm_rms_norm(int type, const void *W, int64_t K, int64_t N, const void *act, int64_t M, float *Y, int64_t ldy,
                       const float *res, int64_t ldr, void *ws, void *stream, const float *norm_w, float eps, void *q8k_out) {
    if (!norm_w || !q8k_out) return -1;
    NormHook h{norm_w, q8k_out, eps, false};
    const int rc = gemm_impl(type, W, nullptr, K, N, act, M, Y, ldy, res, ldr, 0, ws, stream, &h);
    return norm_after(rc, h, Y, ldy, N, M, stream);
}

int kcpp_gemm_q6p_rms_norm(const void *img, const void *W, int64_t K, int64_t N, const void *act, int64_t M, float *Y,
                           int64_t ldy, const float *res, int64_t ldr, void *ws, void *stream, const float *norm_w, float eps,
                           void *q8k_out) {
    if (!norm_w || !q8k_out) return -1;
    NormHook h{norm_w, q8k_out, eps, false};
    const int rc = gemm_q6p_impl(img, W, nullptr, nullptr, K, N, act, M, Y, ldy, res, ldr, 0, ws, stream, &h);
    return norm_after(rc, h, Y, ldy, N, M, stream);
}

int64_t kcpp_gemm_workspace_bytes(int type, int64_t K, int64_t N, int64_t M) {
    if (type == KT_Q8_0_T) return kcpp_q80t_ws_bytes(K, N, M);
    return ws_layout(type, K, N, M).bytes;
}

// grouped expert GEMM (MoE prefill): ng groups of cnt_host[e] token rows (act: Q8_K of all M = sum rows, grouped
// back to back), group e against W + e wstride (and W2 + e wstride); mode 0: Y = X W^T, mode 1: Y = silu(X W^T) *
// (X W2^T) with up [M][N] as scratch.  cnt_dev: the same counts on the device (read by the kernel); Q4_K / Q5_K
// (+ RS), and Q6_K_RS in plain mode; K a multiple of 256.  One launch per mode (+ the GLU product); every row's
// arithmetic is the unsplit kernel's (bitwise the single-expert kcpp_gemm result wherever that runs unsplit)
int64_t kcpp_gemm_grouped_ws_bytes(int type, int64_t K, int64_t M, int ng) {
    if (type != KT_Q6_K_RS) return 0;
    const int64_t Pv = M + 128LL * ng;                  // >= the padded virtual rows
    return ((Pv * K * 2 + 255) & ~255LL) + Pv * (K / 256) * 4;
}

int kcpp_gemm_grouped(int type, const void *W, const void *W2, int64_t wstride, int64_t K, int64_t N, const void *act,
                      int64_t M, const int32_t *cnt_host, const int32_t *cnt_dev, int ng, float *Y, float *up, int mode,
                      void *ws, void *stream) {
    if (type != KT_Q4_K && type != KT_Q4_K_RS && type != KT_Q5_K && type != KT_Q5_K_RS && type != KT_Q6_K_RS) return -1;
    if (K % 256 || ng < 1 || ng > 64 || !cnt_dev || !cnt_host || (mode == 1 && (!W2 || !up)) || mode < 0 || mode > 1)
        return -1;
    const bool q6 = type == KT_Q6_K_RS;
    if (q6 && (mode != 0 || !ws)) return -1;            // plain mode only
    if (!q6 && ((uintptr_t)((const uint8_t *)act + M * K + M * (K / 256) * 4) & 15) != 0) return -3;
    // Pv: the 128-row-padded virtual rows of all groups; tiles: their 128 x 128 tiles
    int64_t Pv = 0, rows = 0;
    for (int e = 0; e < ng; ++e) {
        if (cnt_host[e] < 0) return -1;
        Pv += (cnt_host[e] + 127) / 128 * 128;
        rows += cnt_host[e];
    }
    if (rows != M) return -1;
    if (!Pv) return 0;
    const int64_t tiles = Pv / 128 * ((N + 127) / 128);
    const GemmForce f = gemm_force_of(g_gemm_variant);
    GemmArgs a = {};
    a.type = type;
    a.W = W; a.Y = Y; a.ldy = N;
    a.K = K; a.N = N;
    a.act = act;
    a.gcnt = cnt_dev; a.gne = ng; a.wstride = wstride;
    a.s = (hipStream_t)stream;
    GemmPlan p = {};
    p.rs = type != ks_base_type(type);
    p.ks = p.xg = p.pf = 1;
    if (q6) {
        // k_gemm_q6v3 over the virtual layout (the f16 fragment image of every group, padding rows zero); tile shape
        // (never changes a bit): 128 x 128, 8 waves, unless a variant forces q6v3's
        p.family = GEMM_Q6V3;
        p.tile = f.q6v3_bmt ? f.q6v3_bmt : 4;
        p.waves = f.q6v3_waves ? f.q6v3_waves : 8;
        p.mt = (int)(Pv / (32 * p.tile));
        p.nwg = p.mt * ((N + 127) / 128);
        a.M = a.Mp = Pv;
        a.af = ws;
        a.dy = (float *)((uint8_t *)ws + ((Pv * K * 2 + 255) & ~255LL));
        const int rc = gemm_act_image(GEMM_Q6V3, act, KT_Q8_K, K, M, Pv, a.af, a.dy, nullptr, cnt_dev, ng, a.s);
        return rc ? rc : gemm_q6v3_launch(p, a);
    }
    // v4 (TPW 2), gate and up in one launch
    p.family = GEMM_V4;
    p.tile = 2;
    p.waves = 8;
    p.mt = 1;
    p.nwg = tiles * (mode == 1 ? 2 : 1);
    a.M = a.Mp = M;
    return gemm_run(p, a, mode, W2, nullptr, up, nullptr);
}

}  // extern "C"
