// attn_tile.hip -- the FMA-tiled flash attention, D = 64 or 128 (FA_DEC_TILE of fa_plan.h): k_fa_prefill, 64 queries x
// 64 keys per step, online softmax.  Reached by kcpp_flash_attn (D = 64 at every T; D = 128 prefill at force_path 2 and
// where fa_plan.h's table keeps a GQA ratio from the matrix-core kernel of attn_mfma.hip) and, under the ggml op's
// explicit mask and soft-cap, by kcpp_flash_attn_ext_sc (D = 64 at every T; D = 128 past 16 queries).
#include "attn_common.h"

// ---------------------------------------------------------------- prefill (tiled, online softmax)
// grid (ceil(T/64), H), block 256.  Thread (ty = tid/16, tx = tid%16): query rows 4*ty..4*ty+3,
// S columns tx + 16*j (j<4) and O dims tx*8 .. tx*8+7 (8 dims).
#define FP_BQ 64
#define FP_BK 64
// D = 128 or 64 (TinyLlama-class heads): thread tx owns DPT = D / 16 output dims; n_past from n_past_dev when given
// (single-token decode replayed from a graph)
// CAP (explicit mask form only): scale = the op's scale / cap, the score cap * tanhf(dot * scale) before the mask
template <int D, bool CAP = false>
__global__ void __launch_bounds__(256) k_fa_prefill(const uint16_t *__restrict__ q16, const uint16_t *__restrict__ kc,
                                                    const uint16_t *__restrict__ vc, float *__restrict__ out, int T,
                                                    int H, int HKV, int n_past_arg, float scale,
                                                    const uint16_t *__restrict__ mask, int64_t mask_ld, int n_kv,
                                                    const int32_t *__restrict__ n_past_dev, float cap = 0.0f) {
    constexpr int DPT = D / 16;
    const int n_past = n_past_dev ? n_past_dev[0] : n_past_arg;
    const int qt = blockIdx.x, h = blockIdx.y;
    const int G = H / HKV, hk = h / G;
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int64_t EKV = (int64_t)HKV * D;
    __shared__ float sQ[FP_BQ][D + 1];
    __shared__ float sK[FP_BK][D + 1];
    __shared__ float sV[FP_BK][D];
    const int q0 = qt * FP_BQ;
    for (int i = tid; i < FP_BQ * D; i += 256) {
        const int r = i / D, d = i % D;
        sQ[r][d] = (q0 + r < T) ? h2f(q16[((int64_t)(q0 + r) * H + h) * D + d]) : 0.0f;
    }
    float m[4], l[4], o[4][DPT];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        m[r] = -INFINITY; l[r] = 0.0f;
#pragma unroll
        for (int j = 0; j < DPT; ++j) o[r][j] = 0.0f;
    }
    const int last_q = min(q0 + FP_BQ, T) - 1;
    const bool expl = mask_ld >= 0;                       // explicit ggml mask form (mask may be null)
    const int kend = expl ? n_kv : n_past + last_q + 1;   // keys needed by this tile (exclusive)
    __shared__ int s_dead[FP_BK];
    for (int k0 = 0; k0 < kend; k0 += FP_BK) {
        __syncthreads();
        if (expl && mask && tid < FP_BK) {               // keys masked for every query of the tile are skipped
            int dead = 1;                                // (their V may be anything, as on the CPU)
            const int p = k0 + tid;
            for (int qi = q0; qi <= last_q && dead && p < kend; ++qi) dead = mask[(int64_t)qi * mask_ld + p] == 0xFC00;
            s_dead[tid] = dead;
        }
        __syncthreads();
        for (int i = tid; i < FP_BK * D / 2; i += 256) {
            const int r = i / (D / 2), d2 = i % (D / 2);
            const int p = k0 + r;
            uint32_t kk = 0, vv = 0;
            if (p < kend) {
                kk = *(const uint32_t *)(kc + (int64_t)p * EKV + hk * D + 2 * d2);
                if (!(expl && mask && s_dead[r])) vv = *(const uint32_t *)(vc + (int64_t)p * EKV + hk * D + 2 * d2);
            }
            sK[r][2 * d2] = h2f(kk & 0xFFFF); sK[r][2 * d2 + 1] = h2f(kk >> 16);
            sV[r][2 * d2] = h2f(vv & 0xFFFF); sV[r][2 * d2 + 1] = h2f(vv >> 16);
        }
        __syncthreads();
        float s[4][4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) s[r][j] = 0.0f;
        for (int d = 0; d < D; ++d) {
            float qd[4], kd[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) qd[r] = sQ[4 * ty + r][d];
#pragma unroll
            for (int j = 0; j < 4; ++j) kd[j] = sK[tx + 16 * j][d];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int j = 0; j < 4; ++j) s[r][j] = fmaf(qd[r], kd[j], s[r][j]);
        }
        // online softmax per query row; the 16 threads of a row-group (same ty) share rows
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int qi = q0 + 4 * ty + r;
            const int qpos = n_past + qi;
            float mx = -INFINITY;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int p = k0 + tx + 16 * j;
                if (expl) {
                    const uint16_t mv = (qi < T && p < kend) ? (mask ? mask[(int64_t)qi * mask_ld + p] : (uint16_t)0)
                                                             : (uint16_t)0xFC00;
                    if constexpr (CAP) s[r][j] = mv == 0xFC00 ? -INFINITY : cap * tanhf(s[r][j] * scale) + h2f(mv);
                    else s[r][j] = mv == 0xFC00 ? -INFINITY : s[r][j] * scale + h2f(mv);
                } else {
                    s[r][j] = (qi < T && p <= qpos) ? s[r][j] * scale : -INFINITY;
                }
                mx = fmaxf(mx, s[r][j]);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 1, 64)); mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
            mx = fmaxf(mx, __shfl_xor(mx, 4, 64)); mx = fmaxf(mx, __shfl_xor(mx, 8, 64));
            const float mnew = fmaxf(m[r], mx);
            const float alpha = (mnew == -INFINITY) ? 1.0f : expf(m[r] - mnew);
            float ls = 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                s[r][j] = (s[r][j] == -INFINITY) ? 0.0f : expf(s[r][j] - mnew);
                ls += s[r][j];
            }
            ls += __shfl_xor(ls, 1, 64); ls += __shfl_xor(ls, 2, 64);
            ls += __shfl_xor(ls, 4, 64); ls += __shfl_xor(ls, 8, 64);
            l[r] = l[r] * alpha + ls;
            m[r] = mnew;
#pragma unroll
            for (int j = 0; j < DPT; ++j) o[r][j] *= alpha;
        }
        // O += P V : P row r lives across the 16 tx-threads of the group (4 cols each)
        for (int src = 0; src < 16; ++src) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int kr = src + 16 * j;
                float vr[DPT];
#pragma unroll
                for (int e = 0; e < DPT; ++e) vr[e] = sV[kr][tx * DPT + e];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float pr = __shfl(s[r][j], ((16 * ty) & 63) + src, 64);
#pragma unroll
                    for (int e = 0; e < DPT; ++e) o[r][e] = fmaf(pr, vr[e], o[r][e]);
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int qi = q0 + 4 * ty + r;
        if (qi < T) {
            const float inv = 1.0f / l[r];
#pragma unroll
            for (int e = 0; e < DPT; ++e) out[((int64_t)qi * H + h) * D + tx * DPT + e] = o[r][e] * inv;
        }
    }
}

// explicit mask (a.mask_ld >= 0): the a.n_rows = n_kv keys under the mask; a.cap != 0 (D = 128): CAP at scale / cap
int fa_tile_launch(const FaDecodePlan &p, const FaArgs &a) {
    const dim3 grid(p.grid[0], p.grid[1]), block(64 * p.waves);
    const bool expl = a.mask_ld >= 0;
    const int n_past = expl ? 0 : a.n_past, n_kv = expl ? a.n_rows : 0;
    if (a.D == 64)
        hipLaunchKernelGGL(k_fa_prefill<64>, grid, block, 0, a.s, a.q16, a.kc, a.vc, a.out, a.T, a.H, a.HKV, n_past,
                           a.scale, a.mask, a.mask_ld, n_kv, a.n_past_dev);
    else if (a.cap != 0.0f)
        hipLaunchKernelGGL((k_fa_prefill<128, true>), grid, block, 0, a.s, a.q16, a.kc, a.vc, a.out, a.T, a.H, a.HKV,
                           n_past, a.scale / a.cap, a.mask, a.mask_ld, n_kv, a.n_past_dev, a.cap);
    else
        hipLaunchKernelGGL(k_fa_prefill<128>, grid, block, 0, a.s, a.q16, a.kc, a.vc, a.out, a.T, a.H, a.HKV, n_past,
                           a.scale, a.mask, a.mask_ld, n_kv, a.n_past_dev);
    KCPP_CHECK(hipGetLastError());
    return 0;
}
