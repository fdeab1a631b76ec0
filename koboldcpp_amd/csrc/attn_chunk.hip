// attn_chunk.hip -- the 64-key-chunk decode attention at D = 128 (FA_DEC_CHUNK of fa_plan.h):
//   k_fa_decode  grid (chunks of 64 keys, kv-head, query) -> partial (O, m, l)
//   k_fa_combine one 1024-thread block per (query, head pair) -> f32 out (+ Q8_K quant)
// Reached by kcpp_flash_attn (2..16 queries; force_path 6; one query with qout at G = 1), kcpp_fa_decode_ex variant 0
// and, under the ggml op's explicit mask and soft-cap, kcpp_flash_attn_ext_sc up to 16 queries.
#include "attn_common.h"
#include "gemv_units.h"

// K/V cache layout: [pos][HKV][D] f16, row stride EKV = HKV*D elements.
// Query layout: q16 [T][H][D] f16.  Query t sits at absolute position n_past + t.
// One workgroup = (64-key chunk, kv head, query); its G = H/HKV query heads share every K/V row
// (GQA).  Scores: 16 lanes x 16 B per K row; P.V: lane owns two dims and reads one dword of each V
// row (no cross-lane reduction).  Partials (O, m, l) per chunk, merged by k_fa_combine (the role of the
// reference's flash_attn_combine_results, ggml/src/ggml-cuda/fattn-common.cuh:523).  Used for 2..16
// queries (single-token decode runs k_fa_dec5, attn_dec.hip) and by the ggml-op form.
// CAP (graph form only): scale = the op's scale / cap and the score is cap * tanhf(dot * scale) before the mask
template <int D, int G, bool CAP = false>
__global__ void __launch_bounds__(256) k_fa_decode(const uint16_t *__restrict__ q16, const uint16_t *__restrict__ kc,
                                                   const uint16_t *__restrict__ vc, float *__restrict__ part_o,
                                                   float2 *__restrict__ part_ml, int T, int H,
                                                   int HKV, int n_past_arg, const int32_t *__restrict__ n_past_dev,
                                                   int n_chunks, float scale, const uint16_t *__restrict__ mask,
                                                   int64_t mask_ld, int64_t kv_ld, int64_t kv_hs, float cap = 0.0f) {
    static_assert(D == 128, "head dim 128");
    const int c = blockIdx.x, hk = blockIdx.y, t = blockIdx.z;
    const int n_past = n_past_dev ? n_past_dev[0] : n_past_arg;
    // implicit causal window [0, n_past + t] (mask_ld < 0), or the ggml op's explicit form: all n_kv
    // (= n_past_arg) keys under the mask (none if mask is null)
    const int kend = mask_ld >= 0 ? n_past_arg : n_past + t + 1;   // exclusive
    if (c * FA_CHUNK >= kend) return;                    // chunk unused by this query (graph-static grid)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p0 = c * FA_CHUNK;
    const int p1 = min(p0 + FA_CHUNK, kend);              // exclusive
    const uint16_t *mrow = mask ? mask + (int64_t)t * mask_ld : nullptr;
    __shared__ float s_sc[G][FA_CHUNK];
    __shared__ float s_red[4][G][D];
    __shared__ float s_m[G], s_l[G];

    const int sub = lane & 15, kq = lane >> 4;
    float qv[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const uint4 qq = *(const uint4 *)(q16 + ((int64_t)t * H + hk * G + g) * D + sub * 8);
        const uint32_t w4[4] = {qq.x, qq.y, qq.z, qq.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) { qv[g][2 * i] = h2f(w4[i] & 0xFFFF); qv[g][2 * i + 1] = h2f(w4[i] >> 16); }
    }
    constexpr int KPW = FA_CHUNK / 4;                    // keys per wave
    uint4 kk[KPW / 4];
#pragma unroll
    for (int i = 0; i < KPW / 4; ++i) {
        const int p = p0 + KPW * wave + 4 * i + kq;
        kk[i] = p < p1 ? *(const uint4 *)(kc + (int64_t)p * kv_ld + hk * kv_hs + sub * 8) : make_uint4(0, 0, 0, 0);
    }
    uint32_t vv[KPW];
#pragma unroll
    for (int i = 0; i < KPW; ++i) {
        const int p = p0 + KPW * wave + i;
        // masked keys are skipped like the CPU does (their V never enters the sum, even if not finite)
        const bool use = p < p1 && !(mrow && mrow[p] == 0xFC00);
        vv[i] = use ? *(const uint32_t *)(vc + (int64_t)p * kv_ld + hk * kv_hs + 2 * lane) : 0u;
    }
#pragma unroll
    for (int i = 0; i < KPW / 4; ++i) {
        const int p = p0 + KPW * wave + 4 * i + kq;
        const uint32_t w4[4] = {kk[i].x, kk[i].y, kk[i].z, kk[i].w};
        float kf[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) { kf[2 * e] = h2f(w4[e] & 0xFFFF); kf[2 * e + 1] = h2f(w4[e] >> 16); }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            float sc = 0.0f;
#pragma unroll
            for (int e = 0; e < 8; ++e) sc = fmaf(qv[g][e], kf[e], sc);
            sc += dpp_f<0xB1>(sc); sc += dpp_f<0x4E>(sc); sc += dpp_f<0x141>(sc); sc += dpp_f<0x140>(sc);
            if (sub == 0) {
                float sv = -INFINITY;
                if constexpr (CAP) {
                    const float cs = cap * tanhf(sc * scale);
                    if (p < p1) sv = mrow ? (mrow[p] == 0xFC00 ? -INFINITY : cs + h2f(mrow[p])) : cs;
                } else if (p < p1) sv = mrow ? (mrow[p] == 0xFC00 ? -INFINITY : sc * scale + h2f(mrow[p])) : sc * scale;
                s_sc[g][p - p0] = sv;
            }
        }
    }
    __syncthreads();
    // softmax statistics of the chunk, one wave per head (lanes cover FA_CHUNK keys)
    for (int g = wave; g < G; g += 4) {
        float m = -INFINITY;
        for (int i = lane; i < FA_CHUNK; i += 64) m = fmaxf(m, s_sc[g][i]);
        m = wave_max_dpp(m);
        float l = 0.0f;
        for (int i = lane; i < FA_CHUNK; i += 64) {
            const float sv = s_sc[g][i];
            const float e = (sv == -INFINITY) ? 0.0f : expf(sv - m);
            s_sc[g][i] = e;
            l += e;
        }
        l = wave_sum_f(l);
        if (lane == 0) { s_m[g] = m; s_l[g] = l; }
    }
    __syncthreads();
    float acc[G][2];
#pragma unroll
    for (int g = 0; g < G; ++g) acc[g][0] = acc[g][1] = 0.0f;
#pragma unroll
    for (int i = 0; i < KPW; ++i) {
        const float v0 = h2f(vv[i] & 0xFFFF), v1 = h2f(vv[i] >> 16);
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float pr = s_sc[g][KPW * wave + i];
            acc[g][0] = fmaf(pr, v0, acc[g][0]);
            acc[g][1] = fmaf(pr, v1, acc[g][1]);
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) { s_red[wave][g][2 * lane] = acc[g][0]; s_red[wave][g][2 * lane + 1] = acc[g][1]; }
    __syncthreads();
    for (int i = threadIdx.x; i < G * D; i += 256) {
        const int g = i / D, d = i % D;
        const float o = s_red[0][g][d] + s_red[1][g][d] + s_red[2][g][d] + s_red[3][g][d];
        part_o[(((int64_t)t * H + hk * G + g) * n_chunks + c) * D + d] = o;
    }
    if (threadIdx.x < G) part_ml[((int64_t)t * H + hk * G + threadIdx.x) * n_chunks + c] = make_float2(s_m[threadIdx.x], s_l[threadIdx.x]);
}

// combine split-KV partials; one 1024-thread workgroup covers two heads (= one Q8_K block of 256).
// Latency-bound (a few hundred KB from L2), so it is built for memory-level parallelism: every
// thread issues its 16 partial-O loads (4 threads per output dim split the chunks) together with
// the chunk (m, l) loads, then the chunk weights exp(m_c - M) are formed in LDS and applied.
template <bool QUANT>
__global__ void __launch_bounds__(1024) k_fa_combine(const float *__restrict__ part_o, const float2 *__restrict__ part_ml,
                                                     float *__restrict__ out, uint8_t *__restrict__ qout, int T, int H,
                                                     int D, int n_past_arg, const int32_t *__restrict__ n_past_dev,
                                                     int n_chunks_alloc, int masked) {
    constexpr int MAXCH = FA_MAX_CHUNKS;               // 128k context
    const int t = blockIdx.y;
    const int pair = blockIdx.x;                       // heads 2*pair, 2*pair+1
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hl = tid >> 9, r = tid & 511, d = r & 127, cg = r >> 7;
    const int h = 2 * pair + hl;
    const int n_past = n_past_dev ? n_past_dev[0] : n_past_arg;
    const int nch = masked ? (n_past_arg - 1) / FA_CHUNK + 1    // explicit mask: all n_kv keys
                           : (n_past + t) / FA_CHUNK + 1;     // chunks this query actually used
    __shared__ float s_w[2][MAXCH];
    __shared__ float s_red[16];
    __shared__ float s_sum[2][4][128];
    const float2 *ml = part_ml + ((int64_t)t * H + h) * n_chunks_alloc;
    const float *po = part_o + ((int64_t)t * H + h) * n_chunks_alloc * 128 + d;
    // (m, l) of chunk r (r < nch), and this thread's first 16 O partials, all in flight together
    const float2 mlv = r < nch ? ml[r] : make_float2(-INFINITY, 0.0f);
    float ov[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int c = cg + 4 * k;
        ov[k] = c < nch ? po[(int64_t)c * 128] : 0.0f;
    }
    // M = max_c m_c per head: waves 0-7 hold head 0's chunks, 8-15 head 1's (chunks beyond 512: strided)
    float mloc = mlv.x;
    for (int c = r + 512; c < nch; c += 512) mloc = fmaxf(mloc, ml[c].x);
    float M = wave_max(mloc);
    if (lane == 0) s_red[wave] = M;
    __syncthreads();
    M = s_red[8 * hl];
#pragma unroll
    for (int w = 1; w < 8; ++w) M = fmaxf(M, s_red[8 * hl + w]);
    const float wgt = mlv.x == -INFINITY ? 0.0f : expf(mlv.x - M);
    if (r < MAXCH) s_w[hl][r] = wgt;
    float lsum = wgt * mlv.y;
    for (int c = r + 512; c < nch; c += 512) {
        const float2 v = ml[c];
        const float w2 = v.x == -INFINITY ? 0.0f : expf(v.x - M);
        s_w[hl][c] = w2;
        lsum = fmaf(w2, v.y, lsum);
    }
    float L = wave_sum(lsum);
    __syncthreads();                                   // s_red reuse + s_w visible
    if (lane == 0) s_red[wave] = L;
    __syncthreads();
    L = 0.0f;
#pragma unroll
    for (int w = 0; w < 8; ++w) L += s_red[8 * hl + w];
    float O = 0.0f;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int c = cg + 4 * k;
        if (c < nch) O = fmaf(s_w[hl][c], ov[k], O);
    }
    for (int c0 = 64; c0 < nch; c0 += 64) {            // contexts beyond 64 chunks
#pragma unroll 4
        for (int k = 0; k < 16; ++k) {
            const int c = c0 + cg + 4 * k;
            if (c < nch) O = fmaf(s_w[hl][c], po[(int64_t)c * 128], O);
        }
    }
    s_sum[hl][cg][d] = O;
    __syncthreads();
    if (cg == 0) {
        const float res = ((s_sum[hl][0][d] + s_sum[hl][1][d]) + (s_sum[hl][2][d] + s_sum[hl][3][d])) / L;
        const int64_t e = (int64_t)t * H * 128 + (int64_t)h * 128 + d;
        if (out) out[e] = res;
        s_sum[hl][0][d] = res;
    }
    if constexpr (QUANT) {
        __syncthreads();
        if (tid < 16) {                                // lane j holds elements 16j..16j+15 of the block
            float v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const int e = 16 * tid + k;
                v[k] = s_sum[e >> 7][0][e & 127];
            }
            const int64_t E = (int64_t)H * 128;
            const int64_t nsb = E / 256;
            int8_t *qs = (int8_t *)qout + (int64_t)t * E + pair * 256;
            float *dp = (float *)(qout + (int64_t)T * E) + (int64_t)t * nsb + pair;
            int16_t *bs = (int16_t *)(qout + (int64_t)T * E + (int64_t)T * nsb * 4) + (int64_t)t * (E / 16) + pair * 16;
            q8k_quant16(v, tid, qs, dp, bs);
        }
    }
}

// explicit mask (a.mask_ld >= 0): a.n_past = n_kv, every key under the mask; a.cap != 0: the CAP kernel at scale / cap
int fa_chunk_launch(const FaDecodePlan &p, const FaArgs &a) {
    float *po = (float *)((uint8_t *)a.ws + p.part_o);
    float2 *pml = (float2 *)((uint8_t *)a.ws + p.part_ml);
    const dim3 grid(p.grid[0], p.grid[1], p.grid[2]), cgrid(p.cgrid[0], p.cgrid[1]);
    const int masked = a.mask_ld >= 0;
    const int rc = fa_for_g<1, 2, 3, 4, 5, 6, 7, 8>(a.H / a.HKV, [&](auto g) {
        constexpr int G = decltype(g)::value;
        if (a.cap != 0.0f)
            hipLaunchKernelGGL((k_fa_decode<128, G, true>), grid, dim3(64 * p.waves), 0, a.s, a.q16, a.kc, a.vc, po, pml,
                               a.T, a.H, a.HKV, a.n_past, a.n_past_dev, p.nch, a.scale / a.cap, a.mask, a.mask_ld, a.kv_ld,
                               a.kv_hs, a.cap);
        else
            hipLaunchKernelGGL((k_fa_decode<128, G>), grid, dim3(64 * p.waves), 0, a.s, a.q16, a.kc, a.vc, po, pml, a.T,
                               a.H, a.HKV, a.n_past, a.n_past_dev, p.nch, a.scale, a.mask, a.mask_ld, a.kv_ld, a.kv_hs);
    });
    if (rc) return rc;
    KCPP_CHECK(hipGetLastError());
    if (p.cquant)
        hipLaunchKernelGGL(k_fa_combine<true>, cgrid, dim3(p.cthreads), 0, a.s, po, pml, a.out, (uint8_t *)a.qout, a.T,
                           a.H, a.D, a.n_past, a.n_past_dev, p.nch, masked);
    else
        hipLaunchKernelGGL(k_fa_combine<false>, cgrid, dim3(p.cthreads), 0, a.s, po, pml, a.out, (uint8_t *)nullptr, a.T,
                           a.H, a.D, a.n_past, a.n_past_dev, p.nch, masked);
    KCPP_CHECK(hipGetLastError());
    return 0;
}
