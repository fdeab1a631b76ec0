// attn_d256.hip -- GGML_OP_FLASH_ATTN_EXT at head dim 256 (Gemma-2 2B / 9B), the ggml graph form only.
//
// Semantics as attn.hip's graph form (ggml_compute_forward_flash_attn_ext_f16, reference ggml/src/ggml.c:15667-15875):
// q f32 by byte strides, rounded to f16 first (q_to_vec_dot); K / V f16 cache views (key j of kv head h at
// kc + j k_ld + h k_hs elements); an f16 mask row per query (0 / -inf / any additive value, may be null); keys whose
// mask is -inf are skipped entirely -- their K / V bytes may be NaN, as on the CPU; the optional logit soft-cap
// s = cap * tanhf(q.k * scale / cap) before the mask (:15738-15740, :15804-15810); out f32 [T][H][256].
//
//   1..16 queries: k_fa256_dec + k_fa256_comb, the split-KV pair modelled on k_fa_dec5<GRAPH> + k_fa_comb4.  Grid
//       (NS splits, kv head, query).  The keys are cut into 32-key chunks, chunk c on split c % NS -- a partition of
//       the key index alone, never of the mask.  Wave w owns keys 32 c + 8 w .. + 7 of a chunk: one K row is 512 B, so
//       a lane (sub = lane & 31, kq = lane >> 5) loads 16 B = 8 dims of keys base + 2 i + kq, i < 4 -- every load
//       instruction 1 KiB contiguous per wave (two whole rows) -- and two chunks per wave are in flight.  Scores: 8-dim
//       partial dot, 32-lane reduction (DPP in rows of 16, one permlane swap); online softmax per wave in the exp2
//       domain, f32; P.V in f32, each lane its 8 dims of its own keys, the two key halves summed once at the end,
//       the four waves merged in LDS.  A split without a live key writes (m = -inf, l = 0, O = 0) and gets weight 0
//       in the combine.
//   more queries: k_fa256_mfma, 64 queries x 64 keys per step on v_mfma_f32_16x16x32_f16, the structure of
//       k_fa_prefill_mfma (attn_mfma.hip) under the explicit mask: one workgroup per (64-query tile, head), wave w
//       its queries 16 w .. + 15.  K tile [64][256] and V^T tile [256][64] f16 in LDS (33 + 36 KiB); S^T = K . Q^T
//       (8 MFMAs per 16 keys), f32 online softmax with the lane's query in its column, O^T += V^T . P^T (P rounded
//       to f16, 32 MFMAs per tile).  A key masked for every query of the tile is staged as zeros (never read); a
//       tile of 64 such keys is skipped.
#include "kcpp_common.h"
#include "kcpp_internal.h"
#include "attn_common.h" // fa_for_g; fa_plan.h fa_splits
#include "gemv_units.h"

#include <algorithm>

typedef _Float16 fd_h8 __attribute__((ext_vector_type(8)));
typedef float fd_f4 __attribute__((ext_vector_type(4)));

#define FD_D 256
#define FD_CK 32         // keys per chunk: 8 per wave, 4 waves
#define FD_MAXS 64       // splits at most (the combine's weight table)
#define FD_KP 264        // K tile row pitch (halves): 256 + 8 -> rows 528 B apart (bank spread)
#define FD_VP 72         // V^T tile row pitch (halves): 64 + 8
#define FD_L2E 1.4426950408889634f

template <int G>
struct Fd256Smem {
    float o[4][G][FD_D];
    float ml[4][G][2];
    float w[4][G], L[G];
};

// ---------------------------------------------------------------- 1..16 queries: split decode + combine
template <int G, bool CAP>
__global__ void __launch_bounds__(256) k_fa256_dec(const float *__restrict__ q, int64_t q_ts, int64_t q_hs,
                                                   const uint16_t *__restrict__ kc, const uint16_t *__restrict__ vc,
                                                   int64_t kv_ld, int64_t kv_hs, const uint16_t *__restrict__ mask,
                                                   int64_t mask_ld, float *__restrict__ part_o,
                                                   float2 *__restrict__ part_ml, int H, int n_kv, int NS, float scale,
                                                   float cap) {
    const int sp = blockIdx.x, hk = blockIdx.y, t = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane & 31, kq = lane >> 5;
    __shared__ Fd256Smem<G> sm;
    // CAP: scale = the op's scale / cap, the score cap * tanhf(dot * scale); both then in the exp2 domain
    const float sc2 = CAP ? scale : scale * FD_L2E, cap2 = cap * FD_L2E;
    const uint16_t *mrow = mask ? mask + (int64_t)t * mask_ld : nullptr;
    float4 qa[G], qb[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const float4 *qp = (const float4 *)(q + (int64_t)t * q_ts + (int64_t)(hk * G + g) * q_hs + sub * 8);
        qa[g] = qp[0];
        qb[g] = qp[1];
    }
    const uint16_t *kb = kc + (int64_t)hk * kv_hs + sub * 8, *vb = vc + (int64_t)hk * kv_hs + sub * 8;
    uint4 ka[4], va[4], kn[4], vn[4];
    uint32_t ma[4], mb[4];                              // mask words (f16) of the group's keys
    const int lim = n_kv - 1;                           // rows past the keys clamp to the last one, masked by their index
    auto issue = [&](int base, uint4 *kk, uint4 *vv, uint32_t *mm) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t p = min(base + 2 * i + kq, lim);
            mm[i] = mrow ? mrow[p] : 0u;
            kk[i] = ld_nt(kb + p * kv_ld);
            vv[i] = ld_nt(vb + p * kv_ld);
        }
    };
    issue(FD_CK * sp + 8 * wave, ka, va, ma);
    issue(FD_CK * (sp + NS) + 8 * wave, kn, vn, mb);
    float qv[G][8], m[G], l[G], acc[G][8];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const float v[8] = {qa[g].x, qa[g].y, qa[g].z, qa[g].w, qb[g].x, qb[g].y, qb[g].z, qb[g].w};
        m[g] = -INFINITY; l[g] = 0.0f;
#pragma unroll
        for (int e = 0; e < 8; ++e) { qv[g][e] = h2f(f2h(v[e])); acc[g][e] = 0.0f; }
    }
    // one 8-key group: keys base + 2 i + kq, i < 4
    auto consume = [&](int base, const uint4 *kk, const uint4 *vv, const uint32_t *mm) {
        float s[G][4], md[4];
        bool ok[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            md[i] = h2f((uint16_t)mm[i]) * FD_L2E;      // -inf stays -inf
            ok[i] = base + 2 * i + kq < n_kv && md[i] != -INFINITY;
            const uint32_t w4[4] = {kk[i].x, kk[i].y, kk[i].z, kk[i].w};
            float kf[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) { kf[2 * e] = h2f(w4[e] & 0xFFFF); kf[2 * e + 1] = h2f(w4[e] >> 16); }
#pragma unroll
            for (int g = 0; g < G; ++g) {
                float sc = 0.0f;
#pragma unroll
                for (int e = 0; e < 8; ++e) sc = fmaf(qv[g][e], kf[e], sc);
                s[g][i] = sc;
            }
        }
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int i = 0; i < 4; ++i) s[g][i] += dpp_f<0xB1>(s[g][i]);
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int i = 0; i < 4; ++i) s[g][i] += dpp_f<0x4E>(s[g][i]);
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int i = 0; i < 4; ++i) s[g][i] += dpp_f<0x141>(s[g][i]);
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int i = 0; i < 4; ++i) s[g][i] += dpp_f<0x140>(s[g][i]);
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float sv = xsum16(s[g][i]);             // the key's 32 lanes
                if constexpr (CAP) sv = cap2 * tanhf(sv * sc2);
                else sv = sv * sc2;
                // a dead key's score (its K bytes may be NaN) never enters
                s[g][i] = ok[i] ? __fadd_rn(sv, md[i]) : -INFINITY;
            }
        float al[G], ls[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            const float mx = xmax32(fmaxf(fmaxf(s[g][0], s[g][1]), fmaxf(s[g][2], s[g][3])));
            // a group without a live key keeps m = -inf and adds nothing (mr = 0 keeps exp2 away from -inf - -inf)
            const float mn = fmaxf(m[g], mx);
            const float mr = mn == -INFINITY ? 0.0f : mn;
            al[g] = __builtin_amdgcn_exp2f(m[g] - mr);
            ls[g] = 0.0f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                s[g][i] = __builtin_amdgcn_exp2f(s[g][i] - mr);
                ls[g] += s[g][i];
            }
            m[g] = mn;
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            l[g] = fmaf(l[g], al[g], xsum32(ls[g]));
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[g][e] *= al[g];
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            // dead keys carry weight exp2(-inf) = 0; their V words are zeroed so that 0 * NaN cannot arise
            const uint32_t w4[4] = {ok[i] ? vv[i].x : 0u, ok[i] ? vv[i].y : 0u, ok[i] ? vv[i].z : 0u, ok[i] ? vv[i].w : 0u};
            float vf[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) { vf[2 * e] = h2f(w4[e] & 0xFFFF); vf[2 * e + 1] = h2f(w4[e] >> 16); }
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[g][e] = fmaf(s[g][i], vf[e], acc[g][e]);
        }
    };
    const int nch = (n_kv + FD_CK - 1) / FD_CK;
    for (int c = sp; c < nch; c += 2 * NS) {
        const int b0 = FD_CK * c + 8 * wave;
        if (b0 < n_kv) consume(b0, ka, va, ma);
        issue(FD_CK * (c + 2 * NS) + 8 * wave, ka, va, ma);
        if (c + NS >= nch) break;
        const int b1 = FD_CK * (c + NS) + 8 * wave;
        if (b1 < n_kv) consume(b1, kn, vn, mb);
        issue(FD_CK * (c + 3 * NS) + 8 * wave, kn, vn, mb);
    }
    // the two key halves of the wave, then the four waves in LDS
#pragma unroll
    for (int g = 0; g < G; ++g)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[g][e] = xsum32(acc[g][e]);
    if (kq == 0) {
#pragma unroll
        for (int g = 0; g < G; ++g) {
            *(float4 *)&sm.o[wave][g][sub * 8] = make_float4(acc[g][0], acc[g][1], acc[g][2], acc[g][3]);
            *(float4 *)&sm.o[wave][g][sub * 8 + 4] = make_float4(acc[g][4], acc[g][5], acc[g][6], acc[g][7]);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int g = 0; g < G; ++g) { sm.ml[wave][g][0] = m[g]; sm.ml[wave][g][1] = l[g]; }
    }
    __syncthreads();
    const int64_t hrow = (int64_t)t * H + hk * G;
    if (tid < G) {
        const int g = tid;
        float M = -INFINITY;
#pragma unroll
        for (int w = 0; w < 4; ++w) M = fmaxf(M, sm.ml[w][g][0]);
        float L = 0.0f;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const float wt = M == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f(sm.ml[w][g][0] - M);
            sm.w[w][g] = wt;
            L = fmaf(wt, sm.ml[w][g][1], L);
        }
        part_ml[(hrow + g) * NS + sp] = make_float2(M, L);
    }
    __syncthreads();
    for (int i = tid; i < G * FD_D; i += 256) {
        const int g = i / FD_D, d = i % FD_D;
        float O = 0.0f;
#pragma unroll
        for (int w = 0; w < 4; ++w) O = fmaf(sm.w[w][g], sm.o[w][g][d], O);
        part_o[((hrow + g) * NS + sp) * FD_D + d] = O;
    }
}

// grid (H, T), 256 threads = the head's dims; wave 0 forms the split weights exp2(m_s - M) (m in the exp2 domain)
__global__ void __launch_bounds__(256) k_fa256_comb(const float *__restrict__ part_o, const float2 *__restrict__ part_ml,
                                                    float *__restrict__ out, int H, int NS) {
    const int h = blockIdx.x, t = blockIdx.y, d = threadIdx.x;
    const int64_t row = (int64_t)t * H + h;
    __shared__ float s_w[FD_MAXS];
    __shared__ float s_l;
    if (d < 64) {
        const float2 v = d < NS ? part_ml[row * NS + d] : make_float2(-INFINITY, 0.0f);
        const float M = wave_max_dpp(v.x);
        const float wt = v.x == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f(v.x - M);
        s_w[d] = wt;
        const float L = wave_sum_f(wt * v.y);
        if (d == 0) s_l = L;
    }
    __syncthreads();
    const float *po = part_o + row * NS * FD_D + d;
    float O = 0.0f;
    for (int s = 0; s < NS; ++s) O = fmaf(s_w[s], po[(int64_t)s * FD_D], O);
    out[row * FD_D + d] = O / s_l;
}

// ---------------------------------------------------------------- any T: MFMA tiles under the explicit mask
template <bool CAP>
__global__ void __launch_bounds__(256) k_fa256_mfma(const char *__restrict__ q, int64_t q_nb1, int64_t q_nb2,
                                                    const uint16_t *__restrict__ kc, const uint16_t *__restrict__ vc,
                                                    const uint16_t *__restrict__ mask, int64_t mask_ld,
                                                    float *__restrict__ out, int T, int H, int HKV, int n_kv, float scale,
                                                    float cap) {
    __shared__ __attribute__((aligned(16))) uint16_t sk[64 * FD_KP];
    __shared__ __attribute__((aligned(16))) uint16_t sv[FD_D * FD_VP];
    __shared__ int s_dead[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = blockIdx.x * 64, h = blockIdx.y, hk = h / (H / HKV);
    const int64_t EKV = (int64_t)HKV * FD_D;
    const int ql = lane & 15, g = lane >> 4;
    const int qi = q0 + 16 * wave + ql;                       // this lane's query (column)
    const int last_q = min(q0 + 64, T) - 1;
    // Q fragments (B operand of S^T): Q[qi][32 s + 8 g + j], 8 dim-steps, rounded to f16
    fd_h8 qf[8];
    {
        const float *qp = (const float *)(q + (int64_t)min(qi, T - 1) * q_nb1 + (int64_t)h * q_nb2) + 8 * g;
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const float4 a = *(const float4 *)(qp + 32 * s), b = *(const float4 *)(qp + 32 * s + 4);
            const float v[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) qf[s][e] = (_Float16)v[e];
        }
    }
    const uint16_t *mrow = mask && qi < T ? mask + (int64_t)qi * mask_ld : nullptr;
    fd_f4 o[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) o[i] = fd_f4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.0f;
    for (int k0 = 0; k0 < n_kv; k0 += 64) {
        __syncthreads();                                      // previous tile fully consumed
        int live = 0;
        if (tid < 64) {                                       // keys masked for every query of the tile are dead
            const int p = k0 + tid;
            int dead = 1;
            if (p < n_kv) {
                if (!mask) dead = 0;
                for (int qq = q0; mask && qq <= last_q && dead; ++qq) dead = mask[(int64_t)qq * mask_ld + p] == 0xFC00;
            }
            s_dead[tid] = dead;
            live = !dead;
        }
        if (!__syncthreads_or(live)) continue;                // (uniform) no key of the tile is seen by any query
        // stage K tile [64][256] and V^T tile [256][64]; dead keys as zeros, their bytes never read
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int idx = tid + 256 * i;                    // 2048 16-B pieces per tile
            const int kr = idx >> 5, c8 = idx & 31;
            uint4 kv = make_uint4(0, 0, 0, 0), vv = make_uint4(0, 0, 0, 0);
            if (!s_dead[kr]) {
                const int64_t off = (int64_t)(k0 + kr) * EKV + (int64_t)hk * FD_D + 8 * c8;
                kv = *(const uint4 *)(kc + off);
                vv = *(const uint4 *)(vc + off);
            }
            *(uint4 *)(sk + kr * FD_KP + 8 * c8) = kv;
            const uint32_t w4[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                sv[(8 * c8 + 2 * e) * FD_VP + kr] = (uint16_t)(w4[e] & 0xFFFF);
                sv[(8 * c8 + 2 * e + 1) * FD_VP + kr] = (uint16_t)(w4[e] >> 16);
            }
        }
        __syncthreads();
        // S^T for 4 blocks of 16 keys: sc[b][r] = key k0 + 16 b + 4 g + r against query qi
        fd_f4 sc[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            sc[b] = fd_f4{0.f, 0.f, 0.f, 0.f};
            const uint16_t *kp = sk + (16 * b + ql) * FD_KP + 8 * g;
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const fd_h8 ka = *(const fd_h8 *)(kp + 32 * s);
                sc[b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ka, qf[s], sc[b], 0, 0, 0);
            }
        }
        float mt = -INFINITY;
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int p = k0 + 16 * b + 4 * g + r;
                uint16_t mv = 0xFC00;                         // rows past T and keys past n_kv: masked
                if (qi < T && p < n_kv) mv = mrow ? mrow[p] : (uint16_t)0;
                float v = sc[b][r] * scale;
                if constexpr (CAP) v = cap * tanhf(v);
                v = mv == 0xFC00 ? -INFINITY : v + h2f(mv);
                sc[b][r] = v;
                mt = fmaxf(mt, v);
            }
        mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        const float m_new = fmaxf(m_run, mt);
        const float alpha = m_run == -INFINITY ? 0.0f : expf(m_run - m_new);
        float ls = 0.0f;
        fd_h8 pb[2];                                          // P^T k-slices for the two 32-key steps
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = sc[b][r] == -INFINITY ? 0.0f : expf(sc[b][r] - m_new);
                ls += e;
                pb[b >> 1][4 * (b & 1) + r] = (_Float16)e;
            }
        ls += __shfl_xor(ls, 16, 64);
        ls += __shfl_xor(ls, 32, 64);
        l_run = l_run * alpha + ls;
        m_run = m_new;
#pragma unroll
        for (int i = 0; i < 16; ++i) o[i] *= alpha;
        // O^T += V^T . P^T: dim blocks of 16, key steps of 32 in the lane's k order
#pragma unroll
        for (int st = 0; st < 2; ++st) {
#pragma unroll
            for (int db = 0; db < 16; ++db) {
                const uint16_t *vp = sv + (16 * db + ql) * FD_VP + 32 * st + 4 * g;
                const uint2 lo = *(const uint2 *)vp;          // keys 32 st + 4 g .. + 3
                const uint2 hi = *(const uint2 *)(vp + 16);   // keys 32 st + 16 + 4 g .. + 3
                fd_h8 va;
                const uint32_t w[4] = {lo.x, lo.y, hi.x, hi.y};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    va[2 * e] = __builtin_bit_cast(_Float16, (uint16_t)(w[e] & 0xFFFF));
                    va[2 * e + 1] = __builtin_bit_cast(_Float16, (uint16_t)(w[e] >> 16));
                }
                o[db] = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, pb[st], o[db], 0, 0, 0);
            }
        }
    }
    if (qi >= T) return;
    const float inv = 1.0f / l_run;
    float *op = out + ((int64_t)qi * H + h) * FD_D + 4 * g;
#pragma unroll
    for (int db = 0; db < 16; ++db)
        *(float4 *)(op + 16 * db) = make_float4(o[db][0] * inv, o[db][1] * inv, o[db][2] * inv, o[db][3] * inv);
}

extern "C" {

// partial O [T][H][NS][256] + (m, l) [T][H][NS] behind the workspace header, for the up to 16 queries of the decode pair
int64_t kcpp_fa256_ws_bytes(int T, int H) {
    const int64_t tq = std::min(std::max(T, 1), 16);
    return KCPP_FA_WS_HEADER + tq * H * FD_MAXS * (FD_D * 4 + 8) + 256;
}

int kcpp_fa256_dec(const float *q, int64_t q_nb1, int64_t q_nb2, const uint16_t *kc, const uint16_t *vc, int64_t k_ld,
                   int64_t k_hs, const uint16_t *mask, int64_t mask_ld, float *out, void *ws, int T, int H, int HKV,
                   int n_kv, float scale, float logit_softcap, void *stream) {
    if (T < 1 || T > 16 || HKV < 1 || HKV > 65535 || H % HKV || n_kv < 1 || !ws) return -3;
    // 16-B loads: q rows, K / V rows
    if (q_nb1 % 16 || q_nb2 % 16 || ((uintptr_t)q & 15) || k_ld % 8 || k_hs % 8 || ((uintptr_t)kc & 15) || ((uintptr_t)vc & 15))
        return -3;
    // one workgroup per CU over the splits x kv heads of one query (fa_plan.h fa_splits): independent of n_kv, so the
    // key partition -- and the result, bit for bit -- depends on the keys alone
    const int G = H / HKV, NS = fa_splits(HKV, FD_MAXS);
    hipStream_t s = (hipStream_t)stream;
    float *po = (float *)((uint8_t *)ws + KCPP_FA_WS_HEADER);
    float2 *pml = (float2 *)(po + (int64_t)T * H * NS * FD_D);
    const bool capped = logit_softcap != 0.0f;
    const float cscale = capped ? scale / logit_softcap : scale;
    const int rc = fa_for_g<1, 2, 4, 8>(G, [&](auto g) {
        constexpr int GG = decltype(g)::value;
        if (capped)
            hipLaunchKernelGGL((k_fa256_dec<GG, true>), dim3(NS, HKV, T), dim3(256), 0, s, q, q_nb1 / 4, q_nb2 / 4, kc, vc,
                               k_ld, k_hs, mask, mask_ld, po, pml, H, n_kv, NS, cscale, logit_softcap);
        else
            hipLaunchKernelGGL((k_fa256_dec<GG, false>), dim3(NS, HKV, T), dim3(256), 0, s, q, q_nb1 / 4, q_nb2 / 4, kc, vc,
                               k_ld, k_hs, mask, mask_ld, po, pml, H, n_kv, NS, cscale, 0.0f);
    });
    if (rc) return rc;
    KCPP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_fa256_comb, dim3(H, T), dim3(256), 0, s, po, pml, out, H, NS);
    KCPP_CHECK(hipGetLastError());
    return 0;
}

int kcpp_fa256_prefill(const float *q, int64_t q_nb1, int64_t q_nb2, const uint16_t *kc, const uint16_t *vc,
                       const uint16_t *mask, int64_t mask_ld, float *out, int T, int H, int HKV, int n_kv, float scale,
                       float logit_softcap, void *stream) {
    if (T < 1 || HKV < 1 || H % HKV || H > 65535 || n_kv < 1) return -3;
    if (q_nb1 % 16 || q_nb2 % 16 || ((uintptr_t)q & 15) || ((uintptr_t)kc & 15) || ((uintptr_t)vc & 15) ||
        ((uintptr_t)out & 15))
        return -3;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((T + 63) / 64, H);
    if (logit_softcap != 0.0f)
        hipLaunchKernelGGL((k_fa256_mfma<true>), grid, dim3(256), 0, s, (const char *)q, q_nb1, q_nb2, kc, vc, mask, mask_ld,
                           out, T, H, HKV, n_kv, scale / logit_softcap, logit_softcap);
    else
        hipLaunchKernelGGL((k_fa256_mfma<false>), grid, dim3(256), 0, s, (const char *)q, q_nb1, q_nb2, kc, vc, mask, mask_ld,
                           out, T, H, HKV, n_kv, scale, 0.0f);
    KCPP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
