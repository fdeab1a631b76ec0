// attn_dec.hip -- the single-token split-KV decode attention at D = 128 (FA_DEC_SPLIT4 / SPLIT5 / SHORT of fa_plan.h):
//   k_fa_dec5 (k_fa_dec4: the legacy A/B kernel) grid (splits, kv-head) -> partial (O, m, l), body in attn_dec.h
//   k_fa_comb4 one 256-thread block per head pair -> f32 out (+ Q8_K or KT_Q8_0_TA quant)
//   k_fa_dec5<FINAL>: one 8-wave workgroup per kv head writes the output itself (the short form)
// Reached by kcpp_flash_attn (one query; force_path 7: the short form), kcpp_flash_attn_dec_ta, kcpp_fa_decode_ex
// variants 3, 5, 8 and the tools' 6, 7, and in the GRAPH form (f32 Q, mask row, soft-cap) by kcpp_flash_attn_ext_dec_sc.
#include "attn_common.h"
#include "attn_dec.h"
#include "gemv_units.h"

static void *g_fa_stamps = nullptr;       // diagnostic stamp buffer (tools only; kcpp_fa_set_stamps)

#define FA_STAMP(ph)                                                                                   \
    if (stamps && threadIdx.x == 0) {                                                                  \
        const unsigned long long t_ = __builtin_amdgcn_s_memrealtime();                                \
        __hip_atomic_store(&stamps[wg_id * 8 + (ph)], t_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); \
    }
// ---------------------------------------------------------------- decode v4: streaming splits + wide combine
// One token.  Grid (NS splits, kv head), 256 threads.  Split sp owns keys [sp*per, (sp+1)*per) of [0, n_past].
// Wave w streams 16-key groups base = p0 + 16 w + 64 j: lane (kq = lane >> 4, sub = lane & 15) loads 16 B
// (8 dims) of K and of V for keys base + 4 i + kq, i < 4 -- every load instruction 1 KiB contiguous per wave --
// and the next group's 8 loads are issued before the current one is used.  Scores: 8-dim partial dot, 16-lane
// DPP reduction; online softmax per wave (m, l wave-uniform); O: each lane accumulates its 8 dims over its
// row's keys, rows summed once at the end (permlane swaps), waves merged in LDS.  Partials: O [H][NS][128],
// (m, l) [H][NS] (m = -inf for an empty split).
template <int G, bool NT>
__global__ void __launch_bounds__(256) k_fa_dec4(const uint16_t *__restrict__ q16, const uint16_t *__restrict__ kc,
                                                 const uint16_t *__restrict__ vc, float *__restrict__ part_o,
                                                 float2 *__restrict__ part_ml, int H, int n_past_arg,
                                                 const int32_t *__restrict__ n_past_dev, int NS, float scale,
                                                 int64_t kv_ld, int64_t kv_hs, unsigned long long *stamps) {
    constexpr int D = 128;
    const int sp = blockIdx.x, hk = blockIdx.y;
    const int wg_id = blockIdx.y * gridDim.x + blockIdx.x;
    FA_STAMP(0);
    const int nkv = (n_past_dev ? n_past_dev[0] : n_past_arg) + 1;
    const int per = (nkv + NS - 1) / NS;
    const int p0 = sp * per, p1 = min(p0 + per, nkv);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane & 15, kq = lane >> 4;
    __shared__ fadec::Smem<G> sm;
    // scores in the exp2 domain: s2 = (q . k) * scale * log2(e); partial m in the same domain
    const float sc2 = scale * 1.4426950408889634f;
    fadec::State<G> st;
#pragma unroll
    for (int g = 0; g < G; ++g) fadec::set_q(st, g, *(const uint4 *)(q16 + (int64_t)(hk * G + g) * D + sub * 8));
    if (stamps) { if (st.qv[0][0] == 12345.0f) stamps[0] = 0; FA_STAMP(1); }
    const uint16_t *kb = kc + (int64_t)hk * kv_hs + sub * 8, *vb = vc + (int64_t)hk * kv_hs + sub * 8;
    fadec::init(st);
    uint4 ka[4], va[4], kn[4], vn[4];
    auto issue = [&](int base, uint4 *kk, uint4 *vv) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = base + 4 * i + kq;
            const bool ok = p < p1;
            if constexpr (NT) {      // K/V rows are read once per token: non-temporal (MI355X_MICROARCH.md nt-weights)
                kk[i] = ok ? ld_nt(kb + (int64_t)p * kv_ld) : make_uint4(0, 0, 0, 0);
                vv[i] = ok ? ld_nt(vb + (int64_t)p * kv_ld) : make_uint4(0, 0, 0, 0);
            } else {
                kk[i] = ok ? *(const uint4 *)(kb + (int64_t)p * kv_ld) : make_uint4(0, 0, 0, 0);
                vv[i] = ok ? *(const uint4 *)(vb + (int64_t)p * kv_ld) : make_uint4(0, 0, 0, 0);
            }
        }
    };
    int base = p0 + 16 * wave;
    if (base < p1) issue(base, ka, va);
    for (; base < p1; base += 128) {
        const int b1 = base + 64;
        if (b1 < p1) issue(b1, kn, vn);
        fadec::consume(st, base, p1, kq, sc2, ka, va);
        if (stamps && base == p0 + 16 * wave) { if (st.acc[0][0] == 12345.0f) stamps[0] = 0; FA_STAMP(2); }
        if (b1 >= p1) break;
        if (b1 + 64 < p1) issue(b1 + 64, ka, va);
        fadec::consume(st, b1, p1, kq, sc2, kn, vn);
    }
    FA_STAMP(3);
    fadec::finish(st, sm, hk, sp, NS, part_o, part_ml);
    FA_STAMP(4);
    if (stamps) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); FA_STAMP(5); }
}

// ---------------------------------------------------------------- decode v5: every K/V load in flight from entry
// k_fa_dec4 issued its first 16-key group only after the n_past word arrived (the split range depends on it), and its
// loads sat in lane-conditional branches, so the compiler could not count them: the q conversion waited for nearly
// all of the first group and the second group went out only after the first had landed -- two dependent HBM round
// trips per wave plus the n_past one in front.  Here the key partition does not depend on n_past: 64-key chunks,
// chunk c on split c % NS (chunks sp, sp + NS, ...), wave w owning keys 64 c + 16 w .. + 15 of each, so split sp's
// first chunk is issued at entry beside q (rows clamped to the cache's n_rows), its second as soon as n_past is
// known (rows clamped to n_past), and every load is unconditional (rows past the keys clamp to a valid row and are
// masked by their score), which keeps the compiler's vmcnt accounting exact: two chunks per wave in flight, q waited
// for alone.  Partials as k_fa_dec4 (O [H][NS][128], (m, l) [H][NS], m = -inf for a split without keys); the merge
// is k_fa_comb4.
// GRAPH (the ggml plugin's FLASH_ATTN_EXT with one query, kcpp_flash_attn_ext_dec): q f32 at qf (head stride qf_hs
// floats), rounded to f16 in the kernel; the f16 mask row added to the scores, -inf keys skipped.
// FINAL (short contexts, NS = 1, kcpp_flash_attn force_path 7): one workgroup per kv head walks every key and writes
// the attention output itself (part_o = out [H][128]) -- no combine launch
// CAP (with GRAPH): the op's logit soft-cap; scale = the op's scale / cap, the score cap * tanhf(dot * scale) + mask
template <int G, bool NT, int NW = 4, bool GRAPH = false, bool FINAL = false, bool CAP = false>
__global__ void __launch_bounds__(64 * NW) k_fa_dec5(const uint16_t *__restrict__ q16, const uint16_t *__restrict__ kc,
                                                     const uint16_t *__restrict__ vc, float *__restrict__ part_o,
                                                     float2 *__restrict__ part_ml, int H, int n_past_arg,
                                                     const int32_t *__restrict__ n_past_dev, int NS, float scale,
                                                     int64_t kv_ld, int64_t kv_hs, int n_rows,
                                                     const float *__restrict__ qf = nullptr, int64_t qf_hs = 0,
                                                     const uint16_t *__restrict__ mask = nullptr, float cap = 0.0f) {
    static_assert(!CAP || GRAPH, "the soft-cap exists in the graph form only");
    constexpr int D = 128, CK = 16 * NW;              // keys per chunk: 16 per wave
    const int sp = blockIdx.x, hk = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane & 15, kq = lane >> 4;
    __shared__ fadec::Smem<G, NW> sm;
    const float sc2 = CAP ? scale : scale * 1.4426950408889634f;    // scores in the exp2 domain (CAP: after tanhf)
    const float cap2 = cap * 1.4426950408889634f;
    uint4 qraw[GRAPH ? 1 : G];
    float4 qfa[GRAPH ? G : 1], qfb[GRAPH ? G : 1];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if constexpr (GRAPH) {
            const float4 *qp = (const float4 *)(qf + (int64_t)(hk * G + g) * qf_hs + sub * 8);
            qfa[g] = qp[0];
            qfb[g] = qp[1];
        } else {
            qraw[g] = *(const uint4 *)(q16 + (int64_t)(hk * G + g) * D + sub * 8);
        }
    }
    const uint16_t *kb = kc + (int64_t)hk * kv_hs + sub * 8, *vb = vc + (int64_t)hk * kv_hs + sub * 8;
    uint4 ka[4], va[4], kn[4], vn[4];
    uint32_t ma[GRAPH ? 4 : 1], mb[GRAPH ? 4 : 1];      // mask words (f16) of the group's keys
    auto issue = [&](int base, int lim, uint4 *kk, uint4 *vv, uint32_t *mm) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t p = min(base + 4 * i + kq, lim);
            if constexpr (GRAPH) mm[i] = mask[p];
            if constexpr (NT) {
                kk[i] = ld_nt(kb + p * kv_ld);
                vv[i] = ld_nt(vb + p * kv_ld);
            } else {
                kk[i] = *(const uint4 *)(kb + p * kv_ld);
                vv[i] = *(const uint4 *)(vb + p * kv_ld);
            }
        }
    };
    issue(CK * sp + 16 * wave, n_rows - 1, ka, va, ma);
    const int nkv = (n_past_dev ? n_past_dev[0] : n_past_arg) + 1;
    const int lim = nkv - 1;
    issue(CK * (sp + NS) + 16 * wave, lim, kn, vn, mb);
    fadec::State<G> st;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        if constexpr (GRAPH) fadec::set_q_f32(st, g, qfa[g], qfb[g]);
        else fadec::set_q(st, g, qraw[g]);
    }
    fadec::init(st);
    const float l2e = 1.4426950408889634f;
    auto madd = [&](const uint32_t *mm, float *out) {    // the mask times log2(e); -inf stays -inf
#pragma unroll
        for (int i = 0; i < 4; ++i) out[i] = h2f((uint16_t)mm[i]) * l2e;
    };
    const int nch = (nkv + CK - 1) / CK;
    for (int c = sp; c < nch; c += 2 * NS) {
        const int b0 = CK * c + 16 * wave;
        float md[4];
        if constexpr (GRAPH) madd(ma, md);
        if constexpr (CAP) { if (b0 < nkv) fadec::consume<G, true>(st, b0, nkv, kq, sc2, ka, va, md, cap2); }
        else if (b0 < nkv) fadec::consume(st, b0, nkv, kq, sc2, ka, va, GRAPH ? md : nullptr);
        issue(CK * (c + 2 * NS) + 16 * wave, lim, ka, va, ma);
        if (c + NS >= nch) break;
        const int b1 = CK * (c + NS) + 16 * wave;
        if constexpr (GRAPH) madd(mb, md);
        if constexpr (CAP) { if (b1 < nkv) fadec::consume<G, true>(st, b1, nkv, kq, sc2, kn, vn, md, cap2); }
        else if (b1 < nkv) fadec::consume(st, b1, nkv, kq, sc2, kn, vn, GRAPH ? md : nullptr);
        issue(CK * (c + 3 * NS) + 16 * wave, lim, kn, vn, mb);
    }
    fadec::finish<G, NW, FINAL>(st, sm, hk, sp, NS, part_o, part_ml);
}

// combine of k_fa_dec4's partials (m in the exp2 domain): grid (H / 2), 256 threads = 2 heads x 128 dims
// (one Q8_K block of 256 when quantizing); thread (head, d) issues all NS partial loads of its dim (<= 64, in
// flight together); one wave per head forms the split weights exp2(m_s - M) in LDS.
// QUANT 1: qout = the Q8_K activation; 2: the KT_Q8_0_TA activation of one token (8 Q8_0 blocks per head pair)
template <int QUANT, int NS>
__global__ void __launch_bounds__(256) k_fa_comb4(const float *__restrict__ part_o, const float2 *__restrict__ part_ml,
                                                  float *__restrict__ out, uint8_t *__restrict__ qout, int H,
                                                  unsigned long long *stamps, unsigned *reset) {
    constexpr int D = 128, MAXS = 64;
    const int pair = blockIdx.x, tid = threadIdx.x;
    if (reset && pair == 0 && tid < 15) reset[32 * tid] = 0;   // (a caller's counters: reset once consumed)
    const int wg_id = 2048 + blockIdx.x;
    FA_STAMP(0);
    const int hl = tid >> 7, d = tid & 127, h = 2 * pair + hl;
    __shared__ float s_w[2][MAXS];
    __shared__ float s_l[2];
    __shared__ float s_res[2 * D];
    const float *po = part_o + (int64_t)h * NS * D + d;
    float ov[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) ov[s] = po[(int64_t)s * D];
    if (d < 64) {                                        // wave 0 / 2: split weights of head hl
        const float2 v = d < NS ? part_ml[(int64_t)h * NS + d] : make_float2(-INFINITY, 0.0f);
        const float M = wave_max_dpp(v.x);
        const float wt = v.x == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f(v.x - M);
        s_w[hl][d] = wt;
        const float L = wave_sum_f(wt * v.y);
        if (d == 0) s_l[hl] = L;
    }
    __syncthreads();
    FA_STAMP(1);
    float O0 = 0.0f, O1 = 0.0f, O2 = 0.0f, O3 = 0.0f;
#pragma unroll
    for (int s = 0; s < NS; s += 4) {
        O0 = fmaf(s_w[hl][s], ov[s], O0);
        O1 = fmaf(s_w[hl][s + 1], ov[s + 1], O1);
        O2 = fmaf(s_w[hl][s + 2], ov[s + 2], O2);
        O3 = fmaf(s_w[hl][s + 3], ov[s + 3], O3);
    }
    const float res = ((O0 + O1) + (O2 + O3)) / s_l[hl];
    FA_STAMP(2);
    if (out) out[(int64_t)h * D + d] = res;
    if constexpr (QUANT == 2) {
        s_res[tid] = res;
        __syncthreads();
        if (tid < 16) {                                  // half (tid & 1) of block tid >> 1: k_quant_q80's rounding
            float v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = s_res[16 * tid + k];
            float am = 0.0f;
#pragma unroll
            for (int k = 0; k < 16; ++k) am = fmaxf(am, fabsf(v[k]));
            am = fmaxf(am, __shfl_xor(am, 1, 64));
            const float id = (am != 0.0f) ? 127.f / am : 0.0f;
            uint32_t pk[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                int iv = (int)rintf(__fmul_rn(v[k], id));
                iv = iv > 127 ? 127 : (iv < -128 ? -128 : iv);
                pk[k >> 2] |= (uint32_t)(iv & 0xFF) << (8 * (k & 3));
            }
            const int64_t E = (int64_t)H * D, ib = (int64_t)pair * 8 + (tid >> 1);
            *(uint4 *)(qout + ib * 1024 + (tid & 1) * 512) = make_uint4(pk[0], pk[1], pk[2], pk[3]);
            if ((tid & 1) == 0) ((float *)(qout + 32 * E))[ib * 32] = h2f(f2h(am / 127.f));
        }
    } else if constexpr (QUANT == 1) {
        s_res[tid] = res;
        __syncthreads();
        if (tid < 16) {
            float v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = s_res[16 * tid + k];
            const int64_t E = (int64_t)H * D, nsb = E / 256;
            q8k_quant16(v, tid, (int8_t *)qout + pair * 256, (float *)(qout + E) + pair,
                        (int16_t *)(qout + E + nsb * 4) + pair * 16);
        }
    }
    if (stamps) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); FA_STAMP(3); }
}

#undef FA_STAMP

extern "C" void kcpp_fa_set_stamps(void *p) { g_fa_stamps = p; }   // stamp buffer of k_fa_dec4 / k_fa_comb4 (tools only)

// k_fa_comb4 over the plan's ns partials; -3 for a split count it is not built for
template <int... NSs>
static int fa_comb4_launch(int NS, int quant, const float *po, const float2 *pml, const FaArgs &a, dim3 grid, int threads,
                           unsigned long long *st) {
    return fa_for_ns<NSs...>(NS, [&](auto ns) {
        constexpr int N = decltype(ns)::value;
        if (quant == 2)
            hipLaunchKernelGGL((k_fa_comb4<2, N>), grid, dim3(threads), 0, a.s, po, pml, a.out, (uint8_t *)a.qout, a.H, st,
                               (unsigned *)nullptr);
        else if (quant == 1)
            hipLaunchKernelGGL((k_fa_comb4<1, N>), grid, dim3(threads), 0, a.s, po, pml, a.out, (uint8_t *)a.qout, a.H, st,
                               (unsigned *)nullptr);
        else
            hipLaunchKernelGGL((k_fa_comb4<0, N>), grid, dim3(threads), 0, a.s, po, pml, a.out, (uint8_t *)nullptr, a.H, st,
                               (unsigned *)nullptr);
    });
}

// single-token decode: k_fa_dec5 (k_fa_dec4 where the plan says so: the cache's row count a.n_rows not known, or A/B) +
// k_fa_comb4; a.n_rows: rows the K/V views hold (n_ctx), >= n_past + 1.  a.qf: the GRAPH form (f32 Q, the mask row,
// CAP when a.cap != 0; a.n_past = n_kv - 1).  GQA ratios 3, 5, 6, 7 (the Qwen2.5 sizes) exist as the runtime k_fa_dec5
// alone: the legacy A/B kernel and the GRAPH form are not built for them.
int fa_split_launch(const FaDecodePlan &p, const FaArgs &a) {
    float *po = (float *)((uint8_t *)a.ws + p.part_o);
    float2 *pml = (float2 *)((uint8_t *)a.ws + p.part_ml);
    const dim3 grid(p.grid[0], p.grid[1]), block(64 * p.waves);
    const int G = a.H / a.HKV, NS = p.ns;
    unsigned long long *st = a.qf ? nullptr : (unsigned long long *)g_fa_stamps;
    static const bool nt = [] { const char *e = getenv("KCPP_FA_NT"); return !e || atoi(e) != 0; }();
    int rc;
    if (a.qf)
        rc = fa_for_g<1, 2, 4, 8>(G, [&](auto g) {
            constexpr int G_ = decltype(g)::value;
            if (a.cap != 0.0f)
                hipLaunchKernelGGL((k_fa_dec5<G_, true, 4, true, false, true>), grid, block, 0, a.s,
                                   (const uint16_t *)nullptr, a.kc, a.vc, po, pml, a.H, a.n_past, (const int32_t *)nullptr,
                                   NS, a.scale / a.cap, a.kv_ld, a.kv_hs, a.n_rows, a.qf, a.qf_hs, a.mask, a.cap);
            else
                hipLaunchKernelGGL((k_fa_dec5<G_, true, 4, true>), grid, block, 0, a.s, (const uint16_t *)nullptr, a.kc,
                                   a.vc, po, pml, a.H, a.n_past, (const int32_t *)nullptr, NS, a.scale, a.kv_ld, a.kv_hs,
                                   a.n_rows, a.qf, a.qf_hs, a.mask);
        });
    else if (p.kernel == FA_DEC_SPLIT4)
        rc = fa_for_g<1, 2, 4, 8>(G, [&](auto g) {
            constexpr int G_ = decltype(g)::value;
            if (nt)
                hipLaunchKernelGGL((k_fa_dec4<G_, true>), grid, block, 0, a.s, a.q16, a.kc, a.vc, po, pml, a.H, a.n_past,
                                   a.n_past_dev, NS, a.scale, a.kv_ld, a.kv_hs, st);
            else
                hipLaunchKernelGGL((k_fa_dec4<G_, false>), grid, block, 0, a.s, a.q16, a.kc, a.vc, po, pml, a.H, a.n_past,
                                   a.n_past_dev, NS, a.scale, a.kv_ld, a.kv_hs, st);
        });
    else
        rc = fa_for_g<1, 2, 3, 4, 5, 6, 7, 8>(G, [&](auto g) {
            constexpr int G_ = decltype(g)::value;
            if (nt)
                hipLaunchKernelGGL((k_fa_dec5<G_, true>), grid, block, 0, a.s, a.q16, a.kc, a.vc, po, pml, a.H, a.n_past,
                                   a.n_past_dev, NS, a.scale, a.kv_ld, a.kv_hs, a.n_rows);
            else
                hipLaunchKernelGGL((k_fa_dec5<G_, false>), grid, block, 0, a.s, a.q16, a.kc, a.vc, po, pml, a.H, a.n_past,
                                   a.n_past_dev, NS, a.scale, a.kv_ld, a.kv_hs, a.n_rows);
        });
    if (rc) return rc;
    KCPP_CHECK(hipGetLastError());
    rc = fa_comb4_launch<4, 8, 16, 32, 64>(NS, p.cquant, po, pml, a, dim3(p.cgrid[0]), p.cthreads, st);
    if (rc) return rc;
    KCPP_CHECK(hipGetLastError());
    return 0;
}

// short contexts (n_kv <= KCPP_FA_SHORT_MAX): k_fa_dec5<FINAL> on one 8-wave workgroup per kv head, the output written
// directly (one launch instead of split + combine; at a few hundred keys the split grid mostly holds empty splits and
// the combine is a whole dependent launch).  The caller decides by the host-known position (graphs per regime).
int fa_short_launch(const FaDecodePlan &p, const FaArgs &a) {
    const int rc = fa_for_g<1, 2, 3, 4, 5, 6, 7, 8>(a.H / a.HKV, [&](auto g) {
        hipLaunchKernelGGL((k_fa_dec5<decltype(g)::value, true, 8, false, true>), dim3(p.grid[0], p.grid[1]),
                           dim3(64 * p.waves), 0, a.s, a.q16, a.kc, a.vc, a.out, (float2 *)nullptr, a.H, a.n_past,
                           a.n_past_dev, p.ns, a.scale, a.kv_ld, a.kv_hs, a.n_rows, (const float *)nullptr, (int64_t)0,
                           (const uint16_t *)nullptr);
    });
    if (rc) return rc;
    KCPP_CHECK(hipGetLastError());
    return 0;
}

// kcpp_fa_decode_ex variants 6 / 7, A/B (tools/fa_dec_bench.py): k_fa_dec5 at NS splits (KCPP_FA_NS) x NW waves
// (KCPP_FA_NW), G = 4; 7: without the combine (the split kernel alone)
int fa_dec_tool(int variant, const FaArgs &a) {
    const int NS = getenv("KCPP_FA_NS") ? atoi(getenv("KCPP_FA_NS")) : 32;
    const int NW = getenv("KCPP_FA_NW") ? atoi(getenv("KCPP_FA_NW")) : 4;
    if (a.H / a.HKV != 4 || !a.out) return -1;
    float *po = (float *)((uint8_t *)a.ws + KCPP_FA_WS_HEADER);
    float2 *pml = (float2 *)(po + (int64_t)a.H * NS * 128);
    if (fa_for_g<4, 8, 16>(NW, [&](auto nw) {           // (the same dispatch, over the wave count)
            constexpr int NW_ = decltype(nw)::value;
            hipLaunchKernelGGL((k_fa_dec5<4, true, NW_>), dim3(NS, a.HKV), dim3(64 * NW_), 0, a.s, a.q16, a.kc, a.vc, po,
                               pml, a.H, a.n_past, a.n_past_dev, NS, a.scale, a.kv_ld, a.kv_hs, a.n_rows);
        }))
        return -1;
    if (variant == 6 && fa_comb4_launch<8, 16, 32>(NS, 0, po, pml, a, dim3(a.H / 2), 256, nullptr)) return -1;
    KCPP_CHECK(hipGetLastError());
    return 0;
}
