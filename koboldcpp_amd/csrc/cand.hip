// cand.hip -- the device front end of SampleLogits (gfx950, wave64): sparse logit edits, the bucket cut of the
// reference's top_k(5000) pre-filter and the survivors' compaction.  The passes, the exactness argument and the
// argument block are in cand.h; this file is the kernels and their one launcher.
#include <hip/hip_runtime.h>

#include "cand.h"

using namespace kcand;

namespace {

constexpr int WAVES = CAND_BLOCK / 64;
constexpr int ITERS = CAND_SLICE / CAND_BLOCK;

// 6.4f * v + 64.f in two roundings: contracted to an FMA, values next to a bucket edge would change buckets
__device__ __forceinline__ float cand_f(float v) { return __fadd_rn(__fmul_rn(6.4f, v), 64.0f); }
__device__ __forceinline__ int cand_bucket(float f) { return !(f > 0.0f) ? 0 : (f >= 127.0f ? 127 : (int)f); }
__device__ __forceinline__ bool cand_finite(float v) { return fabsf(v) < INFINITY; }       // false for NaN

// the minimum over a workgroup (NaN never taken: v < m is false for it); every thread returns it
__device__ __forceinline__ float block_min(float m, float *sm) {
    for (int o = 32; o > 0; o >>= 1) {
        const float t = __shfl_down(m, o);
        m = t < m ? t : m;
    }
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    m = sm[0];
    for (int w = 1; w < WAVES; ++w) m = sm[w] < m ? sm[w] : m;
    __syncthreads();
    return m;
}

// scratch = logits; minpart[slice] = the slice's minimum
__global__ void __launch_bounds__(CAND_BLOCK) k_cand_copy_min(const float *__restrict__ logits, float *__restrict__ scratch,
                                                              float *__restrict__ minpart, int n) {
    __shared__ float sm[WAVES];
    const int base = blockIdx.x * CAND_SLICE;
    float m = INFINITY;
    for (int it = 0; it < ITERS; ++it) {
        const int id = base + it * CAND_BLOCK + threadIdx.x;
        if (id < n) {
            const float v = logits[id];
            scratch[id] = v;
            m = v < m ? v : m;
        }
    }
    m = block_min(m, sm);
    if (threadIdx.x == 0) minpart[blockIdx.x] = m;
}

// low = LowestLogit of the raw logits (with a set-low list); the thread at the head of an id's run of ops applies the run
__global__ void __launch_bounds__(CAND_BLOCK) k_cand_apply(const Op *__restrict__ ops, int nops, int n_set,
                                                           const float *__restrict__ minpart, int nblk,
                                                           float *__restrict__ scratch, float *__restrict__ low_out, int n) {
    __shared__ float sm[WAVES];
    float low = 0.0f;
    if (n_set > 0) {
        float m = INFINITY;
        for (int i = threadIdx.x; i < nblk; i += CAND_BLOCK) m = minpart[i] < m ? minpart[i] : m;
        m = block_min(m, sm);
        low = m < 0.0f ? __fsub_rn(m, 8.0f) : 0.0f;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *low_out = low;
    const int i = blockIdx.x * CAND_BLOCK + threadIdx.x;
    if (i >= nops) return;
    const int id = ops[i].id;
    if (id < 0 || id >= n || (i > 0 && ops[i - 1].id == id)) return;
    float v = scratch[id];
    for (int j = i; j < nops && ops[j].id == id; ++j) {
        const int kind = ops[j].kind;
        if (kind == CAND_SET) v = low;
        else if (kind == CAND_ADD) v = __fadd_rn(v, ops[j].v);
        else v = __fsub_rn(v, ops[j].v);
    }
    scratch[id] = v;
}

// is id rejected: bit id % 32 of word id / 32 (32 consecutive ids share a word, a wave reads two)
__device__ __forceinline__ bool cand_rejected(const uint32_t *__restrict__ mask, int id) {
    return (mask[id >> 5] >> (id & 31)) & 1u;
}

// hist[slice][128], bad[slice]; raw: the unedited logits when their finiteness counts too (a set-low list), else null.
// MASKED: a rejected id goes to bucket 0 whatever its value and is counted in rej[slice]; bad counts as without a mask
template <bool MASKED>
__global__ void __launch_bounds__(CAND_BLOCK) k_cand_hist(const float *__restrict__ e, const float *__restrict__ raw, int n,
                                                          int32_t *__restrict__ hist, int32_t *__restrict__ bad,
                                                          const uint32_t *__restrict__ mask, int32_t *__restrict__ rej) {
    __shared__ int h[CAND_NB];
    __shared__ int nbad, nrej;
    if (threadIdx.x < CAND_NB) h[threadIdx.x] = 0;
    if (threadIdx.x == 0) nbad = 0, nrej = 0;
    __syncthreads();
    const int base = blockIdx.x * CAND_SLICE;
    for (int it = 0; it < ITERS; ++it) {
        const int id = base + it * CAND_BLOCK + threadIdx.x;
        if (id < n) {
            const float v = e[id], f = cand_f(v);
            if (MASKED && cand_rejected(mask, id)) {
                atomicAdd(&h[0], 1);
                atomicAdd(&nrej, 1);
            } else {
                atomicAdd(&h[cand_bucket(f)], 1);
            }
            bool b = !cand_finite(v) || !(fabsf(f) < 2147483648.0f);
            if (raw) b = b || !cand_finite(raw[id]);
            if (b) atomicAdd(&nbad, 1);
        }
    }
    __syncthreads();
    if (threadIdx.x < CAND_NB) hist[(size_t)blockIdx.x * CAND_NB + threadIdx.x] = h[threadIdx.x];
    if (threadIdx.x == 0) {
        bad[blockIdx.x] = nbad;
        if (MASKED) rej[blockIdx.x] = nrej;
    }
}

// one workgroup: totals, the walk from bucket 127 down to the cut, the header, and each slice's survivor count scanned
// into its offset.  MASKED: hdr is an HdrM; with the cut in bucket 0 the survivors are the ids that are not rejected
template <bool MASKED>
__global__ void __launch_bounds__(CAND_BLOCK) k_cand_cut(const int32_t *__restrict__ hist, const int32_t *__restrict__ bad,
                                                         int nblk, int k, const float *__restrict__ low, Hdr *__restrict__ hdr,
                                                         int32_t *__restrict__ off, const int32_t *__restrict__ rej) {
    __shared__ int tot[CAND_NB];
    __shared__ int sc[CAND_BLOCK];
    __shared__ int s_ib, s_bad, s_rej;
    const int t = threadIdx.x;
    if (t == 0) s_bad = 0, s_rej = 0;
    __syncthreads();
    if (t < CAND_NB) {
        int s = 0;
        for (int b = 0; b < nblk; ++b) s += hist[(size_t)b * CAND_NB + t];
        tot[t] = s;
    } else {
        int s = 0;
        for (int b = t - CAND_NB; b < nblk; b += CAND_BLOCK - CAND_NB) s += bad[b];
        if (s) atomicAdd(&s_bad, s);
        if (MASKED) {
            int r = 0;
            for (int b = t - CAND_NB; b < nblk; b += CAND_BLOCK - CAND_NB) r += rej[b];
            if (r) atomicAdd(&s_rej, r);
        }
    }
    __syncthreads();
    if (t == 0) {
        int nhave = 0, ib = CAND_NB - 1;
        for (; ib > 0; --ib) {
            nhave += tot[ib];
            if (nhave >= k) break;
        }
        if (ib == 0) nhave += tot[0];          // k <= n: the walk ends at bucket 0 at the latest
        if (MASKED) {
            if (ib == 0) nhave -= s_rej;
            HdrM *hm = (HdrM *)hdr;
            hm->n_rej = s_rej;
            hm->pad = 0;
        }
        s_ib = ib;
        hdr->low = low ? *low : 0.0f;
        hdr->ib = ib;
        hdr->nhave = nhave;
        hdr->n_bad = s_bad;
    }
    __syncthreads();
    const int ib = s_ib;
    if (t < CAND_NB) hdr->hist[t] = tot[t];
    // thread t owns slices [t nper, (t + 1) nper)
    const int nper = (nblk + CAND_BLOCK - 1) / CAND_BLOCK;
    const int b0 = min(t * nper, nblk), b1 = min(b0 + nper, nblk);
    int mine = 0;
    for (int b = b0; b < b1; ++b) {
        int c = 0;
        for (int j = ib; j < CAND_NB; ++j) c += hist[(size_t)b * CAND_NB + j];
        if (MASKED && ib == 0) c -= rej[b];
        off[b] = c;
        mine += c;
    }
    sc[t] = mine;
    __syncthreads();
    for (int d = 1; d < CAND_BLOCK; d <<= 1) {
        const int add = t >= d ? sc[t - d] : 0;
        __syncthreads();
        sc[t] += add;
        __syncthreads();
    }
    int at = sc[t] - mine;
    for (int b = b0; b < b1; ++b) {
        const int c = off[b];
        off[b] = at;
        at += c;
    }
}

// the slice's survivors (bucket >= ib; MASKED: and not rejected) to pairs[off[slice] ...] in ascending id, nothing at
// or past cap
template <bool MASKED>
__global__ void __launch_bounds__(CAND_BLOCK) k_cand_compact(const float *__restrict__ e, int n, const Hdr *__restrict__ hdr,
                                                             const int32_t *__restrict__ off, Pair *__restrict__ pairs, int cap,
                                                             const uint32_t *__restrict__ mask) {
    __shared__ int wc[WAVES];
    const int ib = hdr->ib;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int base = blockIdx.x * CAND_SLICE;
    int run = off[blockIdx.x];
    for (int it = 0; it < ITERS; ++it) {
        const int id = base + it * CAND_BLOCK + threadIdx.x;
        float v = 0.0f;
        bool keep = false;
        if (id < n) {
            v = e[id];
            keep = cand_bucket(cand_f(v)) >= ib;
            if (MASKED) keep = keep && !cand_rejected(mask, id);
        }
        const unsigned long long kept = __ballot(keep);
        if (lane == 0) wc[wave] = __popcll(kept);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < WAVES; ++w) {
            if (w < wave) before += wc[w];
            total += wc[w];
        }
        const int pos = run + before + __popcll(kept & ((1ull << lane) - 1ull));
        if (keep && pos >= 0 && pos < cap) pairs[pos] = Pair{id, v};
        run += total;
        __syncthreads();
    }
}

}  // namespace

int kcpp_cand_launch(const Plan &p, const Args &a, void *stream) {
    hipStream_t s = (hipStream_t)stream;
    if (p.rc || p.nblk < 1 || a.n < 1 || (int64_t)p.nblk * CAND_SLICE < a.n || a.k < 1 || a.k > a.n || a.cap < 0 || a.nops < 0 ||
        !a.logits || !a.hist || !a.bad || !a.off || !a.out || (a.nops > 0 && (!a.ops || !a.scratch || !a.minpart || !a.low)) ||
        (a.mask && !a.rej))
        return -2;
    const float *e = a.logits;
    if (a.nops > 0) {
        hipLaunchKernelGGL(k_cand_copy_min, dim3(p.nblk), dim3(CAND_BLOCK), 0, s, a.logits, a.scratch, a.minpart, a.n);
        hipLaunchKernelGGL(k_cand_apply, dim3((a.nops + CAND_BLOCK - 1) / CAND_BLOCK), dim3(CAND_BLOCK), 0, s, a.ops, a.nops,
                           a.n_set, a.minpart, p.nblk, a.scratch, a.low, a.n);
        e = a.scratch;
    }
    Hdr *hdr = (Hdr *)a.out;
    const float *raw = a.n_set > 0 ? a.logits : (const float *)nullptr;
    const float *low = a.nops > 0 ? a.low : (const float *)nullptr;
    if (a.mask) {
        Pair *pairs = (Pair *)((HdrM *)a.out + 1);
        hipLaunchKernelGGL(k_cand_hist<true>, dim3(p.nblk), dim3(CAND_BLOCK), 0, s, e, raw, a.n, a.hist, a.bad, a.mask, a.rej);
        hipLaunchKernelGGL(k_cand_cut<true>, dim3(1), dim3(CAND_BLOCK), 0, s, a.hist, a.bad, p.nblk, a.k, low, hdr, a.off, a.rej);
        hipLaunchKernelGGL(k_cand_compact<true>, dim3(p.nblk), dim3(CAND_BLOCK), 0, s, e, a.n, hdr, a.off, pairs, a.cap, a.mask);
    } else {
        hipLaunchKernelGGL(k_cand_hist<false>, dim3(p.nblk), dim3(CAND_BLOCK), 0, s, e, raw, a.n, a.hist, a.bad,
                           (const uint32_t *)nullptr, (int32_t *)nullptr);
        hipLaunchKernelGGL(k_cand_cut<false>, dim3(1), dim3(CAND_BLOCK), 0, s, a.hist, a.bad, p.nblk, a.k, low, hdr, a.off,
                           (const int32_t *)nullptr);
        hipLaunchKernelGGL(k_cand_compact<false>, dim3(p.nblk), dim3(CAND_BLOCK), 0, s, e, a.n, hdr, a.off, (Pair *)(hdr + 1),
                           a.cap, (const uint32_t *)nullptr);
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
