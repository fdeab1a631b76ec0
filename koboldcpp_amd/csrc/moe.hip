// moe.hip -- mixture-of-experts pieces around the expert mat-vecs / GEMMs (GGML_OP_MUL_MAT_ID path).
//
// Reference: llm_build_moe_ffn (src/llama.cpp:9416-9520) and its CUDA execution ggml_cuda_mul_mat_id
// (ggml/src/ggml-cuda.cu:2003-2139), which copies the expert ids to the host and synchronizes on every
// MoE mat-mul.  Here:
//   * k_moe_route: router logits (F16 weights: the activation rounded to f16 first, as the CPU's
//     vec_dot_f16 does; or F32), softmax (ggml_float sum), top-k by the CPU argsort's exchange order,
//     weights normalized by their sum -- one workgroup per token (wave w: experts w, w+4, ..., all loads of
//     an expert in flight at once), results stay on the device; build_qwen2moe (src/llama.cpp:12248-12392) takes
//     the probabilities unnormalized and adds a shared expert behind silu(z)/z, z = ffn_gate_inp_shexp . x: the
//     RAW / GT instances (kcpp_moe_route_ex) and k_moe_combine_shexp;
//   * decode reads the expert id inside the expert mat-vec kernels (DecArgs.eid), so a whole token
//     remains one hipGraph replay with no host round trip;
//   * prefill groups tokens per expert on the host (one sync per layer, like the reference) and runs
//     each expert as a dense GEMM over its gathered rows; k_moe_scatter writes w * out into the token's
//     top-k slot, and k_moe_combine sums the slots in top-k order and adds the residual
//     (ggml_add chain over the weighted experts view, then ggml_add(moe_out, ffn_inp)).
#include "kcpp_common.h"
#include "kcpp_internal.h"

#define MOE_MAX_EXPERT 64

// four consecutive elements of a router / gate row (F16 rows widened)
template <int WT>
__device__ __forceinline__ float4 route_row4(const void *w, int64_t i) {
    if constexpr (WT == KT_F16) {
        const uint2 h = *(const uint2 *)((const uint16_t *)w + i);
        return make_float4(h2f(h.x & 0xFFFF), h2f(h.x >> 16), h2f(h.y & 0xFFFF), h2f(h.y >> 16));
    } else {
        return *(const float4 *)((const float *)w + i);
    }
}
// the activation as the row's vec_dot sees it: ggml converts src1 to the F16 vec_dot_type of an F16 row
template <int WT>
__device__ __forceinline__ float4 route_act4(float4 v) {
    if constexpr (WT == KT_F16) return make_float4(h2f(f2h_rn(v.x)), h2f(f2h_rn(v.y)), h2f(f2h_rn(v.z)), h2f(f2h_rn(v.w)));
    return v;
}
// one wave's dot of row wr with the token's row: lane: 4 consecutive elements per 256-element step, 4 steps in flight
template <int WT>
__device__ __forceinline__ float route_dot_wave(const float *__restrict__ xr, const void *__restrict__ wr, int K, int lane) {
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int i0 = 4 * lane; i0 < K; i0 += 1024) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + 256 * u;
            if (i >= K) break;
            const float4 xv = route_act4<WT>(*(const float4 *)(xr + i));
            const float4 wv = route_row4<WT>(wr, i);
            acc[u] = fmaf(xv.x, wv.x, acc[u]);
            acc[u] = fmaf(xv.y, wv.y, acc[u]);
            acc[u] = fmaf(xv.z, wv.z, acc[u]);
            acc[u] = fmaf(xv.w, wv.w, acc[u]);
        }
    }
    return wave_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
}

// NORM: x is the residual stream and the router input is rms_norm(x) * nw computed here exactly as k_rms_norm
// does for K <= 4096 (same thread -> element map, double partial sums in the same order), one launch less.
// RAW: the weights are the selected softmax probabilities themselves (llm_build_moe_ffn with norm_w = false, as
// build_qwen2moe calls it): no sum, no division.
// GT (KT_F32 / KT_F16, -1 = none): the shared expert's gate row gw [K] (ffn_gate_inp_shexp) is dotted with the same
// input row as one more "expert" of the dot only -- never in the softmax, never selectable -- and
// gate[t] = silu(z) / z as the reference's nodes compute it (ggml_silu: z / (1 + expf(-z)); ggml_div by z)
template <int WT, bool NORM = false, bool RAW = false, int GT = -1>
__global__ void __launch_bounds__(256) k_moe_route(const float *__restrict__ x, int64_t ldx, const void *__restrict__ w,
                                                   int K, int NE, int NU, int32_t *__restrict__ ids,
                                                   float *__restrict__ wts, const float *__restrict__ nw = nullptr,
                                                   float eps = 0.0f, const void *__restrict__ gw = nullptr,
                                                   float *__restrict__ gate = nullptr) {
    constexpr bool GATE = GT >= 0;
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float *xr = x + (int64_t)t * ldx;
    __shared__ float s_logit[MOE_MAX_EXPERT + 1];        // [NE]: the gate row's dot
    __shared__ float s_part[4][8];
    __shared__ float s_gpart[4];
    if (NE <= 8) {
        // all experts at once: thread tid owns elements 16 tid .. +15 of every 4096-element chunk, the loads of
        // all NE router rows in flight together (one memory round trip per chunk)
        float acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        float gacc = 0.0f;
        float nscale = 1.0f;
        // NORM (K <= 4096, one chunk): the router rows' loads go out first -- they do not wait for the norm -- so
        // the weight and residual round trips overlap
        float4 wpre[NORM ? 8 : 1][4], gpre[4], gwpre[4];
        if constexpr (NORM) {
#pragma unroll
            for (int u = 0; u < 4; ++u)
                gpre[u] = 16 * tid + 4 * u < K ? *(const float4 *)(nw + 16 * tid + 4 * u) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int e = 0; e < 8; ++e)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = 16 * tid + 4 * u;
                    wpre[e][u] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (e < NE && i < K) wpre[e][u] = route_row4<WT>(w, (int64_t)e * K + i);
                }
            if constexpr (GATE) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = 16 * tid + 4 * u;
                    gwpre[u] = i < K ? route_row4<GT>(gw, i) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
        }
        if constexpr (NORM) {                            // K <= 4096: one chunk, elements 16 tid .. +15
            double ss = 0.0;
            if (16 * tid < K) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float4 f = *(const float4 *)(xr + 16 * tid + 4 * u);
                    ss += (double)__fmul_rn(f.x, f.x); ss += (double)__fmul_rn(f.y, f.y);
                    ss += (double)__fmul_rn(f.z, f.z); ss += (double)__fmul_rn(f.w, f.w);
                }
            }
            ss = wave_sum(ss);
            __shared__ double red[4];
            if (lane == 0) red[wave] = ss;
            __syncthreads();
            double sum = 0.0;
            for (int i = 0; i < 4; ++i) sum += red[i];
            const float mean = (float)(sum / (double)K);
            nscale = 1.0f / sqrtf(mean + eps);
        }
        for (int i0 = 16 * tid; i0 < K; i0 += 4096) {
            float4 xv[4], xg[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                xv[u] = i0 + 4 * u < K ? *(const float4 *)(xr + i0 + 4 * u) : make_float4(0.f, 0.f, 0.f, 0.f);
                if constexpr (NORM) {
                    if (i0 + 4 * u < K) {
                        const float4 g = gpre[u];
                        xv[u] = make_float4(__fmul_rn(__fmul_rn(xv[u].x, nscale), g.x), __fmul_rn(__fmul_rn(xv[u].y, nscale), g.y),
                                            __fmul_rn(__fmul_rn(xv[u].z, nscale), g.z), __fmul_rn(__fmul_rn(xv[u].w, nscale), g.w));
                    }
                }
                if constexpr (GATE) xg[u] = route_act4<GT>(xv[u]);      // the gate row's own vec_dot_type
                xv[u] = route_act4<WT>(xv[u]);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (e >= NE) break;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = i0 + 4 * u;
                    if (i >= K) break;
                    float4 wv;
                    if constexpr (NORM) wv = wpre[e][u];
                    else wv = route_row4<WT>(w, (int64_t)e * K + i);
                    acc[e] = fmaf(xv[u].x, wv.x, acc[e]);
                    acc[e] = fmaf(xv[u].y, wv.y, acc[e]);
                    acc[e] = fmaf(xv[u].z, wv.z, acc[e]);
                    acc[e] = fmaf(xv[u].w, wv.w, acc[e]);
                }
            }
            if constexpr (GATE) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int i = i0 + 4 * u;
                    if (i >= K) break;
                    float4 wv;
                    if constexpr (NORM) wv = gwpre[u];
                    else wv = route_row4<GT>(gw, i);
                    gacc = fmaf(xg[u].x, wv.x, gacc);
                    gacc = fmaf(xg[u].y, wv.y, gacc);
                    gacc = fmaf(xg[u].z, wv.z, gacc);
                    gacc = fmaf(xg[u].w, wv.w, gacc);
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (e >= NE) break;
            const float v = wave_sum(acc[e]);
            if (lane == 0) s_part[wave][e] = v;
        }
        if constexpr (GATE) {
            const float v = wave_sum(gacc);
            if (lane == 0) s_gpart[wave] = v;
        }
        __syncthreads();
        if (tid < NE) s_logit[tid] = (s_part[0][tid] + s_part[1][tid]) + (s_part[2][tid] + s_part[3][tid]);
        if constexpr (GATE)
            if (tid == 64) s_logit[NE] = (s_gpart[0] + s_gpart[1]) + (s_gpart[2] + s_gpart[3]);
    } else {
        // wave w: experts w, w+4, ... (the gate row is row NE of that sequence)
        for (int e = wave; e < NE + (GATE ? 1 : 0); e += 4) {
            float a;
            if (GATE && e == NE) a = route_dot_wave<GATE ? GT : WT>(xr, gw, K, lane);
            else if constexpr (WT == KT_F16) a = route_dot_wave<WT>(xr, (const uint16_t *)w + (int64_t)e * K, K, lane);
            else a = route_dot_wave<WT>(xr, (const float *)w + (int64_t)e * K, K, lane);
            if (lane == 0) s_logit[e] = a;
        }
    }
    __syncthreads();
    if constexpr (GATE) {
        if (tid == 64) {                                 // beside thread 0's serial top-k, on another wave
            const float z = s_logit[NE];
            gate[t] = (z / (1.0f + expf(-z))) / z;
        }
    }
    if (tid != 0) return;
    if (NE <= 8) {      // register arrays (constant indices after unrolling; the generic path keeps p / idx in scratch)
        moe_topk8<RAW>(s_logit, NE, NU, ids + t * NU, wts + t * NU);
        return;
    }
    float p[MOE_MAX_EXPERT];
    float mx = -INFINITY;
    for (int e = 0; e < NE; ++e) {
        p[e] = s_logit[e];
        mx = fmaxf(mx, p[e]);
    }
    double sum = 0.0;                                    // ggml_vec_soft_max_f32: ggml_float sum
    for (int e = 0; e < NE; ++e) { p[e] = expf(p[e] - mx); sum += (double)p[e]; }
    const float inv = (float)(1.0 / sum);
    for (int e = 0; e < NE; ++e) p[e] *= inv;
    int idx[MOE_MAX_EXPERT];
    for (int e = 0; e < NE; ++e) idx[e] = e;
    for (int j = 0; j < NU; ++j)                         // argsort descending (exchange order), first NU
        for (int k = j + 1; k < NE; ++k)
            if (p[idx[j]] < p[idx[k]]) { const int tmp = idx[j]; idx[j] = idx[k]; idx[k] = tmp; }
    if constexpr (RAW) {
        for (int j = 0; j < NU; ++j) {
            ids[t * NU + j] = idx[j];
            wts[t * NU + j] = p[idx[j]];
        }
        return;
    }
    double ws = 0.0;
    for (int j = 0; j < NU; ++j) ws += (double)p[idx[j]];
    const float wsum = (float)ws;
    for (int j = 0; j < NU; ++j) {
        ids[t * NU + j] = idx[j];
        wts[t * NU + j] = p[idx[j]] / wsum;
    }
}

__global__ void k_moe_gather(const float *__restrict__ src, int64_t lds, const int32_t *__restrict__ rows, int n,
                             int64_t E, float *__restrict__ dst) {
    const int i = blockIdx.y;
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && c < E) dst[(int64_t)i * E + c] = src[(int64_t)rows[i] * lds + c];
}

__global__ void k_moe_scatter(float *__restrict__ dst, int64_t ldd, const float *__restrict__ src,
                              const int32_t *__restrict__ rows, const float *__restrict__ w, int n, int64_t E) {
    const int i = blockIdx.y;
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && c < E) {
        const float v = src[(int64_t)i * E + c];
        dst[(int64_t)rows[i] * ldd + c] = w ? __fmul_rn(v, w[i]) : v;          // w null: plain row scatter
    }
}

// x[t] = ((slot0[t] + slot1[t]) + ...) + x[t]
__global__ void k_moe_combine(float *__restrict__ x, const float *__restrict__ slots, int64_t slot_stride, int nu,
                              int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float acc = slots[i];
    for (int j = 1; j < nu; ++j) acc = __fadd_rn(acc, slots[j * slot_stride + i]);
    x[i] = __fadd_rn(acc, x[i]);
}

// x[t][i] = (((slot0[t][i] + slot1[t][i]) + ...) + gate[t] * sh[t][i]) + x[t][i]: build_qwen2moe's
// ggml_add(moe_out, ggml_mul(ffn_shexp, gate)) then ggml_add(.., ffn_inp); workgroup row t, four floats per thread
__global__ void k_moe_combine_shexp(float *__restrict__ x, const float *__restrict__ slots, int64_t slot_stride, int nu,
                                    const float *__restrict__ gate, const float *__restrict__ sh, int64_t E) {
    const int64_t c = 4 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x);
    if (c >= E) return;
    const int64_t i = (int64_t)blockIdx.y * E + c;
    const float g = gate[blockIdx.y];
    float4 acc = *(const float4 *)(slots + i);
    for (int j = 1; j < nu; ++j) {
        const float4 v = *(const float4 *)(slots + j * slot_stride + i);
        acc = make_float4(__fadd_rn(acc.x, v.x), __fadd_rn(acc.y, v.y), __fadd_rn(acc.z, v.z), __fadd_rn(acc.w, v.w));
    }
    const float4 h = *(const float4 *)(sh + i), r = *(const float4 *)(x + i);
    acc = make_float4(__fadd_rn(acc.x, __fmul_rn(g, h.x)), __fadd_rn(acc.y, __fmul_rn(g, h.y)),
                      __fadd_rn(acc.z, __fmul_rn(g, h.z)), __fadd_rn(acc.w, __fmul_rn(g, h.w)));
    *(float4 *)(x + i) = make_float4(__fadd_rn(acc.x, r.x), __fadd_rn(acc.y, r.y), __fadd_rn(acc.z, r.z), __fadd_rn(acc.w, r.w));
}

// the _ex entry points' instance: router row type x raw weights x gate row type
struct RouteArgs {
    const float *x; int64_t ldx; const void *w; int K, NE, NU; int32_t *ids; float *wts;
    const float *nw; float eps; const void *gw; float *gate; int T; hipStream_t s;
};
template <int WT, bool NORM, bool RAW, int GT>
static void route_launch(const RouteArgs &a) {
    hipLaunchKernelGGL((k_moe_route<WT, NORM, RAW, GT>), dim3(a.T), dim3(256), 0, a.s, a.x, a.ldx, a.w, a.K, a.NE, a.NU, a.ids,
                       a.wts, a.nw, a.eps, a.gw, a.gate);
}
template <int WT, bool NORM, bool RAW>
static int route_gate(const RouteArgs &a, int gtype) {
    if (!a.gw) route_launch<WT, NORM, RAW, -1>(a);
    else if (gtype == KT_F32) route_launch<WT, NORM, RAW, KT_F32>(a);
    else if (gtype == KT_F16) route_launch<WT, NORM, RAW, KT_F16>(a);
    else return -3;
    return 0;
}
template <bool NORM>
static int route_ex(const RouteArgs &a, int wtype, int moe_norm_w, int gtype) {
    if (a.T <= 0) return 0;
    if (a.gw && !a.gate) return -1;
    int rc;
    if (wtype == KT_F16) rc = moe_norm_w ? route_gate<KT_F16, NORM, false>(a, gtype) : route_gate<KT_F16, NORM, true>(a, gtype);
    else if (wtype == KT_F32) rc = moe_norm_w ? route_gate<KT_F32, NORM, false>(a, gtype) : route_gate<KT_F32, NORM, true>(a, gtype);
    else return -3;
    if (rc) return rc;
    KCPP_CHECK(hipGetLastError());
    return 0;
}

extern "C" {

int kcpp_moe_route_ex(const float *x, int64_t ldx, const void *w_router, int wtype, int64_t K, int n_expert, int k,
                      int moe_norm_w, const void *w_gate, int gtype, int32_t *ids, float *weights, float *gate, int T,
                      void *stream) {
    if (n_expert < 1 || n_expert > MOE_MAX_EXPERT || k < 1 || k > n_expert) return -1;
    if (K % 4 || ldx % 4) return -1;                    // float4 / 4-half loads
    const RouteArgs a{x, ldx, w_router, (int)K, n_expert, k, ids, weights, nullptr, 0.0f, w_gate, gate, T, (hipStream_t)stream};
    return route_ex<false>(a, wtype, moe_norm_w, gtype);
}

int kcpp_moe_route_norm_ex(const float *x, int64_t ldx, const float *norm_w, float eps, const void *w_router, int wtype,
                           int64_t K, int n_expert, int k, int moe_norm_w, const void *w_gate, int gtype, int32_t *ids,
                           float *weights, float *gate, int T, void *stream) {
    if (n_expert < 1 || n_expert > 8 || k < 1 || k > n_expert || K > 4096 || K % 16 || ldx % 4) return -3;
    const RouteArgs a{x, ldx, w_router, (int)K, n_expert, k, ids, weights, norm_w, eps, w_gate, gate, T, (hipStream_t)stream};
    return route_ex<true>(a, wtype, moe_norm_w, gtype);
}

int kcpp_moe_combine_shexp(float *x, const float *slots, int64_t slot_stride, int k, const float *gate, const float *sh,
                           int64_t E, int T, void *stream) {
    if (T <= 0 || E <= 0) return 0;
    if (k < 1 || E % 4 || slot_stride % 4 || T > 65535) return -1;   // float4 rows; T is the grid's y
    hipLaunchKernelGGL(k_moe_combine_shexp, dim3((unsigned)((E / 4 + 255) / 256), T), dim3(256), 0, (hipStream_t)stream, x,
                       slots, slot_stride, k, gate, sh, E);
    KCPP_CHECK(hipGetLastError());
    return 0;
}

int kcpp_moe_route_norm(const float *x, int64_t ldx, const float *norm_w, float eps, const void *w_router, int wtype,
                        int64_t K, int n_expert, int k, int32_t *ids, float *weights, int T, void *stream) {
    if (n_expert < 1 || n_expert > 8 || k < 1 || k > n_expert || K > 4096 || K % 16 || ldx % 4) return -3;
    hipStream_t s = (hipStream_t)stream;
    if (wtype == KT_F16)
        hipLaunchKernelGGL((k_moe_route<KT_F16, true>), dim3(T), dim3(256), 0, s, x, ldx, w_router, (int)K, n_expert, k, ids,
                           weights, norm_w, eps);
    else if (wtype == KT_F32)
        hipLaunchKernelGGL((k_moe_route<KT_F32, true>), dim3(T), dim3(256), 0, s, x, ldx, w_router, (int)K, n_expert, k, ids,
                           weights, norm_w, eps);
    else
        return -3;
    KCPP_CHECK(hipGetLastError());
    return 0;
}

int kcpp_moe_route(const float *x, int64_t ldx, const void *w_router, int wtype, int64_t K, int n_expert, int k,
                   int32_t *ids, float *weights, int T, void *stream) {
    if (n_expert < 1 || n_expert > MOE_MAX_EXPERT || k < 1 || k > n_expert) return -1;
    if (K % 4 || ldx % 4) return -1;                    // float4 / 4-half loads
    hipStream_t s = (hipStream_t)stream;
    if (wtype == KT_F16)
        hipLaunchKernelGGL((k_moe_route<KT_F16, false>), dim3(T), dim3(256), 0, s, x, ldx, w_router, (int)K, n_expert, k, ids, weights);
    else if (wtype == KT_F32)
        hipLaunchKernelGGL((k_moe_route<KT_F32, false>), dim3(T), dim3(256), 0, s, x, ldx, w_router, (int)K, n_expert, k, ids, weights);
    else
        return -3;
    KCPP_CHECK(hipGetLastError());
    return 0;
}

int kcpp_moe_gather(const float *src, int64_t lds, const int32_t *rows, int n, int64_t E, float *dst, void *stream) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_moe_gather, dim3((unsigned)((E + 255) / 256), n), dim3(256), 0, (hipStream_t)stream, src, lds,
                       rows, n, E, dst);
    KCPP_CHECK(hipGetLastError());
    return 0;
}

int kcpp_moe_scatter(float *dst, int64_t ldd, const float *src, const int32_t *rows, const float *w, int n, int64_t E,
                     void *stream) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_moe_scatter, dim3((unsigned)((E + 255) / 256), n), dim3(256), 0, (hipStream_t)stream, dst, ldd,
                       src, rows, w, n, E);
    KCPP_CHECK(hipGetLastError());
    return 0;
}

int kcpp_moe_combine(float *x, const float *slots, int64_t slot_stride, int k, int64_t n, void *stream) {
    if (n <= 0) return 0;
    hipLaunchKernelGGL(k_moe_combine, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, slots,
                       slot_stride, k, n);
    KCPP_CHECK(hipGetLastError());
    return 0;
}

}  // extern "C"
