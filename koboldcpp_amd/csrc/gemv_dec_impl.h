// gemv_dec_impl.h -- the single-token decode mat-vec with its neighbours fused in.
// Included once per quant type by gemv_dec_<type>.hip (parallel compilation).
//
// The reference runs, per layer, rms_norm -> mul -> quantize_q8_1 -> mul_mat_vec_q (x3) -> rope (x2)
// -> cpy K/V into the cache as separate ggml nodes, each a kernel launch (ggml-cuda.cu:2145-2349,
// norm.cu:101, quantize.cu:4, mmvq.cu:50, rope.cu:31, cpy.cu:34).  On MI355X a decode token is
// launch/latency bound before it is bandwidth bound, so one launch here does:
//   prologue  (PRO=1) rms_norm(x)*w -> Q8_K (or Q8_0) activation, computed per workgroup into LDS
//             while the workgroup's first weight loads are already in flight;  (PRO=2) quantize
//             only (ffn_down input);  (PRO=0) activation already quantized in global memory.
//   body      up to three weight segments of one quant type (e.g. wq|wk|wv), R rows per wave,
//             the same integer unit dots as gemv.hip (CPU vec_dot semantics).
//   epilogue  MODE 0: y (+ residual);  MODE 1: silu(gate)*up;  MODE 2: RoPE (table built exactly
//             like ggml_rope_cache_init) + f16 store of q, and of K/V straight into the cache.
#pragma once
#include "gemv_units.h"
#include "kcpp_internal.h"

#include <algorithm>
#include <cstdlib>



__device__ __forceinline__ float wave_sum_dpp(float v) {
    v += dpp_f<0xB1>(v);
    v += dpp_f<0x4E>(v);
    v += dpp_f<0x141>(v);
    v += dpp_f<0x140>(v);
    return xsum32(xsum16(v));
}

// Q8_0 quantization (AVX2 quantize_row_q8_0, ggml-quants.c:940-1000) of 16 elements held by one lane,
// two lanes per 32-block.  Writes qs (16 B), and lane-even writes d (f16-rounded, as float) and asum.
__device__ __forceinline__ void q80_quant16(const float (&v)[16], int l16, int8_t *qs16, float *dblk, int16_t *sblk) {
    float am = 0.0f;
#pragma unroll
    for (int e = 0; e < 16; ++e) am = fmaxf(am, fabsf(v[e]));
    am = fmaxf(am, dpp_f<0xB1>(am));                 // partner lane (xor 1) holds the other half
    const float d = am / 127.f;
    const float id = (am != 0.0f) ? 127.f / am : 0.0f;
    int q[16], s = 0;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int iv = (int)rintf(__fmul_rn(v[e], id));
        q[e] = iv > 127 ? 127 : (iv < -128 ? -128 : iv);
        s += q[e];
    }
    s += dpp_i<0xB1>(s);
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        w[k] = (uint32_t)(q[4 * k] & 0xFF) | ((uint32_t)(q[4 * k + 1] & 0xFF) << 8) |
               ((uint32_t)(q[4 * k + 2] & 0xFF) << 16) | ((uint32_t)(q[4 * k + 3] & 0xFF) << 24);
    *(uint4 *)qs16 = make_uint4(w[0], w[1], w[2], w[3]);
    if ((l16 & 1) == 0) { *dblk = h2f(f2h(d)); *sblk = (int16_t)s; }
}

// activation prologue into LDS: layout identical to the global act buffer with M = 1.
// Single pass: each thread keeps its <= MAXC chunks of 16 inputs in registers across the
// sum-of-squares block reduction (rms_norm, ggml.c:12059-12103) and the quantization.
template <int VT, int PRO, int MAXC>
__device__ __forceinline__ void prologue(const DecArgs &a, uint8_t *lds) {
    // MAXC chunks of 16 per thread: K <= 256 * 16 * MAXC
    const int tid = threadIdx.x;
    const int64_t K = a.K;
    const int nchunk = (int)(K / 16);
    float v[MAXC][16];
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
        const int c = tid + 256 * i;
        if (c < nchunk) {
            const float4 *p = (const float4 *)(a.x + 16 * (int64_t)c);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 f = p[k];
                v[i][4 * k] = f.x; v[i][4 * k + 1] = f.y; v[i][4 * k + 2] = f.z; v[i][4 * k + 3] = f.w;
            }
        }
    }
    if constexpr (PRO == 1) {
        double ss = 0.0;
#pragma unroll
        for (int i = 0; i < MAXC; ++i)
            if (tid + 256 * i < nchunk) {
#pragma unroll
                for (int e = 0; e < 16; ++e) ss += (double)__fmul_rn(v[i][e], v[i][e]);
            }
        ss = wave_sum_d(ss);
        __shared__ double red[4];
        if ((tid & 63) == 0) red[tid >> 6] = ss;
        __syncthreads();
        const double sum = red[0] + red[1] + red[2] + red[3];
        const float mean = (float)(sum / (double)K);
        const float scale = 1.0f / sqrtf(mean + a.eps);   // ggml.c:12089
#pragma unroll
        for (int i = 0; i < MAXC; ++i) {
            const int c = tid + 256 * i;
            if (c < nchunk) {
                const float4 *wp = (const float4 *)(a.nw + 16 * (int64_t)c);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float4 f = wp[k];
                    v[i][4 * k] = __fmul_rn(__fmul_rn(v[i][4 * k], scale), f.x);
                    v[i][4 * k + 1] = __fmul_rn(__fmul_rn(v[i][4 * k + 1], scale), f.y);
                    v[i][4 * k + 2] = __fmul_rn(__fmul_rn(v[i][4 * k + 2], scale), f.z);
                    v[i][4 * k + 3] = __fmul_rn(__fmul_rn(v[i][4 * k + 3], scale), f.w);
                }
            }
        }
    }
    int8_t *qs = (int8_t *)lds;
    float *d = (float *)(lds + K);
    int16_t *bs = (int16_t *)(lds + K + (VT == KT_Q8_K ? K / 256 : K / 32) * 4);
#pragma unroll
    for (int i = 0; i < MAXC; ++i) {
        const int c = tid + 256 * i;
        if (c < nchunk) {                          // uniform per aligned 16-lane group
            if constexpr (VT == KT_Q8_K) {
                const int sb = c >> 4;
                q8k_quant16(v[i], c & 15, qs + sb * 256, d + sb, bs + sb * 16);
            } else {
                q80_quant16(v[i], c & 15, qs + 16 * c, d + (c >> 1), bs + (c >> 1));
            }
        }
    }
    __syncthreads();
}

// copy an already-quantized global activation (M = 1) into LDS (PRO == 0)
__device__ __forceinline__ void act_to_lds(const uint8_t *__restrict__ act, uint8_t *lds, int64_t bytes) {
    for (int64_t i = (int64_t)threadIdx.x * 16; i < bytes; i += (int64_t)blockDim.x * 16) {
        if (i + 16 <= bytes) *(uint4 *)(lds + i) = *(const uint4 *)(act + i);
        else for (int64_t j = i; j < bytes; ++j) lds[j] = act[j];
    }
    __syncthreads();
}

// Persistent-style: each wave walks row groups g = wave_id, wave_id + n_waves, ...  All K-slices
// (IT = ceil(units_per_row / 64)) of a group's R rows are loaded at once, and the loads of group
// g + n_waves are issued before group g is computed (two register buffers), so a wave keeps
// 2 x IT x R units (48-80 B each per lane) in flight.
template <int TYPE, int R, int MODE, int PRO, int MC, int IT>
__global__ void __launch_bounds__(256) k_gemv_dec(const DecArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_act[];
    const int KB_BID = (int)blockIdx.x, KB_NBLK = (int)gridDim.x;
#define KB_ARGS a
#include "gemv_dec_body.inc"
#undef KB_ARGS
}

// The built instances (R, MODE, PRO, MC), each at IT 1 / 2 / 4 (PRO 2: 2 / 4 / 8): what the plan's GEMV_UNIT rules name
// (gemv_plan.h), nothing else
#define KCPP_UNIT_INSTANCES(X)                                                                                        \
    X(2, 2, 1, 1) X(2, 2, 1, 2) X(2, 1, 1, 1) X(2, 1, 1, 2) X(1, 1, 1, 1) X(1, 1, 1, 2) X(4, 0, 0, 1) X(2, 0, 0, 1)    \
    X(1, 0, 0, 1) X(2, 0, 1, 1) X(2, 0, 1, 2) X(1, 0, 1, 1) X(1, 0, 1, 2) X(1, 0, 2, 2) X(1, 0, 2, 4) X(1, 0, 2, 8)

template <int TYPE>
int gemv_unit_launch(const GemvPlan &p, const DecArgs &a, hipStream_t s) {
    void (*k)(const DecArgs) = nullptr;
#define KCPP_UNIT_PICK(R_, MODE_, PRO_, MC_)                                                                          \
    if (p.R == R_ && p.mode == MODE_ && p.pro == PRO_ && p.MC == MC_) {                                               \
        constexpr int I0 = PRO_ == 2 ? 2 : 1;                                                                         \
        if (p.IT == I0) k = k_gemv_dec<TYPE, R_, MODE_, PRO_, MC_, I0>;                                               \
        if (p.IT == 2 * I0) k = k_gemv_dec<TYPE, R_, MODE_, PRO_, MC_, 2 * I0>;                                       \
        if (p.IT == 4 * I0) k = k_gemv_dec<TYPE, R_, MODE_, PRO_, MC_, 4 * I0>;                                       \
    }
    KCPP_UNIT_INSTANCES(KCPP_UNIT_PICK)
#undef KCPP_UNIT_PICK
    void *args[] = {(void *)&a};
    return gemv_go(p.type == TYPE ? (const void *)k : nullptr, p.nblk, p.block, p.lds_bytes, args, s);
}
