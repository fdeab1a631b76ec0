// gemm_q80s.hip -- k_gemm_q80s2 + k_q80s_reduce: Q8_0 at M <= 32, weights streamed once at full bandwidth.
#include "gemm_common.h"

// ================================================================ Q8_0 small-batch GEMM (M <= 32)
// BASELINE config 3 (Llama-3-8B Q8_0, ubatch 32) is HBM-bound: the weights must stream at full bandwidth while
// only 32 tokens use them.  One v_mfma_i32_32x32x32_i8 per 32-block computes the exact integer block dot of
// ggml_vec_dot_q8_0_q8_0 (ggml-quants.c:5519) straight from the raw int8 weight and activation bytes (no
// dequantization, no LDS operand staging); the block result is scaled sumi * (d_w * d_x) in fp32 as the
// scalar CPU path does.  Workgroup = 128 weight rows (wave: 32 rows x the 32 tokens) x one K range; S K ranges
// per row tile give >= ~384 workgroups, their fp32 partials [S][32][N] are summed in split order by
// k_q80s_reduce (deterministic), which also applies the residual or silu(g) * u.
// (the K ranges: gemm_plan.h gemm_ks_q80s)

// The small-batch Q8_0 GEMM: the weight tile streams through LDS in row-contiguous pieces (a first version's direct
// fragment loads touched 32 rows x 32 B per wave instruction, 32 cache lines for 1 KiB; removed); every LDS-DMA wave
// instruction reads 64 / (2 CH) rows x 32 CH bytes (CH blocks of each row) into an XOR-swizzled [row][32 CH B] image
// (16-B piece c of row n at slot c ^ (n % 2CH)), double-buffered by CH-block chunks with the activation chunk beside
// it; CH = 4 (40 KiB of LDS: three workgroups per CU keep more weight bytes in flight than CH = 8 at one).  Same block math and
// split-K partials.
// CH blocks per chunk (4: 40 KiB of LDS, three workgroups per CU)
#ifndef Q80_CH
#define Q80_CH 4
#endif
#ifndef Q80_ST
#define Q80_ST 2        // ring depth; 3 measured slower on config 3 (6.51k vs 6.71k tok/s: 2 instead of 3 workgroups per CU)
#endif
struct Q80s2Smem {
    uint8_t w[Q80_ST][128 * 32 * Q80_CH];  // weight chunk [stage][row][32 CH B] (swizzled 16-B pieces)
    i32x4 a[Q80_ST][Q80_CH][64];           // activation fragments [stage][block][lane]
    float dx[48 * 32];                     // token scales of the split's blocks [block][token] (q80s_splits: <= 48 blocks)
};

__global__ void __launch_bounds__(256) k_gemm_q80s2(const Q80Segs sg, int64_t K, int64_t N,
                                                   const uint8_t *__restrict__ act, int64_t M, float *__restrict__ part) {
    __shared__ Q80s2Smem S;
    float *sdx = S.dx;        // static LDS: the compiler can tell it from the DMA targets (a dynamic array made it
                              // wait for every outstanding LDS-DMA before each read of a token scale)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 31, kg = lane >> 5;
    const int64_t nb = K / 32, S_ = gridDim.y;
    const int64_t bps = (nb + S_ - 1) / S_, b0 = (int64_t)blockIdx.y * bps, b1 = std::min<int64_t>(nb, b0 + bps);
    const int64_t nt0 = (int64_t)blockIdx.x * 128;
    const int seg = (sg.nseg > 1 && nt0 >= sg.N[0]) ? ((sg.nseg > 2 && nt0 >= sg.N[0] + sg.N[1]) ? 2 : 1) : 0;
    const int64_t soff = seg == 0 ? 0 : (seg == 1 ? sg.N[0] : sg.N[0] + sg.N[1]);
    const int64_t Ns = seg == 0 ? sg.N[0] : (seg == 1 ? sg.N[1] : sg.N[2]);
    const uint8_t *W = seg == 0 ? sg.W[0] : (seg == 1 ? sg.W[1] : sg.W[2]);
    const uint16_t *dwp = (const uint16_t *)(W + Ns * nb * 32);
    const int64_t trow = std::min<int64_t>(lr, M - 1);
    const int8_t *qx = (const int8_t *)act + trow * K + 16 * kg;
    const float *dx = (const float *)(act + M * K);
    // weight LDS-DMA: a wave instruction covers RPI rows of 2 CH pieces (16 B per lane); lane -> (row, slot)
    constexpr int PPR = 2 * Q80_CH, RPI = 64 / PPR, IPW = 128 / RPI / 4;   // pieces per row, rows / instr, instr / wave
    const int wsub = lane / PPR, wslot = lane % PPR;
    auto stage = [&](int buf, int64_t cb) {                      // chunk = blocks [cb, cb + CH)
#pragma unroll
        for (int i = 0; i < IPW; ++i) {
            const int rl = RPI * (IPW * wave + i) + wsub;        // local row 0..127
            const int64_t row = std::min<int64_t>(nt0 - soff + rl, Ns - 1);
            const int piece = wslot ^ (rl % PPR);                // the 16-B piece this LDS slot holds
            const int64_t blk = std::min<int64_t>(cb + (piece >> 1), b1 - 1);
            dma16(W + (row * nb + blk) * 32 + 16 * (piece & 1), &S.w[buf][(IPW * wave + i) * 1024]);
        }
        if (wave < Q80_CH) dma16(qx + std::min<int64_t>(cb + wave, b1 - 1) * 32, &S.a[buf][wave][0]);
    };
    for (int64_t i = tid; i < (b1 - b0) * 32; i += 256) {
        const int64_t b = i >> 5, t = i & 31;
        sdx[i] = t < M ? dx[t * nb + b0 + b] : 0.0f;
    }
    float tot[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) tot[r] = 0.0f;
    const int nl = 32 * wave + lr;                               // this lane's B row within the tile
    const int64_t nrow = std::min<int64_t>(nt0 - soff + nl, Ns - 1);
    // Q80_ST-stage ring: chunk i in stage i % Q80_ST, issued Q80_ST - 1 chunks ahead
#pragma unroll
    for (int q = 0; q < Q80_ST - 1; ++q)
        if (b0 + q * Q80_CH < b1) stage(q, b0 + q * Q80_CH);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int64_t cb = b0; cb < b1; cb += Q80_CH) {
        const int ci = (int)((cb - b0) / Q80_CH);
        const int buf = ci % Q80_ST;
        const bool ahead = cb + (Q80_ST - 1) * Q80_CH < b1;
        // the weight block scales (plain global loads) are taken -- and waited for -- BEFORE the next chunk's LDS-DMA
        // goes out: the compiler does not see the DMA, so the vmcnt it places in front of the first use of a scale
        // would otherwise also wait for the whole prefetch and expose its latency every chunk
        float dwv[Q80_CH];
#pragma unroll
        for (int u = 0; u < Q80_CH; ++u) dwv[u] = h2f(dwp[nrow * nb + std::min<int64_t>(cb + u, b1 - 1)]);
#pragma unroll
        for (int u = 0; u < Q80_CH; ++u) asm volatile("" ::"v"(dwv[u]));
        if (ahead) stage((ci + Q80_ST - 1) % Q80_ST, cb + (Q80_ST - 1) * Q80_CH);
#pragma unroll
        for (int u = 0; u < Q80_CH; ++u) {
            if (cb + u >= b1) break;
            const int piece = 2 * u + kg;
            const i32x4 wv = *(const i32x4 *)&S.w[buf][nl * 32 * Q80_CH + ((piece ^ (nl % PPR)) * 16)];
            i32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0;
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(S.a[buf][u][lane], wv, acc, 0, 0, 0);
            const float *sd = sdx + (cb + u - b0) * 32;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 d4 = *(const float4 *)(sd + 8 * q + 4 * kg);
                const float dv[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    tot[4 * q + e] = __fadd_rn(tot[4 * q + e], __fmul_rn((float)acc[4 * q + e], __fmul_rn(dwv[u], dv[e])));
            }
        }
        // chunk ci + 1 must have landed; with three stages chunk ci + 2 (issued this iteration, last) may stay in flight
        if (Q80_ST == 3 && ahead) {
            static_assert(Q80_ST != 3 || (128 / (64 / (2 * Q80_CH)) / 4 == 4 && Q80_CH == 4), "vmcnt below: 4 + 1 per stage");
            asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
    }
    const int64_t n = nt0 + nl;
    if (n >= N) return;
    float *pp = part + (int64_t)blockIdx.y * 32 * N + n;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int t = (r & 3) + 8 * (r >> 2) + 4 * kg;
        pp[(int64_t)t * N] = tot[r];
    }
}

// Y[t][n] = sum_s part[s][t][n] (+ res), or silu(sum_s g) * (sum_s u) with u partials in part2
__global__ void k_q80s_reduce(const float *__restrict__ part, const float *__restrict__ part2, int S, int64_t M,
                              int64_t N, float *__restrict__ Y, int64_t ldy, const float *res, int64_t ldr,
                              uint8_t *__restrict__ qout = nullptr) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * N) return;                            // N % 32 == 0 with qout: whole 32-lane blocks retire together
    const int64_t t = i / N, n = i % N;
    float g = part[t * N + n];
    for (int s = 1; s < S; ++s) g = __fadd_rn(g, part[((int64_t)s * 32 + t) * N + n]);
    if (part2) {
        float u = part2[t * N + n];
        for (int s = 1; s < S; ++s) u = __fadd_rn(u, part2[((int64_t)s * 32 + t) * N + n]);
        const float h = (g / (1.0f + expf(-g))) * u;
        if (!qout) {
            Y[t * ldy + n] = h;
            return;
        }
        // h quantized to Q8_0 for the down projection, as k_quant_q80: one 32-lane group per block
        float am = fabsf(h);
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) am = fmaxf(am, __shfl_xor(am, o, 32));
        const float id = (am != 0.0f) ? 127.f / am : 0.0f;
        int q = (int)rintf(__fmul_rn(h, id));
        q = q > 127 ? 127 : (q < -128 ? -128 : q);
        int sq = q;
#pragma unroll
        for (int o = 1; o < 32; o <<= 1) sq += __shfl_xor(sq, o, 32);
        const int64_t nb = N / 32, b = t * nb + n / 32;
        ((int8_t *)qout)[t * N + n] = (int8_t)q;
        if ((n & 31) == 0) {
            ((float *)(qout + M * N))[b] = h2f(f2h(am / 127.f));
            ((int16_t *)(qout + M * N + M * nb * 4))[b] = (int16_t)sq;
        }
    } else {
        Y[t * ldy + n] = res ? __fadd_rn(g, res[t * ldr + n]) : g;
    }
}

int gemm_q80s_run(Q80Segs sg, const void *W2, int64_t K, int64_t N, const void *act, int64_t M, float *Y, int64_t ldy,
                  const float *res, int64_t ldr, int mode, uint8_t *qout, float *part, hipStream_t s) {
    const int S = gemm_ks_q80s(K, N);
    float *part2 = part + (int64_t)S * 32 * N;
    const dim3 grid((unsigned)((N + 127) / 128), (unsigned)S);
    auto q80 = [&](float *pt) {
        hipLaunchKernelGGL(k_gemm_q80s2, grid, dim3(256), 0, s, sg, K, N, (const uint8_t *)act, M, pt);
    };
    q80(part);
    KCPP_CHECK(hipGetLastError());
    if (mode == 1) {
        sg.W[0] = (const uint8_t *)W2;
        q80(part2);
        KCPP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_q80s_reduce, dim3((unsigned)((M * N + 255) / 256)), dim3(256), 0, s, part, mode == 1 ? part2 : nullptr,
                       S, M, N, Y, ldy, mode == 1 ? nullptr : res, ldr, qout);
    KCPP_CHECK(hipGetLastError());
    return 0;
}
