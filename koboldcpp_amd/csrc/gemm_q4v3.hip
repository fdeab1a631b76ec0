// gemm_q4v3.hip -- k_gemm_q4v3: Q4_K (both layouts), register-dequantized weights, LDS-DMA activation.
// Activation image: k_act_frag3 (gemm.hip).
#include "gemm_common.h"

// ================================================================ Q4_K GEMM v3
// Same exact-integer formulation and per-super-block epilogue as k_gemm_kq (bit-identical results: every
// integer partial sum is exact in fp32), re-tiled so the activation is read from L2 once per 128 weight
// rows instead of once per 64 and the weights never pass through LDS:
//   * workgroup = 128 tokens x 128 weight rows; wave w = rows [32w, 32w+32) x all 128 tokens (4 MFMA
//     32x32x16 tiles);
//   * A (activation, f16 integers) staged in LDS by global_load_lds (16 B per lane; the fragment images
//     are lane-linear, so the LDS-DMA writes them as they are read), two buffers: super-block sb+1's copy
//     is in flight while sb is multiplied, one barrier per super-block;
//   * B: each lane dequantizes its own weight row straight into MFMA fragments from raw Q4_K bytes
//     loaded one super-block ahead.  The k order inside a sub-block pair is permuted so that a lane's 8
//     k-values are the low and high nibbles of 4 consecutive qs bytes (one dword -> one fragment):
//       MFMA step s = 4p + st (p = sub-block pair, st = 0..3), lane half kg = lane >> 5, half e:
//       e < 4 : k = 64p + 16kg + 4st + e        (sub-block 2p, low nibble of qs byte 32p + 16kg + 4st + e)
//       e >= 4: k = 64p + 32 + 16kg + 4st + e-4 (sub-block 2p+1, high nibble of the same byte)
//     and k_act_frag3 writes A in the same order.

#ifndef V3_PRIO_DEF
#define V3_PRIO_DEF 1
#endif
constexpr bool V3_PRIO = V3_PRIO_DEF;

template <int BMT> struct Q4v3Smem {
    h8v a[2][BMT][16 * 64];   // activation fragments [buf][token tile][step * 64 + lane]   (16 KiB per tile)
    h8v bs[2][BMT][64];       // Q8_K bsum fragments  [buf][token tile][lane]
    float dy[2][32 * BMT];    // activation scale of the super-block per token [buf][token]
};

// one qs dword (4 bytes of a sub-block pair) -> fragment: 4 low nibbles * s0, 4 high nibbles * s1 (exact)
__device__ __forceinline__ h8v frag_q4v3(uint32_t w, float s0, float s1) {
    const uint32_t lo = w & 0x0F0F0F0Fu, hi = (w >> 4) & 0x0F0F0F0Fu;
    const _Float16 a = (_Float16)s0, ab = (_Float16)(-1024.0f * s0);
    const _Float16 b = (_Float16)s1, bb = (_Float16)(-1024.0f * s1);
    const h2v x0 = scale2(bias_lo(lo), a, ab), x1 = scale2(bias_hi(lo), a, ab);
    const h2v x2 = scale2(bias_lo(hi), b, bb), x3 = scale2(bias_hi(hi), b, bb);
    h8v r;
    r[0] = x0[0]; r[1] = x0[1]; r[2] = x1[0]; r[3] = x1[1]; r[4] = x2[0]; r[5] = x2[1]; r[6] = x3[0]; r[7] = x3[1];
    return r;
}

// grid: MT * ceil(N / 128) workgroups (MT = Mp / (32 BMT)), 64 NW threads, one workgroup per CU.
// Workgroup = 32 BMT tokens x 128 weight rows.  Wave w owns weight rows [32 (w % 4), +32) against the
// TPW = 4 BMT / NW token tiles [TPW (w / 4), +TPW): NW = 4 dequantizes every B fragment once per workgroup and
// feeds it to TPW MFMAs; NW = 8 (two waves per SIMD, so one wave's LDS reads and dequantization hide under the
// other's MFMAs) dequantizes each row twice.  BMT = 2 doubles the grid of small-N shapes (wo, q|k|v, down).
// (XCD-aware tile order: gemm_common.h xcd_tile)
template <int LAY, int NW, int BMT, int PF>
__global__ void __launch_bounds__(64 * NW, NW == 4 ? 2 : 1) k_gemm_q4v3(const uint8_t *__restrict__ W, int64_t K, int64_t N,
                                                         const h8v *__restrict__ af, const float *__restrict__ dyT,
                                                         const h8v *__restrict__ bsf, int64_t M, int64_t Mp, int MT,
                                                         float *__restrict__ Y, int64_t ldy, const float *res, int64_t ldr,
                                                         int KS, float *__restrict__ part, int XG) {
    constexpr int TPW = 4 * BMT / NW;         // token tiles per wave
    constexpr int SPW = 16 * BMT / NW;        // A staging: LDS-DMA steps per wave and super-block
    static_assert(TPW >= 1 && SPW >= 1, "tile shape");
    __shared__ Q4v3Smem<BMT> S;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave & 3, wt = wave >> 2;
    const int lr = lane & 31, kg = lane >> 5;
    // XCD-aware tile order (as k_gemm_kq): ids with equal id % 8 share a token tile when MT divides 8
    // KS > 1: split-K -- the grid is KS copies of the tile grid, copy `split` covers super-blocks
    // [split nsb / KS, (split + 1) nsb / KS) and writes its fp32 partial tile to part [KS][Mp][N]
    const int64_t nwg = gridDim.x / KS, id = blockIdx.x % nwg;
    const int split = (int)(blockIdx.x / nwg);
    int64_t mt, nt;
    xcd_tile(id, nwg, MT, (N + 127) / 128, XG, mt, nt);
    const int64_t m0 = mt * 32 * BMT, n0 = nt * 128;
    const int64_t nsb = K / 256, bpr = nsb;
    // this lane's weight row; clamped at N (its results are not stored)
    const int64_t nrow = min(n0 + 32 * wr + lr, N - 1);
    const uint8_t *hp, *qp;
    if constexpr (LAY == 1) {
        hp = W + nrow * 144 * bpr;
        qp = hp + 16 * bpr + 16 * kg;
    } else {
        hp = W + nrow * bpr * 144;
        qp = hp + 16 + 16 * kg;
    }
    constexpr int64_t HS = LAY == 1 ? 16 : 144, QS = LAY == 1 ? 128 : 144;   // bytes per super-block
    // LDS-DMA: wave w copies steps [SPW (w / BMT), +SPW) of token tile w % BMT (16 KiB per tile and
    // super-block); waves < BMT the bsum fragments of tile w; wave 0: dy (128 BMT bytes)
    const int stt = wave % BMT, st0 = SPW * (wave / BMT);
    const h8v *asrc = af + (m0 / 32 + stt) * (K / 16) * 64 + lane;
    const h8v *bsrc = bsf + (m0 / 32 + stt) * nsb * 64 + lane;
    const float *dsrc = dyT + m0 + 4 * lane;
    auto stage = [&](int buf, int64_t sb) {
#pragma unroll
        for (int st = 0; st < SPW; ++st) dma16(asrc + (16 * sb + st0 + st) * 64, &S.a[buf][stt][(st0 + st) * 64]);
        if (wave < BMT) dma16(bsrc + sb * 64, &S.bs[buf][stt][0]);
        if (wave == 0 && lane < 8 * BMT) dma16(dsrc + sb * Mp, &S.dy[buf][0]);
    };
    // raw weight super-blocks are loaded PF ahead into register sets X / Y (PF = 2: ping-pong, the loop unrolled
    // by two so each set stays in fixed registers); sb's set is copied out before it is refilled with sb + PF
    uint4 hX, qX[4], hY, qY[4];
    auto load_raw = [&](int64_t sb, uint4 &h, uint4 (&q)[4]) {
        h = ldg16(hp + HS * sb);
#pragma unroll
        for (int p = 0; p < 4; ++p) q[p] = ldg16(qp + QS * sb + 32 * p);
    };

    const int64_t sbb = nsb * split / KS, sbe = nsb * (split + 1) / KS;
    f16acc tot[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) tot[j][i] = 0.0f;
    stage(0, sbb);
    load_raw(sbb, hX, qX);
    if (PF == 2 && sbb + 1 < sbe) load_raw(sbb + 1, hY, qY);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    auto body = [&](int64_t sb, int buf, uint4 &hs, uint4 (&qs)[4]) {
        const uint4 hc = hs;
        uint32_t sc_lo, sc_hi, m_lo, m_hi;
        k4_all(hc, sc_lo, sc_hi, m_lo, m_hi);
        uint4 qc[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) qc[p] = qs[p];
#if KCPP_GEMM_PROBE != 1 && KCPP_GEMM_PROBE != 4
        if (sb + 1 < sbe) stage(buf ^ 1, sb + 1);
#endif
#if KCPP_GEMM_PROBE != 1 && KCPP_GEMM_PROBE != 5
        if (sb + PF < sbe) load_raw(sb + PF, hs, qs);
#endif
        f16acc acc[TPW];
#pragma unroll
        for (int j = 0; j < TPW; ++j)
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[j][i] = 0.0f;
        // 16 MFMA steps; the A fragments of step s+1 are read from LDS before step s's MFMAs are issued
        const h8v *abase = &S.a[buf][TPW * wt][lane];
        h8v an[TPW];
#pragma unroll
        for (int j = 0; j < TPW; ++j) an[j] = abase[j * 1024];
        int s0 = 0, s1 = 0;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            h8v ac[TPW];
#pragma unroll
            for (int j = 0; j < TPW; ++j) ac[j] = an[j];
            if (s + 1 < 16) {
#pragma unroll
                for (int j = 0; j < TPW; ++j) an[j] = abase[j * 1024 + (s + 1) * 64];
            }
            const int p = s >> 2, st = s & 3;
            if (st == 0) {                        // sub-blocks 2p, 2p+1: bytes 2(p&1), +1 of the low / high dword
                const uint32_t sdw = p < 2 ? sc_lo : sc_hi;
                s0 = (int)((sdw >> (16 * (p & 1))) & 0xFF);
                s1 = (int)((sdw >> (16 * (p & 1) + 8)) & 0xFF);
            }
            const h8v b = frag_q4v3(u4c(qc[p], st), (float)s0, (float)s1);
            if constexpr (V3_PRIO) __builtin_amdgcn_s_setprio(1);
#if KCPP_GEMM_PROBE == 2
#pragma unroll
            for (int j = 0; j < TPW; ++j) acc[j][0] += (float)ac[j][0] * (float)b[0];
#else
#pragma unroll
            for (int j = 0; j < TPW; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ac[j], b, acc[j], 0, 0, 0);
#endif
            if constexpr (V3_PRIO) __builtin_amdgcn_s_setprio(0);
        }
        // epilogue: tot -= dy * dmin * (sum_j m_j bsum_j), then tot += dy * (d * S)  (k_gemm_kq's order)
        h8v bm;                                   // mins of sub-blocks 4kg .. 4kg+3, each for its two 16-groups
        const uint32_t mdw = kg ? m_hi : m_lo;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const _Float16 mn = (_Float16)(float)((mdw >> (8 * e)) & 0xFF);
            bm[2 * e] = mn;
            bm[2 * e + 1] = mn;
        }
        const float dw = h2f((uint16_t)(hc.x & 0xFFFF)), dm = h2f((uint16_t)(hc.x >> 16));
#pragma unroll
        for (int j = 0; j < TPW; ++j) {
            const int tt = TPW * wt + j;
            float dyv[16];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 v = *(const float4 *)&S.dy[buf][32 * tt + 8 * q + 4 * kg];
                dyv[4 * q] = v.x; dyv[4 * q + 1] = v.y; dyv[4 * q + 2] = v.z; dyv[4 * q + 3] = v.w;
            }
            f16acc accm;
#pragma unroll
            for (int i = 0; i < 16; ++i) accm[i] = 0.0f;
            accm = __builtin_amdgcn_mfma_f32_32x32x16_f16(S.bs[buf][tt][lane], bm, accm, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 16; ++r) tot[j][r] = fmaf(-__fmul_rn(dyv[r], dm), accm[r], tot[j][r]);
#pragma unroll
            for (int r = 0; r < 16; ++r) tot[j][r] = fmaf(dyv[r], __fmul_rn(dw, acc[j][r]), tot[j][r]);
        }
        // the next super-block's A copy (and, PF = 2, its raw weights) must have landed; sb + 2's raw loads, issued
        // last, may stay in flight (loads retire in order)
        if (PF == 2 && sb + 2 < sbe) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#if KCPP_GEMM_PROBE != 3
        __syncthreads();
#endif
    };
    if constexpr (PF == 2) {
        int64_t sb = sbb;
        for (; sb + 1 < sbe; sb += 2) {
            body(sb, 0, hX, qX);
            __builtin_amdgcn_sched_barrier(0);
            body(sb + 1, 1, hY, qY);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (sb < sbe) body(sb, 0, hX, qX);
    } else {
        for (int64_t sb = sbb; sb < sbe; ++sb) body(sb, (int)((sb - sbb) & 1), hX, qX);
    }
    const int64_t n = n0 + 32 * wr + lr;
    if (n >= N) return;
#pragma unroll
    for (int j = 0; j < TPW; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t t = m0 + 32 * (TPW * wt + j) + (r & 3) + 8 * (r >> 2) + 4 * kg;
            if (KS > 1) part[((int64_t)split * Mp + t) * N + n] = tot[j][r];
            else if (t < M) Y[t * ldy + n] = res ? __fadd_rn(tot[j][r], res[t * ldr + n]) : tot[j][r];
        }
}

// grid: p.nwg = p.mt * ceil(N / 128) * p.ks workgroups of 64 p.waves threads; p.ks > 1 leaves partials in a.part
int gemm_q4v3_launch(const GemmPlan &p, const GemmArgs &a) {
#define KCPP_V3(L_, NW_, B_, PF_)                                                                                       \
    hipLaunchKernelGGL((k_gemm_q4v3<L_, NW_, B_, PF_>), dim3((unsigned)p.nwg), dim3(64 * NW_), 0, a.s,                  \
                       (const uint8_t *)a.W, a.K, a.N, (const h8v *)a.af, a.dy, (const h8v *)a.bsf, a.M, a.Mp, p.mt, a.Y, \
                       a.ldy, a.res, a.ldr, p.ks, a.part, p.xg)
#define KCPP_V3P(L_, NW_, B_) { if (p.pf == 2) KCPP_V3(L_, NW_, B_, 2); else KCPP_V3(L_, NW_, B_, 1); }
#define KCPP_V3B(L_, B_) { if (p.waves == 4) KCPP_V3P(L_, 4, B_) else KCPP_V3P(L_, 8, B_) }
    if (p.rs) { if (p.tile == 2) KCPP_V3B(1, 2) else KCPP_V3B(1, 4) }
    else { if (p.tile == 2) KCPP_V3B(0, 2) else KCPP_V3B(0, 4) }
#undef KCPP_V3B
#undef KCPP_V3P
#undef KCPP_V3
    KCPP_CHECK(hipGetLastError());
    return 0;
}
