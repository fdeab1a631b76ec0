// gemm_q4v4.hip -- k_gemm_q4v4 (v4 / v5): Q4_K and Q5_K on the int8 matrix cores straight from the Q8_K activation
// (no activation image), plain, one-launch GLU and grouped (MoE prefill).
#include "gemm_common.h"

// ================================================================ Q4_K GEMM v4 (int8 matrix cores)
// v3 is bound by moving operands, not by the matrix cores (probes at M = 512, gate|up 4096 x 28672: 266 us, 142 us
// with the in-loop loads removed, 216 us with the MFMAs removed): its f16 activation image is twice the Q8_K bytes
// and every weight row is loaded by two waves one super-block ahead.  v4 multiplies the Q8_K bytes themselves on
// v_mfma_i32_32x32x32_i8, one MFMA per 32-element sub-block and token tile, with an exact int32 accumulator:
//   sum_k q*sc*a = 8 * sum_k (q*(sc>>3))*a + sum_k (q*(sc&7))*a,  q*(sc>>3), q*(sc&7) <= 105 (int8),
// so each sub-block takes two MFMAs into acc_h / acc_l and isum = 8 acc_h + acc_l is the CPU's int32 sumi exactly
// (v3 holds the same integer in fp32); the per-super-block epilogue is v3's, so the results are bit-identical.
// Operands are staged with LDS-DMA straight from the Q8_K buffer (no fragment-image kernel): per super-block the
// workgroup's 128 token rows x 256 B of int8, their bsums and scales, and its 128 weight rows' 144 B, the weights
// in a 3-stage ring two super-blocks ahead (HBM latency), the activations double-buffered one ahead (L2 hits).
// Workgroup = 128 tokens x 128 weight rows, 8 waves; wave w: weight rows 32 (w & 3) .. +32 x token tiles
// 2 (w >> 2), +1.  Fragment k order: lane half g of token / weight row r holds bytes 16g .. 16g+15 of the
// sub-block (any order common to both operands is exact); the Q4_K byte j of pair p holds element j of sub-block
// 2p (low nibble) and 2p+1 (high nibble).
// Swizzled LDS images: one LDS-DMA instruction (64 lanes x 16 B, lane-linear in LDS) fetches 8 rows x 8 chunks of
// 16 B -- one 128-B line per row (a fragment-ordered fetch touches 32 lines per instruction) -- lane j: row
// 8k + (j & 7), chunk 8h + (j >> 3), at slot 72 (4h + k) + j (72: rows 8 apart start 8 slots apart mod 16, so the
// 16-lane groups of a fragment read hit 16 distinct bank quads: conflict-free).  Chunk c of row m of a 32-row tile:
// slot 72 (4 (c >> 3) + (m >> 3)) + (m & 7) + 8 (c & 7).
// (swz: gemm_common.h)

// TPW = 2 (v4): 4 row tiles (128 rows) x 2 token halves, 3 weight stages; TPW = 4 (v5): 8 row tiles (256 rows), every
// wave against all 4 token tiles, so each dequantized weight fragment feeds twice the MFMAs; 2 weight stages (LDS).
// Slot counts: the highest swizzled slot + 1 (activations 16 chunks: 568, weights 8 chunks: 280).
template <int WR, int NST> struct Q4v4Smem {
    i32x4 a[2][4][568];      // [buf][token tile][swz(row, chunk)]: 16 activation bytes, chunks 0..15 of the 256
    i32x4 bs[2][4][64];      // [buf][token tile][lane]: 8 bsums (int16) of the lane half's 128 elements
    float dy[2][128];        // [buf][token]: Q8_K scale of the super-block
    uint4 wh[NST][WR][32];   // [stage][row tile][row]: Q4_K header (d, dmin, 12 B scales / mins)
    i32x4 wq[NST][WR][280];  // [stage][row tile][swz(row, chunk)]: qs chunks 0..7 (pair p, half g: chunk 2p + g)
};
// Q5_K adds the fifth bits: qh bytes 16 g .. 16 g + 15 of row r (bit j = sub-block j) at slot 32 g + r
template <int WR, int NST> struct Q5v4Smem : Q4v4Smem<WR, NST> {
    i32x4 wqh[NST][WR][64];  // [stage][row tile][32 g + row]
};

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
// bytes of x (each <= 15) times s (<= 7), per byte: two 16-bit lanes, no carry out of a byte (v_pk_mul_lo_u16;
// the scalar factor is taken for both halves by op_sel)
__device__ __forceinline__ int mulb(uint32_t x, uint32_t s) {
    const u16x2 f = {(unsigned short)s, (unsigned short)s};
    return (int)__builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, x) * f);
}

// Q5_K (TYPE = KT_Q5_K, TPW = 2 only -- the qh stages do not fit v5's LDS): q = lo + 16 hb, lo <= 15, hb <= 1, so
//   sum_k q*sc*a = 8 (sum_k (lo*(sc>>3))*a + sum_k (hb*2sc)*a) + sum_k (lo*(sc&7))*a,  hb*2sc <= 126,
// a third MFMA per sub-block, into acc_h; isum = 8 acc_h + acc_l is again the CPU's exact int32 sumi
// (ggml_vec_dot_q5_K_q8_K, ggml-quants.c), and the epilogue is unchanged.
template <int TYPE, int LAY, int TPW>
// GLU: W2 / Y2 set -- the grid's second half computes the up matrix into Y2 (one launch for both: twice the
// workgroups on the small expert grids, no second ramp; every tile's arithmetic unchanged).
// Grouped (MoE prefill, gcnt set, KS = 1): act holds gne groups of token rows back to back (Q8_K planes of M rows in
// all), group e = gcnt[e] rows against weight matrix W + e wstride; the grid is every group's tile grid in order,
// each group's outputs at its first row of Y (and Y2).
__global__ void __launch_bounds__(512, 1) k_gemm_q4v4(const uint8_t *__restrict__ W, int64_t K, int64_t N,
                                                     const uint8_t *__restrict__ act, int64_t M, int64_t Mp, int MT,
                                                     float *__restrict__ Y, int64_t ldy, const float *res, int64_t ldr,
                                                     int KS, float *__restrict__ part, int XG, const uint8_t *W2,
                                                     float *Y2, int64_t ldy2, const int32_t *gcnt, int gne,
                                                     int64_t wstride) {
    constexpr int WT = 4 / TPW, WR = 8 / WT, NR = 32 * WR, NST = TPW == 2 ? 3 : 2, NI = WR / 2;
    constexpr bool Q5 = TYPE == KT_Q5_K;
    static_assert(TYPE == KT_Q4_K || (Q5 && TPW == 2), "v4 int8 GEMM: Q4_K (TPW 2 / 4) or Q5_K (TPW 2)");
    __shared__ std::conditional_t<Q5, Q5v4Smem<WR, NST>, Q4v4Smem<WR, NST>> S;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave % WR, wt = wave / WR;
    const int lr = lane & 31, kg = lane >> 5;
    const int64_t per = W2 ? gridDim.x / 2 : gridDim.x;       // workgroups per matrix
    const bool second = blockIdx.x >= per;
    int64_t bid = second ? blockIdx.x - per : blockIdx.x;
    if (second) { W = W2; Y = Y2; ldy = ldy2; res = nullptr; }
    const int64_t nsb = K / 256, bpr = nsb;
    const int8_t *qs = (const int8_t *)act;
    const float *dq = (const float *)(act + M * K);
    const int16_t *bsq = (const int16_t *)(act + M * K + M * nsb * 4);
    int64_t nwg = per / KS;
    if (gcnt) {                 // uniform scan for this workgroup's group (<= 64 groups)
        const int64_t ntn = (N + NR - 1) / NR;
        int64_t t0 = 0, r0 = 0;
        int e = 0;
        for (; e < gne; ++e) {
            const int64_t te = (gcnt[e] + 127) / 128 * ntn;
            if (bid < t0 + te) break;
            t0 += te;
            r0 += gcnt[e];
        }
        if (e >= gne) return;
        bid -= t0;
        W += e * wstride;
        Y += r0 * ldy;
        qs += r0 * K;
        dq += r0 * nsb;
        bsq += r0 * (K / 16);
        M = gcnt[e];
        MT = (int)((M + 127) / 128);
        nwg = MT * ntn;
    }
    const int64_t id = bid % nwg;
    const int split = (int)(bid / nwg);
    int64_t mt, nt;
    xcd_tile(id, nwg, MT, (N + NR - 1) / NR, XG, mt, nt);
    const int64_t m0 = mt * 128, n0 = nt * NR;
    // DMA assignments (per super-block): A: token tile wave & 3, sub-blocks 4 (wave >> 2) .. +4; bsums: waves 0-3
    // (tile = wave); dy: waves 4, 5 (tokens 64 (wave - 4) .. +64); weights: NI groups of 8 rows, group i = 8u + wave
    // (row tile i >> 2, rows 8 (i & 3) ..); headers: waves 0 .. NI - 1 (row tiles 2 wave + (lane >> 5))
    // A: token tile wave & 3, chunk half wave >> 2, row groups 0..3; lane: row 8k + (lane & 7), chunk 8h + (lane >> 3)
    const int att = wave & 3, ah8 = wave >> 2;
    const int8_t *arow = qs + min(m0 + 32 * att + (lane & 7), M - 1) * K + 16 * (8 * ah8 + (lane >> 3));
    const int16_t *bsrow = bsq + min(m0 + 32 * wave + lr, M - 1) * (K / 16) + 8 * kg;
    const float *dyrow = dq + min(m0 + 64 * max(wave - 4, 0) + lane, M - 1) * nsb;
    // bytes per super-block and row: Q4_K 144 (header 16, qs 128), Q5_K 176 (header 16, qh 32, qs 128); LAY 1 keeps
    // each row's headers, qs and (Q5_K) qh as planes: [nsb][16] ++ [nsb][128] ++ [nsb][32]
    constexpr int64_t BPB = Q5 ? 176 : 144;
    constexpr int64_t HS = LAY == 1 ? 16 : BPB, QS = LAY == 1 ? 128 : BPB, QHS = LAY == 1 ? 32 : BPB;
    const int64_t qoff = LAY == 1 ? 16 * bpr : (Q5 ? 48 : 16), qhoff = LAY == 1 ? 144 * bpr : 16;
    const uint8_t *wq0[NI];
#pragma unroll
    for (int u = 0; u < NI; ++u) {
        const int i = 8 * u + wave;
        const int64_t row = min(n0 + 32 * (i >> 2) + 8 * (i & 3) + (lane & 7), N - 1);
        wq0[u] = W + row * BPB * bpr + qoff + 16 * (lane >> 3);
    }
    const int hrt = 2 * wave + kg;
    const int64_t hrow = min(n0 + 32 * hrt + lr, N - 1);
    const uint8_t *wh0 = W + hrow * BPB * bpr;
    // qh (Q5_K): waves 4 .. 7, row tile wave - 4, lane = 32 g + row
    const uint8_t *wqh0 = W + min(n0 + 32 * max(wave - 4, 0) + lr, N - 1) * BPB * bpr + qhoff + 16 * kg;
    auto stage_a = [&](int buf, int64_t sb) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            dma16(arow + (int64_t)min(8 * k, (int)max<int64_t>(M - 1 - (m0 + 32 * att + (lane & 7)), 0)) * K + sb * 256,
                  &S.a[buf][att][72 * (4 * ah8 + k)]);
        if (wave < 4) dma16(bsrow + sb * 16, &S.bs[buf][wave][0]);
        else if (wave < 6) dma4(dyrow + sb, &S.dy[buf][64 * (wave - 4)]);
    };
    auto stage_w = [&](int st, int64_t sb) {
#pragma unroll
        for (int u = 0; u < NI; ++u) {
            const int i = 8 * u + wave;
            dma16(wq0[u] + QS * sb, &S.wq[st][i >> 2][72 * (i & 3)]);
        }
        if (wave < NI) dma16(wh0 + HS * sb, &S.wh[st][2 * wave][0]);
        if constexpr (Q5)
            if (wave >= 4) dma16(wqh0 + QHS * sb, &S.wqh[st][wave - 4][0]);
    };

    const int64_t sbb = nsb * split / KS, sbe = nsb * (split + 1) / KS;
    f16acc tot[TPW];
#pragma unroll
    for (int j = 0; j < TPW; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) tot[j][i] = 0.0f;
    stage_a(0, sbb);
#pragma unroll
    for (int q = 0; q < NST - 1; ++q)
        if (sbb + q < sbe) stage_w(q, sbb + q);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    int st = 0;
    // waves 4-7 (the later-dispatched half, each sharing a SIMD with one of waves 0-3 running the same program) at
    // static priority 1: the arbitration loser otherwise (MI355X_MICROARCH.md, two waves per SIMD, item 4); bitwise
    // the same results.  tools/gemm_ab.py: q|k|v 53.3 -> 50.5 us, bench prefill 34.16k -> 34.56k tok/s
    if (wave >= 4) __builtin_amdgcn_s_setprio(1);
    for (int64_t sb = sbb; sb < sbe; ++sb) {
        const int buf = (int)((sb - sbb) & 1);
        const bool wn = sb + NST - 1 < sbe && KCPP_GEMM_PROBE != 1 && KCPP_GEMM_PROBE != 5;
#if KCPP_GEMM_PROBE != 1 && KCPP_GEMM_PROBE != 4
        if (sb + 1 < sbe) stage_a(buf ^ 1, sb + 1);
#endif
        if (wn) stage_w(st == 0 ? NST - 1 : st - 1, sb + NST - 1);
        const uint4 hc = S.wh[st][wr][lr];
        uint32_t sc_lo, sc_hi, m_lo, m_hi;
        k4_all(hc, sc_lo, sc_hi, m_lo, m_hi);
        // the super-block's weight fragments dequantized once (bw[p]: q*(sc>>3), q*(sc&7) of sub-blocks 2p, 2p+1),
        // then per token tile its 16 MFMAs and right behind them its epilogue (v3's: tot -= dy * dmin * (sum_j m_j
        // bsum_j), then tot += dy * (d * isum)), so only one tile's integer accumulators are live
        i32x4 bw[4][4];
        i32x4 qhv;
        if constexpr (Q5) qhv = S.wqh[st][wr][32 * kg + lr];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const i32x4 w4 = S.wq[st][wr][swz(lr, 2 * p + kg)];
            const uint32_t sdw = p < 2 ? sc_lo : sc_hi;
            const uint32_t s0 = (sdw >> (16 * (p & 1))) & 0xFF, s1 = (sdw >> (16 * (p & 1) + 8)) & 0xFF;
            const uint32_t h0 = s0 >> 3, l0 = s0 & 7, h1 = s1 >> 3, l1 = s1 & 7;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t x = (uint32_t)w4[e];
                const uint32_t lo = x & 0x0F0F0F0Fu, hi = (x >> 4) & 0x0F0F0F0Fu;
                bw[p][0][e] = mulb(lo, h0);
                bw[p][1][e] = mulb(lo, l0);
                bw[p][2][e] = mulb(hi, h1);
                bw[p][3][e] = mulb(hi, l1);
            }
        }
        h8v bm;
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
            i32x16 ah, al;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const i32x4 a0 = S.a[buf][tt][swz(lr, 4 * p + kg)], a1 = S.a[buf][tt][swz(lr, 4 * p + 2 + kg)];
                // Q5_K: hb*sc of sub-blocks 2p, 2p+1, made per token tile (held for all four pairs they spill)
                i32x4 bh0, bh1;
                if constexpr (Q5) {
                    const uint32_t sdw = p < 2 ? sc_lo : sc_hi;
                    const uint32_t s0 = (sdw >> (16 * (p & 1))) & 0xFF, s1 = (sdw >> (16 * (p & 1) + 8)) & 0xFF;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {     // hb * 2sc
                        const uint32_t hx = (uint32_t)qhv[e];
                        bh0[e] = mulb((hx >> (2 * p)) & 0x01010101u, 2 * s0);
                        bh1[e] = mulb((hx >> (2 * p + 1)) & 0x01010101u, 2 * s1);
                    }
                }
#if KCPP_GEMM_PROBE == 2
                ah[0] += a0[0] * bw[p][0][0] + a1[1] * bw[p][3][1];
                al[0] += a0[1] * bw[p][1][0] + a1[0] * bw[p][2][1];
                continue;
#endif
                if (p == 0) {
                    i32x16 z;
#pragma unroll
                    for (int i = 0; i < 16; ++i) z[i] = 0;
                    ah = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, bw[p][0], z, 0, 0, 0);
                    al = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, bw[p][1], z, 0, 0, 0);
                    if constexpr (Q5) ah = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, bh0, ah, 0, 0, 0);
                } else {
                    ah = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, bw[p][0], ah, 0, 0, 0);
                    al = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, bw[p][1], al, 0, 0, 0);
                    if constexpr (Q5) ah = __builtin_amdgcn_mfma_i32_32x32x32_i8(a0, bh0, ah, 0, 0, 0);
                }
                ah = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, bw[p][2], ah, 0, 0, 0);
                al = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, bw[p][3], al, 0, 0, 0);
                if constexpr (Q5) ah = __builtin_amdgcn_mfma_i32_32x32x32_i8(a1, bh1, ah, 0, 0, 0);
            }
            float dyv[16];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 v = *(const float4 *)&S.dy[buf][32 * tt + 8 * q + 4 * kg];
                dyv[4 * q] = v.x; dyv[4 * q + 1] = v.y; dyv[4 * q + 2] = v.z; dyv[4 * q + 3] = v.w;
            }
            const i32x4 bsv = S.bs[buf][tt][lane];
            h8v ab;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                ab[2 * e] = (_Float16)(int16_t)(bsv[e] & 0xFFFF);
                ab[2 * e + 1] = (_Float16)(int16_t)((uint32_t)bsv[e] >> 16);
            }
            f16acc accm;
#pragma unroll
            for (int i = 0; i < 16; ++i) accm[i] = 0.0f;
            accm = __builtin_amdgcn_mfma_f32_32x32x16_f16(ab, bm, accm, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 16; ++r) tot[j][r] = fmaf(-__fmul_rn(dyv[r], dm), accm[r], tot[j][r]);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float is = (float)(ah[r] * 8 + al[r]);
                tot[j][r] = fmaf(dyv[r], __fmul_rn(dw, is), tot[j][r]);
            }
        }
        // A (sb + 1) and W (sb + 1) must have landed; with three stages W (sb + 2), issued last, may stay in flight
        // (in-order retire)
        if (NST == 3 && wn) {
            static_assert(NST != 3 || NI == 2, "vmcnt counts below assume two weight groups per wave");
            if (wave < NI || (Q5 && wave >= 4)) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");   // 3 weight DMAs
            else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
        st = st == NST - 1 ? 0 : st + 1;
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

// grid: p.nwg workgroups of 512 threads = p.mt * row tiles (128 rows, p.tile 4: 256) * p.ks, twice that with a.W2
// (GLU: the second half computes W2 into a.Y2); p.ks > 1 leaves partials in a.part.  a.gcnt set: every group's tile
// grid in order (unsplit)
int gemm_q4v4_launch(const GemmPlan &p, const GemmArgs &a) {
    const bool q5 = ks_base_type(a.type) == KT_Q5_K;
    if (q5 && p.tile != 2) return -3;
    auto kern = q5 ? (p.rs ? k_gemm_q4v4<KT_Q5_K, 1, 2> : k_gemm_q4v4<KT_Q5_K, 0, 2>)
                : p.rs ? (p.tile == 4 ? k_gemm_q4v4<KT_Q4_K, 1, 4> : k_gemm_q4v4<KT_Q4_K, 1, 2>)
                       : (p.tile == 4 ? k_gemm_q4v4<KT_Q4_K, 0, 4> : k_gemm_q4v4<KT_Q4_K, 0, 2>);
    hipLaunchKernelGGL(kern, dim3((unsigned)p.nwg), dim3(512), 0, a.s, (const uint8_t *)a.W, a.K, a.N,
                       (const uint8_t *)a.act, a.M, a.Mp, p.mt, a.Y, a.ldy, a.res, a.ldr, p.ks, a.part, p.xg,
                       (const uint8_t *)a.W2, a.Y2, a.ldy2, a.gcnt, a.gne, a.wstride);
    KCPP_CHECK(hipGetLastError());
    return 0;
}
