// gemm_v1.hip -- k_gemm, the first MFMA GEMM: every quantized type, the 64 x 256 weight tile dequantized into LDS
// (the formulation: gemm.hip's header).  Activation image: k_act_to_f16 (gemm.hip).
#include "gemm_common.h"
#include "iq_grid.h"

template <int NB> struct GemmSmem {
    h8v bf[NB][2 * 16 * 64];      // [plane][tile*16*64 + step*64 + lane]
    h8v bm[2 * 64];               // mins fragment [tile*64 + lane]
    float wd[GB_N][8];            // K-quants: [0]=d, [1]=dmin ; Q4_0/Q8_0: d per 32-block
    float dy[GB_M][8];            // K-quants: [0]=dy of this super-block ; Q4_0/Q8_0: per 32-block
    float wm[GB_N][8];            // Q4_1 / Q5_1: m per 32-block
    float sy[GB_M][8];            // Q4_1 / Q5_1: block_q8_1.s per 32-block
};

// dequantize the 64 x 256 weight tile of super-block `sb` into LDS (thread t: row t>>2, chunk t&3)
template <int TYPE, typename SM>
__device__ __forceinline__ void stage_weights(SM &S, const uint8_t *__restrict__ W, int64_t K, int64_t N,
                                              int64_t n0, int64_t sb) {
    const int t = threadIdx.x, nl = t >> 2, c = t & 3;
    const int64_t n = min(n0 + nl, N - 1);
    const int64_t bpr = K / ks_block_elems(TYPE);
    const int64_t nbt = bpr * N;
    if constexpr (TYPE == KT_Q4_K || TYPE == KT_Q5_K) {
        const int BB = TYPE == KT_Q4_K ? 144 : 176;
        const uint8_t *blk = W + (n * bpr + sb) * BB;
        const uint4 hdr = *(const uint4 *)blk;
        const uint4 q0 = *(const uint4 *)(blk + (TYPE == KT_Q4_K ? 16 : 48) + 32 * c);
        const uint4 q1 = *(const uint4 *)(blk + (TYPE == KT_Q4_K ? 32 : 64) + 32 * c);
        uint4 h0 = make_uint4(0, 0, 0, 0), h1 = h0;
        if constexpr (TYPE == KT_Q5_K) { h0 = *(const uint4 *)(blk + 16); h1 = *(const uint4 *)(blk + 32); }
        int s0, m0, s1, m1;
        k4_sm(hdr, 2 * c, s0, m0);
        k4_sm(hdr, 2 * c + 1, s1, m1);
        const uint32_t qd[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
        const uint32_t hd[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint32_t lo0 = qd[2 * i] & 0x0F0F0F0Fu, lo1 = qd[2 * i + 1] & 0x0F0F0F0Fu;
            uint32_t hi0 = (qd[2 * i] >> 4) & 0x0F0F0F0Fu, hi1 = (qd[2 * i + 1] >> 4) & 0x0F0F0F0Fu;
            if constexpr (TYPE == KT_Q5_K) {
                lo0 |= ((hd[2 * i] >> (2 * c)) & 0x01010101u) << 4;
                lo1 |= ((hd[2 * i + 1] >> (2 * c)) & 0x01010101u) << 4;
                hi0 |= ((hd[2 * i] >> (2 * c + 1)) & 0x01010101u) << 4;
                hi1 |= ((hd[2 * i + 1] >> (2 * c + 1)) & 0x01010101u) << 4;
            }
            S.bf[0][bslot(nl, 64 * c + 8 * i)] = frag8(lo0, lo1, (float)s0, 0.0f);
            S.bf[0][bslot(nl, 64 * c + 32 + 8 * i)] = frag8(hi0, hi1, (float)s1, 0.0f);
        }
        // mins fragment: k = g (0..15) holds m_{g/2}; this thread owns g = 4c..4c+3
        _Float16 *bm = (_Float16 *)&S.bm[(nl >> 5) * 64 + (c >> 1) * 32 + (nl & 31)] + 4 * (c & 1);
        bm[0] = (_Float16)m0; bm[1] = (_Float16)m0; bm[2] = (_Float16)m1; bm[3] = (_Float16)m1;
        if (c == 0) {
            S.wd[nl][0] = h2f((uint16_t)(hdr.x & 0xFFFF));
            S.wd[nl][1] = h2f((uint16_t)(hdr.x >> 16));
        }
    } else if constexpr (TYPE == KT_Q6_K) {
        const int64_t b = n * bpr + sb;
        const uint8_t *q = W + b * 192;
        const int8_t *scp = (const int8_t *)(W + nbt * 192 + b * 16);
        const int hh = c >> 1;                   // 128-element half
        const int pb = 2 * (c & 1);              // planes pb, pb+1
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
            const int p = pb + pp;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint2 ql = *(const uint2 *)(q + 64 * hh + 32 * (p & 1) + 8 * i);
                const uint2 qh = *(const uint2 *)(q + 128 + 32 * hh + 8 * i);
                const int sh4 = 4 * (p >> 1);
                const uint32_t v0 = ((ql.x >> sh4) & 0x0F0F0F0Fu) | (((qh.x >> (2 * p)) & 0x03030303u) << 4);
                const uint32_t v1 = ((ql.y >> sh4) & 0x0F0F0F0Fu) | (((qh.y >> (2 * p)) & 0x03030303u) << 4);
                const int scv = scp[8 * hh + (i >> 1) + 2 * p];
                const int shi = scv >> 3, slo = scv & 7;
                const int k = 128 * hh + 32 * p + 8 * i;
                S.bf[0][bslot(nl, k)] = frag8_sub(v0, v1, (float)(8 * shi), 32.0f);
                S.bf[1][bslot(nl, k)] = frag8_sub(v0, v1, (float)slo, 32.0f);
            }
        }
        if (c == 0) S.wd[nl][0] = h2f(*(const uint16_t *)(W + nbt * 208 + b * 2));
    } else if constexpr (TYPE == KT_Q2_K) {
        // chunk c = quarter c (half n = c >> 1, shifts 2 (c & 1), +1); weights (sc & 15) q exact (<= 45); mins
        // (sc >> 4) per 16-group straight into the bsum fragment; SoA planes: scales [nb][16], qs [nb][64], d/dmin
        const int64_t b = n * bpr + sb;
        const int hn = c >> 1, j0 = 2 * (c & 1);
        const uint8_t *qp = W + nbt * 16 + b * 64 + 32 * hn;
        const uint4 q0 = *(const uint4 *)qp, q1 = *(const uint4 *)(qp + 16);
        const uint32_t sw = *(const uint32_t *)(W + b * 16 + 4 * c);
        const uint32_t qd[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int j = j0 + (i >> 2), w0 = 2 * (i & 3);
            const int sc = (int)((sw >> (8 * (2 * (i >> 2) + ((i & 3) >> 1)))) & 0xF);
            S.bf[0][bslot(nl, 64 * c + 8 * i)] = frag8((qd[w0] >> (2 * j)) & 0x03030303u, (qd[w0 + 1] >> (2 * j)) & 0x03030303u,
                                                       (float)sc, 0.0f);
        }
        _Float16 *bm = (_Float16 *)&S.bm[(nl >> 5) * 64 + (c >> 1) * 32 + (nl & 31)] + 4 * (c & 1);
#pragma unroll
        for (int t = 0; t < 4; ++t) bm[t] = (_Float16)(float)((sw >> (8 * t + 4)) & 0xF);
        if (c == 0) {
            const uint32_t dd = *(const uint32_t *)(W + nbt * 80 + b * 4);
            S.wd[nl][0] = h2f((uint16_t)(dd & 0xFFFF));
            S.wd[nl][1] = h2f((uint16_t)(dd >> 16));
        }
    } else if constexpr (TYPE == KT_Q3_K) {
        // chunk c = quarter c of the super-block (half n = c >> 1, shifts j0 = 2 (c & 1), j0 + 1); weights
        // (sc - 32) (v - 4) with v = 2 low bits | hmask bit << 2 -- exact f16 integers (|.| <= 128); SoA planes
        // (quant.hip kl_store_block): hmask [nb][32], qs [nb][64], scales [nb][12], d [nb][2]
        const int64_t b = n * bpr + sb;
        const int hn = c >> 1, j0 = 2 * (c & 1);
        const uint4 h0 = *(const uint4 *)(W + b * 32), h1 = *(const uint4 *)(W + b * 32 + 16);
        const uint8_t *qp = W + nbt * 32 + b * 64 + 32 * hn;
        const uint4 q0 = *(const uint4 *)qp, q1 = *(const uint4 *)(qp + 16);
        const uint32_t *scp = (const uint32_t *)(W + nbt * 96 + b * 12);
        const uint32_t a0 = scp[0], a1 = scp[1], a2 = scp[2];
        const uint32_t k1 = 0x03030303u, k2 = 0x0f0f0f0fu;
        const uint32_t sw = c == 0 ? (a0 & k2) | ((a2 & k1) << 4)
                          : c == 1 ? (a1 & k2) | (((a2 >> 2) & k1) << 4)
                          : c == 2 ? ((a0 >> 4) & k2) | (((a2 >> 4) & k1) << 4)
                                   : ((a1 >> 4) & k2) | (((a2 >> 6) & k1) << 4);
        const uint32_t qd[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
        const uint32_t hd[8] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w};
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int j = j0 + (i >> 2), w0 = 2 * (i & 3);            // elements l = 8 (i & 3) .. + 7
            const uint32_t v0 = ((qd[w0] >> (2 * j)) & 0x03030303u) | (((hd[w0] >> (4 * hn + j)) & 0x01010101u) << 2);
            const uint32_t v1 = ((qd[w0 + 1] >> (2 * j)) & 0x03030303u) | (((hd[w0 + 1] >> (4 * hn + j)) & 0x01010101u) << 2);
            const int sc = (int)((sw >> (8 * (2 * (i >> 2) + ((i & 3) >> 1)))) & 0xFF) - 32;
            S.bf[0][bslot(nl, 64 * c + 8 * i)] = frag8_sub(v0, v1, (float)sc, 4.0f);
        }
        if (c == 0) S.wd[nl][0] = h2f(*(const uint16_t *)(W + nbt * 108 + b * 2));
    } else if constexpr (TYPE == KT_Q4_0) {
        // this thread: 32-blocks 2c, 2c+1 of the 8 in the super-step
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) {
            const int jb = 2 * c + bb;
            const int64_t b = n * bpr + sb * 8 + jb;
            const uint4 qv = *(const uint4 *)(W + b * 16);
            const uint32_t qd[4] = {qv.x, qv.y, qv.z, qv.w};
            S.bf[0][bslot(nl, 32 * jb + 0)] = frag8(qd[0] & 0x0F0F0F0Fu, qd[1] & 0x0F0F0F0Fu, 1.0f, 8.0f);
            S.bf[0][bslot(nl, 32 * jb + 8)] = frag8(qd[2] & 0x0F0F0F0Fu, qd[3] & 0x0F0F0F0Fu, 1.0f, 8.0f);
            S.bf[0][bslot(nl, 32 * jb + 16)] = frag8((qd[0] >> 4) & 0x0F0F0F0Fu, (qd[1] >> 4) & 0x0F0F0F0Fu, 1.0f, 8.0f);
            S.bf[0][bslot(nl, 32 * jb + 24)] = frag8((qd[2] >> 4) & 0x0F0F0F0Fu, (qd[3] >> 4) & 0x0F0F0F0Fu, 1.0f, 8.0f);
            S.wd[nl][jb] = h2f(*(const uint16_t *)(W + nbt * 16 + b * 2));
        }
    } else if constexpr (TYPE == KT_Q5_0) {
        // as Q4_0 with the fifth bit: (q | h << 4) - 16 in [-16, 15], exact in f16
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) {
            const int jb = 2 * c + bb;
            const int64_t b = n * bpr + sb * 8 + jb;
            const uint4 qv = *(const uint4 *)(W + b * 16);
            const uint32_t h = *(const uint32_t *)(W + nbt * 16 + b * 4);
            const uint32_t qd[4] = {qv.x, qv.y, qv.z, qv.w};
            auto hb = [&](int sh) { return (((h >> sh) & 0xFu) * 0x00204081u & 0x01010101u) << 4; };
            S.bf[0][bslot(nl, 32 * jb + 0)] = frag8((qd[0] & 0x0F0F0F0Fu) | hb(0), (qd[1] & 0x0F0F0F0Fu) | hb(4), 1.0f, 16.0f);
            S.bf[0][bslot(nl, 32 * jb + 8)] = frag8((qd[2] & 0x0F0F0F0Fu) | hb(8), (qd[3] & 0x0F0F0F0Fu) | hb(12), 1.0f, 16.0f);
            S.bf[0][bslot(nl, 32 * jb + 16)] = frag8(((qd[0] >> 4) & 0x0F0F0F0Fu) | hb(16), ((qd[1] >> 4) & 0x0F0F0F0Fu) | hb(20),
                                                     1.0f, 16.0f);
            S.bf[0][bslot(nl, 32 * jb + 24)] = frag8(((qd[2] >> 4) & 0x0F0F0F0Fu) | hb(24), ((qd[3] >> 4) & 0x0F0F0F0Fu) | hb(28),
                                                     1.0f, 16.0f);
            S.wd[nl][jb] = h2f(*(const uint16_t *)(W + nbt * 20 + b * 2));
        }
    } else if constexpr (TYPE == KT_Q4_1 || TYPE == KT_Q5_1) {
        // q (| h << 4) in [0, 31] as is (s = 1, off = 0); d and m per block (SoA: qs [nb][16] (++ qh [nb][4]) ++ dm [nb][4])
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) {
            const int jb = 2 * c + bb;
            const int64_t b = n * bpr + sb * 8 + jb;
            const uint4 qv = *(const uint4 *)(W + b * 16);
            const uint32_t qd[4] = {qv.x, qv.y, qv.z, qv.w};
            uint32_t h = 0;
            if constexpr (TYPE == KT_Q5_1) h = *(const uint32_t *)(W + nbt * 16 + b * 4);
            auto hb = [&](int sh) { return (((h >> sh) & 0xFu) * 0x00204081u & 0x01010101u) << 4; };
            S.bf[0][bslot(nl, 32 * jb + 0)] = frag8((qd[0] & 0x0F0F0F0Fu) | hb(0), (qd[1] & 0x0F0F0F0Fu) | hb(4), 1.0f, 0.0f);
            S.bf[0][bslot(nl, 32 * jb + 8)] = frag8((qd[2] & 0x0F0F0F0Fu) | hb(8), (qd[3] & 0x0F0F0F0Fu) | hb(12), 1.0f, 0.0f);
            S.bf[0][bslot(nl, 32 * jb + 16)] = frag8(((qd[0] >> 4) & 0x0F0F0F0Fu) | hb(16), ((qd[1] >> 4) & 0x0F0F0F0Fu) | hb(20),
                                                     1.0f, 0.0f);
            S.bf[0][bslot(nl, 32 * jb + 24)] = frag8(((qd[2] >> 4) & 0x0F0F0F0Fu) | hb(24), ((qd[3] >> 4) & 0x0F0F0F0Fu) | hb(28),
                                                     1.0f, 0.0f);
            const uint32_t dm = *(const uint32_t *)(W + nbt * (TYPE == KT_Q5_1 ? 20 : 16) + b * 4);
            S.wd[nl][jb] = h2f((uint16_t)(dm & 0xFFFF));
            S.wm[nl][jb] = h2f((uint16_t)(dm >> 16));
        }
    } else if constexpr (TYPE == KT_IQ4_NL) {
        // code-book values kvalues_iq4nl[q] in [-127, 113] through v_perm (iq4nl_lut4), as Q8_0's biased bytes
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) {
            const int jb = 2 * c + bb;
            const int64_t b = n * bpr + sb * 8 + jb;
            const uint4 qv = *(const uint4 *)(W + b * 16);
            const uint32_t qd[4] = {qv.x, qv.y, qv.z, qv.w};
            auto lv = [&](uint32_t x) { return iq4nl_lut4(x & 0x0F0F0F0Fu) ^ 0x80808080u; };
            S.bf[0][bslot(nl, 32 * jb + 0)] = frag8(lv(qd[0]), lv(qd[1]), 1.0f, 128.0f);
            S.bf[0][bslot(nl, 32 * jb + 8)] = frag8(lv(qd[2]), lv(qd[3]), 1.0f, 128.0f);
            S.bf[0][bslot(nl, 32 * jb + 16)] = frag8(lv(qd[0] >> 4), lv(qd[1] >> 4), 1.0f, 128.0f);
            S.bf[0][bslot(nl, 32 * jb + 24)] = frag8(lv(qd[2] >> 4), lv(qd[3] >> 4), 1.0f, 128.0f);
            S.wd[nl][jb] = h2f(*(const uint16_t *)(W + nbt * 16 + b * 2));
        }
    } else if constexpr (TYPE == KT_IQ4_XS) {
        // sub-blocks 2c, 2c+1: (ls - 32) kv split as 8 (sc >> 3) kv + (sc & 7) kv over two planes (as Q6_K), both exact
        // f16 integers; SoA: qs [nb][128] ++ (d, scales_h, scales_l[4]) [nb][8]
        const int64_t b = n * bpr + sb;
        const uint2 hv = *(const uint2 *)(W + nbt * 128 + b * 8);
        const uint32_t shv = hv.x >> 16, slv = hv.y;
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) {
            const int ib = 2 * c + bb;
            const uint4 qv = *(const uint4 *)(W + b * 128 + 16 * ib);
            const uint32_t qd[4] = {qv.x, qv.y, qv.z, qv.w};
            const int sc = (int)(((slv >> (8 * (ib >> 1) + 4 * (ib & 1))) & 0xF) | (((shv >> (2 * ib)) & 3) << 4)) - 32;
            const float shi = (float)(8 * (sc >> 3)), slo = (float)(sc & 7);
            auto lv = [&](uint32_t x) { return iq4nl_lut4(x & 0x0F0F0F0Fu) ^ 0x80808080u; };
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int sh = i < 2 ? 0 : 4, w0 = 2 * (i & 1);
                const uint32_t t0 = lv(qd[w0] >> sh), t1 = lv(qd[w0 + 1] >> sh);
                S.bf[0][bslot(nl, 32 * ib + 8 * i)] = frag8_sub(t0, t1, shi, 128.0f);
                S.bf[1][bslot(nl, 32 * ib + 8 * i)] = frag8_sub(t0, t1, slo, 128.0f);
            }
        }
        if (c == 0) S.wd[nl][0] = h2f((uint16_t)(hv.x & 0xFFFF));
    } else if constexpr (kIqGrid<TYPE>) {
        // the grid types (iq_grid.h, ggml layout): sub-blocks 2c, 2c+1; codes biased to bytes (+128), times the group's
        // integer scale: exact f16 integers (|code ls| <= 62 x 31); d C per super-block
        const uint8_t *blk = W + (n * bpr + sb) * ks_block_bytes(TYPE);
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) {
            const int ib = 2 * c + bb;
            IqSub q;
            iq_sub<TYPE>(blk, ib, q);
#pragma unroll
            for (int l = 0; l < 4; ++l)
                S.bf[0][bslot(nl, 32 * ib + 8 * l)] = frag8(q.v[2 * l] ^ 0x80808080u, q.v[2 * l + 1] ^ 0x80808080u,
                                                           (float)q.ls[l], 128.0f);
        }
        if (c == 0) S.wd[nl][0] = iq_d<TYPE>(blk) * iq_const<TYPE>();
    } else {   // Q8_0: int8 -> (q ^ 0x80) = q + 128 as a byte
#pragma unroll
        for (int bb = 0; bb < 2; ++bb) {
            const int jb = 2 * c + bb;
            const int64_t b = n * bpr + sb * 8 + jb;
            const uint4 q0 = *(const uint4 *)(W + b * 32), q1 = *(const uint4 *)(W + b * 32 + 16);
            const uint32_t qd[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
#pragma unroll
            for (int i = 0; i < 4; ++i)
                S.bf[0][bslot(nl, 32 * jb + 8 * i)] = frag8(qd[2 * i] ^ 0x80808080u, qd[2 * i + 1] ^ 0x80808080u, 1.0f, 128.0f);
            S.wd[nl][jb] = h2f(*(const uint16_t *)(W + nbt * 32 + b * 2));
        }
    }
}

template <int TYPE>
__global__ void __launch_bounds__(256, 2) k_gemm(const uint8_t *__restrict__ W, int64_t K, int64_t N,
                                              const _Float16 *__restrict__ a16, const float *__restrict__ dyg,
                                              const _Float16 *__restrict__ bs16, int64_t M, float *__restrict__ Y,
                                              int64_t ldy, const float *res, int64_t ldr, const float *__restrict__ sg,
                                              float *__restrict__ part, int64_t Mp) {
    using T = GemmTraits<TYPE>;
    __shared__ GemmSmem<T::NB> S;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n0 = (int64_t)blockIdx.x * GB_N, m0 = (int64_t)blockIdx.y * GB_M;
    // split-K (gridDim.z > 1): this workgroup's super-block range; partials to part [z][Mp][N], summed in order by
    // k_splitk_reduce
    const int64_t nsb_all = K / GB_K, nsb_z = nsb_all / gridDim.z;
    const int64_t sb0 = (int64_t)blockIdx.z * nsb_z, nsb = sb0 + nsb_z;
    const int64_t G = T::SB ? 256 : 32;
    const int lr = lane & 31, lh = lane >> 5;
    const int64_t arow = m0 + 32 * wave + lr;                  // token row this lane feeds into A
    const _Float16 *ap = a16 + arow * K + 8 * lh;
    f16acc tot[2];
#pragma unroll
    for (int i = 0; i < 16; ++i) { tot[0][i] = 0.0f; tot[1][i] = 0.0f; }

    for (int64_t sb = sb0; sb < nsb; ++sb) {
        __syncthreads();                                        // previous step done with LDS
        stage_weights<TYPE>(S, W, K, N, n0, sb);
        // K-quants: the super-block's 16 A fragments, issued behind the weight loads (one latency per step, not one
        // per MFMA pair); per-32 types load theirs per half super-block below (register pressure of 8 epilogues)
        h8v av[16];
        if constexpr (T::SB) {
#pragma unroll
            for (int s = 0; s < 16; ++s) av[s] = *(const h8v *)(ap + sb * GB_K + 16 * s);
        }
        if (threadIdx.x < GB_M) {
            if constexpr (T::SB) S.dy[threadIdx.x][0] = dyg[(m0 + threadIdx.x) * (K / 256) + sb];
            else {
#pragma unroll
                for (int j = 0; j < 8; ++j) S.dy[threadIdx.x][j] = dyg[(m0 + threadIdx.x) * (K / 32) + sb * 8 + j];
                if constexpr (kGemmM1<TYPE>) {
                    const bool ok = m0 + threadIdx.x < M;
#pragma unroll
                    for (int j = 0; j < 8; ++j) S.sy[threadIdx.x][j] = ok ? sg[(m0 + threadIdx.x) * (K / 32) + sb * 8 + j] : 0.0f;
                }
            }
        }
        __syncthreads();
        if constexpr (T::SB) {
            f16acc acc[2], accm[2];
#pragma unroll
            for (int i = 0; i < 16; ++i) { acc[0][i] = acc[1][i] = 0.0f; accm[0][i] = accm[1][i] = 0.0f; }
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const h8v a = av[s];
#pragma unroll
                for (int tl = 0; tl < 2; ++tl) {
                    acc[tl] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, S.bf[0][(tl * 16 + s) * 64 + lane], acc[tl], 0, 0, 0);
                    if constexpr (T::NB == 2)
                        acc[tl] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, S.bf[T::NB - 1][(tl * 16 + s) * 64 + lane], acc[tl], 0, 0, 0);
                }
            }
            if constexpr (T::MINS) {
                const h8v am = *(const h8v *)(bs16 + arow * (K / 16) + sb * 16 + 8 * lh);
#pragma unroll
                for (int tl = 0; tl < 2; ++tl)
                    accm[tl] = __builtin_amdgcn_mfma_f32_32x32x16_f16(am, S.bm[tl * 64 + lane], accm[tl], 0, 0, 0);
            }
            // epilogue: tot += dy*d*sumi - dy*dmin*summ  (ggml_vec_dot_q4_K_q8_K, ggml-quants.c:7796-7859)
#pragma unroll
            for (int tl = 0; tl < 2; ++tl) {
                const float dw = S.wd[tl * 32 + lr][0];
                const float dm = T::MINS ? S.wd[tl * 32 + lr][1] : 0.0f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int tk = 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * lh;
                    const float dy = S.dy[tk][0];
                    float v = __fmul_rn(__fmul_rn(dy, dw), acc[tl][r]);
                    if constexpr (T::MINS) v = __fsub_rn(v, __fmul_rn(__fmul_rn(dy, dm), accm[tl][r]));
                    tot[tl][r] = __fadd_rn(tot[tl][r], v);
                }
            }
        } else {
            // Q4_1 / Q5_1: + sum_j m_w[j] s_a[j] over the 8 blocks, an fp32 product of the [tokens x 8] s and
            // [8 x rows] m tiles on the matrix cores (ggml_vec_dot_q4_1_q8_1 / _q5_1_q8_1, ggml-quants.c:4503,5145)
            if constexpr (kGemmM1<TYPE>) {
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) {
                    const float a = S.sy[32 * wave + lr][2 * kk + lh];
#pragma unroll
                    for (int tl = 0; tl < 2; ++tl)
                        tot[tl] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, S.wm[tl * 32 + lr][2 * kk + lh], tot[tl], 0, 0, 0);
                }
            }
#pragma unroll 1
            for (int hb = 0; hb < 2; ++hb) {
#pragma unroll
            for (int s = 0; s < 8; ++s) av[s] = *(const h8v *)(ap + sb * GB_K + 128 * hb + 16 * s);
#pragma unroll
            for (int jq = 0; jq < 4; ++jq) {
                const int jb = 4 * hb + jq;
                f16acc acc[2];
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[0][i] = acc[1][i] = 0.0f;
#pragma unroll
                for (int ss = 0; ss < 2; ++ss) {
                    const int s = 2 * jb + ss;
                    const h8v a = av[2 * jq + ss];
#pragma unroll
                    for (int tl = 0; tl < 2; ++tl)
                        acc[tl] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, S.bf[0][(tl * 16 + s) * 64 + lane], acc[tl], 0, 0, 0);
                }
                // tot += sumi * (d_w * d_a)   (ggml_vec_dot_q8_0_q8_0 scalar tail, ggml-quants.c:5519)
#pragma unroll
                for (int tl = 0; tl < 2; ++tl) {
                    const float dw = S.wd[tl * 32 + lr][jb];
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int tk = 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * lh;
                        tot[tl][r] = __fadd_rn(tot[tl][r], __fmul_rn(acc[tl][r], __fmul_rn(dw, S.dy[tk][jb])));
                    }
                }
            }
            }
        }
    }
    // store (+ residual)
#pragma unroll
    for (int tl = 0; tl < 2; ++tl) {
        const int64_t n = n0 + tl * 32 + lr;
        if (n >= N) continue;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t t = m0 + 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * lh;
            if (gridDim.z > 1) { if (t < M) part[((int64_t)blockIdx.z * Mp + t) * N + n] = tot[tl][r]; }
            else if (t < M) Y[t * ldy + n] = res ? __fadd_rn(tot[tl][r], res[t * ldr + n]) : tot[tl][r];
        }
    }
}

// grid (row tiles, token tiles, KS): KS > 1 leaves partials in a.part
int gemm_v1_launch(const GemmPlan &p, const GemmArgs &a) {
    const dim3 grid((unsigned)((a.N + GB_N - 1) / GB_N), (unsigned)(a.Mp / GB_M), (unsigned)p.ks);
#define KCPP_V1(T)                                                                                                         \
    case T: hipLaunchKernelGGL(k_gemm<T>, grid, dim3(256), 0, a.s, (const uint8_t *)a.W, a.K, a.N, (const _Float16 *)a.af, \
                               a.dy, (const _Float16 *)a.bsf, a.M, a.Y, a.ldy, a.res, a.ldr, a.s81, a.part, a.Mp); break;
    switch (a.type) {
    KCPP_V1(KT_Q2_K) KCPP_V1(KT_Q3_K) KCPP_V1(KT_Q4_0) KCPP_V1(KT_Q5_0) KCPP_V1(KT_Q8_0) KCPP_V1(KT_Q4_1) KCPP_V1(KT_Q5_1)
    KCPP_V1(KT_IQ4_NL) KCPP_V1(KT_IQ4_XS)
    KCPP_IQ_CASES(KCPP_V1)
    default: return -3;
    }
#undef KCPP_V1
    KCPP_CHECK(hipGetLastError());
    return 0;
}
