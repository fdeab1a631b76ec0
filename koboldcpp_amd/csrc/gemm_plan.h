// gemm_plan.h -- which kernel kcpp_gemm launches for a shape, and with what geometry.  Host-only plain C++ (no HIP):
// the one place that holds the split-K rules, the tile rules and the meaning of the kcpp_gemm_set_variant numbers.
// gemm.hip runs the plan (gemm_run); kcpp_gemm_plan exposes it, so tests/test_gemm_plan.py checks it without a GPU.
//
// Two kinds of choice live here.  The split-K factor changes output bits (the f32 order of the partial sums), so
// every split rule reads the weight shape only, never M: a prompt gives the same bits however it is cut into
// ubatches (tests/test_gpu_fullsize.py).  Everything else (family among the bitwise-equal K-quant kernels, tile,
// waves, XG, PF) changes speed only.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "../../include/kcpp_synth.h"

enum GemmFamily {
    GEMM_COLS = 0,   // exact mat-vec over groups of 8 columns (gemv.hip gemv_cols)
    GEMM_Q80S = 1,   // Q8_0 at M <= 32 (gemm_q80s.hip)
    GEMM_V1 = 2,     // k_gemm: every type, weights dequantized into LDS
    GEMM_V2 = 3,     // k_gemm_kq: Q4_K / Q5_K / Q6_K, both layouts
    GEMM_Q4V3 = 4,   // k_gemm_q4v3
    GEMM_Q6V3 = 5,   // k_gemm_q6v3 (Q6_K_RS)
    GEMM_V4 = 6,     // k_gemm_q4v4: int8 MFMA, Q4_K (TPW 2 = v4, 4 = v5) and Q5_K (TPW 2)
    GEMM_Q6P = 7,    // k_gemm_q6p: the Q6_K prefill image (kcpp_gemm_q6p only; gemm_plan_q6p)
};

struct GemmPlan {
    int family;      // GemmFamily
    int rs;          // weight layout: 0 base (kcpp), 1 the row-major decode layout (KT_*_RS)
    int tile;        // V2: TM (128 TM tokens per workgroup); Q4V3 / Q6V3: BMT (32 BMT tokens); V4: TPW; COLS: columns
    int waves;       // waves per workgroup
    int ks;          // split-K factor (1 = unsplit); Q80S: its K ranges
    int xg;          // token tiles per XCD group (xcd_tile)
    int pf;          // Q4V3: raw weight super-blocks loaded ahead
    int mt;          // token tiles of the grid
    int64_t nwg;     // workgroups of one launch (V4 GLU: gate and up in that one launch; COLS: 0)
};

// kcpp_gemm_set_variant's overrides, by name; all zero = the rules
enum { GEMM_SPLIT_RULE = 0, GEMM_SPLIT_NEVER = 1, GEMM_SPLIT_ALWAYS = 2 };   // ALWAYS: wherever the mode and K allow
enum { GEMM_V4_RULE = 0, GEMM_V4_NEVER = 1, GEMM_V4_ALWAYS = 2 };           // ALWAYS: wherever v4 can run
struct GemmForce {
    uint8_t v4;                        // GEMM_V4_*
    uint8_t no_v3;                     // 1: Q4V3 / Q6V3 off (what v4 does not take runs v2)
    uint8_t cols;                      // 1: the mat-vec path at every M for the types that have it
    uint8_t split1, split3, split4;    // GEMM_SPLIT_* of V1, of Q4V3 / Q6V3, of V4
    uint8_t q4v3_waves, q4v3_xg, q4v3_pf;   // 0 = by rule
    uint8_t q6v3_bmt, q6v3_waves;           // 0 = by rule
    uint8_t v4_tpw, v4_xg;                  // 0 = by rule
};

// The kcpp_gemm_set_variant numbers -- here and nowhere else.  Every number not listed behaves like 2.
inline GemmForce gemm_force_of(int variant) {
    constexpr uint8_t R = GEMM_SPLIT_RULE, NO = GEMM_SPLIT_NEVER, ALL = GEMM_SPLIT_ALWAYS;
    static const struct { int variant; GemmForce f; } table[] = {
        //      v4              no_v3 cols  split1 3   4    q4v3: waves xg pf   q6v3: bmt waves   v4: tpw xg
        {0,  {GEMM_V4_RULE,   0, 0,  R, R,   R,    0, 0, 0,   0, 0,   0, 0}},   // the rules
        {2,  {GEMM_V4_NEVER,  1, 0,  R, NO,  R,    0, 0, 0,   0, 0,   0, 0}},   // v2 for every K-quant
        {3,  {GEMM_V4_NEVER,  0, 0,  R, NO,  R,    0, 0, 0,   0, 0,   0, 0}},   // v3, unsplit
        {4,  {GEMM_V4_NEVER,  0, 0,  R, ALL, R,    0, 0, 0,   0, 0,   0, 0}},   // v3, split wherever allowed
        {5,  {GEMM_V4_NEVER,  0, 0,  R, NO,  R,    0, 0, 2,   0, 0,   0, 0}},   // v3 unsplit, weights two ahead
        {6,  {GEMM_V4_NEVER,  0, 0,  R, NO,  R,    4, 0, 2,   0, 0,   0, 0}},   //   ... and 4 waves
        {7,  {GEMM_V4_NEVER,  0, 0,  R, NO,  R,    4, 0, 0,   0, 0,   0, 0}},   // v3 unsplit, 4 waves
        {8,  {GEMM_V4_NEVER,  0, 0,  R, NO,  R,    0, 2, 0,   0, 0,   0, 0}},   // v3 unsplit, XG 2
        {9,  {GEMM_V4_NEVER,  0, 0,  R, NO,  R,    0, 4, 0,   0, 0,   0, 0}},   //   XG 4
        {10, {GEMM_V4_NEVER,  0, 0,  R, NO,  R,    0, 8, 0,   0, 0,   0, 0}},   //   XG 8
        {11, {GEMM_V4_ALWAYS, 0, 0,  R, NO,  R,    0, 0, 0,   0, 0,   0, 0}},   // v4 (its split rule), else v3 unsplit
        {12, {GEMM_V4_ALWAYS, 0, 0,  R, NO,  R,    0, 0, 0,   0, 0,   0, 2}},   //   ... v4 with XG 2
        {13, {GEMM_V4_ALWAYS, 0, 0,  R, NO,  NO,   0, 0, 0,   0, 0,   0, 0}},   // v4 unsplit, else v3 unsplit
        {14, {GEMM_V4_ALWAYS, 1, 0,  R, NO,  R,    0, 0, 0,   0, 0,   4, 0}},   // v5 (Q4_K; Q5_K v4), else v2
        {15, {GEMM_V4_NEVER,  0, 0,  R, R,   R,    0, 0, 0,   4, 4,   0, 0}},   // v3 (split rule), q6v3 tile (4, 4)
        {16, {GEMM_V4_NEVER,  0, 0,  R, R,   R,    0, 0, 0,   4, 8,   0, 0}},   //   q6v3 tile (4, 8)
        {17, {GEMM_V4_NEVER,  0, 0,  R, R,   R,    0, 0, 0,   2, 8,   0, 0}},   //   q6v3 tile (2, 8)
        {20, {GEMM_V4_NEVER,  1, 1,  R, NO,  R,    0, 0, 0,   0, 0,   0, 0}},   // 2 + the mat-vec path at every M
        {21, {GEMM_V4_NEVER,  1, 0,  NO, NO, R,    0, 0, 0,   0, 0,   0, 0}},   // 2 + v1 unsplit
    };
    if (variant < 0) variant = 0;
    const GemmForce *two = nullptr;
    for (const auto &row : table) {
        if (row.variant == variant) return row.f;
        if (row.variant == 2) two = &row.f;
    }
    return *two;
}

// ---------------------------------------------------------------- the split-K rules, each once
// v1: on grids under 512 workgroups (two per CU) at a 512-token ubatch the K range is split 2 .. 8 ways
inline int gemm_ks_v1(int64_t K, int64_t N, int split = GEMM_SPLIT_RULE) {
    if (split == GEMM_SPLIT_NEVER) return 1;
    const int64_t nwg = (N + 63) / 64 * (512 / 128);
    int ks = 1;
    while (ks < 8 && nwg * ks * 2 <= 1024 && (K / 256) % (ks * 2) == 0) ks *= 2;
    return ks;
}
// v3's big grid: >= 384 workgroups of 128 tokens x 128 rows (its own tile shape; never split)
inline bool gemm_big(int64_t Mp, int64_t N) { return Mp / 128 * ((N + 127) / 128) >= 384; }
// q4v3 / q6v3 / q6p: plain mode, an even super-block count, a small grid, and few row tiles (< 16) or a long K
// (>= 32 super-blocks): K in two halves
inline int gemm_ks_v3(int64_t K, int64_t N, int64_t Mp, int mode, int split = GEMM_SPLIT_RULE) {
    const int64_t nsb = K / 256, nt = (N + 127) / 128;
    if (mode != 0 || nsb % 2 || split == GEMM_SPLIT_NEVER) return 1;
    if (split == GEMM_SPLIT_ALWAYS) return 2;
    return !gemm_big(Mp, N) && (nt < 16 || nsb >= 32) ? 2 : 1;
}
// v4: plain mode, an even super-block count, at most 32 row tiles (<= 128 tiles at the 512-token ubatch)
inline int gemm_ks_v4(int64_t K, int64_t N, int mode, int split = GEMM_SPLIT_RULE) {
    if (split == GEMM_SPLIT_NEVER) return 1;
    return mode == 0 && (K / 256) % 2 == 0 && (N + 127) / 128 <= 32 ? 2 : 1;
}
// Q8_0 small batch: K ranges per 128-row tile for >= ~384 workgroups, <= 48 blocks each (the kernel's LDS)
constexpr int kQ80sUnroll = 8;
inline int gemm_ks_q80s(int64_t K, int64_t N) {
    const int64_t nt = (N + 127) / 128, nb = K / 32;
    int64_t S = (384 + nt - 1) / nt;
    S = std::min<int64_t>(S, std::max<int64_t>(1, nb / (2 * kQ80sUnroll)));
    S = std::max<int64_t>(S, (nb + 47) / 48);
    return (int)std::max<int64_t>(S, 1);
}
// the most split-K partials [Mp][N] a type's workspace holds (Q5_K keeps room for v1's count, which it never runs)
inline int gemm_ks_max(int type, int64_t K, int64_t N) {
    const int base = ks_base_type(type);
    const int v34 = 2;                  // gemm_ks_v3 / gemm_ks_v4: in two at most
    if (base == KT_Q4_K || type == KT_Q6_K_RS) return v34;
    if (base == KT_Q5_K) return std::max(v34, gemm_ks_v1(K, N));
    return gemm_ks_v1(K, N);
}

inline bool gemm_has_cols(int type) {
    return type == KT_Q4_1 || type == KT_Q5_1 || type == KT_IQ4_NL || type == KT_IQ4_XS || is_iq_grid_type(type);
}

// What kcpp_gemm launches for (type, K, N, M, mode); K a multiple of 256.  bs_aligned: the Q8_K bsums of the
// activation buffer sit on a 16-byte boundary (v4 stages them by 16-byte LDS-DMA).
inline GemmPlan gemm_plan(int type, int64_t K, int64_t N, int64_t M, int mode, bool bs_aligned, const GemmForce &f) {
    const int base = ks_base_type(type);
    const int64_t Mp = (M + 127) / 128 * 128, nt = (N + 127) / 128;
    GemmPlan p = {GEMM_V1, type != base, 1, 4, 1, 1, 1, (int)(Mp / 128), 0};
    if (gemm_has_cols(type) && (M <= 16 || f.cols)) {
        // past 16 columns the MFMA GEMM is faster (tools/gemm_lowbit_ab.py: Q4_1 4096 x 14336 at 16 / 37 / 512
        // tokens: mat-vec 52 / 125 / 1592 us, GEMM 67 / 72 / 229 us)
        p.family = GEMM_COLS;
        p.tile = 8;
        p.mt = (int)((M + 7) / 8);
        return p;
    }
    if (type == KT_Q8_0 && M <= 32) {
        p.family = GEMM_Q80S;
        p.ks = gemm_ks_q80s(K, N);
        p.mt = 1;
        p.nwg = nt * p.ks;
        return p;
    }
    const bool q4 = base == KT_Q4_K, q5 = base == KT_Q5_K;
    // v4 for every Q4_K shape past the small-batch range (tools/gemm_ab.py, M = 512, v3 -> v4: gate|up 28672 rows
    // 249 -> 216 us, down 14336 -> 4096 122 -> 101, q|k|v 6144 rows 59.4 -> 52.1 (unsplit), wo 4096 rows 43.1 ->
    // 38.5 (split-K)).
    // Q5_K: v4 with the fifth-bit MFMA (TPW 2 only) for the plain / residual projections it splits along K (v2 ->
    // v4: Mixtral expert down 14336 -> 4096 M = 128 134.3 -> 96.3 us, M = 512 151.4 -> 124.6; wo 4096^2 42.6 -> 34.6
    // / 49.1 -> 45.4) -- a weight-shape rule, as the split changes bits -- and for GLU (gate + up in one launch) up
    // to 256 tokens: 4096 -> 2 x 14336 M = 128 93.9 -> 73.1.  Unsplit shapes stay on v2 (GLU M = 512 ~270 vs ~305;
    // dense gate|up 4096 -> 28672 M = 512 ~240 vs ~271; q|k|v 6144 rows M = 128 43.6 vs 55.7); unsplit v4 and v2
    // are bitwise equal (test_gemm_v4_int8_matches_v2_bitwise), so the GLU token-count rule does not change a bit.
    const bool v4_rule = q4 || (q5 && (gemm_ks_v4(K, N, mode) == 2 || (mode == 1 && Mp <= 256)));
    const bool v4 = (q4 || q5) && (f.v4 == GEMM_V4_ALWAYS || (f.v4 == GEMM_V4_RULE && v4_rule));
    if (v4 && bs_aligned && M > 32) {
        p.family = GEMM_V4;
        p.waves = 8;
        p.ks = gemm_ks_v4(K, N, mode, f.split4);
        // v5 (TPW = 4: 256-row tiles, each dequantized fragment feeding all 128 tokens' MFMAs) wherever its grid
        // still covers ~7/8 of the CUs; same per-element arithmetic and order as v4 (and KS = 1 on both), so the
        // choice never changes a bit (tools/gemm_ab.py, M = 512, v4 -> v5: gate|up 28672 rows 214.1 -> 188.6 us,
        // gate + up 14336 rows 217.7 -> 201.0; q|k|v 6144 rows 52.3 -> 86.0 on its 96-workgroup grid, so not there)
        const int64_t nt256 = (N + 255) / 256;
        const bool v5 = q4 && (f.v4_tpw == 4 || (f.v4 == GEMM_V4_RULE && p.ks == 1 && p.mt * nt256 >= 224));
        p.tile = v5 ? 4 : 2;
        p.xg = f.v4_xg ? f.v4_xg : 1;
        p.nwg = p.mt * (v5 ? nt256 : nt) * p.ks * (mode == 1 ? 2 : 1);
        return p;
    }
    if (q4 && !f.no_v3) {
        // measured at M = 512 (tools/gemm_ab.py): 128 x 128 tiles with 8 waves for gate|up (247 vs v2 301 us),
        // 64 x 128 tiles with 4 waves for the 128-192-tile shapes (wo 44.7 vs 46.7, down 131.5 vs 137.2 us); the
        // split on those small grids: down 14336 x 4096 122.9 -> 112.3 us, wo 4096 x 4096 43.3 -> 45.6 (not split),
        // gate|up (big grid) 236.8 -> 273.0 (not split)
        const bool big = gemm_big(Mp, N);
        p.family = GEMM_Q4V3;
        p.tile = big ? 4 : 2;
        p.waves = f.q4v3_waves ? f.q4v3_waves : (big ? 8 : 4);
        p.xg = f.q4v3_xg ? f.q4v3_xg : 1;
        p.pf = f.q4v3_pf ? f.q4v3_pf : 1;
        p.ks = gemm_ks_v3(K, N, Mp, mode, f.split3);
    } else if (type == KT_Q6_K_RS && !f.no_v3) {
        // long K (ffn_down, K/256 >= 32, split in two) also takes 128-token x 128-row tiles with 8 waves while that
        // grid still has a workgroup per CU: tools/gemm_ab.py, M = 512, down 14336 x 4096 195.3 -> 171.5 us (attn_v
        // 4096 x 1024: 34.5 stays on 64-token tiles, 49.8 / 53.9 on 128; split 56.7 -> 33.9); never changes a bit
        const bool wide = gemm_big(Mp, N) ||
                          (K / 256 >= 32 && mode == 0 && (K / 256) % 2 == 0 && Mp / 128 * nt * 2 >= 256);
        p.family = GEMM_Q6V3;
        p.tile = f.q6v3_bmt ? f.q6v3_bmt : (wide ? 4 : 2);
        p.waves = f.q6v3_waves ? f.q6v3_waves : (wide ? 8 : 4);
        p.ks = gemm_ks_v3(K, N, Mp, mode, f.split3);
    } else if (q4 || q5 || base == KT_Q6_K) {
        p.family = GEMM_V2;
        p.tile = q4 && Mp % 256 == 0 && N >= 8192 ? 2 : 1;
        p.mt = (int)(Mp / (128 * p.tile));
        p.nwg = p.mt * ((N + 63) / 64);
        return p;
    } else {
        // v1 split-K: a lone workgroup otherwise walks all of K, one load latency a step
        p.ks = gemm_ks_v1(K, N, f.split1);
        p.nwg = (N + 63) / 64 * p.mt * p.ks;
        return p;
    }
    p.mt = (int)(Mp / (32 * p.tile));
    p.nwg = p.mt * nt * p.ks;
    return p;
}

// kcpp_gemm_q6p: q6v3's split rule (so the f32 summation order -- and every bit -- is q6v3's); 128 x 128 tiles,
// a row tile's token tiles on one XCD when they divide the 8
inline GemmPlan gemm_plan_q6p(int64_t K, int64_t N, int64_t M, int mode, int waves) {
    const int64_t Mp = (M + 127) / 128 * 128;
    GemmPlan p = {GEMM_Q6P, 1, 4, waves, gemm_ks_v3(K, N, Mp, mode), 1, 1, (int)(Mp / 128), 0};
    p.xg = 8 % p.mt == 0 ? p.mt : 1;
    p.nwg = p.mt * (N / 128) * p.ks;
    return p;
}
