// fa_plan.h -- which attention kernel runs a shape, and with what grid and workspace layout.  Host-only plain C++ (no
// HIP), the idiom of gemm_plan.h.  Prefill at D = 128 (fa_prefill_plan): attn_mfma.hip launches what it says (grid, ch,
// nsp), runtime.cpp asks it whether the MFMA kernel takes a GQA ratio, kcpp_fa_prefill_plan exposes it,
// tests/test_fa_prefill_plan.py checks it without a GPU.  Decode and the ggml-op forms (fa_decode_plan, at the end): the
// entries of attn.hip launch what it says through the launchers of attn_common.h, kcpp_fa_decode_plan exposes it,
// tests/test_fa_decode_plan.py checks it without a GPU.
//
// k_fa_prefill_mfma3's workgroup has four SLOTS of 16 queries x 1 head (NW = 8: two waves per slot, one per key half).
// A slot is a (head, 16-query block) pair, G = H / HKV:
//   GH heads per workgroup = 4 (G % 4 == 0), 2 (G % 2 == 0), else 1;   QB = 4 / GH consecutive query blocks;
//   slot s -> head hk G + GH gsub + s % GH, query block QB qbg + s / GH      (gsub < GS = G / GH, qbg < ceil(nqb / QB))
// so every staged K/V tile feeds 4 slots at every ratio and the grid is ceil(nqb / QB) HKV GS workgroups -- (T / 16) (H /
// 4), what G = 4 launches at equal H.  Workgroup order (XCD-aware, 1-D): bid -> hk fastest (bid & 7 first when HKV % 8
// == 0), then gsub, then qbg; the key splits outermost.  G = 4 is GH = 4, GS = 1, QB = 1: the grid it always had.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>

#define FM_Q 16          // queries per slot
#define FM_K 64          // keys per tile
#define FM_SPLIT_T 64    // key-split prefill (k_fa_prefill_mfma3<8, true>): ubatches up to this many tokens,
#define FM_SPLITS 32     // at most this many key splits
#define FM_PQ 132        // split partial of one (query, head): 128 dims, m, l, pad
#define FM_PS (16 * FM_PQ)
#define FM_MAXG 8        // GQA ratios 1..8
// the decode kernels (attn_chunk.hip, attn_dec.hip)
#define FA_CHUNK 64              // keys per workgroup of k_fa_decode
#define FA_MAXG 8                // GQA ratios 1..8
#define FA_MAX_CHUNKS 2048       // k_fa_combine's chunk-weight table: 2048 x 64 = 131072 keys
#define FA_MAXS 64               // k_fa_comb4's split-weight table
// bytes in front of the flash-attention workspace's partials (spare header words for in-launch hand-offs)
#define KCPP_FA_WS_HEADER 2048

enum { FA_PREFILL_FMA = 0, FA_PREFILL_MFMA = 1, FA_PREFILL_MFMA_SPLIT = 2 };

struct FaPrefillPlan {
    int kernel;          // FA_PREFILL_*
    int gh, qb;          // heads and query blocks per workgroup (gh qb = 4)
    int nb0;             // workgroups per split
    int nsp;             // key splits (1 = unsplit)
    int ch;              // 64-key tiles per split (unsplit: every tile)
    int merge_grid;      // workgroups of k_fa_split_merge (0 = unsplit)
    int64_t part_bytes;  // bytes of partials written behind the workspace header (0 = unsplit)
};

inline int fa_gh(int G) { return G % 4 == 0 ? 4 : (G % 2 == 0 ? 2 : 1); }

// The one table: which ratios the auto path (kcpp_flash_attn force_path 0, the runtime's Q8_0-tile branch) gives to
// the MFMA kernel.  A ratio is on iff the whole suite passes with it on and tools/fa_ab.py shows it faster than
// k_fa_prefill<128> at every measured n_past ("Measured").  KCPP_FA_PREFILL_MFMA=0 (read
// once) turns every ratio but 4 off, for A/B runs.
inline bool fa_prefill_mfma_auto(int G) {
    // G = 8 is off: tests/test_gpu_config4.py::test_70b_stage_properties holds a 12-token ubatch (f32 chunk kernels)
    // against a 24-token one to 1e-5 of scale on 75 % of the rows, and P rounded to f16 flips enough int8 roundings of
    // the Q8_K activations behind it to leave 58 % there; force_path 3 and the direct entries run it
    //                                          G = 0  1  2  3  4  5  6  7  8
    static const uint8_t on[FM_MAXG + 1] = {0, 1, 1, 1, 1, 1, 1, 1, 0};
    static const bool env_on = [] { const char *e = getenv("KCPP_FA_PREFILL_MFMA"); return !e || atoi(e) != 0; }();
    if (G < 1 || G > FM_MAXG) return false;
    return G == 4 || (on[G] && env_on);
}

// forced: what the direct entries (kcpp_flash_attn_prefill_mfma, _ex, force_path 3) run -- the table is not asked.
// Returns 0, or -3 for what the MFMA kernel does not cover.
inline int fa_prefill_plan(int T, int H, int HKV, int D, int n_past, bool have_ws, bool forced, FaPrefillPlan *p) {
    if (D != 128 || T <= 0 || HKV <= 0 || H <= 0 || H % HKV || H / HKV > FM_MAXG || n_past < 0) return -3;
    const int G = H / HKV;
    p->gh = fa_gh(G);
    p->qb = 4 / p->gh;
    const int nqb = (T + FM_Q - 1) / FM_Q;
    p->nb0 = (nqb + p->qb - 1) / p->qb * HKV * (G / p->gh);
    const int ntile = (n_past + T + FM_K - 1) / FM_K;
    p->kernel = FA_PREFILL_MFMA;
    p->nsp = 1;
    p->ch = ntile;
    p->merge_grid = 0;
    p->part_bytes = 0;
    if (have_ws && T <= FM_SPLIT_T && p->nb0 <= 512) {
        // keys split so that the grid has ~512 workgroups (at most FM_SPLITS splits of whole 64-key tiles)
        const int want = std::min(FM_SPLITS, std::max(1, 512 / p->nb0));
        const int ch = (ntile + want - 1) / want;
        const int nsp = (ntile + ch - 1) / ch;
        if (nsp > 1) {
            p->kernel = FA_PREFILL_MFMA_SPLIT;
            p->nsp = nsp;
            p->ch = ch;
            p->merge_grid = p->nb0 * 4;                  // one workgroup per slot
            p->part_bytes = (int64_t)p->nb0 * nsp * 4 * FM_PS * 4;
        }
    }
    if (!forced && !fa_prefill_mfma_auto(G)) p->kernel = FA_PREFILL_FMA;
    return 0;
}

// ---------------------------------------------------------------- decode and the ggml-op forms
enum {
    FA_DEC_CHUNK = 0,    // k_fa_decode + k_fa_combine (attn_chunk.hip)
    FA_DEC_SPLIT4 = 1,   // k_fa_dec4 + k_fa_comb4 (attn_dec.hip; the legacy A/B kernel)
    FA_DEC_SPLIT5 = 2,   // k_fa_dec5 + k_fa_comb4
    FA_DEC_SHORT = 3,    // k_fa_dec5<FINAL>, 8 waves, no combine
    FA_DEC_TILE = 4,     // not a decode kernel: k_fa_prefill<D> (attn_tile.hip)
    FA_DEC_MFMA = 5      // not a decode kernel: kcpp_flash_attn_prefill_mfma (fa_prefill_plan has its geometry)
};
// which entry asks: kcpp_flash_attn (and kcpp_flash_attn_dec_ta), kcpp_fa_decode_ex, kcpp_flash_attn_ext_dec_sc (one
// query of the ggml op), kcpp_flash_attn_ext_sc (T queries of the ggml op)
enum { FA_FORM_RUNTIME = 0, FA_FORM_EX = 1, FA_FORM_GRAPH1 = 2, FA_FORM_GRAPHT = 3 };
enum { FA_PLAN_CAP = 1, FA_PLAN_NO_OUT = 2 };        // flags: a logit soft-cap is set; no f32 out is given

struct FaDecodePlan {
    int kernel;              // FA_DEC_*
    int ns, nch;             // key splits (split pair, short form) / 64-key chunks (chunk pair); else 0
    int waves;               // waves per workgroup of the main launch
    int grid[3];             // the main launch
    int cgrid[2], cthreads;  // the combine launch (all 0: none)
    int cquant;              // the combine's quantizer: 0 none, 1 Q8_K, 2 KT_Q8_0_TA
    int64_t part_o, part_ml; // byte offsets of the partials from the start of the workspace (0: none)
    int64_t ws_bytes;        // bytes of workspace the launches touch, from its start (0: none)
    int64_t q16;             // FA_FORM_GRAPHT: byte offset of the f16 copy of Q (0: none)
};

// split count of the split pair: one workgroup per CU (256 / HKV splits, rounded down to a power of two in [4, maxs];
// measured at 3850 cached keys, tools/fa_dec_bench.py: 7.8 us vs 8.7 at 512 workgroups).  Independent of the
// context size, so the key partition -- and the result, bit for bit -- depends on the cached keys only.
inline int fa_splits(int HKV, int maxs = FA_MAXS) {
    int ns = 4;
    while (ns < maxs && 2 * ns * HKV <= 256) ns *= 2;
    return ns;
}

// KCPP_FA_DEC=4 (read once): the split pair runs k_fa_dec4 where it is built, for A/B
inline bool fa_dec5_default() {
    static const bool on = [] { const char *e = getenv("KCPP_FA_DEC"); return !e || atoi(e) != 4; }();
    return on;
}

extern "C" int64_t kcpp_fa_workspace_bytes(int T, int H, int n_kv_max);

// What the entries of attn.hip run.  nkv: the key bound (runtime forms: n_kv_max when n_past_dev is given, else
// n_past + T; ggml-op forms: n_kv).  n_rows: rows the K/V views hold (runtime forms: n_kv_max when n_past_dev is given,
// else n_past + 1; ggml-op forms: n_kv), 0 = unknown.  qkind: the quantized output, 0 none, 1 Q8_K, 2 KT_Q8_0_TA.
// sel: kcpp_flash_attn's force_path, kcpp_fa_decode_ex's variant, else unused.  Returns 0 or the entry's error code.
//
// The rules, G = H / HKV:
//   FA_FORM_RUNTIME
//     D not in {64, 128}, H % HKV or odd H: -1.  D = 64: FA_DEC_TILE at every T and force_path (-2 without out).
//     D = 128: G > 8: -1.
//     force_path 7: T = 1, out and no qout, else -1; FA_DEC_SHORT.
//     The decode family = force_path 1, 6, and 0 with T <= 16:
//       the split pair when T = 1, force_path != 6 and (no qout or G >= 2); every other case FA_DEC_CHUNK (so T = 1
//       with qout at G = 1 is FA_DEC_CHUNK).
//     Otherwise prefill (-2 without out): FA_DEC_MFMA at force_path 3, and at force_path 0 when fa_prefill_mfma_auto
//     gives the ratio to it; else FA_DEC_TILE.  (What the MFMA entry refuses -- T < 1, n_past < 0 -- is -3 at force_path
//     3 and runs the tiles at force_path 0, so FA_DEC_MFMA carries the tiles' grid.)
//   FA_FORM_EX (T = 1, D = 128)
//     H % HKV, G outside 1..8, odd H or HKV > 64: -1.  qout at G = 1: -1.
//     variant 3 / 5: the split pair (3 asks for k_fa_dec4, 5 for k_fa_dec5); 8: FA_DEC_SHORT (-1 with qout or without
//     out); 0: FA_DEC_CHUNK; any other: -1.  6 and 7, the tools' A/B forms, are checked as 5 and then run by attn_dec.hip
//     fa_dec_tool, which takes G = 4 alone and its split and wave counts from the environment (KCPP_FA_NS, KCPP_FA_NW).
//   FA_FORM_GRAPH1 (T = 1; D = 256 is kcpp_fa256_dec's)
//     D != 128, H % HKV, odd H, nkv < 1 or G not in {1, 2, 4, 8}: -3.  Always FA_DEC_SPLIT5 (the entry refuses a missing
//     mask and a misaligned Q with -3, and picks GRAPH / CAP).
//   FA_FORM_GRAPHT (D = 256 is attn_d256.hip's)
//     D not in {64, 128}, H % HKV, G > 8, odd H or nkv < 1: -1.  A cap at D = 64: -1.
//     D = 64: FA_DEC_TILE at every T.  D = 128: FA_DEC_CHUNK for T <= 16 (any G 1..8), else FA_DEC_TILE.
//   The split pair: -1 when neither output is given; G in {3, 5, 6, 7} is always FA_DEC_SPLIT5, and -1 when n_rows < 1.
//     Else FA_DEC_SPLIT5 when k_fa_dec5 is asked for (FA_FORM_RUNTIME: unless KCPP_FA_DEC=4; FA_FORM_EX: variant 5;
//     FA_FORM_GRAPH1: always) and n_rows >= 1, else FA_DEC_SPLIT4.  ns = fa_splits(HKV), grid (ns, HKV) of 256 threads,
//     combine grid H / 2 of 256 threads; partials O [H][ns][128] f32 then (m, l) [H][ns] behind the header.
//   FA_DEC_SHORT: grid (1, HKV) of 512 threads, no combine, no workspace.
//   FA_DEC_CHUNK: nch = ceil(nkv / 64), -4 when nch > 2048; grid (nch, HKV, T) of 256 threads, combine grid (H / 2, T) of
//     1024 threads; partials O [T][H][nch][128] f32 then (m, l) [T][H][nch] behind the header.
//   FA_DEC_TILE: grid (ceil(T / 64), H) of 256 threads, no workspace.
//   FA_FORM_GRAPHT keeps the f16 copy of Q [T][H][D] at kcpp_fa_workspace_bytes(T, H, nkv) rounded up to 256.
//   A ratio no kernel is built for (G = 0) is the launcher's -3.
inline int fa_decode_plan(int form, int T, int H, int HKV, int D, int nkv, int n_rows, int qkind, int sel, int flags,
                          FaDecodePlan *p) {
    *p = FaDecodePlan{};
    const bool have_out = form >= FA_FORM_GRAPH1 || !(flags & FA_PLAN_NO_OUT);      // (the op always has its dst)
    const bool capped = flags & FA_PLAN_CAP, have_q = qkind != 0;
    if (form == FA_FORM_EX || form == FA_FORM_GRAPH1) T = 1;
    if (HKV == 0) return form == FA_FORM_GRAPH1 ? -3 : -1;
    const int G = H / HKV;
    bool split = false, want5 = true;
    switch (form) {
    case FA_FORM_RUNTIME: {
        if ((D != 128 && D != 64) || H % HKV || H % 2) return -1;
        if (D == 64) {
            if (!have_out) return -2;
            p->kernel = FA_DEC_TILE;
            break;
        }
        if (G > FA_MAXG) return -1;
        const bool family = sel == 1 || sel == 6 || (sel == 0 && T <= 16);
        if (sel == 7) {
            if (T != 1 || !have_out || have_q) return -1;
            p->kernel = FA_DEC_SHORT;
        } else if (family && T == 1 && sel != 6 && (!have_q || G >= 2)) {
            split = true;
            want5 = fa_dec5_default();
        } else if (family) {
            p->kernel = FA_DEC_CHUNK;
        } else {
            if (!have_out) return -2;
            p->kernel = sel == 3 || (sel == 0 && fa_prefill_mfma_auto(G)) ? FA_DEC_MFMA : FA_DEC_TILE;
        }
        break;
    }
    case FA_FORM_EX:
        if (H % HKV || G < 1 || G > FA_MAXG || H % 2 || HKV > 64) return -1;
        if (have_q && G < 2) return -1;
        if (sel == 3 || (sel >= 5 && sel <= 7)) {
            split = true;
            want5 = sel != 3;
        } else if (sel == 8) {
            if (have_q || !have_out) return -1;
            p->kernel = FA_DEC_SHORT;
        } else if (sel == 0) {
            p->kernel = FA_DEC_CHUNK;
        } else {
            return -1;
        }
        break;
    case FA_FORM_GRAPH1:
        if (D != 128 || H % HKV || H % 2 || nkv < 1) return -3;
        if (!(G == 1 || G == 2 || G == 4 || G == 8)) return -3;
        split = true;
        n_rows = nkv;                                // the views hold the op's n_kv keys
        break;
    case FA_FORM_GRAPHT:
        if ((D != 128 && D != 64) || H % HKV || G > FA_MAXG || H % 2 || nkv < 1) return -1;
        if (capped && D != 128) return -1;
        p->kernel = D == 128 && T <= 16 ? FA_DEC_CHUNK : FA_DEC_TILE;
        break;
    default: return -1;
    }
    if (split) {
        const bool only5 = G == 3 || G == 5 || G == 6 || G == 7;
        if (!have_q && !have_out) return -1;
        if (n_rows < 1 && only5) return -1;      // k_fa_dec5 only: it needs the views' row count
        p->kernel = only5 || (want5 && n_rows > 0) ? FA_DEC_SPLIT5 : FA_DEC_SPLIT4;
        p->ns = fa_splits(HKV);
        p->waves = 4;
        p->grid[0] = p->ns, p->grid[1] = HKV, p->grid[2] = 1;
        p->cgrid[0] = H / 2, p->cgrid[1] = 1, p->cthreads = 256;
        p->cquant = qkind;
        p->part_o = KCPP_FA_WS_HEADER;
        p->part_ml = p->part_o + (int64_t)H * p->ns * 128 * 4;
        p->ws_bytes = p->part_ml + (int64_t)H * p->ns * 8;
    } else if (p->kernel == FA_DEC_SHORT) {
        p->ns = 1;
        p->waves = 8;
        p->grid[0] = 1, p->grid[1] = HKV, p->grid[2] = 1;
    } else if (p->kernel == FA_DEC_CHUNK) {
        p->nch = (nkv + FA_CHUNK - 1) / FA_CHUNK;
        if (p->nch > FA_MAX_CHUNKS) return -4;       // k_fa_combine's chunk-weight table (128k context)
        p->waves = 4;
        p->grid[0] = p->nch, p->grid[1] = HKV, p->grid[2] = T;
        p->cgrid[0] = H / 2, p->cgrid[1] = T, p->cthreads = 1024;
        p->cquant = have_q ? 1 : 0;
        p->part_o = KCPP_FA_WS_HEADER;
        p->part_ml = p->part_o + (int64_t)T * H * p->nch * 128 * 4;
        p->ws_bytes = p->part_ml + (int64_t)T * H * p->nch * 8;
    } else {                                         // FA_DEC_TILE, and FA_DEC_MFMA's fall-back
        p->waves = 4;
        p->grid[0] = (T + 63) / 64, p->grid[1] = H, p->grid[2] = 1;
    }
    if (form == FA_FORM_GRAPHT) {
        p->q16 = (kcpp_fa_workspace_bytes(T, H, nkv) + 255) & ~(int64_t)255;
        p->ws_bytes = p->q16 + (int64_t)T * H * D * 2;
    }
    return 0;
}
