// fa_plan.h -- which prefill attention kernel runs a shape at D = 128, and with what grid.  Host-only plain C++ (no
// HIP), the idiom of gemm_plan.h: attn_mfma.hip launches what this says (grid, ch, nsp), attn.hip and runtime.cpp ask it
// whether the MFMA kernel takes a GQA ratio, kcpp_fa_prefill_plan exposes it, tests/test_fa_prefill_plan.py checks it
// without a GPU.
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
