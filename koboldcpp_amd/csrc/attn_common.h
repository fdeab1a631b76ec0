// attn_common.h -- shared by the flash attention's translation units (attn.hip and one attn_*.hip per kernel family):
// the arguments of a launch, the compile-time dispatch over the GQA ratio, and the host interface between the entries
// (attn.hip) and each family's launcher.  What runs, its grid and its workspace layout come from fa_plan.h.
#pragma once
#include "kcpp_common.h"
#include "kcpp_internal.h"

#include <cstdlib>
#include <type_traits>

// K/V cache: key p of kv head hk at kc + p * kv_ld + hk * kv_hs elements (position-major: kv_ld = HKV * D, kv_hs = D).
// Query t sits at absolute position n_past + t under the implicit causal mask (mask_ld < 0); under the ggml op's
// explicit mask (mask_ld >= 0, mask may be null) every query sees the n_past = n_rows = n_kv keys the mask leaves.
struct FaArgs {
    const uint16_t *q16;         // Q f16 [T][H][D]
    const float *qf;             // the one-query graph form: Q f32, head stride qf_hs floats (q16 null)
    int64_t qf_hs;
    const uint16_t *kc, *vc;
    int64_t kv_ld, kv_hs;
    const uint16_t *mask;        // f16 rows of mask_ld elements
    int64_t mask_ld;
    float *out;                  // f32 [T][H][D], may be null where a launcher writes qout
    void *qout;                  // quantized activation (the plan's cquant), may be null
    void *ws;
    int T, H, HKV, D;
    int n_past;
    const int32_t *n_past_dev;   // device-resident n_past (graph-replayable decode), may be null
    int n_rows;                  // rows the K/V views hold
    float scale, cap;            // cap != 0: the op's logit soft-cap
    hipStream_t s;
};

// f(std::integral_constant<int, G>) for the G of the allowed list; -3 for a ratio no kernel is built for
template <int... Allowed, class F>
static inline int fa_for_g(int G, F &&f) {
    int rc = -3;
    (void)((G == Allowed ? (f(std::integral_constant<int, Allowed>{}), rc = 0, true) : false) || ...);
    return rc;
}
// the same over the split count of k_fa_comb4
template <int... Allowed, class F>
static inline int fa_for_ns(int NS, F &&f) {
    return fa_for_g<Allowed...>(NS, f);
}

// attn_chunk.hip: FA_DEC_CHUNK, implicit or explicit mask, with or without cap
int fa_chunk_launch(const FaDecodePlan &p, const FaArgs &a);
// attn_dec.hip: FA_DEC_SPLIT4 / FA_DEC_SPLIT5 (a.qf: the graph form), FA_DEC_SHORT, and kcpp_fa_decode_ex's variants
// 6 / 7 (the tools' A/B forms of k_fa_dec5)
int fa_split_launch(const FaDecodePlan &p, const FaArgs &a);
int fa_short_launch(const FaDecodePlan &p, const FaArgs &a);
int fa_dec_tool(int variant, const FaArgs &a);
// attn_tile.hip: FA_DEC_TILE, D 64 or 128, implicit or explicit mask, with or without cap
int fa_tile_launch(const FaDecodePlan &p, const FaArgs &a);
