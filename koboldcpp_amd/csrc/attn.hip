// attn.hip -- flash attention over the F16 KV cache (GGML_OP_FLASH_ATTN_EXT): the entries.
//
// Semantics: ggml_compute_forward_flash_attn_ext_f16 (reference ggml/src/ggml.c:15667-15875):
// Q is rounded to f16 (q_to_vec_dot), s = (q16 . k16) * scale + mask, softmax over the
// causal window, V-weighted sum.  The CPU accumulates V in f16 (ggml_vec_mad_f16); we keep
// f32 accumulators (strictly more accurate; parity within the f16 rounding of the CPU path).
// The reference GPU path (ggml/src/ggml-cuda/fattn-vec-f16.cuh:4-299) is a 32-lane vector
// kernel with half accumulators; this is a wave64 split-KV design instead.
// Every entry here is: check, plan (fa_plan.h fa_decode_plan says which kernel runs, its grid and its workspace
// layout), launch (attn_common.h: attn_chunk.hip, attn_dec.hip, attn_tile.hip; the matrix-core prefill of
// attn_mfma.hip), and kcpp_quantize_act where no combine wrote the quantized output.  The ggml-op (graph) forms at the
// end of the file also take the op's logit soft-cap and hand head dim 256 to attn_d256.hip.
#include "attn_common.h"

#include <algorithm>

// the planned launch; force_path: kcpp_flash_attn's (the MFMA entry's -3 runs the tiles unless 3 forced it)
static int fa_launch(const FaDecodePlan &p, const FaArgs &a, int force_path = 0) {
    switch (p.kernel) {
    case FA_DEC_CHUNK: return fa_chunk_launch(p, a);
    case FA_DEC_SPLIT4:
    case FA_DEC_SPLIT5: return fa_split_launch(p, a);
    case FA_DEC_SHORT: return fa_short_launch(p, a);
    case FA_DEC_MFMA: {
        const int rc = kcpp_flash_attn_prefill_mfma(a.q16, a.kc, a.vc, a.out, a.T, a.H, a.HKV, a.D, a.n_past, a.scale, a.s);
        if (rc != -3 || force_path == 3) return rc;
    }   // fall through
    default: return fa_tile_launch(p, a);
    }
}

extern "C" {

// partial O + (m, l) per (query, head, chunk / split) behind a 2048-B header
int64_t kcpp_fa_workspace_bytes(int T, int H, int n_kv_max) {
    const int64_t nch = (n_kv_max + FA_CHUNK - 1) / FA_CHUNK;
    // partial slots: T x nch chunks (k_fa_decode), at least the 64 splits the split pair may use
    const int64_t slots = std::max<int64_t>((int64_t)T * nch, FA_MAXS);
    return std::max<int64_t>(KCPP_FA_WS_HEADER + (int64_t)H * slots * (128 * 4 + 8) + (int64_t)T * H * 4 + 256,
                             kcpp_fa_split_ws_bytes(H));      // the key-split prefill (attn_mfma.hip)
}

// out = {kernel (FA_DEC_*), ns, nch, waves, grid x, y, z, combine grid x, y, combine threads, combine quantizer, then
// as (low, high) 32-bit halves: part_o, part_ml, ws_bytes, q16} (fa_plan.h FaDecodePlan)
int kcpp_fa_decode_plan(int form, int T, int H, int HKV, int D, int nkv, int n_rows, int qkind, int sel, int flags,
                        int32_t out[19]) {
    FaDecodePlan p;
    const int rc = fa_decode_plan(form, T, H, HKV, D, nkv, n_rows, qkind, sel, flags, &p);
    if (rc) return rc;
    const int32_t v[11] = {p.kernel, p.ns, p.nch, p.waves, p.grid[0], p.grid[1], p.grid[2], p.cgrid[0], p.cgrid[1],
                           p.cthreads, p.cquant};
    const int64_t w[4] = {p.part_o, p.part_ml, p.ws_bytes, p.q16};
    for (int i = 0; i < 11; ++i) out[i] = v[i];
    for (int i = 0; i < 4; ++i) { out[11 + 2 * i] = (int32_t)(w[i] & 0xFFFFFFFF); out[12 + 2 * i] = (int32_t)(w[i] >> 32); }
    return 0;
}

// the runtime forms' arguments: position-major cache, implicit causal mask
static FaArgs fa_runtime_args(const uint16_t *q16, const uint16_t *kc, const uint16_t *vc, float *out, void *qout, void *ws,
                              int T, int H, int HKV, int D, int n_past, const int32_t *n_past_dev, int n_kv_max, float scale,
                              void *stream) {
    FaArgs a = {};
    a.q16 = q16, a.kc = kc, a.vc = vc, a.kv_ld = (int64_t)HKV * 128, a.kv_hs = 128, a.mask_ld = -1;
    a.out = out, a.qout = qout, a.ws = ws, a.T = T, a.H = H, a.HKV = HKV, a.D = D;
    a.n_past = n_past, a.n_past_dev = n_past_dev, a.n_rows = n_past_dev ? n_kv_max : n_past + 1;
    a.scale = scale, a.s = (hipStream_t)stream;
    return a;
}

// single-token decode attention (the split pair) whose combine writes the KT_Q8_0_TA activation of one token
// (attn_output in the KT_Q8_0_T layout) instead of a separate kcpp_quantize_act; out f32 may be null.  -3: not covered
int kcpp_flash_attn_dec_ta(const uint16_t *q16, const uint16_t *kc, const uint16_t *vc, float *out, void *qta, void *ws,
                           int H, int HKV, int D, int n_past, const int32_t *n_past_dev, int n_kv_max, float scale,
                           void *stream) {
    if (D != 128 || H % HKV || H % 2 || !qta) return -3;
    const int G = H / HKV;
    if (G < 2 || G > FA_MAXG) return -3;
    const FaArgs a = fa_runtime_args(q16, kc, vc, out, qta, ws, 1, H, HKV, D, n_past, n_past_dev, n_kv_max, scale, stream);
    FaDecodePlan p;
    const int rc = fa_decode_plan(FA_FORM_RUNTIME, 1, H, HKV, D, a.n_rows, a.n_rows, 2, 1, 0, &p);
    return rc ? rc : fa_launch(p, a);
}

// out f32 [T][H][D] (may be null), qout Q8_K act [T][H*D] (may be null), ws from kcpp_fa_workspace_bytes
// n_past_dev (optional): device-resident n_past (graph-replayable decode); then n_kv_max
// bounds the grid and the kernels read the real n_past from memory.
// force_path 0: auto (T <= 16 decode kernels, else prefill), 1: decode kernels, 2: tiled prefill, 3: MFMA
// prefill, 6: the 64-key-chunk decode kernel even for T = 1 (tests), 7: single-pass decode (short contexts: the caller
// keeps n_kv <= KCPP_FA_SHORT_MAX)
int kcpp_flash_attn(const uint16_t *q16, const uint16_t *kc, const uint16_t *vc, float *out, void *qout, void *ws,
                    int T, int H, int HKV, int D, int n_past, const int32_t *n_past_dev, int n_kv_max, float scale,
                    int force_path, void *stream) {
    FaArgs a = fa_runtime_args(q16, kc, vc, out, qout, ws, T, H, HKV, D, n_past, n_past_dev, n_kv_max, scale, stream);
    FaDecodePlan p;
    int rc = fa_decode_plan(FA_FORM_RUNTIME, T, H, HKV, D, n_past_dev ? n_kv_max : n_past + T, a.n_rows, qout ? 1 : 0,
                            force_path, out ? 0 : FA_PLAN_NO_OUT, &p);
    if (rc) return rc;
    if (D == 128 && p.kernel >= FA_DEC_TILE) a.n_past_dev = nullptr;     // the D = 128 prefill kernels take the host's n_past
    rc = fa_launch(p, a, force_path);
    if (rc || !qout || p.cquant) return rc;
    return kcpp_quantize_act(KT_Q8_K, out, (int64_t)H * D, qout, (int64_t)H * D, T, stream);
}

// single-token decode attention with explicit cache strides (elements): key p of kv head hk starts at
// kc + p * kv_ld + hk * kv_hs.  Position-major ggml view: kv_ld = HKV*D, kv_hs = D; head-major: kv_ld = D,
// kv_hs = n_ctx*D.  variant 0: 64-key chunks + k_fa_combine; 3: k_fa_dec4 + k_fa_comb4 (the legacy pair);
// 5: k_fa_dec5 + k_fa_comb4 (the production pair; n_kv_max = the views' row count); 8: the short-context single launch
// (one workgroup per kv head, no combine; kcpp_flash_attn force_path 7); 6, 7: attn_dec.hip fa_dec_tool.  A/B entry for
// tools/fa_dec_bench.py.
int kcpp_fa_decode_ex(const uint16_t *q16, const uint16_t *kc, const uint16_t *vc, int64_t kv_ld, int64_t kv_hs,
                      float *out, void *qout, void *ws, int H, int HKV, int n_past, const int32_t *n_past_dev,
                      int n_kv_max, float scale, int variant, void *stream) {
    FaArgs a = fa_runtime_args(q16, kc, vc, out, qout, ws, 1, H, HKV, 128, n_past, n_past_dev, n_kv_max, scale, stream);
    a.kv_ld = kv_ld, a.kv_hs = kv_hs;
    FaDecodePlan p;
    const int rc = fa_decode_plan(FA_FORM_EX, 1, H, HKV, 128, a.n_rows, a.n_rows, qout ? 1 : 0, variant,
                                  out ? 0 : FA_PLAN_NO_OUT, &p);
    if (rc) return rc;
    if (variant == 6 || variant == 7) return fa_dec_tool(variant, a);
    return fa_launch(p, a);
}

// one query of GGML_OP_FLASH_ATTN_EXT in the graph form (the b1 backend's decode): k_fa_dec5<GRAPH> over the views
// (key j of kv head h at kc + j k_ld + h k_hs elements), the f16 mask row (may be null), q f32 [H][D] with head
// stride q_nb2 bytes rounded to f16 in the kernel, then k_fa_comb4 into out [H][D].  -3: shape not covered.
// logit_softcap != 0 (op_params[2], Gemma-2): s = cap * tanhf(q.k * scale / cap) before the mask.  D = 256: the
// kernels of attn_d256.hip.
int kcpp_flash_attn_ext_dec_sc(const float *q, int64_t q_nb2, const uint16_t *kc, const uint16_t *vc, int64_t k_ld,
                               int64_t k_hs, const uint16_t *mask, float *out, void *ws, int H, int HKV, int D, int n_kv,
                               float scale, void *stream, float logit_softcap) {
    if (D == 256)
        return kcpp_fa256_dec(q, 0, q_nb2, kc, vc, k_ld, k_hs, mask, 0, out, ws, 1, H, HKV, n_kv, scale, logit_softcap,
                              stream);
    FaDecodePlan p;
    if (fa_decode_plan(FA_FORM_GRAPH1, 1, H, HKV, D, n_kv, n_kv, 0, 0, logit_softcap != 0.0f ? FA_PLAN_CAP : 0, &p)) return -3;
    if (q_nb2 % 16 || ((uintptr_t)q & 15) || !mask) return -3;        // (llama.cpp always passes the KQ mask)
    FaArgs a = {};
    a.qf = q, a.qf_hs = q_nb2 / 4, a.kc = kc, a.vc = vc, a.kv_ld = k_ld, a.kv_hs = k_hs, a.mask = mask;
    a.out = out, a.ws = ws, a.T = 1, a.H = H, a.HKV = HKV, a.D = D, a.n_past = n_kv - 1, a.n_rows = n_kv;
    a.scale = scale, a.cap = logit_softcap, a.s = (hipStream_t)stream;
    return fa_launch(p, a);
}
int kcpp_flash_attn_ext_dec(const float *q, int64_t q_nb2, const uint16_t *kc, const uint16_t *vc, int64_t k_ld,
                            int64_t k_hs, const uint16_t *mask, float *out, void *ws, int H, int HKV, int D, int n_kv,
                            float scale, void *stream) {
    return kcpp_flash_attn_ext_dec_sc(q, q_nb2, kc, vc, k_ld, k_hs, mask, out, ws, H, HKV, D, n_kv, scale, stream, 0.0f);
}

// GGML_OP_FLASH_ATTN_EXT as the ggml graph states it (the b1 backend path): q f32 [D][T][H] with byte
// strides (q_nb1 between queries, q_nb2 between heads), K/V f16 cache views [n_kv][HKV][D] (row stride
// HKV*D), mask f16 [T_pad][n_kv] (row stride mask_ld elements, 0 / -inf, may be null = no mask), out f32
// [T][H][D].  Q is rounded to f16 first (q_to_vec_dot of ggml_compute_forward_flash_attn_ext_f16,
// ggml.c:15667); keys whose mask is -inf are skipped.  ws: kcpp_fa_workspace_bytes(T, H, n_kv) + T*H*D*2.
int64_t kcpp_fa_ext_workspace_bytes(int T, int H, int n_kv, int D) {
    if (D > 128) return kcpp_fa256_ws_bytes(T, H);      // 256 floats per partial (attn_d256.hip)
    return ((kcpp_fa_workspace_bytes(T, H, n_kv) + 255) & ~(int64_t)255) + (int64_t)T * H * D * 2 + 256;
}

__global__ void k_q_to_f16(const char *__restrict__ q, int64_t nb1, int64_t nb2, int T, int H, int D,
                           uint16_t *__restrict__ q16) {
    const int t = blockIdx.x, h = blockIdx.y;
    for (int d = threadIdx.x; d < D; d += blockDim.x)
        q16[((int64_t)t * H + h) * D + d] = f2h(((const float *)(q + t * nb1 + h * nb2))[d]);
}

// logit_softcap != 0 (D = 128 or 256): s = cap * tanhf(q.k * scale / cap) before the mask (ggml.c:15738-15810)
int kcpp_flash_attn_ext_sc(const float *q, int64_t q_nb1, int64_t q_nb2, const uint16_t *kc, const uint16_t *vc,
                           const uint16_t *mask, int64_t mask_ld, float *out, void *ws, int T, int H, int HKV, int D,
                           int n_kv, float scale, void *stream, float logit_softcap) {
    hipStream_t s = (hipStream_t)stream;
    if (D == 256) {
        if (H % HKV || n_kv < 1 || T < 1) return -1;
        if (mask_ld < 0) mask_ld = 0;
        // up to 16 queries: the split decode kernel, one grid plane per query; more: the MFMA tile kernel
        // (a GQA ratio the decode kernel is not built for: the tile kernel, which takes any)
        if (T <= 16) {
            const int rc = kcpp_fa256_dec(q, q_nb1, q_nb2, kc, vc, (int64_t)HKV * 256, 256, mask, mask_ld, out, ws, T, H,
                                          HKV, n_kv, scale, logit_softcap, stream);
            if (rc != -3) return rc;
        }
        return kcpp_fa256_prefill(q, q_nb1, q_nb2, kc, vc, mask, mask_ld, out, T, H, HKV, n_kv, scale, logit_softcap,
                                  stream);
    }
    FaDecodePlan p;
    const int rc = fa_decode_plan(FA_FORM_GRAPHT, T, H, HKV, D, n_kv, n_kv, 0, 0, logit_softcap != 0.0f ? FA_PLAN_CAP : 0, &p);
    if (rc) return rc;
    uint16_t *q16 = (uint16_t *)((uint8_t *)ws + p.q16);
    hipLaunchKernelGGL(k_q_to_f16, dim3(T, H), dim3(128), 0, s, (const char *)q, q_nb1, q_nb2, T, H, D, q16);
    KCPP_CHECK(hipGetLastError());
    FaArgs a = {};
    a.q16 = q16, a.kc = kc, a.vc = vc, a.kv_ld = (int64_t)HKV * 128, a.kv_hs = 128, a.mask = mask;
    a.mask_ld = mask_ld < 0 ? 0 : mask_ld, a.out = out, a.ws = ws, a.T = T, a.H = H, a.HKV = HKV, a.D = D;
    a.n_past = n_kv, a.n_rows = n_kv, a.scale = scale, a.cap = logit_softcap, a.s = s;
    return fa_launch(p, a);
}
int kcpp_flash_attn_ext(const float *q, int64_t q_nb1, int64_t q_nb2, const uint16_t *kc, const uint16_t *vc,
                        const uint16_t *mask, int64_t mask_ld, float *out, void *ws, int T, int H, int HKV, int D,
                        int n_kv, float scale, void *stream) {
    return kcpp_flash_attn_ext_sc(q, q_nb1, q_nb2, kc, vc, mask, mask_ld, out, ws, T, H, HKV, D, n_kv, scale, stream,
                                  0.0f);
}

}  // extern "C"
