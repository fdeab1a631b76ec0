"""ctypes binding of koboldcpp_hipblas.so (include/kcpp_mi355x.h).

Host-side mirror of the reference's operator interface for this path: the same ggml type ids,
the same op semantics (mul_mat / rms_norm / rope_ext / flash_attn_ext) and the same error
behaviour (a non-zero return is raised as KcppError instead of aborting the process).
Fails loudly when the native library is absent -- there is no Python/CPU fallback.
"""
import ctypes
import os

from . import LIB_PATH

F32, F16, Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q8_1, Q2_K, Q3_K, Q4_K, Q5_K, Q6_K, Q8_K = 0, 1, 2, 3, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15
IQ4_NL, IQ4_XS = 20, 23
# device-internal row-major decode layouts of Q4_K / Q6_K (include/kcpp_synth.h; never ggml ids)
Q4_K_RS, Q5_K_RS, Q6_K_RS = 112, 113, 114
# device-internal Q8_0 tile layout and its activation layout (kcpp_common.h, csrc/gemm_q80t.hip)
Q8_0_T, Q8_0_TA = 115, 116
BLOCK = {F32: (1, 4), F16: (1, 2), Q4_0: (32, 18), Q4_1: (32, 20), Q5_0: (32, 22), Q5_1: (32, 24), Q8_0: (32, 34), Q8_1: (32, 36), Q2_K: (256, 84), Q3_K: (256, 110), Q4_K: (256, 144),
         Q5_K: (256, 176), Q6_K: (256, 210), Q8_K: (256, 292), Q4_K_RS: (256, 144), Q5_K_RS: (256, 176), Q6_K_RS: (256, 210),
         IQ4_NL: (32, 18), IQ4_XS: (256, 136), Q8_0_T: (32, 34)}
# the lattice-grid types (ggml-common.h:340-405), kept in the ggml layout on the device (csrc/iq_grid.h)
IQ2_XXS, IQ2_XS, IQ3_XXS, IQ1_S, IQ3_S, IQ2_S, IQ1_M = 16, 17, 18, 19, 21, 22, 29
BLOCK.update({IQ2_XXS: (256, 66), IQ2_XS: (256, 74), IQ2_S: (256, 82), IQ3_XXS: (256, 98), IQ3_S: (256, 110),
              IQ1_S: (256, 50), IQ1_M: (256, 56)})


class KcppError(RuntimeError):
    pass


if not os.path.exists(LIB_PATH):
    raise ImportError("native library missing: %s (run __graft_entry__.build())" % LIB_PATH)

_L = ctypes.CDLL(LIB_PATH)
P, I, I64, U64, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_float

_SIGS = {
    "kcpp_weight_repack": [I, P, P, I64, I64, I, P],
    "kcpp_weight_synth": [I, U64, U64, P, I64, I64, P],
    "kcpp_dequantize": [I, P, P, I64, I64, P],
    "kcpp_get_rows": [I, P, I64, I64, P, I64, P, I64, P],
    "kcpp_quantize_act": [I, P, I64, P, I64, I64, P],
    "kcpp_quantize_act_glu": [P, I64, I64, P, I64, I64, P],
    "kcpp_gemv": [I, P, P, I64, I64, P, I64, P, I64, P, I64, I, P],
    "kcpp_gemm": [I, P, P, I64, I64, P, I64, P, I64, P, I64, I, P, P],
    "kcpp_q6p_image_bytes": [I64, I64],
    "kcpp_gemm_rms_norm": [I, P, I64, I64, P, I64, P, I64, P, I64, P, P, P, Fl, P],
    "kcpp_gemm_q6p_rms_norm": [P, P, I64, I64, P, I64, P, I64, P, I64, P, P, P, Fl, P],
    "kcpp_reduce_rms_norm": [P, I, I64, P, I64, P, I64, P, P, I64, I64, Fl, P],
    "kcpp_q6p_build": [P, I64, I64, P, P],
    "kcpp_gemm_q6p": [P, P, P, P, I64, I64, P, I64, P, I64, P, I64, I, P, P],
    "kcpp_rms_norm": [P, I64, P, P, I64, P, I64, I64, Fl, P],
    "kcpp_rms_norm_q80": [P, I64, P, P, I64, I64, Fl, P],
    "kcpp_gemm_q80_glu_q80": [P, P, I64, I64, P, I64, P, P, P],
    "kcpp_rope_table": [P, I, I, Fl, Fl, P, Fl, Fl, Fl, Fl, I],
    "kcpp_rope_row": [P, I, I, Fl, Fl, Fl, Fl, Fl, Fl, I],
    "kcpp_kv_shift_rows": [P, P, P, P, I64, I, P, P],
    "kcpp_moe_route_norm": [P, I64, P, Fl, P, I, I64, I, I, P, P, I, P],
    "kcpp_model_kv_shift": [P, I, I, I],
    "kcpp_rope_kv": [P, I64, P, P, P, P, I, I, I, I, I, P, P, P],
    "kcpp_rope_kv_ex": [P, I64, P, P, P, P, I, I, I, I, I, P, P, I, P, P, P, P],
    "kcpp_kv_shift_rows_ex": [P, P, P, P, I64, I, P, I, P],
    "kcpp_rope_qk_inplace_ex": [P, I64, I, I, I, I, I, P, P, I, P, P, P, P],
    "kcpp_model_set_rope_mode": [P, I],
    "kcpp_model_set_norm_mode": [P, I],
    "kcpp_model_set_parallel_block": [P, I],
    "kcpp_model_set_logit_scale": [P, Fl],
    "kcpp_layer_norm": [P, I64, P, P, I64, P, I64, I64, Fl, P],
    "kcpp_layer_norm_q80": [P, I64, P, P, I64, I64, Fl, I, P],
    "kcpp_scale": [P, Fl, I64, P],
    "kcpp_gemv_rs_qkv_mixed_pro": [P, I, P],
    "kcpp_model_set_qkv_bias": [P, I, P, P, P],
    "kcpp_flash_attn": [P, P, P, P, P, P, I, I, I, I, I, P, I, Fl, I, P],
    "kcpp_flash_attn_prefill_mfma": [P, P, P, P, I, I, I, I, I, Fl, P],
    "kcpp_flash_attn_prefill_mfma_ex": [P, P, P, P, P, P, I, I, I, I, I, Fl, P],
    "kcpp_fa_split_ws_bytes": [I],
    "kcpp_fa_prefill_plan": [I, I, I, I, I, I, P],
    "kcpp_fa_decode_plan": [I, I, I, I, I, I, I, I, I, I, P],
    "kcpp_gemv_dec_plan": [I, I, I64, I, I64, I64, I64, I, I, I, I, I, I, I, I, I, I, P],
    "kcpp_gemv_qkv_mixed_plan": [I64, I64, I64, I64, I, I, I, I, I, P],
    "kcpp_gemv_qkv_mixed_plan_pro": [I64, I64, I64, I64, I, I, I, I, I, I, P],
    "kcpp_gemv_qkv_dual_plan": [I, I64, I, P, I, I64, I, P, I, P],
    "kcpp_flash_attn_dec_ta": [P, P, P, P, P, P, I, I, I, I, P, I, Fl, P],
    "kcpp_fa_decode_ex": [P, P, P, I64, I64, P, P, P, I, I, I, P, I, Fl, I, P],
    "kcpp_fa_set_stamps": [P],
    "kcpp_gguf_check": [ctypes.c_char_p, ctypes.c_char_p, I],
    "kcpp_pretokenize": [ctypes.c_char_p, ctypes.c_char_p, P, I],
    "kcpp_tokenize_probe": [ctypes.c_char_p, ctypes.c_char_p, I, P, I],
    "kcpp_pieces_probe": [ctypes.c_char_p, P, I64, P, I],
    "kcpp_tokenizer_special_ids": [ctypes.c_char_p, P],
    "kcpp_engine_bench": [P, P, I, I, P, U64, I, I, I, I, P],
    "kcpp_engine_bench_ex": [P, P, P, I, I, P, U64, I, I, I, I, P],
    "kcpp_expose_synth_weights": [U64],
    "kcpp_gemm_q80t": [P, P, I, P, I64, P, I64, P, I64, P, I64, I, P, P, P],
    "kcpp_gemm_q80t_qkv_rope": [P, P, I64, P, I64, P, I, P, I, P, P, P, P, P],
    "kcpp_rms_norm_q80t": [P, I64, P, P, I64, I64, Fl, P],
    "kcpp_q80t_ws_bytes": [I64, I64, I64],
    "kcpp_pipeline_trace": [I, I, I, I, I, ctypes.c_char_p, I],
    "kcpp_split_layers": [I, I, P, P],
    "kcpp_model_argmax_async": [P],
    "kcpp_model_step_dev": [P, I],
    "kcpp_add": [P, P, P, I64, P],
    "kcpp_silu_mul": [P, P, P, I64, P],
    "kcpp_moe_route": [P, I64, P, I, I64, I, I, P, P, I, P],
    "kcpp_moe_route_ex": [P, I64, P, I, I64, I, I, I, P, I, P, P, P, I, P],
    "kcpp_moe_route_norm_ex": [P, I64, P, Fl, P, I, I64, I, I, I, P, I, P, P, P, I, P],
    "kcpp_moe_combine_shexp": [P, P, I64, I, P, P, I64, I, P],
    "kcpp_moe_gather": [P, I64, P, I, I64, P, P],
    "kcpp_moe_scatter": [P, I64, P, P, P, I, I64, P],
    "kcpp_moe_combine": [P, P, I64, I, I64, P],
    "kcpp_ggml_binary": [I, P, P, P, P, P, P, P],
    "kcpp_ggml_unary": [I, P, P, P, P, Fl, P],
    "kcpp_ggml_cpy": [I, P, P, I, P, P, P],
    "kcpp_ggml_rms_norm": [P, P, P, P, Fl, P],
    "kcpp_ggml_rms_norm_mul": [P, P, P, P, P, P, P, P, Fl, P],
    "kcpp_ggml_rope": [P, P, P, P, P, P, I, I, I, Fl, Fl, Fl, Fl, Fl, Fl, P],
    "kcpp_ggml_rope_f16": [P, P, P, P, P, P, P, I, I, I, Fl, Fl, Fl, Fl, Fl, Fl, P],
    "kcpp_ggml_soft_max": [P, P, P, I, I64, I64, P, P, Fl, P],
    "kcpp_ggml_argsort": [P, P, P, I64, I, P],
    "kcpp_ggml_sum_rows": [P, P, P, P, P],
    "kcpp_ggml_get_rows": [I, P, P, P, P, P, P, P],
    "kcpp_ggml_mul_mat_f": [I, P, P, P, P, P, P, P],
    "kcpp_flash_attn_ext": [P, I64, I64, P, P, P, I64, P, P, I, I, I, I, I, Fl, P],
    "kcpp_flash_attn_ext_sc": [P, I64, I64, P, P, P, I64, P, P, I, I, I, I, I, Fl, P, Fl],
    "kcpp_flash_attn_ext_dec_sc": [P, I64, P, P, I64, I64, P, P, P, I, I, I, I, Fl, P, Fl],
    "kcpp_ggml_gelu_table_init": [],
    "kcpp_model_create": [P, P, I, I, I, I, I, I],
    "kcpp_model_create_ex": [P, P, P, I, I, I, I, I, I],
    "kcpp_model_synth_weights": [P, U64],
    "kcpp_model_set_tensor": [P, I, P, I64],
    "kcpp_model_free": [P],
    "kcpp_model_decode": [P, P, I, I, P],
    "kcpp_model_decode_async": [P, P, I, I],
    "kcpp_model_device": [P],
    "kcpp_model_hidden": [P],
    "kcpp_model_read_hidden": [P, P, I64, I64],
    "kcpp_model_stream": [P],
    "kcpp_model_hidden_io": [P, P, I64, I64, I],
    "kcpp_model_sync": [P],
    "kcpp_model_read_logits": [P, P],
    "kcpp_model_forward_hidden": [P, I, I],
    "kcpp_model_argmax": [P, P],
    "kcpp_model_decode_greedy": [P, I, P],
    "kcpp_model_decode_greedy_lagged": [P, I, P],
    "kcpp_model_greedy_drain": [P, P],
    "kcpp_model_set_graphs": [P, I],
    "kcpp_model_set_fused_decode": [P, I],
    "kcpp_model_set_row_split": [P, I, P, P],
    "kcpp_row_split_range": [I64, I, P, I, P, P],
    "kcpp_gemm_plan": [I, I64, I64, I64, I, I, P],
    "kcpp_model_set_fa_exact": [P, I],
    "kcpp_model_set_rope_freqs": [P, P, I],
    "kcpp_gradient_ai_rope_base": [Fl, I, I, I],
    "kcpp_model_moe_ids": [P, P, I],
    "kcpp_model_moe_trace": [P, I],
    "kcpp_model_moe_trace_read": [P, P, I],
    "kcpp_model_set_fused_route": [P, I],
    "kcpp_model_fused_route_count": [P],
    "kcpp_model_set_moe_grouped": [P, I],
    "kcpp_model_moe_grouped_count": [P],
    "kcpp_gemm_grouped": [I, P, P, I64, I64, I64, P, I64, P, P, I, P, P, I, P, P],
    "kcpp_gemm_grouped_ws_bytes": [I, I64, I64, I],
    "kcpp_flash_attn_exact": [P, P, P, P, I, I, I, I, I, P, Fl, P],
    "kcpp_flash_attn_ext_exact": [P, I64, I64, P, P, P, I64, P, I, I, I, I, I, Fl, P],
    "kcpp_flash_attn_ext_exact_sc": [P, I64, I64, P, P, P, I64, P, I, I, I, I, I, Fl, P, Fl],
    "kcpp_model_weight_bytes": [P],
    "kcpp_model_set_kv_types": [P, I, I],
    "kcpp_rope_qk_inplace": [P, I64, I, I, I, I, I, P, P, P],
    "kcpp_kv_store_q": [I, I, P, I64, I64, I64, I, I64, P, P, I64, I, P, P],
    "kcpp_flash_attn_q": [I, I, P, I64, P, P, P, I, I, I, I, I64, I, P, Fl, P],
    "kcpp_logit_candidates": [P, I, I, P, I, P, I, P, I, P, P, P, I, P],
    "kcpp_model_candidates": [P, I, P, I, P, I, P, I, P, P, P, I],
    "kcpp_cand_plan": [I64, P],
    "kcpp_cand_front_ref": [P, I, I, P, I, P, I, P, I, P, P, P, I],
    "kcpp_expose_set_sample_front": [I],
    "kcpp_expose_sample_front_stats": [P],
    "kcpp_expose_last_tokens": [P, I],
    "kcpp_expose_mirostat_mu": [I, Fl],
    "kcpp_logit_candidates_masked": [P, I, I, P, I, P, I, P, I, P, P, P, P, I, P],
    "kcpp_model_candidates_masked": [P, I, P, I, P, I, P, I, P, P, P, P, I],
    "kcpp_cand_front_ref_masked": [P, I, I, P, I, P, I, P, I, P, P, P, P, I],
    "kcpp_model_argmax_masked": [P, P, P, P],
    "kcpp_logit_argmax_masked": [P, I, P, P, P, P],
    "kcpp_expose_grammar_stats": [P],
    "kcpp_expose_grammar_mask_ms": [],
    "kcpp_grammar_create": [ctypes.c_char_p],
    "kcpp_grammar_free": [P],
    "kcpp_grammar_rules": [P, P, I, P, I, P],
    "kcpp_grammar_n_stacks": [P],
    "kcpp_grammar_reject": [P, P, P, I, I, I, I, P],
    "kcpp_grammar_accept_piece": [P, P, I, I],
    "kcpp_grammar_partial": [P, P],
}
_RES = {"kcpp_gradient_ai_rope_base": Fl, "kcpp_q6p_image_bytes": I64, "kcpp_model_fused_route_count": I64, "kcpp_model_moe_grouped_count": I64, "kcpp_gemm_grouped_ws_bytes": I64, "kcpp_fa_split_ws_bytes": I64, "kcpp_q80t_ws_bytes": I64, "kcpp_act_bytes": I64, "kcpp_fa_ext_workspace_bytes": I64, "kcpp_fa_workspace_bytes": I64, "kcpp_gemm_workspace_bytes": I64,
        "kcpp_model_create": P, "kcpp_model_create_ex": P, "kcpp_model_hidden": P, "kcpp_model_stream": P, "kcpp_model_weight_bytes": I64,
        "kcpp_last_error": ctypes.c_char_p, "kcpp_model_free": None, "kcpp_fa_set_stamps": None,
        "kcpp_expose_set_sample_front": None, "kcpp_expose_sample_front_stats": None, "kcpp_expose_mirostat_mu": Fl,
        "kcpp_expose_grammar_stats": None, "kcpp_expose_grammar_mask_ms": ctypes.c_double, "kcpp_grammar_create": P,
        "kcpp_grammar_free": None, "kcpp_grammar_partial": None}
_L.kcpp_act_bytes.argtypes = [I, I64, I64]
_L.kcpp_kv_cache_bytes.argtypes = [I, I64, I64]
_L.kcpp_kv_cache_bytes.restype = I64
_L.kcpp_fa_workspace_bytes.argtypes = [I, I, I]
_L.kcpp_fa_ext_workspace_bytes.argtypes = [I, I, I, I]
_L.kcpp_gemm_workspace_bytes.argtypes = [I, I64, I64, I64]
_L.kcpp_vec_dot_type.argtypes = [I]
_L.kcpp_gemv_dec.argtypes = [I, P, I, I, I, P]
_L.kcpp_gemv_dec_args_size.restype = I64
_L.kcpp_gemv_stream.argtypes = [I, P, I, I, P]
_L.kcpp_gemv_q4k.argtypes = [P, I, I, P]
_L.kcpp_gemv_rs.argtypes = [I, P, I, I, P]
_L.kcpp_rs_supported.argtypes = [I, I64]
for _n, _a in _SIGS.items():
    getattr(_L, _n).argtypes = _a
for _n, _r in _RES.items():
    getattr(_L, _n).restype = _r


def exported_symbols():
    return sorted(set(_SIGS) | set(_RES) | {"kcpp_vec_dot_type", "kcpp_gemv_dec", "kcpp_gemv_dec_args_size",
                                             "kcpp_gemv_stream", "kcpp_gemv_q4k",
                                             "kcpp_gemv_rs", "kcpp_rs_supported"})


def raw():
    return _L


def _chk(rc, name):
    if rc != 0:
        raise KcppError("%s failed rc=%d: %s" % (name, rc, (_L.kcpp_last_error() or b"").decode()))


def call(name, *args):
    _chk(getattr(_L, name)(*args), name)


def row_bytes(t, k):
    e, b = BLOCK[t]
    return k // e * b


def act_bytes(wtype, K, M):
    return int(_L.kcpp_act_bytes(wtype, K, M))


def vec_dot_type(wtype):
    return int(_L.kcpp_vec_dot_type(wtype))


def fa_workspace_bytes(T, H, n_kv):
    return int(_L.kcpp_fa_workspace_bytes(T, H, n_kv))


class TDesc(ctypes.Structure):
    """struct kcpp_tdesc: ggml shape ne[4] and byte strides nb[4] (innermost first)"""
    _fields_ = [("ne", I64 * 4), ("nb", I64 * 4)]


def tdesc(t):
    """kcpp_tdesc of a torch tensor (any strides): ne/nb are the reversed shape/strides, in bytes"""
    shape, strides = list(t.shape)[::-1], [s * t.element_size() for s in t.stride()][::-1]
    while len(shape) < 4:
        shape.append(1)
        strides.append(strides[-1] * shape[-2] if strides else t.element_size())
    d = TDesc()
    for i in range(4):
        d.ne[i], d.nb[i] = int(shape[i]), int(strides[i])
    return d


def fa_ext_workspace_bytes(T, H, n_kv, D=128):
    return int(_L.kcpp_fa_ext_workspace_bytes(T, H, n_kv, D))


class DecArgs(ctypes.Structure):
    """mirror of struct DecArgs (koboldcpp_amd/csrc/kcpp_internal.h), checked against
    kcpp_gemv_dec_args_size() at import"""
    _fields_ = [("W", P * 3), ("Y", P * 3), ("N", I64 * 3), ("role", I * 3), ("nseg", I), ("W2", P), ("K", I64),
                ("act", P), ("x", P), ("nw", P), ("eps", Fl), ("res", P), ("q16", P), ("kc", P), ("vc", P),
                ("ekv", I64), ("D", I), ("pos", P), ("rope_tab", P), ("eid", P), ("ebytes", I64), ("escale", P),
                ("act_mtot", I64), ("act_col", I64), ("n_exp", I64), ("pre", P), ("eid1", P),
                ("route_w", P), ("route_wt", I), ("route_ne", I), ("route_ids", P), ("route_wts", P),
                ("bias", P * 3), ("rope_neox", I)]


if ctypes.sizeof(DecArgs) != _L.kcpp_gemv_dec_args_size():
    raise ImportError("DecArgs layout mismatch: %d vs %d" % (ctypes.sizeof(DecArgs), _L.kcpp_gemv_dec_args_size()))


def gemv_dec(wtype, args, mode, pro, rows_per_wave, stream):
    """fused single-token mat-vec; returns the native rc (-8 = K too large for the fused kernel)"""
    return int(_L.kcpp_gemv_dec(wtype, ctypes.byref(args), mode, pro, rows_per_wave, stream))


class HParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int) for n in ("n_vocab", "n_embd", "n_head", "n_head_kv", "n_layer", "n_ff", "n_ctx")] + \
               [(n, ctypes.c_float) for n in ("eps", "rope_base", "rope_freq_scale")] + \
               [(n, ctypes.c_int) for n in ("n_expert", "n_expert_used")]


def hparams(hp):
    return HParams(*[int(hp[n]) for n in ("n_vocab", "n_embd", "n_head", "n_head_kv", "n_layer", "n_ff", "n_ctx")],
                   float(hp["eps"]), float(hp["rope_base"]), float(hp.get("rope_freq_scale", 1.0)),
                   int(hp.get("n_expert", 0)), int(hp.get("n_expert_used", 0)))


class ModelEx(ctypes.Structure):
    """kcpp_model_ex: what build_qwen2moe needs beside kcpp_hparams"""
    _fields_ = [("n_ff_shexp", ctypes.c_int), ("moe_norm_w", ctypes.c_int)]


def engine_bench(hp, types, n_dev, n_prompt, ubatch, n_warm, n_steps, seed=1234, tensor_split=None):
    """the drop-in engine (load_model's layer-split stages over n_dev GPUs, RCCL / copy hand-off, greedy tokens moved
    home on device) on synthetic weights: {prefill_s, decode_s, n_past, rccl}"""
    h = hparams(hp)
    t = (ctypes.c_int * len(types))(*types)
    ts = (ctypes.c_float * 16)(*((tensor_split or [1.0] * n_dev) + [0.0] * (16 - n_dev)))
    out = (ctypes.c_double * 4)()
    if "n_ff_shexp" in hp or "moe_norm_w" in hp:          # qwen2moe shapes: kcpp_model_create_ex's extension
        ex = ModelEx(int(hp.get("n_ff_shexp", 0)), int(hp.get("moe_norm_w", 1)))
        _chk(_L.kcpp_engine_bench_ex(ctypes.byref(h), ctypes.byref(ex), t, len(types), n_dev, ts, seed, n_prompt, ubatch,
                                     n_warm, n_steps, out), "engine_bench_ex")
    else:
        _chk(_L.kcpp_engine_bench(ctypes.byref(h), t, len(types), n_dev, ts, seed, n_prompt, ubatch, n_warm, n_steps, out),
             "engine_bench")
    return {"prefill_s": out[0], "decode_s": out[1], "n_past": int(out[2]), "rccl": bool(out[3])}


class Model:
    """One pipeline stage of a Llama model on one GPU (kcpp_model_*)."""

    def __init__(self, hp, types, device=0, il0=0, il1=None, has_embed=True, has_output=True, max_ubatch=512):
        self.hp = dict(hp)
        self._h = hparams(hp)
        self._t = (ctypes.c_int * len(types))(*types)
        il1 = hp["n_layer"] if il1 is None else il1
        if "n_ff_shexp" in hp or "moe_norm_w" in hp:      # qwen2moe: a shared expert, raw top-k weights
            self._ex = ModelEx(int(hp.get("n_ff_shexp", 0)), int(hp.get("moe_norm_w", 1)))
            self.m = _L.kcpp_model_create_ex(ctypes.byref(self._h), ctypes.byref(self._ex), self._t, device, il0, il1,
                                             int(has_embed), int(has_output), max_ubatch)
        else:
            self.m = _L.kcpp_model_create(ctypes.byref(self._h), self._t, device, il0, il1, int(has_embed),
                                          int(has_output), max_ubatch)
        if not self.m:
            raise KcppError("kcpp_model_create%s failed: %s" % ("_ex" if hasattr(self, "_ex") else "",
                                                                (_L.kcpp_last_error() or b"").decode()))

    def kv_shift(self, p0, diff, n_past):
        """context shift: cache rows [p0+diff, n_past) -> [p0, n_past-diff), K re-rotated by -diff"""
        _chk(_L.kcpp_model_kv_shift(self.m, p0, diff, n_past), "kv_shift")

    def synth(self, seed):
        _chk(_L.kcpp_model_synth_weights(self.m, seed), "synth")

    def set_tensor(self, idx, arr):
        _chk(_L.kcpp_model_set_tensor(self.m, idx, arr.ctypes.data_as(P), arr.nbytes), "set_tensor")

    def decode(self, tokens, n_past, want_logits=True, n_tokens=None):
        """llama_decode of len(tokens) tokens at n_past.  A stage without the embedding takes
        tokens=None and n_tokens=T: its input is the residual stream placed with hidden_io."""
        import numpy as np
        if tokens is None:
            tok, T = None, int(n_tokens)
        else:
            tok = np.ascontiguousarray(tokens, dtype=np.int32)
            T = len(tok)
        logits = np.empty(self.hp["n_vocab"], np.float32) if want_logits else None
        _chk(_L.kcpp_model_decode(self.m, tok.ctypes.data_as(P) if tok is not None else None, T, n_past,
                                  logits.ctypes.data_as(P) if want_logits else None), "decode")
        return logits

    def decode_async(self, tokens, n_past, n_tokens=None):
        """enqueue the decode on the stage stream without a host sync (prefill ubatches of a pipeline); the
        token array is copied before this returns"""
        import numpy as np
        if tokens is None:
            tok, T = None, int(n_tokens)
        else:
            tok = np.ascontiguousarray(tokens, dtype=np.int32)
            T = len(tok)
        _chk(_L.kcpp_model_decode_async(self.m, tok.ctypes.data_as(P) if tok is not None else None, T, n_past),
             "decode_async")

    def argmax(self):
        v = ctypes.c_int32(0)
        _chk(_L.kcpp_model_argmax(self.m, ctypes.byref(v)), "argmax")
        return v.value

    def decode_greedy(self, n_past):
        """one greedy step on the device-resident previous argmax; returns this step's token"""
        v = ctypes.c_int32(0)
        _chk(_L.kcpp_model_decode_greedy(self.m, n_past, ctypes.byref(v)), "decode_greedy")
        return v.value

    def decode_greedy_lagged(self, n_past):
        """one greedy step, the host one token behind: returns the previous step's token (-1 after a drain)"""
        v = ctypes.c_int32(0)
        _chk(_L.kcpp_model_decode_greedy_lagged(self.m, n_past, ctypes.byref(v)), "decode_greedy_lagged")
        return v.value

    def greedy_drain(self):
        """the last lagged step's token; resets the readback ring"""
        v = ctypes.c_int32(0)
        _chk(_L.kcpp_model_greedy_drain(self.m, ctypes.byref(v)), "greedy_drain")
        return v.value

    def forward_hidden(self, T, n_past):
        _chk(_L.kcpp_model_forward_hidden(self.m, T, n_past), "forward_hidden")

    def read_hidden(self, n, offset=0):
        import numpy as np
        out = np.empty(n, np.float32)
        _chk(_L.kcpp_model_read_hidden(self.m, out.ctypes.data_as(P), n, offset), "read_hidden")
        return out

    def hidden_io(self, ptr, n, offset=0, to_buf=False):
        """stream-ordered copy between the residual stream and ptr (device or host address)"""
        _chk(_L.kcpp_model_hidden_io(self.m, ptr, n, offset, int(to_buf)), "hidden_io")

    def sync(self):
        _chk(_L.kcpp_model_sync(self.m), "sync")

    def hidden_ptr(self):
        return _L.kcpp_model_hidden(self.m)

    def stream(self):
        return _L.kcpp_model_stream(self.m)

    def set_fused_decode(self, on):
        _L.kcpp_model_set_fused_decode(self.m, int(on))

    def set_rope_freqs(self, ff):
        """rope frequency factors (rope_freqs.weight: head_dim / 2 float32)"""
        import numpy as np
        a = np.ascontiguousarray(ff, dtype=np.float32)
        _chk(_L.kcpp_model_set_rope_freqs(self.m, a.ctypes.data_as(P), len(a)), "set_rope_freqs")

    def set_rope_mode(self, mode):
        """0 = NORM pairs (Llama, the default), 2 = NeoX pairs (Qwen2)"""
        _chk(_L.kcpp_model_set_rope_mode(self.m, int(mode)), "set_rope_mode")

    def set_norm_mode(self, mode):
        """0 = RMS norm (the default), 1 = LayerNorm for attn_norm and output_norm (Command-R; eps = layer_norm_epsilon)"""
        _chk(_L.kcpp_model_set_norm_mode(self.m, int(mode)), "set_norm_mode")

    def set_parallel_block(self, on):
        """attention and the FFN both read attn_norm(x); layer output (ffn_out + x) + attn_out (Command-R)"""
        _chk(_L.kcpp_model_set_parallel_block(self.m, int(bool(on))), "set_parallel_block")

    def set_logit_scale(self, scale):
        """every logit times scale where the head writes them (Command-R logit_scale); 0 or 1 = none"""
        _chk(_L.kcpp_model_set_logit_scale(self.m, float(scale)), "set_logit_scale")

    def set_qkv_bias(self, il, bq, bk, bv):
        """q / k / v projection biases of layer il (float32 n_embd, n_embd_gqa, n_embd_gqa); all None clears them"""
        import numpy as np
        arrs = [None if b is None else np.ascontiguousarray(b, dtype=np.float32) for b in (bq, bk, bv)]
        hp = self.hp
        ekv = hp["n_head_kv"] * (hp["n_embd"] // hp["n_head"])
        for a, n in zip(arrs, (hp["n_embd"], ekv, ekv)):
            if a is not None and a.size != n:
                raise ValueError("set_qkv_bias: expected %d values, got %d" % (n, a.size))
        _chk(_L.kcpp_model_set_qkv_bias(self.m, int(il), *[None if a is None else a.ctypes.data_as(P) for a in arrs]),
             "set_qkv_bias")

    def set_fa_exact(self, on):
        """strict-parity attention (reference order, f16 accumulation); see kcpp_flash_attn_exact"""
        _chk(_L.kcpp_model_set_fa_exact(self.m, int(on)), "set_fa_exact")

    def set_kv_types(self, type_k, type_v):
        """K / V cache types: F16 (default) or Q8_0 / Q4_0 for both (koboldcpp --quantkv); clears the caches"""
        _chk(_L.kcpp_model_set_kv_types(self.m, int(type_k), int(type_v)), "set_kv_types")

    def moe_ids(self, T, k):
        import numpy as np
        out = np.zeros((T, k), np.int32)
        _chk(_L.kcpp_model_moe_ids(self.m, out.ctypes.data, T * k), "moe_ids")
        return out

    def moe_trace(self, on):
        _chk(_L.kcpp_model_moe_trace(self.m, int(on)), "moe_trace")

    def set_fused_route(self, on, pair_down=None):
        """MoE decode fusions (default on): the router inside the two-slot gate|up launch, and (pair_down, default =
        on) both slots' down projections in one launch; off = the separate router launch / two chained launches"""
        pd = on if pair_down is None else pair_down
        _chk(_L.kcpp_model_set_fused_route(self.m, int(bool(on)) | (2 * int(bool(pd)))), "set_fused_route")

    def fused_route_count(self):
        """(routed gate|up launches, two-slot down launches) enqueued so far"""
        v = int(_L.kcpp_model_fused_route_count(self.m))
        return v & 0xFFFFFFFF, v >> 32

    def set_moe_grouped(self, on):
        """MoE prefill: grouped expert GEMMs (default) or the per-expert loop; returns the previous setting"""
        return bool(_L.kcpp_model_set_moe_grouped(self.m, int(bool(on))))

    def moe_grouped_count(self):
        """grouped MoE prefill layers run so far"""
        return int(_L.kcpp_model_moe_grouped_count(self.m))

    def moe_trace_read(self, n_layer, k):
        import numpy as np
        out = np.zeros((n_layer, k), np.int32)
        _chk(_L.kcpp_model_moe_trace_read(self.m, out.ctypes.data, n_layer * k), "moe_trace_read")
        return out

    def set_graphs(self, on):
        _L.kcpp_model_set_graphs(self.m, int(on))

    def set_row_split(self, devices, tensor_split):
        """LLAMA_SPLIT_MODE_ROW over `devices` (lanes may repeat a GPU); before synth / set_tensor"""
        n = len(devices)
        d = (ctypes.c_int * n)(*devices)
        ts = (ctypes.c_float * n)(*tensor_split)
        _chk(_L.kcpp_model_set_row_split(self.m, n, d, ts), "set_row_split")


    def weight_bytes(self):
        return int(_L.kcpp_model_weight_bytes(self.m))

    def close(self):
        if getattr(self, "m", None):
            _L.kcpp_model_free(self.m)
            self.m = None

    def __del__(self):
        self.close()


def row_split_range(nrows, tensor_split, i):
    """(lo, hi) of device i's rows (kcpp_row_split_range)"""
    n = len(tensor_split)
    ts = (ctypes.c_float * n)(*tensor_split)
    lo, hi = ctypes.c_int64(0), ctypes.c_int64(0)
    _chk(_L.kcpp_row_split_range(int(nrows), n, ts, int(i), ctypes.byref(lo), ctypes.byref(hi)), "row_split_range")
    return lo.value, hi.value


GEMM_FAMILY = ("cols", "q80s", "v1", "v2", "q4v3", "q6v3", "v4")


def gemm_plan(t, K, N, M, mode=0, bs_aligned=True):
    """what kcpp_gemm would launch under the current variant (kcpp_gemm_plan; host only): dict of family (a
    GEMM_FAMILY name), rs, tile (v2 TM / v3 BMT / v4 TPW), waves, ks, xg, pf, nwg"""
    out = (ctypes.c_int32 * 8)()
    _chk(_L.kcpp_gemm_plan(int(t), int(K), int(N), int(M), int(mode), int(bool(bs_aligned)), out), "gemm_plan")
    d = dict(zip(("family", "rs", "tile", "waves", "ks", "xg", "pf", "nwg"), out))
    d["family"] = GEMM_FAMILY[d["family"]]
    return d


FA_PREFILL_KERNEL = ("fma", "mfma", "mfma_split")


def fa_prefill_plan(T, H, HKV, D=128, n_past=0, have_ws=False):
    """what the prefill attention launches at D = 128 (kcpp_fa_prefill_plan; host only): dict of kernel (a
    FA_PREFILL_KERNEL name, as the auto path chooses), gh / qb (heads / 16-query blocks per workgroup), nb0 (workgroups
    per split), nsp, ch (64-key tiles per split), merge_grid, part_bytes; None for a shape the MFMA kernel does not cover"""
    out = (ctypes.c_int32 * 8)()
    rc = _L.kcpp_fa_prefill_plan(int(T), int(H), int(HKV), int(D), int(n_past), int(bool(have_ws)), out)
    if rc == -3:
        return None
    _chk(rc, "fa_prefill_plan")
    d = dict(zip(("kernel", "gh", "qb", "nb0", "nsp", "ch", "merge_grid", "part_bytes"), out))
    d["kernel"] = FA_PREFILL_KERNEL[d["kernel"]]
    return d


FA_DEC_KERNEL = ("chunk", "split4", "split5", "short", "tile", "mfma")
FA_FORM = ("runtime", "ex", "graph1", "grapht")


def fa_decode_plan(form, T, H, HKV, D=128, nkv=1, n_rows=0, qkind=0, sel=0, cap=False, have_out=True):
    """what a decode / ggml-op attention entry launches (kcpp_fa_decode_plan; host only).  form: a FA_FORM name; sel: the
    force_path or variant.  Returns the entry's error code (a negative int), or a dict of kernel (a FA_DEC_KERNEL name),
    ns, nch, waves, grid, cgrid, cthreads, cquant and the workspace byte offsets part_o, part_ml, ws_bytes, q16"""
    out = (ctypes.c_int32 * 19)()
    rc = _L.kcpp_fa_decode_plan(FA_FORM.index(form), int(T), int(H), int(HKV), int(D), int(nkv), int(n_rows), int(qkind),
                                int(sel), int(bool(cap)) | (0 if have_out else 2), out)
    if rc:
        return rc
    v = list(out)
    d = dict(zip(("kernel", "ns", "nch", "waves"), v[:4]), grid=tuple(v[4:7]), cgrid=tuple(v[7:9]), cthreads=v[9],
             cquant=v[10])
    for i, k in enumerate(("part_o", "part_ml", "ws_bytes", "q16")):
        d[k] = (v[11 + 2 * i] & 0xFFFFFFFF) | (v[12 + 2 * i] << 32)
    d["kernel"] = FA_DEC_KERNEL[d["kernel"]]
    return d


GEMV_KERNEL = ("rs", "rs_aux", "q4k", "stream", "unit")
GEMV_ENTRY = ("dec", "rs", "rs_aux", "q4k", "stream", "unit")
# what a DecArgs / AuxOut hold (gemv_plan.h GEMV_F_*)
GEMV_FLAGS = {"eid": 1, "eid1": 2, "escale": 4, "route_w": 8, "route_out": 16, "ex": 32, "neox": 64, "nw": 128, "aux": 256,
              "aux_p0h0": 512, "aux_glu": 1024, "aux_rope": 2048, "aux_rope_ok": 4096}
_GEMV_PLAN_FIELDS = ("rc", "kernel", "type", "mode", "pro", "NI", "IT", "LPR", "R", "MC", "PF", "waves", "XL", "ROUTE", "EX",
                     "block", "nblk", "lds_bytes")


def _gemv_flags(flags):
    return sum(GEMV_FLAGS[f] for f in flags)


def gemv_dec_plan(entry, wtype, K, N, mode, pro, rows_per_wave=1, flags=(), role=(0, 1, 2), D=0, route_wt=0, route_ne=0):
    """what a fused single-token mat-vec entry runs (kcpp_gemv_dec_plan; host only).  entry: a GEMV_ENTRY name; N: the
    segments' row counts; flags: GEMV_FLAGS names.  Returns the entry's error code (a negative int), or a dict of kernel
    (a GEMV_KERNEL name), the instance parameters type, mode, pro, NI, IT, LPR, R, MC, PF, waves, XL, ROUTE, EX and the
    launch's nblk, block, lds_bytes"""
    out = (ctypes.c_int32 * 18)()
    n = list(N) + [0] * (3 - len(N))
    rc = _L.kcpp_gemv_dec_plan(GEMV_ENTRY.index(entry), int(wtype), int(K), len(N), n[0], n[1], n[2], role[0], role[1], role[2],
                               int(D), int(mode), int(pro), int(rows_per_wave), _gemv_flags(flags), int(route_wt),
                               int(route_ne), out)
    if rc:
        return rc
    d = dict(zip(_GEMV_PLAN_FIELDS, out))
    d["kernel"] = GEMV_KERNEL[d["kernel"]]
    return d


def gemv_qkv_mixed_plan(K, N, flags=(), role=(0, 1, 2), D=0, pro=None):
    """what kcpp_gemv_rs_qkv_mixed launches (host only): its error code, or a dict of NIA, NIB, MC, EX, block, nblk,
    lds_bytes; with pro (1 = rms_norm, 3 = LayerNorm) kcpp_gemv_rs_qkv_mixed_pro's, the dict then holds PRO too"""
    if pro is not None:
        out = (ctypes.c_int32 * 9)()
        rc = _L.kcpp_gemv_qkv_mixed_plan_pro(int(K), N[0], N[1], N[2], role[0], role[1], role[2], int(D), _gemv_flags(flags),
                                             int(pro), out)
        return rc if rc else dict(zip(("rc", "NIA", "NIB", "MC", "EX", "block", "nblk", "lds_bytes", "PRO"), out))
    out = (ctypes.c_int32 * 8)()
    rc = _L.kcpp_gemv_qkv_mixed_plan(int(K), N[0], N[1], N[2], role[0], role[1], role[2], int(D), _gemv_flags(flags), out)
    return rc if rc else dict(zip(("rc", "NIA", "NIB", "MC", "EX", "block", "nblk", "lds_bytes"), out))


def gemv_qkv_dual_plan(qtype, K, Na, Nb, flags_a=(), flags_b=(), Kb=None):
    """what kcpp_gemv_qkv_dual launches (host only): its error code, or a dict of nblk, lds_bytes and the two halves'
    a_nblk, a_lds_bytes, a_NI (the RS launch of q) and b_nblk, b_lds_bytes, b_IT (the unit launch of k|v in Q8_0)"""
    out = (ctypes.c_int32 * 9)()
    na, nb = (ctypes.c_int64 * 3)(*Na), (ctypes.c_int64 * 3)(*Nb)
    rc = _L.kcpp_gemv_qkv_dual_plan(int(qtype), int(K), len(Na), na, _gemv_flags(flags_a), int(K if Kb is None else Kb), len(Nb),
                                    nb, _gemv_flags(flags_b), out)
    return rc if rc else dict(zip(("rc", "nblk", "lds_bytes", "a_nblk", "a_lds_bytes", "a_NI", "b_nblk", "b_lds_bytes", "b_IT"),
                                  out))


class CandHdr(ctypes.Structure):
    """struct kcpp_cand_hdr: the sampling front end's result header"""
    _fields_ = [("low", Fl), ("ib", ctypes.c_int32), ("nhave", ctypes.c_int32), ("n_bad", ctypes.c_int32),
                ("hist", ctypes.c_int32 * 128)]


class CandHdrMasked(ctypes.Structure):
    """struct kcpp_cand_hdr_masked: the header of the entries that take a grammar's reject mask"""
    _fields_ = [("h", CandHdr), ("n_rej", ctypes.c_int32), ("pad", ctypes.c_int32)]


CAND_GUARD_ID, CAND_GUARD_BITS = -77, 0x7FC0DEAD       # what candidates() leaves in entries the call did not write


def cand_plan(n):
    """the sampling front end's launch plan for n logits (kcpp_cand_plan; host only): dict of slice, block, nblk"""
    out = (ctypes.c_int32 * 4)()
    _chk(_L.kcpp_cand_plan(int(n), out), "cand_plan")
    return dict(zip(("rc", "slice", "block", "nblk"), out))


def candidates(where, logits, k, set_ids=(), adds=(), subs=(), cap=16384, guard=0, stream=None, mask=None):
    """The sampling front end on n logits: set_ids set to the lowest logit, adds / subs = [(id, value), ...] added /
    subtracted in list order, then the candidates at or above top_k(k)'s bucket cut.  where: "ref" (the CPU model,
    logits a float32 array), "dev" (kcpp_logit_candidates, logits = (device address, n)) or a Model (its last logits).
    mask (uint32 words, bit i % 32 of word i / 32 set = id i rejected): the masked entries; the header returned is then
    a CandHdrMasked (h, n_rej).
    Returns (CandHdr, ids, vals): int32 / float32 arrays of cap + guard entries, min(nhave, cap) of them written and the
    rest left at CAND_GUARD_ID / CAND_GUARD_BITS"""
    import numpy as np
    edit = np.dtype([("id", np.int32), ("v", np.float32)])
    s = np.ascontiguousarray(set_ids, dtype=np.int32)
    a, b = np.array(list(adds), dtype=edit), np.array(list(subs), dtype=edit)
    hdr = CandHdr() if mask is None else CandHdrMasked()
    ids = np.full(cap + guard, CAND_GUARD_ID, np.int32)
    vals = np.full(cap + guard, CAND_GUARD_BITS, np.uint32).view(np.float32)
    lists = (s.ctypes.data_as(P), len(s), a.ctypes.data_as(P), len(a), b.ctypes.data_as(P), len(b), ctypes.byref(hdr),
             ids.ctypes.data_as(P), vals.ctypes.data_as(P), int(cap))
    if mask is not None:
        mk = np.ascontiguousarray(mask, dtype=np.uint32)
        lists = lists[:6] + (mk.ctypes.data_as(P),) + lists[6:]
        if isinstance(where, Model):
            _chk(_L.kcpp_model_candidates_masked(where.m, int(k), *lists), "model_candidates_masked")
        elif where == "dev":
            assert len(mk) == (int(logits[1]) + 31) // 32
            _chk(_L.kcpp_logit_candidates_masked(logits[0], int(logits[1]), int(k), *lists, stream), "logit_candidates_masked")
        else:
            lg = np.ascontiguousarray(logits, dtype=np.float32)
            assert len(mk) == (len(lg) + 31) // 32
            _chk(_L.kcpp_cand_front_ref_masked(lg.ctypes.data_as(P), len(lg), int(k), *lists), "cand_front_ref_masked")
        return hdr, ids, vals
    if isinstance(where, Model):
        _chk(_L.kcpp_model_candidates(where.m, int(k), *lists), "model_candidates")
    elif where == "dev":
        _chk(_L.kcpp_logit_candidates(logits[0], int(logits[1]), int(k), *lists, stream), "logit_candidates")
    else:
        lg = np.ascontiguousarray(logits, dtype=np.float32)
        _chk(_L.kcpp_cand_front_ref(lg.ctypes.data_as(P), len(lg), int(k), *lists), "cand_front_ref")
    return hdr, ids, vals


def pipeline_trace(n_stages, ubatch, T, n_past, steps):
    """the pipeline schedule's enqueue order (expose.cpp forward / greedy_step over the trace backend): host only"""
    buf = ctypes.create_string_buffer(1 << 16)
    n = _L.kcpp_pipeline_trace(n_stages, ubatch, T, n_past, steps, buf, len(buf))
    if n < 0:
        raise KcppError("kcpp_pipeline_trace failed")
    return buf.value.decode().split()


def split_layers(n_layer, n_dev, tensor_split=None):
    """load_model's layer placement: (device per layer, output head's device)"""
    ts = (ctypes.c_float * 16)(*((list(tensor_split) if tensor_split else [1.0] * n_dev) + [0.0] * (16 - n_dev)))
    out = (ctypes.c_int * (n_layer + 1))()
    if _L.kcpp_split_layers(n_layer, n_dev, ts, out) != 0:
        raise KcppError("kcpp_split_layers failed")
    return list(out[:n_layer]), out[n_layer]
