"""TEST INFRASTRUCTURE: the tiny Qwen2-MoE models (build_qwen2moe, src/llama.cpp:12248-12392) of the qwen2moe tests --
hyper-parameters per tag, the 14-entry per-layer tensor order of kcpp_model_create_ex, per-tag tensor types, the
synthetic weights (refharness.synth per canonical index, what Model.synth(seed) makes on the device) and the shared
expert's gate vectors (an integer hash, so a gate vector is its parameters).  The q / k / v biases and the prompt are
qwen2_gguf's."""
import numpy as np

import qwen2_gguf as Q
import refharness as R

SEED = Q.SEED
N_PROMPT, N_GEN = Q.N_PROMPT, Q.N_GEN
TAGS = ("a27", "a14", "top2", "q8_0", "shq8")
PER_LAYER = 14      # attn_norm, wq, wk, wv, wo, ffn_norm, gate_exps, up_exps, down_exps, ffn_gate_inp,
#                     ffn_gate_inp_shexp, ffn_gate_shexp, ffn_up_shexp, ffn_down_shexp
J_GATE_VEC = 10

_BASE = dict(n_vocab=512, n_layer=2, n_ctx=256, eps=1e-6, rope_base=1000000.0, moe_norm_w=0)
# n_ff is the width of one routed expert (kcpp_hparams.n_ff with n_expert > 0)
HP = {
    # Qwen1.5-MoE-A2.7B's ratio 1 and its expert width 1408 (no multiple of 256: ffn_down_exps cannot be a K-quant)
    "a27": dict(_BASE, n_embd=1024, n_head=8, n_head_kv=8, n_expert=12, n_expert_used=4, n_ff=1408, n_ff_shexp=1024),
    # Qwen2-57B-A14B's ratio 7, top-8
    "a14": dict(_BASE, n_embd=1792, n_head=14, n_head_kv=2, n_expert=12, n_expert_used=8, n_ff=2560, n_ff_shexp=2048),
    # top-2 of 8 in the row-major decode layouts: the pair path, which must not add the residual twice
    "top2": dict(_BASE, n_embd=2048, n_head=16, n_head_kv=2, n_expert=8, n_expert_used=2, n_ff=1024, n_ff_shexp=1024),
}
HP["q8_0"] = dict(HP["a27"])
# top2 with a Q8_0 ffn_down_shexp: the routed sum is carried through the row-major down projections, and the shared
# expert's down projection is of a kernel family whose store does not take it
HP["shq8"] = dict(HP["top2"])


def tag_hp(tag):
    return HP[tag]


def tag_types(tag):
    """a27 / a14: Q4_K_M's choices (with 2 layers, layer 1 is the 'more bits' layer: attn_v and the down projections
    Q6_K), except a27's ffn_down_exps, whose rows of 1408 take llama.cpp's fallback types: Q5_0 in layer 0, Q8_0 in
    layer 1.  Routers: a27 / q8_0 F32, a14 / top2 F16; gate vectors F32 (top2: F16).  shq8: top2's types with both
    layers' ffn_down_shexp Q8_0 (a mixed quant that keeps the shared expert at more bits)."""
    if tag == "q8_0":
        ty = [R.Q8_0, R.F32, R.Q8_0]
        for _ in range(2):
            ty += [R.F32] + [R.Q8_0] * 4 + [R.F32] + [R.Q8_0] * 3 + [R.F32, R.F32] + [R.Q8_0] * 3
        return ty
    ty = [R.Q4_K, R.F32, R.Q6_K]
    for il in range(2):
        more = il == 1 and tag not in ("top2", "shq8")
        v = R.Q6_K if more else R.Q4_K
        down_exps = v if tag != "a27" else (R.Q8_0 if il == 1 else R.Q5_0)
        router = R.F32 if tag == "a27" else R.F16
        gvec = R.F16 if tag in ("top2", "shq8") else R.F32
        down_sh = R.Q8_0 if tag == "shq8" else v
        ty += [R.F32, R.Q4_K, R.Q4_K, v, R.Q4_K, R.F32, R.Q4_K, R.Q4_K, down_exps, router, gvec, R.Q4_K, R.Q4_K, down_sh]
    return ty


def weight_shapes(hp):
    """(K, N) per canonical index: tok_embd, output_norm, output, then PER_LAYER per layer (expert tensors: per slice)"""
    E, F, FS, V = hp["n_embd"], hp["n_ff"], hp["n_ff_shexp"], hp["n_vocab"]
    EKV = hp["n_head_kv"] * (E // hp["n_head"])
    s = [(E, V), (E, 1), (E, V)]
    for _ in range(hp["n_layer"]):
        s += [(E, 1), (E, E), (E, EKV), (E, EKV), (E, E), (E, 1), (E, F), (E, F), (F, E), (E, hp["n_expert"]),
              (E, 1), (E, FS), (E, FS), (FS, E)]
    return s


def n_slices(hp, idx):
    return hp["n_expert"] if idx >= 3 and (idx - 3) % PER_LAYER in (6, 7, 8) else 1


def gate_vector(hp, il, t=R.F32, seed=SEED):
    """ffn_gate_inp_shexp of layer il: a bell-shaped hash scaled so that z = g . ffn_norm(x) has a spread near 1.5 and
    the gate sigmoid(z) lies on both sides of one half over the fixture's tokens"""
    E = hp["n_embd"]
    g = R._hash_bell(seed + 104729 * il, 200, E).astype(np.float64) * (1.5 / (37837.0 * np.sqrt(E)))
    return g.astype(np.float16 if t == R.F16 else np.float32)


def synth_tensor(hp, t, seed, idx):
    """bytes of canonical tensor idx as Model.synth(seed) + the gate vectors make them; expert e: tid idx * 256 + e"""
    k, n = weight_shapes(hp)[idx]
    if idx >= 3 and (idx - 3) % PER_LAYER == J_GATE_VEC:
        return gate_vector(hp, (idx - 3) // PER_LAYER, t, seed).view(np.uint8)
    ns = n_slices(hp, idx)
    if ns == 1:
        return R.synth(t, seed, idx, k, n)
    return np.concatenate([R.synth(t, seed, idx * 256 + e, k, n) for e in range(ns)])


def prompt_tokens(hp, seed=SEED):
    return Q.prompt_tokens(hp, seed)


def model(K, tag, types=None, ub=512, hp=None, **kw):
    """the runtime's model of a tag: synthetic weights, the gate vectors, NeoX pairs, the q / k / v biases"""
    hp = tag_hp(tag) if hp is None else hp
    types = tag_types(tag) if types is None else types
    m = K.Model(hp, types, max_ubatch=ub, **kw)
    m.synth(SEED)
    m.set_rope_mode(2)
    il0, il1 = kw.get("il0", 0), kw.get("il1", None) or hp["n_layer"]
    for il in range(il0, il1):
        m.set_qkv_bias(il, *Q.qkv_bias(hp, il))
        if hp.get("n_ff_shexp", 0):
            idx = 3 + PER_LAYER * il + J_GATE_VEC
            m.set_tensor(idx, np.ascontiguousarray(gate_vector(hp, il, types[idx])))
    return m


LAYER_NAMES = ["attn_norm", "attn_q", "attn_k", "attn_v", "attn_output", "ffn_norm", "ffn_gate_exps", "ffn_up_exps",
               "ffn_down_exps", "ffn_gate_inp", "ffn_gate_inp_shexp", "ffn_gate_shexp", "ffn_up_shexp", "ffn_down_shexp"]


def qwen2moe_gguf(path, hp, types, seed=SEED, drop=(), kv_extra=None, raw=None):
    """a qwen2moe GGUF (keys under the qwen2moe. prefix, 3-D *_exps tensors, the four *_shexp tensors, the q / k / v
    biases) with synth_tensor()'s weights; drop: tensor names left out; raw: {name: (type, dims, bytes)} put in place
    of a tensor as it is (the loader's refusal tests)"""
    import gguf_writer as GW
    arch = "qwen2moe"
    toks, scores, ttypes = GW.spm_vocab(hp["n_vocab"], GW.WORDS)
    kv = {
        "general.architecture": arch,
        "general.alignment": 32,
        arch + ".context_length": int(hp["n_ctx"]),
        arch + ".embedding_length": int(hp["n_embd"]),
        arch + ".block_count": int(hp["n_layer"]),
        arch + ".feed_forward_length": int(hp["n_ff_shexp"]),
        arch + ".expert_feed_forward_length": int(hp["n_ff"]),
        arch + ".expert_shared_feed_forward_length": int(hp["n_ff_shexp"]),
        arch + ".expert_count": int(hp["n_expert"]),
        arch + ".expert_used_count": int(hp["n_expert_used"]),
        arch + ".attention.head_count": int(hp["n_head"]),
        arch + ".attention.head_count_kv": int(hp["n_head_kv"]),
        arch + ".attention.layer_norm_rms_epsilon": float(hp["eps"]),
        arch + ".rope.freq_base": float(hp["rope_base"]),
        "tokenizer.ggml.model": "llama",
        "tokenizer.ggml.tokens": (GW.STR, toks),
        "tokenizer.ggml.scores": (GW.F32, scores),
        "tokenizer.ggml.token_type": (GW.I32, ttypes),
        "tokenizer.ggml.bos_token_id": 1,
        "tokenizer.ggml.eos_token_id": 2,
    }
    if kv_extra:
        kv.update(kv_extra)
    names = ["token_embd.weight", "output_norm.weight", "output.weight"]
    for il in range(hp["n_layer"]):
        names += ["blk.%d.%s.weight" % (il, n) for n in LAYER_NAMES]
    raw = raw or {}
    tensors = []
    for idx, ((k, n), t) in enumerate(zip(weight_shapes(hp), types)):
        if names[idx] in raw:
            tensors.append((names[idx],) + tuple(raw[names[idx]]))
            continue
        ns = n_slices(hp, idx)
        dims = [k] if n == 1 else ([k, n] if ns == 1 else [k, n, ns])
        tensors.append((names[idx], t, dims, np.ascontiguousarray(synth_tensor(hp, t, seed, idx)).tobytes()))
    for il in range(hp["n_layer"]):
        for nm, b in zip(("attn_q", "attn_k", "attn_v"), Q.qkv_bias(hp, il, seed)):
            tensors.append(("blk.%d.%s.bias" % (il, nm), R.F32, [len(b)], b.tobytes()))
    GW.write(path, kv, [t for t in tensors if t[0] not in drop])
    return toks
