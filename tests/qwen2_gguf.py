"""TEST INFRASTRUCTURE: the tiny Qwen2 model of the Qwen2 tests -- its hyper-parameters, per-tag tensor types, the
q / k / v biases (an integer hash, so a bias is its parameters) and a GGUF writer for it (general.architecture
= qwen2, keys under the qwen2. prefix, blk.N.attn_{q,k,v}.bias; built on gguf_writer.write).  The weights are
refharness.synth_tensor's, the bytes Model.synth(seed) makes on the device."""
import numpy as np

import gguf_writer as GW
import refharness as R

# G = 14 / 2 = 7 (the Qwen2.5-7B ratio), D = 128, n_embd = 7 x 256
TINY_QWEN2 = dict(n_vocab=512, n_embd=1792, n_head=14, n_head_kv=2, n_layer=2, n_ff=1024, n_ctx=256,
                  eps=1e-6, rope_base=1000000.0)
# the same at n_embd 2048 = 8 x 256, the narrowest width with a row-major Q6_K layout (kcpp_rs_supported): there the
# Q4_K_M 'more bits' layer (attn_q / attn_k Q4_K + attn_v Q6_K) decodes through the one-launch mixed q|k|v kernel.
# 16 / 2 heads: G = 8, D = 128 (Qwen2.5-3B's ratio)
WIDE_QWEN2 = dict(TINY_QWEN2, n_embd=2048, n_head=16)
SEED = 1234
N_PROMPT, N_GEN = 17, 6
TAGS = ("q4km", "q4k", "q8_0", "q4km_w")


def tag_hp(tag):
    return WIDE_QWEN2 if tag.endswith("_w") else TINY_QWEN2


def tag_types(tag, n_layer=2):
    """q4km: the Q4_K_M policy (with 2 layers, layer 1 is a 'more bits' layer: attn_v / ffn_down Q6_K beside Q4_K
    attn_q / attn_k; layer 0 is all Q4_K); q4k: the same with layer 1's attn_v and ffn_down in Q4_K too (q|k|v of one
    type in every layer: k_gemv_rs mode 2); q8_0: everything Q8_0 (no fused q|k|v kernel carries bias / NeoX there:
    the unfused fallback)"""
    if tag in ("q4km", "q4km_w"):        # _w: WIDE_QWEN2, where layer 1's q|k + v is the mixed launch
        return R.q4_k_m_types(n_layer)
    if tag == "q4k":
        ty = R.q4_k_m_types(n_layer)
        ty[3 + 9 * 1 + 3] = R.Q4_K
        ty[3 + 9 * 1 + 8] = R.Q4_K
        return ty
    if tag == "q8_0":
        return R.uniform_types(n_layer, R.Q8_0)
    raise KeyError(tag)


def qkv_bias(hp, il, seed=SEED):
    """(bq, bk, bv) float32 of layer il: bell-shaped multiples of 2^-16 with |b| < 2 (std 0.58); every 61st element of
    bk (from a per-layer offset) is +-50, as real Qwen2 k-biases carry a few very large entries"""
    E = hp["n_embd"]
    EKV = hp["n_head_kv"] * (E // hp["n_head"])
    out = []
    for j, n in enumerate((E, EKV, EKV)):
        b = (R._hash_bell(seed + 7919 * il, 100 + j, n).astype(np.float64) / 65536.0).astype(np.float32)
        if j == 1:
            idx = np.arange((5 + 13 * il) % 61, n, 61)
            b[idx] = np.where(idx % 2 == 0, np.float32(50.0), np.float32(-50.0))
        out.append(b)
    return tuple(out)


# NeoX rope cases of the fixture (name: T, H, HKV, D, positions); rope base = TINY_QWEN2's
ROPE_CASES = {"rope128": (4, 6, 2, 128, [0, 37, 38, 4000]), "rope64": (3, 4, 2, 64, [0, 37, 255])}


def rope_case_input(name):
    """q|k|v staging rows [T][(H + 2 HKV) D] f32 of ROPE_CASES[name]: multiples of 2^-15, std 1.15"""
    import zlib
    T, H, HKV, D, _ = ROPE_CASES[name]
    n = T * (H + 2 * HKV) * D
    return (R._hash_bell(zlib.crc32(name.encode()), 9, n).astype(np.float64) / 32768.0).astype(np.float32).reshape(T, -1)


def prompt_tokens(hp, seed=SEED):
    """the fixture's 17 prompt tokens, hashed into [1, n_vocab)"""
    return [int(v) for v in (R._hash64(seed, 55, N_PROMPT) % np.uint64(hp["n_vocab"] - 1)).astype(np.int64) + 1]


def qwen2_gguf(path, hp, types, seed, words=GW.WORDS, arch="qwen2", drop=(), kv_extra=None):
    """Qwen2 GGUF with the runtime's synthetic weights and qkv_bias()'s biases; drop: tensor names left out"""
    toks, scores, ttypes = GW.spm_vocab(hp["n_vocab"], words)
    kv = {
        "general.architecture": arch,
        "general.alignment": 32,
        arch + ".context_length": int(hp["n_ctx"]),
        arch + ".embedding_length": int(hp["n_embd"]),
        arch + ".block_count": int(hp["n_layer"]),
        arch + ".feed_forward_length": int(hp["n_ff"]),
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
        names += ["blk.%d.%s.weight" % (il, n) for n in GW.LAYER_NAMES]
    tensors = []
    for idx, ((k, n), t) in enumerate(zip(R.weight_shapes(hp), types)):
        data = R.synth(t, seed, idx, k, n)
        tensors.append((names[idx], t, [k] if n == 1 else [k, n], np.ascontiguousarray(data).tobytes()))
    for il in range(hp["n_layer"]):
        for nm, b in zip(("attn_q", "attn_k", "attn_v"), qkv_bias(hp, il, seed)):
            tensors.append(("blk.%d.%s.bias" % (il, nm), R.F32, [len(b)], b.tobytes()))
    tensors = [t for t in tensors if t[0] not in drop]
    GW.write(path, kv, tensors)
    return toks
