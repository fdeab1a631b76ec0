"""TEST INFRASTRUCTURE: the tiny Command-R model of the Command-R tests -- its hyper-parameters, per-tag tensor types, the
token embedding (synthetic rows plus a per-row constant, so LayerNorm can be told from RMS norm), how a runtime Model is
set up for it, and a GGUF writer (general.architecture = command-r, keys under the command-r. prefix, no output.weight
and no ffn_norm; built on gguf_writer.write).  Every other weight but output_norm (output_norm_f32) is
refharness.synth_tensor's, the bytes Model.synth(seed) makes on the device.

The embedding is tied (build_command_r has no output.weight), so it is also the head's weight and has to be a type the
mat-vec kernels take: its rows are hashed f32 values quantized to Q8_0 (no F16 mat-vec exists here)."""
import numpy as np

import gguf_writer as GW
import refharness as R

# 2048 = 8 x 256: the narrowest width with a row-major Q6_K layout, so the mixed q|k + v launch is reachable; D = 128
TINY_CMDR = dict(n_vocab=512, n_embd=2048, n_head=16, n_head_kv=16, n_layer=2, n_ff=1024, n_ctx=256,
                 eps=1e-5, rope_base=8000000.0, logit_scale=0.0625)
SEED = 1234
N_PROMPT, N_GEN = 17, 6
TAGS = ("q4k", "q4km", "q8_0")
EMB_TYPE = R.Q8_0
HP_KEYS = ("n_vocab", "n_embd", "n_head", "n_head_kv", "n_layer", "n_ff", "n_ctx", "eps", "rope_base")


def tag_hp(tag):
    """q4k: 16 / 16 heads (the v01 MHA layout); q4km: 16 / 2 (ratio 8, the 08-2024 layout); q8_0: 16 / 16"""
    return dict(TINY_CMDR, n_head_kv=2) if tag == "q4km" else dict(TINY_CMDR)


def model_hp(hp):
    """the kcpp_hparams part of hp (logit_scale travels through Model.set_logit_scale)"""
    return {k: hp[k] for k in HP_KEYS}


def tag_types(tag, n_layer=2):
    """q4k: every matrix Q4_K (each decode launch of a layer runs its LayerNorm prologue instance); q4km: the Q4_K_M
    policy (with 2 layers, layer 1 is a 'more bits' layer: attn_v / ffn_down Q6_K beside Q4_K attn_q / attn_k -- the mixed
    q|k + v launch; layer 0 is all Q4_K); q8_0: everything Q8_0 (no LayerNorm prologue there: the unfused fallback).
    Entries 0 and 2 are the tied embedding's type."""
    if tag == "q4k":
        ty = R.uniform_types(n_layer, R.Q4_K)
    elif tag == "q4km":
        ty = R.q4_k_m_types(n_layer)
    elif tag == "q8_0":
        ty = R.uniform_types(n_layer, R.Q8_0)
    else:
        raise KeyError(tag)
    ty[0] = ty[2] = EMB_TYPE
    for il in range(n_layer):
        ty[3 + 9 * il] = ty[3 + 9 * il + 5] = R.F32
    return ty


def embedding_f32(hp, seed=SEED):
    """[n_vocab][n_embd] f32: bell-shaped multiples of 2^-16 (std 0.58) plus a per-row constant of 1-2 x that std with
    a hashed sign.  Without the constant a synthetic row has a mean near zero and LayerNorm equals RMS norm; with it
    the second layer's input (the row plus a layer output of std near 4) still has |mean| / std above 0.25.  The
    embedding is also the head, so a step's input token scores about 6 sigma above the rest and the greedy sequence soon
    repeats a token: the comparisons are of logits, teacher-forced.  (A smaller random part beside the same constant
    avoids that, but then each logit's error is the row constant times one sum of the head activation's rounding errors
    -- a single random number per step -- and the reference's own spread measures nothing else.)"""
    V, E = hp["n_vocab"], hp["n_embd"]
    x = (R._hash_bell(seed, 71, V * E).astype(np.float64) / 65536.0).reshape(V, E)
    h = R._hash64(seed, 72, V)
    mag = 0.58 * (1.0 + (h & np.uint64(0xFFFF)).astype(np.float64) / 65536.0)
    sign = np.where((h >> np.uint64(16)) & np.uint64(1), 1.0, -1.0)
    return (x + (mag * sign)[:, None]).astype(np.float32)


def output_norm_f32(hp, seed=SEED):
    """output_norm.weight: the synthetic values (1 +- 0.006) times 1/4.  The head's rows are 16 x as large as the other
    synthetic matrices' (the per-row constant), logit_scale undoes 1/16 of that, and this the rest: the logits and
    their sensitivity to summation order come out at the other tiny models' scale, which the absolute bar shared with
    them (test_gpu_model.TOL_MAX) presumes."""
    return (R.synth(R.F32, seed, 1, hp["n_embd"], 1).view(np.float32) * np.float32(0.25)).astype(np.float32)


_emb = {}


def embedding_bytes(hp, seed=SEED):
    """the tied embedding as EMB_TYPE rows (the reference's own row quantizer through the oracle)"""
    key = (hp["n_vocab"], hp["n_embd"], seed)
    if key not in _emb:
        _emb[key] = np.concatenate([R.quantize(EMB_TYPE, r) for r in embedding_f32(hp, seed)])
    return _emb[key]


def prompt_tokens(hp, seed=SEED):
    """17 prompt tokens hashed into [1, n_vocab)"""
    return [int(v) for v in (R._hash64(seed, 55, N_PROMPT) % np.uint64(hp["n_vocab"] - 1)).astype(np.int64) + 1]


def setup_model(m, hp, seed=SEED, norm_mode=1, parallel=1, logit_scale=None):
    """synthetic weights, the tied embedding in entries 0 and 2, output_norm, and the three Command-R switches"""
    m.synth(seed)
    emb = embedding_bytes(hp, seed)
    for idx in (0, 2):          # (a stage that lacks one of them ignores the upload, as for load_model)
        m.set_tensor(idx, emb)
    m.set_tensor(1, output_norm_f32(hp, seed))
    m.set_norm_mode(norm_mode)
    m.set_parallel_block(parallel)
    m.set_logit_scale(hp["logit_scale"] if logit_scale is None else logit_scale)
    return m


def commandr_gguf(path, hp, types, seed=SEED, words=GW.WORDS, arch="command-r", drop=(), kv_extra=None, kv_drop=(),
                  extra_tensors=()):
    """Command-R GGUF: the runtime's synthetic weights, embedding_bytes() as token_embd.weight, no output.weight and no
    blk.N.ffn_norm; drop / kv_drop: tensor names / keys left out, extra_tensors: (name, type, ne, bytes) appended"""
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
        arch + ".attention.layer_norm_epsilon": float(hp["eps"]),
        arch + ".rope.freq_base": float(hp["rope_base"]),
        arch + ".logit_scale": float(hp["logit_scale"]),
        "tokenizer.ggml.model": "llama",
        "tokenizer.ggml.tokens": (GW.STR, toks),
        "tokenizer.ggml.scores": (GW.F32, scores),
        "tokenizer.ggml.token_type": (GW.I32, ttypes),
        "tokenizer.ggml.bos_token_id": 1,
        "tokenizer.ggml.eos_token_id": 2,
    }
    if kv_extra:
        kv.update(kv_extra)
    for k in kv_drop:
        kv.pop(k, None)
    names = ["token_embd.weight", "output_norm.weight", None]
    for il in range(hp["n_layer"]):
        names += ["blk.%d.%s.weight" % (il, n) if n != "ffn_norm" else None for n in GW.LAYER_NAMES]
    tensors = []
    for idx, ((k, n), t) in enumerate(zip(R.weight_shapes(hp), types)):
        if names[idx] is None:
            continue
        data = embedding_bytes(hp, seed) if idx == 0 else (output_norm_f32(hp, seed) if idx == 1 else R.synth(t, seed, idx, k, n))
        tensors.append((names[idx], t, [k] if n == 1 else [k, n], np.ascontiguousarray(data).tobytes()))
    tensors = [t for t in tensors if t[0] not in drop] + list(extra_tensors)
    GW.write(path, kv, tensors)
    return toks
