"""Command-R GGUFs through the koboldcpp drop-in ABI: load_model + generate on a synthetic command-r file
(tests/commandr_gguf.py: tied embedding, no ffn_norm, layer_norm_epsilon and logit_scale keys) equals the in-process
runtime with the three Command-R switches, per tag and on two virtual stages; a seeded sampled request draws the same
tokens with the device front end as without it (both see the scaled logits); a Q8_0 K / V cache loads and generates; a
context-shift request erases the span once; every refusal of load_model returns false with a message naming the key or
the tensor, each in a child process of its own (load_model replaces the process-wide model, and a refused load must
leave nothing behind).  Every test loads its own model."""
import os
import subprocess
import sys

import numpy as np
import pytest

import commandr_gguf as C
import gguf_writer as GW
import refharness as R
from test_gpu_expose import WORDS, piece
from test_gpu_qwen2_expose import _greedy, _inputs

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    from koboldcpp_amd import expose as X
    return X.init_library(), X


def _runtime_tokens(hp, types, ids, n, ub=512):
    import koboldcpp_amd.lib as K
    m = C.setup_model(K.Model(C.model_hp(hp), types, max_ubatch=ub), hp)
    m.decode(ids, 0, want_logits=False)
    want = [m.argmax()]
    p = len(ids)
    for _ in range(n - 1):
        want.append(m.decode_greedy(p))
        p += 1
    m.close()
    return want


def _text(hp, toks, ids):
    _, _, ttypes = GW.spm_vocab(hp["n_vocab"], WORDS)
    return b"".join(piece(toks, ttypes, t) for t in ids)


@pytest.mark.parametrize("tag", C.TAGS)
def test_generate_greedy_matches_runtime(lib, tmp_path, tag):
    h, X = lib
    hp, types = C.tag_hp(tag), C.tag_types(tag)
    path = str(tmp_path / "cmdr.gguf")
    toks = C.commandr_gguf(path, hp, types)
    assert h.load_model(_inputs(X, path))
    prompt = b"hello world the a b of to the"
    r = h.token_count(prompt, True)
    ids = [r.ids[i] for i in range(r.count)]
    out = h.generate(_greedy(X, prompt, 12))
    assert out.status == 1 and h.get_last_token_count() == 12
    assert out.text == _text(hp, toks, _runtime_tokens(hp, types, ids, 12))


def test_two_virtual_stages_equal_one(lib, tmp_path, monkeypatch):
    """the three switches reach every stage of a layer split"""
    h, X = lib
    hp, types = C.tag_hp("q4km"), C.tag_types("q4km")
    path = str(tmp_path / "cmdr2.gguf")
    C.commandr_gguf(path, hp, types)
    prompt = b" ".join([b"hello world the a b of to"] * 3)
    texts = []
    for nstage in (1, 2):
        monkeypatch.setenv("KCPP_VIRTUAL_DEVICES", str(nstage))
        li = _inputs(X, path, ub=16)
        for i in range(nstage):
            li.tensor_split[i] = 1.0
        assert h.load_model(li)
        out = h.generate(_greedy(X, prompt, 10))
        assert out.status == 1
        texts.append(out.text)
    assert texts[0] == texts[1]


def test_sampled_request_same_tokens_with_and_without_front_end(lib, tmp_path):
    """temperature 1, top-k 40, a fixed seed: the device candidate front end and the host sampler (KCPP_SAMPLE_DEV=0's
    path, switched per call) read the same scaled logits"""
    import koboldcpp_amd.lib as K
    from test_gpu_sample_front import _request, _run
    h, X = lib
    hp = dict(C.tag_hp("q4km"), n_vocab=8192)       # the front end serves vocabularies above its 5000 candidates
    path = str(tmp_path / "cmdr.gguf")
    C.commandr_gguf(path, hp, C.tag_types("q4km"))
    assert h.load_model(_inputs(X, path))
    gi = _request(X, temperature=1.0, top_k=40, top_p=1.0, max_length=32)
    _run(K, h, gi, False)                                    # the prompt into the KV cache (see test_gpu_sample_front)
    on, s_on = _run(K, h, gi, True)
    off, s_off = _run(K, h, gi, False)
    assert s_on == [32, 0, 0, 0] and s_off == [0, 0, 0, 0]
    assert len(on) == 32 and on == off
    assert len(set(on)) > 4


def test_quantized_kv_loads_and_generates(lib, tmp_path):
    h, X = lib
    hp, types = C.tag_hp("q4km"), C.tag_types("q4km")
    path = str(tmp_path / "cmdr.gguf")
    toks = C.commandr_gguf(path, hp, types)
    li = _inputs(X, path)
    li.quant_k = li.quant_v = 1
    li.flash_attention = True
    assert h.load_model(li)
    prompt = b"hello world the a b of to the"
    out = h.generate(_greedy(X, prompt, 8))
    assert out.status == 1 and h.get_last_token_count() == 8
    import koboldcpp_amd.lib as K
    r = h.token_count(prompt, True)
    ids = [r.ids[i] for i in range(r.count)]
    m = C.setup_model(K.Model(C.model_hp(hp), types), hp)
    m.set_kv_types(R.Q8_0, R.Q8_0)
    m.decode(ids, 0, want_logits=False)
    want = [m.argmax()]
    for i in range(7):
        want.append(m.decode_greedy(len(ids) + i))
    m.close()
    assert out.text == _text(hp, toks, want)


def test_context_shift_request_erases_once(lib, tmp_path, capfd):
    """as tests/test_gpu_context_shift.py checks for Llama: the second prompt is the first with 30 words cut after a
    20-word head plus 30 new ones; generate() erases the span (NORM pairs, the existing K-shift kernel) once"""
    h, X = lib
    hp = C.tag_hp("q4k")
    path = str(tmp_path / "cmdr.gguf")
    C.commandr_gguf(path, hp, C.tag_types("q4k"))
    words = ["hello", "world", "the"]
    rng = np.random.default_rng(11)
    A = [words[i] for i in rng.integers(0, len(words), size=235)]
    B = A[:20] + A[50:] + [words[i] for i in rng.integers(0, len(words), size=30)]
    outs = []
    for shift in (True, False):
        assert h.load_model(_inputs(X, path, shift=shift))
        res = []
        for ws in (A, B):
            out = h.generate(_greedy(X, " ".join(ws).encode(), 4))
            assert out.status == 1
            res.append([h.new_token(i) for i in range(h.get_stream_count())])
        outs.append(res)
    err = capfd.readouterr().err
    assert err.count("Context Shifting: Erased") == 1, err
    assert outs[0][0] == outs[1][0]
    assert outs[0][1][:1] == outs[1][1][:1]


P = "command-r."
E, EKV = C.TINY_CMDR["n_embd"], C.TINY_CMDR["n_embd"]
# name: (writer arguments -- hp: hyper-parameter overrides --, what the message must name)
REFUSALS = {
    "no_eps": (dict(kv_drop=(P + "attention.layer_norm_epsilon",)), P + "attention.layer_norm_epsilon"),
    "no_logit_scale": (dict(kv_drop=(P + "logit_scale",)), P + "logit_scale"),
    "q_norm": (dict(extra_tensors=[("blk.1.attn_q_norm.weight", R.F32, [128, 16], bytes(128 * 16 * 4))]),
               "blk.1.attn_q_norm"),
    "k_norm": (dict(extra_tensors=[("blk.0.attn_k_norm.weight", R.F32, [128, 16], bytes(128 * 16 * 4))]),
               "blk.0.attn_k_norm"),
    "plus_depth": (dict(kv_extra={P + "block_count": 64}), P + "block_count"),
    "gqa_12": (dict(hp=dict(n_head=24, n_head_kv=2, n_embd=3072)), P + "attention.head_count_kv"),
    "gqa_not_whole": (dict(hp=dict(n_head_kv=3)), P + "attention.head_count_kv"),
    "head_dim": (dict(hp=dict(n_head=8)), "head_dim"),
    "experts": (dict(kv_extra={P + "expert_count": 4}), P + "expert_count"),
    "yarn": (dict(kv_extra={P + "rope.scaling.type": "yarn"}), "YaRN"),
    "row_blocks": (dict(hp=dict(n_ff=1056)), "ffn_down"),          # ffn_down rows of 1056 elements in Q4_K
    "f16_head": (dict(emb_f16=True), "token_embd.weight"),
    "partial_bias": (dict(extra_tensors=[("blk.0.attn_q.bias", R.F32, [E], bytes(E * 4)),
                                         ("blk.0.attn_v.bias", R.F32, [EKV], bytes(EKV * 4))]), "blk.0.attn_k.bias"),
}

CHILD = r"""
import sys
sys.path.insert(0, sys.argv[2]); sys.path.insert(0, sys.argv[3])
from koboldcpp_amd import expose as X
from test_gpu_qwen2_expose import _inputs
h = X.init_library()
ok = h.load_model(_inputs(X, sys.argv[1]))
print("LOADED" if ok else "REFUSED")
"""


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals(tmp_path, name):
    kw, needle = REFUSALS[name]
    kw = dict(kw)
    hp = dict(C.TINY_CMDR, **kw.pop("hp", {}))
    types = C.tag_types("q4k")
    path = str(tmp_path / (name + ".gguf"))
    if kw.pop("emb_f16", False):         # a tied F16 embedding: token_embd.weight replaced by an F16 tensor
        emb = C.embedding_f32(hp).astype(np.float16)
        kw.update(drop=("token_embd.weight",),
                  extra_tensors=[("token_embd.weight", R.F16, [hp["n_embd"], hp["n_vocab"]], emb.tobytes())])
    C.commandr_gguf(path, hp, types, **kw)
    r = subprocess.run([sys.executable, "-c", CHILD, path, os.path.dirname(HERE), HERE], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "REFUSED" in r.stdout and "LOADED" not in r.stdout, (r.stdout, r.stderr[-2000:])
    assert needle in r.stderr, r.stderr[-2000:]


def test_biases_load_when_complete(lib, tmp_path):
    """blk.N.attn_{q,k,v}.bias are optional in build_command_r: all three of a layer go through set_qkv_bias (that
    layer's q|k|v then decodes unfused: no LayerNorm prologue instance carries a bias)"""
    import koboldcpp_amd.lib as K
    h, X = lib
    hp, types = C.tag_hp("q4k"), C.tag_types("q4k")
    n = hp["n_embd"]
    bias = [(np.arange(n) % 7 - 3).astype(np.float32) * np.float32(0.125 * (j + 1)) for j in range(3)]
    extra = [("blk.0.attn_%s.bias" % c, R.F32, [n], b.tobytes()) for c, b in zip("qkv", bias)]
    path = str(tmp_path / "cmdr_bias.gguf")
    toks = C.commandr_gguf(path, hp, types, extra_tensors=extra)
    assert h.load_model(_inputs(X, path))
    prompt = b"hello world the a b of to the"
    out = h.generate(_greedy(X, prompt, 8))
    assert out.status == 1
    r = h.token_count(prompt, True)
    ids = [r.ids[i] for i in range(r.count)]
    m = C.setup_model(K.Model(C.model_hp(hp), types), hp)
    m.set_qkv_bias(0, *bias)
    m.decode(ids, 0, want_logits=False)
    want = [m.argmax()]
    for i in range(7):
        want.append(m.decode_greedy(len(ids) + i))
    m.close()
    assert out.text == _text(hp, toks, want)
