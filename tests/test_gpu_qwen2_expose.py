"""Qwen2 GGUFs through the koboldcpp drop-in ABI: load_model + greedy generate on a synthetic qwen2 file
(tests/qwen2_gguf.py) equals the in-process runtime with set_rope_mode(2) + set_qkv_bias, on one stage and on three
virtual stages; a context-shift request runs; a file without a bias tensor, or of architecture qwen2moe, is refused.
Every test loads its own model: load_model replaces the process-wide one."""
import numpy as np
import pytest

import gguf_writer as GW
import qwen2_gguf as Q
from test_gpu_expose import WORDS, piece

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    from koboldcpp_amd import expose as X
    return X.init_library(), X


def _inputs(X, path, ub=512, shift=False):
    li = X.load_model_inputs()
    li.model_filename = path.encode()
    li.max_context_length = 248
    li.blasbatchsize = ub
    li.gpulayers = 999
    li.rope_freq_base = 10000.0
    li.rope_freq_scale = 0.0     # koboldcpp.py default --ropeconfig 0: automatic RoPE (a base of 1e6 is the model's own)
    li.use_contextshift = shift
    return li


def _greedy(X, prompt, n):
    gi = X.generation_inputs()
    gi.prompt = prompt
    gi.memory = b""
    gi.max_context_length = 248
    gi.max_length = n
    gi.temperature = 0.0
    gi.top_k = 1
    gi.rep_pen = 1.0
    gi.bypass_eos_token = True
    gi.seed = 7
    return gi


def _runtime_text(hp, types, ids, n, toks, ub=512):
    import koboldcpp_amd.lib as K
    m = K.Model(hp, types, max_ubatch=ub)
    m.synth(Q.SEED)
    m.set_rope_mode(2)
    for il in range(hp["n_layer"]):
        m.set_qkv_bias(il, *Q.qkv_bias(hp, il))
    m.decode(ids, 0, want_logits=False)
    want = [m.argmax()]
    p = len(ids)
    for _ in range(n - 1):
        want.append(m.decode_greedy(p))
        p += 1
    m.close()
    _, _, ttypes = GW.spm_vocab(hp["n_vocab"], WORDS)
    return b"".join(piece(toks, ttypes, t) for t in want)


@pytest.mark.parametrize("tag", ["q4k", "q8_0", "q4km_w"])
def test_generate_greedy_matches_runtime(lib, tmp_path, tag):
    h, X = lib
    hp = dict(Q.tag_hp(tag))
    types = Q.tag_types(tag)
    path = str(tmp_path / "qwen2.gguf")
    toks = Q.qwen2_gguf(path, hp, types, Q.SEED)
    assert h.load_model(_inputs(X, path))
    prompt = b"hello world the a b of to the"
    r = h.token_count(prompt, True)
    ids = [r.ids[i] for i in range(r.count)]
    out = h.generate(_greedy(X, prompt, 12))
    assert out.status == 1 and h.get_last_token_count() == 12
    assert out.text == _runtime_text(hp, types, ids, 12, toks)


def test_three_virtual_stages_equal_one(lib, tmp_path, monkeypatch):
    """biases and the rope mode reach every stage of a layer split for the layers it owns"""
    h, X = lib
    hp = dict(Q.TINY_QWEN2, n_layer=3)
    types = Q.tag_types("q4k", 3)
    path = str(tmp_path / "qwen2_3.gguf")
    toks = Q.qwen2_gguf(path, hp, types, Q.SEED)
    prompt = b" ".join([b"hello world the a b of to"] * 3)
    texts = []
    for nstage in (1, 3):
        monkeypatch.setenv("KCPP_VIRTUAL_DEVICES", str(nstage))
        li = _inputs(X, path, ub=16)
        for i in range(nstage):
            li.tensor_split[i] = 1.0
        assert h.load_model(li)
        out = h.generate(_greedy(X, prompt, 10))
        assert out.status == 1
        texts.append(out.text)
    assert texts[0] == texts[1]
    r = h.token_count(prompt, True)
    assert texts[0] == _runtime_text(hp, types, [r.ids[i] for i in range(r.count)], 10, toks, ub=16)


def test_context_shift_request_runs(lib, tmp_path, capfd):
    """the second prompt is the first with 30 words cut after a 20-word head plus 30 new ones: generate() erases the
    span (the K-shift on NeoX pairs) and continues with the token the unshifted run gives"""
    h, X = lib
    hp = dict(Q.TINY_QWEN2)
    path = str(tmp_path / "qwen2.gguf")
    Q.qwen2_gguf(path, hp, Q.tag_types("q4k"), Q.SEED)
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


def test_refusals(lib, tmp_path, capfd):
    h, X = lib
    hp = dict(Q.TINY_QWEN2)
    types = Q.tag_types("q4k")
    p1 = str(tmp_path / "nobias.gguf")
    Q.qwen2_gguf(p1, hp, types, Q.SEED, drop=("blk.0.attn_k.bias",))
    assert not h.load_model(_inputs(X, p1))
    assert "blk.0.attn_k.bias" in capfd.readouterr().err
    p2 = str(tmp_path / "moe.gguf")
    Q.qwen2_gguf(p2, hp, types, Q.SEED, arch="qwen2moe")
    assert not h.load_model(_inputs(X, p2))
    assert "architecture 'qwen2moe' not supported" in capfd.readouterr().err
