"""Qwen2-MoE GGUFs through the koboldcpp drop-in ABI: load_model + greedy generate on a synthetic qwen2moe file
(tests/qwen2moe_gguf.py) equals the in-process runtime, which tests/test_gpu_qwen2moe_model.py holds to the reference's
fixture (generate() takes text, the fixture's prompt is token ids, so the tokens are compared through the runtime); on
three virtual stages the text is the same; a quantized KV cache loads and generates; a context-shift request erases a
span once; files the runtime cannot take are refused at load with the tensor or key named.
Every test loads its own model: load_model replaces the process-wide one."""
import numpy as np
import pytest

import gguf_writer as GW
import qwen2moe_gguf as QM
import refharness as R
from test_gpu_expose import WORDS, piece
from test_gpu_qwen2_expose import _greedy, _inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import torch
    assert torch.cuda.is_available()
    from koboldcpp_amd import expose as X
    return X.init_library(), X


def _runtime_text(tag, hp, types, ids, n, toks, ub=512):
    import koboldcpp_amd.lib as K
    m = QM.model(K, tag, types=types, ub=ub, hp=hp)
    m.decode(ids, 0, want_logits=False)
    want = [m.argmax()]
    p = len(ids)
    for _ in range(n - 1):
        want.append(m.decode_greedy(p))
        p += 1
    m.close()
    _, _, ttypes = GW.spm_vocab(hp["n_vocab"], WORDS)
    return b"".join(piece(toks, ttypes, t) for t in want)


@pytest.mark.parametrize("tag", ["a27", "top2"])
def test_generate_greedy_matches_runtime(lib, tmp_path, tag):
    h, X = lib
    hp, types = dict(QM.tag_hp(tag)), QM.tag_types(tag)
    path = str(tmp_path / "qwen2moe.gguf")
    toks = QM.qwen2moe_gguf(path, hp, types)
    assert h.load_model(_inputs(X, path))
    prompt = b"hello world the a b of to the"
    r = h.token_count(prompt, True)
    ids = [r.ids[i] for i in range(r.count)]
    out = h.generate(_greedy(X, prompt, 12))
    assert out.status == 1 and h.get_last_token_count() == 12
    assert out.text == _runtime_text(tag, hp, types, ids, 12, toks)


def test_three_virtual_stages_and_quantized_kv(lib, tmp_path, monkeypatch):
    """the shared expert's tensors follow their layer to its stage; quant_k = quant_v = 1 loads and generates"""
    h, X = lib
    tag = "top2"
    hp, types = dict(QM.tag_hp(tag)), QM.tag_types(tag)
    path = str(tmp_path / "qwen2moe.gguf")
    toks = QM.qwen2moe_gguf(path, hp, types)
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
    assert texts[0] == _runtime_text(tag, hp, types, [r.ids[i] for i in range(r.count)], 10, toks, ub=16)
    monkeypatch.setenv("KCPP_VIRTUAL_DEVICES", "1")
    li = _inputs(X, path)
    li.quant_k = li.quant_v = 1
    assert h.load_model(li)
    out = h.generate(_greedy(X, prompt, 6))
    assert out.status == 1 and h.get_last_token_count() == 6


def test_context_shift_erases_a_span_once(lib, tmp_path, capfd):
    h, X = lib
    tag = "top2"
    path = str(tmp_path / "qwen2moe.gguf")
    QM.qwen2moe_gguf(path, QM.tag_hp(tag), QM.tag_types(tag))
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


def test_refusals_name_the_cause(lib, tmp_path, capfd, monkeypatch):
    h, X = lib
    tag = "a27"
    hp, types = dict(QM.tag_hp(tag)), QM.tag_types(tag)
    E, F, NE = hp["n_embd"], hp["n_ff"], hp["n_expert"]
    cases = {
        "65 experts": (dict(kv_extra={"qwen2moe.expert_count": 65}), "qwen2moe.expert_count 65"),
        "no ffn_down_shexp": (dict(drop=("blk.1.ffn_down_shexp.weight",)), "blk.1.ffn_down_shexp.weight"),
        # rows of 1408 are 5.5 Q4_K blocks: llama.cpp's quantizer falls back to Q5_0 / Q8_0 there
        "Q4_K ffn_down_exps at K 1408": (dict(raw={"blk.0.ffn_down_exps.weight": (
            R.Q4_K, [F, E, NE], bytes(F // 256 * 144 * E * NE))}), "blk.0.ffn_down_exps.weight"),
        "Q8_0 gate vector": (dict(raw={"blk.0.ffn_gate_inp_shexp.weight": (R.Q8_0, [E], bytes(E // 32 * 34))}),
                             "blk.0.ffn_gate_inp_shexp.weight"),
    }
    for what, (kw, named) in cases.items():
        path = str(tmp_path / "bad.gguf")
        QM.qwen2moe_gguf(path, hp, types, **kw)
        assert not h.load_model(_inputs(X, path)), what
        err = capfd.readouterr().err
        assert named in err, (what, err)
    # row split: MoE expert tensors cannot be split
    QM.qwen2moe_gguf(path, hp, types)
    monkeypatch.setenv("KCPP_VIRTUAL_DEVICES", "2")
    li = _inputs(X, path)
    li.use_rowsplit = True
    li.tensor_split[0] = li.tensor_split[1] = 1.0
    assert not h.load_model(li)
    assert "row split" in capfd.readouterr().err
