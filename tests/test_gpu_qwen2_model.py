"""The Qwen2 graph end to end in the runtime: K.Model(TINY_QWEN2) + synth + set_rope_mode(2) + set_qkv_bias against the
reference's logits (tests/golden/qwen2_tiny.npz, from tests/golden/make_qwen2.py), teacher-forced with the reference's
own greedy tokens.

Bars (all four numbers per tag come from the fixture, max over its steps):
* production attention: max and median |dlogit| per step <= 2 x max(spread, fagap) -- spread = the reference's AVX2
  vs scalar builds, fagap = its flash-attention graph vs its flash-attention-off graph (f16 vs f32 accumulation of
  P.V); the gap is allowed because production accumulates P.V in f32 where the reference's flash attention keeps f16;
* set_fa_exact(1): <= 1.5 x spread, as the strict mode is held to elsewhere (tests/test_gpu_fa_exact.py).
Self-consistency under the bars tests/test_gpu_model.py uses for the same Llama comparisons: fused decode vs
set_fused_decode(0) (max < TOL_MAX, median < 1e-5), graphs on vs off (equal), ubatch 8 vs 512 (atol TOL_MAX).

Tags (the first three on TINY_QWEN2, n_embd 1792; q4km_w on WIDE_QWEN2, n_embd 2048): q4km (layer 0 all Q4_K: the
fused k_gemv_rs launch with bias and NeoX pairs; layer 1 attn_v Q6_K, which has no Q6_K_RS layout at n_embd 1792, so
that layer's q|k|v decode through the unfused fallback), q4k (q|k|v all Q4_K: every
layer fused), q8_0 (the unfused fallback on the Q8_0 chain), q4km_w (layer 1 is the one-launch mixed Q4_K + Q6_K q|k|v
kernel with bias and NeoX pairs, reached through forward_layers_dec's own argument block)."""
import os

import numpy as np
import pytest

import qwen2_gguf as Q
import refharness as R
from test_gpu_model import TOL_MAX

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def K():
    import torch
    assert torch.cuda.is_available()
    import koboldcpp_amd.lib as K
    return K


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "qwen2_tiny.npz"))


def qwen2_model(K, types, ub, hp):
    m = K.Model(hp, types, max_ubatch=ub)
    m.synth(Q.SEED)
    m.set_rope_mode(2)
    for il in range(hp["n_layer"]):
        m.set_qkv_bias(il, *Q.qkv_bias(hp, il))
    return m


def run_forced(K, types, prompt, forced, exact=False, fused=True, graphs=True, ub=512, hp=Q.TINY_QWEN2):
    m = qwen2_model(K, types, ub, hp)
    m.set_graphs(graphs)
    m.set_fa_exact(exact)
    m.set_fused_decode(fused)
    out = [m.decode(prompt, 0)]
    n = len(prompt)
    for tok in forced:
        out.append(m.decode([int(tok)], n))
        n += 1
    m.close()
    return np.array(out)


@pytest.mark.parametrize("exact", [False, True], ids=["production", "strict"])
@pytest.mark.parametrize("tag", Q.TAGS)
def test_qwen2_vs_reference(K, fx, tag, exact):
    types = [int(t) for t in fx[tag + "_types"]]
    prompt = [int(t) for t in fx[tag + "_prompt"]]
    L = fx[tag + "_logits"]
    got = run_forced(K, types, prompt, fx[tag + "_tokens"], exact=exact, hp=Q.tag_hp(tag))
    d = np.abs(got - L)
    sp_max, sp_med = float(fx[tag + "_spread_max"].max()), float(fx[tag + "_spread_med"].max())
    fa_max, fa_med = float(fx[tag + "_fagap_max"].max()), float(fx[tag + "_fagap_med"].max())
    if exact:
        bar_max, bar_med = 1.5 * sp_max, 1.5 * sp_med
    else:
        bar_max, bar_med = 2 * max(sp_max, fa_max), 2 * max(sp_med, fa_med)
    print("%s %s: max per step %s (bar %.4g), median per step %s (bar %.4g)" % (
        tag, "strict" if exact else "production", np.round(d.max(axis=1), 4), bar_max,
        np.round(np.median(d, axis=1), 5), bar_med))
    top2 = np.sort(L, axis=1)[:, -2:]
    clear = top2[:, 1] - top2[:, 0] > 2 * bar_max          # steps whose greedy token the bar cannot flip
    assert np.all(np.argmax(got, axis=1)[clear] == np.argmax(L, axis=1)[clear])
    assert np.all(d.max(axis=1) <= bar_max), d.max(axis=1)
    assert np.all(np.median(d, axis=1) <= bar_med), np.median(d, axis=1)


@pytest.mark.parametrize("tag", Q.TAGS)
def test_qwen2_self_consistency(K, fx, tag):
    types = [int(t) for t in fx[tag + "_types"]]
    prompt = [int(t) for t in fx[tag + "_prompt"]]
    forced = fx[tag + "_tokens"]
    hp = Q.tag_hp(tag)
    base = run_forced(K, types, prompt, forced, hp=hp)
    d = np.abs(base - run_forced(K, types, prompt, forced, fused=False, hp=hp))
    print("%s fused vs unfused: max %.3g median %.3g" % (tag, d.max(), np.median(d)))
    assert d.max() < TOL_MAX and np.median(d) < 1e-5, (d.max(), np.median(d))
    assert np.array_equal(base, run_forced(K, types, prompt, forced, graphs=False, hp=hp))
    np.testing.assert_allclose(base, run_forced(K, types, prompt, forced, ub=8, hp=hp), rtol=0, atol=TOL_MAX)


def test_bias_and_mode_change_the_logits(K, fx):
    """the fixture is not reachable without the feature: NORM pairs, or no bias, move the logits far past the bar"""
    tag = "q4k"
    types = [int(t) for t in fx[tag + "_types"]]
    prompt = [int(t) for t in fx[tag + "_prompt"]]
    L = fx[tag + "_logits"]
    for mode, bias in ((0, True), (2, False)):
        m = K.Model(Q.TINY_QWEN2, types)
        m.synth(Q.SEED)
        m.set_rope_mode(mode)
        if bias:
            for il in range(Q.TINY_QWEN2["n_layer"]):
                m.set_qkv_bias(il, *Q.qkv_bias(Q.TINY_QWEN2, il))
        d = np.abs(m.decode(prompt, 0) - L[0]).max()
        m.close()
        assert d > 10 * float(fx[tag + "_fagap_max"].max()), (mode, bias, d)


def test_set_qkv_bias_arguments(K):
    m = K.Model(Q.TINY_QWEN2, Q.tag_types("q4k"))
    bq, bk, bv = Q.qkv_bias(Q.TINY_QWEN2, 0)
    assert K.raw().kcpp_model_set_rope_mode(m.m, 1) == -1
    assert K.raw().kcpp_model_set_qkv_bias(m.m, 2, bq.ctypes.data, bk.ctypes.data, bv.ctypes.data) == -1    # not a layer
    assert K.raw().kcpp_model_set_qkv_bias(m.m, 0, bq.ctypes.data, None, bv.ctypes.data) == -1             # all or none
    m.set_qkv_bias(0, bq, bk, bv)
    m.set_qkv_bias(0, None, None, None)
    m.close()


def test_llama_unchanged_by_default_mode_calls(K):
    """a Llama-typed model with set_rope_mode(0) and cleared biases gives bitwise the logits it gives without those
    calls (prefill and graph-replayed decode)"""
    types = R.q4_k_m_types(R.TINY["n_layer"])
    prompt = list(range(3, 20))
    outs = []
    for calls in (False, True):
        m = K.Model(R.TINY, types)
        m.synth(1234)
        if calls:
            m.set_rope_mode(0)
            m.set_qkv_bias(0, None, None, None)
        lg = [m.decode(prompt, 0)]
        n = len(prompt)
        for tok in (7, 100, 3):
            lg.append(m.decode([tok], n))
            n += 1
        m.close()
        outs.append(np.array(lg))
    assert np.array_equal(outs[0], outs[1])
