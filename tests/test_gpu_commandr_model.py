"""The Command-R graph end to end in the runtime: K.Model(TINY_CMDR) + synth + the tied embedding + set_norm_mode(1) +
set_parallel_block(1) + set_logit_scale against the reference's logits (tests/golden/commandr_tiny.npz, from
tests/golden/make_commandr.py), teacher-forced with the reference's own greedy tokens.

Bars (all four numbers per tag come from the fixture, max over its steps), the ones tests/test_gpu_qwen2_model.py uses
for the same reasons:
* production attention: max and median |dlogit| per step <= 2 x max(spread, fagap);
* set_fa_exact(1): <= 1.5 x spread;
* the greedy token equal on the steps whose top-2 margin exceeds 2 x the bar.
Self-consistency under tests/test_gpu_model.py's bars: fused decode vs set_fused_decode(0) (max < TOL_MAX, median <
1e-5), graphs on vs off (equal), ubatch 8 vs 512 and two layer-split stages vs one (atol TOL_MAX); a Q8_0 K / V cache
against the fixture's Q8_0-cache run under tests/test_gpu_kvq.py's bar.

Tags: q4k (16 / 16 heads, every matrix Q4_K: each decode launch of a layer runs its LayerNorm prologue instance), q4km
(16 / 2 heads, layer 1 through the mixed q|k + v launch), q8_0 (no LayerNorm prologue: the unfused fallback inside the
graph).  The head has 512 rows, below the prologue's instance, so it runs norm -> quantize -> PRO 0 in every tag."""
import os

import numpy as np
import pytest

import commandr_gguf as C
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
    return np.load(os.path.join(HERE, "golden", "commandr_tiny.npz"))


def cmdr_model(K, tag, ub=512, **kw):
    hp = C.tag_hp(tag)
    sw = {k: kw.pop(k) for k in ("norm_mode", "parallel", "logit_scale") if k in kw}
    return C.setup_model(K.Model(C.model_hp(hp), C.tag_types(tag), max_ubatch=ub, **kw), hp, **sw)


def run_forced(K, tag, prompt, forced, exact=False, fused=True, graphs=True, ub=512, kv=None):
    m = cmdr_model(K, tag, ub)
    if kv is not None:
        m.set_kv_types(kv, kv)
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


_base = {}


def base_run(K, fx, tag):
    """the production run of a tag, computed once and shared (never modified)"""
    if tag not in _base:
        _base[tag] = run_forced(K, tag, [int(t) for t in fx[tag + "_prompt"]], fx[tag + "_tokens"])
        _base[tag].setflags(write=False)
    return _base[tag]


@pytest.mark.parametrize("exact", [False, True], ids=["production", "strict"])
@pytest.mark.parametrize("tag", C.TAGS)
def test_commandr_vs_reference(K, fx, tag, exact):
    assert [int(t) for t in fx[tag + "_types"]] == C.tag_types(tag)
    prompt = [int(t) for t in fx[tag + "_prompt"]]
    L = fx[tag + "_logits"]
    got = run_forced(K, tag, prompt, fx[tag + "_tokens"], exact=True) if exact else base_run(K, fx, tag)
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
    assert clear.sum() >= 1
    assert np.all(np.argmax(got, axis=1)[clear] == np.argmax(L, axis=1)[clear])
    assert np.all(d.max(axis=1) <= bar_max), d.max(axis=1)
    assert np.all(np.median(d, axis=1) <= bar_med), np.median(d, axis=1)


@pytest.mark.parametrize("tag", C.TAGS)
def test_commandr_self_consistency(K, fx, tag):
    prompt = [int(t) for t in fx[tag + "_prompt"]]
    forced = fx[tag + "_tokens"]
    base = base_run(K, fx, tag)
    d = np.abs(base - run_forced(K, tag, prompt, forced, fused=False))
    print("%s fused vs unfused: max %.3g median %.3g" % (tag, d.max(), np.median(d)))
    assert d.max() < TOL_MAX and np.median(d) < 1e-5, (d.max(), np.median(d))
    assert np.array_equal(base, run_forced(K, tag, prompt, forced, graphs=False))
    np.testing.assert_allclose(base, run_forced(K, tag, prompt, forced, ub=8), rtol=0, atol=TOL_MAX)


@pytest.mark.parametrize("tag", ("q4km", "q8_0"))
def test_commandr_layer_split(K, fx, tag):
    """two stages (layer 0 with the embedding | layer 1 with the head), the residual row handed over: the hand-off is the
    Llama one, (ffn + x) + attn_out is complete when a stage ends"""
    hp = C.tag_hp(tag)
    E = hp["n_embd"]
    prompt = [int(t) for t in fx[tag + "_prompt"]]
    m0 = cmdr_model(K, tag, il0=0, il1=1, has_embed=True, has_output=False)
    m1 = cmdr_model(K, tag, il0=1, il1=2, has_embed=False, has_output=True)
    out, n = [], 0
    for toks in [prompt] + [[int(t)] for t in fx[tag + "_tokens"]]:
        T = len(toks)
        m0.decode(toks, n, want_logits=False)
        h = np.ascontiguousarray(m0.read_hidden(T * E))
        m1.hidden_io(h.ctypes.data, T * E, 0, to_buf=False)
        out.append(m1.decode(None, n, n_tokens=T))
        n += T
    m0.close()
    m1.close()
    d = np.abs(np.array(out) - base_run(K, fx, tag))
    print("%s two stages vs one: max %.3g" % (tag, d.max()))
    assert d.max() <= TOL_MAX


@pytest.mark.parametrize("tag", ("q4km", "q8_0"))
def test_commandr_quantized_kv(K, fx, tag):
    """Q8_0 K / V cache (the per-op path: LayerNorm, the parallel block and the logit scale outside the fused chain):
    graphs on == graphs off; for the tag the fixture holds a Q8_0-cache reference run of, per step within 2 x that run's
    own AVX2-vs-scalar spread, the bar tests/test_gpu_kvq.py holds the Llama model to"""
    prompt = [int(t) for t in fx[tag + "_prompt"]]
    forced = fx[tag + "_tokens"]
    a = run_forced(K, tag, prompt, forced, kv=R.Q8_0)
    assert np.array_equal(a, run_forced(K, tag, prompt, forced, kv=R.Q8_0, graphs=False))
    if tag != "q4km":
        return
    d = np.abs(a - fx["kvq8_logits"])
    print("%s q8_0 kv vs reference: max per step %s median %s" % (tag, np.round(d.max(axis=1), 4), np.round(np.median(d, axis=1), 5)))
    assert np.all(d.max(axis=1) <= 2 * float(fx["kvq8_spread_max"].max()))
    assert np.all(np.median(d, axis=1) <= 2 * float(fx["kvq8_spread_med"].max()))


def test_each_switch_changes_the_logits(K, fx):
    """the fixture is not reachable without the feature: RMS norm, the serial block, or no logit scale, each alone,
    move step 0's logits by more than 10 x fagap_max"""
    tag = "q4k"
    prompt = [int(t) for t in fx[tag + "_prompt"]]
    L = fx[tag + "_logits"]
    bar = 10 * float(fx[tag + "_fagap_max"].max())
    assert np.abs(base_run(K, fx, tag)[0] - L[0]).max() < bar
    for off in (dict(norm_mode=0), dict(parallel=0), dict(logit_scale=0.0)):
        m = cmdr_model(K, tag, **off)
        d = np.abs(m.decode(prompt, 0) - L[0]).max()
        m.close()
        print(off, "moves step 0 by", d, "bar", bar)
        assert d > bar, (off, d)


def test_setter_arguments(K):
    m = K.Model(C.model_hp(C.TINY_CMDR), C.tag_types("q4k"))
    assert K.raw().kcpp_model_set_norm_mode(m.m, 2) == -1
    assert K.raw().kcpp_model_set_parallel_block(m.m, 2) == -1
    assert K.raw().kcpp_model_set_logit_scale(m.m, float("nan")) == -1
    m.set_norm_mode(1)
    m.set_parallel_block(1)
    m.set_logit_scale(0.0625)
    m.close()
    moe = K.Model(R.TINY_MOE, R.moe_types(R.TINY_MOE["n_layer"]))
    assert K.raw().kcpp_model_set_norm_mode(moe.m, 1) == -1
    assert K.raw().kcpp_model_set_parallel_block(moe.m, 1) == -1
    moe.close()


def test_llama_unchanged_by_default_switches(K):
    """a Llama-typed model with the three switches set to their defaults gives bitwise the logits it gives without
    those calls (prefill and graph-replayed decode)"""
    types = R.q4_k_m_types(R.TINY["n_layer"])
    prompt = list(range(3, 20))
    outs = []
    for calls in (False, True):
        m = K.Model(R.TINY, types)
        m.synth(1234)
        if calls:
            m.set_norm_mode(0)
            m.set_parallel_block(0)
            m.set_logit_scale(1.0)
        lg = [m.decode(prompt, 0)]
        n = len(prompt)
        for tok in (7, 100, 3):
            lg.append(m.decode([tok], n))
            n += 1
        m.close()
        outs.append(np.array(lg))
    assert np.array_equal(outs[0], outs[1])
