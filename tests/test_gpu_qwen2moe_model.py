"""build_qwen2moe end to end in the runtime: K.Model with kcpp_model_create_ex's extension (a shared expert, raw top-k
weights) + synth + the gate vectors + NeoX pairs + q / k / v biases (qwen2moe_gguf.model) against the reference's logits
and routing (tests/golden/qwen2moe_tiny.npz, from tests/golden/make_qwen2moe.py), teacher-forced with the reference's
own greedy tokens.

Bars, all from the fixture (max over its steps), as tests/test_gpu_qwen2_model.py sets them:
* production attention: max and median |dlogit| per step <= 2 x max(spread, fagap);
* set_fa_exact(1): <= 1.5 x spread;
* argmax equal wherever the reference's top-2 gap exceeds twice the bar.
Routing is compared exactly and nothing is left out (the fixture's routing gaps are >= 1e-4, ten times the bar
tests/test_gpu_moe.py calls clear): the prompt's layer-0 ids of all 17 tokens (a stage that ends after layer 0,
kcpp_model_moe_ids), the last layer's ids of the last prompt token, and both layers' ids of every decode step
(kcpp_model_moe_trace).  That comparison runs under set_fa_exact(1), the mode held to the reference's own arithmetic:
production attention accumulates P.V in f32 where the reference's flash attention keeps f16, a difference that moves
the reference's own router probabilities by up to 1.2e-3 between its two attention graphs (make_qwen2moe.py, "own
margin"), more than the fixture's smallest gaps; production attention is held to the fixture's set of experts in every row and to its order wherever the row's gaps
exceed twice own_dp (test_qwen2moe_production_routing; measured
on an MI355X: a27, top2, q8_0 none of 12 decode rows; a14 one of 12 -- its 7th and 8th expert the other way round, the
reference's probabilities 0.04838 / 0.04822).
Self-consistency under test_gpu_model.py's bars: fused decode vs set_fused_decode(0), graphs on vs off (equal), ubatch
8 vs 512, grouped vs per-expert prefill.

Tags: a27 (ratio 1, top-4 of 12, expert width 1408 with Q5_0 / Q8_0 down experts: slots + combine, per-expert
prefill), a14 (ratio 7, top-8, F16 router), top2 (the two-slot row-major pair path, F16 gate vector), q8_0 (every
matrix Q8_0)."""
import os

import numpy as np
import pytest

import qwen2moe_gguf as QM
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
    return np.load(os.path.join(HERE, "golden", "qwen2moe_tiny.npz"))


def run_forced(K, tag, fx, exact=False, fused=True, graphs=True, ub=512, grouped=True, trace=False, hp=None, tweak=None):
    prompt = [int(t) for t in fx[tag + "_prompt"]]
    hp = QM.tag_hp(tag) if hp is None else hp
    m = QM.model(K, tag, ub=ub, hp=hp)
    if tweak:
        tweak(m)
    m.set_graphs(graphs)
    m.set_fa_exact(exact)
    m.set_fused_decode(fused)
    m.set_moe_grouped(grouped)
    if trace:
        m.moe_trace(True)
    k = hp["n_expert_used"]
    out = [m.decode(prompt, 0)]
    ids = [m.moe_ids(len(prompt), k)[-1]] if trace else []
    tr = []
    n = len(prompt)
    for tok in fx[tag + "_tokens"]:
        out.append(m.decode([int(tok)], n))
        if trace:
            tr.append(m.moe_trace_read(hp["n_layer"], k))
        n += 1
    m.close()
    return (np.array(out), np.array(ids), np.array(tr)) if trace else np.array(out)


@pytest.fixture(scope="module")
def base(K, fx):
    """production logits per tag, computed once and shared"""
    return {tag: run_forced(K, tag, fx, trace=True) for tag in QM.TAGS}


@pytest.fixture(scope="module")
def strict(K, fx):
    """the same under set_fa_exact(1)"""
    return {tag: run_forced(K, tag, fx, exact=True, trace=True) for tag in QM.TAGS}


def _bars(fx, tag, exact):
    sp_max, sp_med = float(fx[tag + "_spread_max"].max()), float(fx[tag + "_spread_med"].max())
    fa_max, fa_med = float(fx[tag + "_fagap_max"].max()), float(fx[tag + "_fagap_med"].max())
    return (1.5 * sp_max, 1.5 * sp_med) if exact else (2 * max(sp_max, fa_max), 2 * max(sp_med, fa_med))


@pytest.mark.parametrize("exact", [False, True], ids=["production", "strict"])
@pytest.mark.parametrize("tag", QM.TAGS)
def test_qwen2moe_vs_reference(K, fx, base, strict, tag, exact):
    L = fx[tag + "_logits"]
    got = strict[tag][0] if exact else base[tag][0]
    d = np.abs(got - L)
    bar_max, bar_med = _bars(fx, tag, exact)
    print("%s %s: max per step %s (bar %.4g), median per step %s (bar %.4g)" % (
        tag, "strict" if exact else "production", np.round(d.max(axis=1), 4), bar_max,
        np.round(np.median(d, axis=1), 5), bar_med))
    top2 = np.sort(L, axis=1)[:, -2:]
    clear = top2[:, 1] - top2[:, 0] > 2 * bar_max
    assert np.all(np.argmax(got, axis=1)[clear] == np.argmax(L, axis=1)[clear])
    assert np.all(d.max(axis=1) <= bar_max), d.max(axis=1)
    assert np.all(np.median(d, axis=1) <= bar_med), np.median(d, axis=1)


def _layer0_prompt_ids(K, tag, prompt, k, exact):
    """layer 0's routing of every prompt token, from a stage that ends after layer 0"""
    m = QM.model(K, tag, il0=0, il1=1, has_output=False)
    m.set_fa_exact(exact)
    m.decode(prompt, 0, want_logits=False)
    got = m.moe_ids(len(prompt), k)
    m.close()
    return got


@pytest.mark.parametrize("tag", QM.TAGS)
def test_qwen2moe_routes_like_the_reference(K, fx, strict, tag):
    """strict mode: every layer's ids equal to the fixture's in order, prefill and decode, nothing left out"""
    hp = QM.tag_hp(tag)
    k = hp["n_expert_used"]
    prompt = [int(t) for t in fx[tag + "_prompt"]]
    _, last_ids, trace = strict[tag]
    assert np.array_equal(trace.reshape(-1, hp["n_layer"], k), fx[tag + "_ids"][1:])
    assert np.array_equal(last_ids[0], fx[tag + "_ids"][0, hp["n_layer"] - 1])
    assert np.array_equal(_layer0_prompt_ids(K, tag, prompt, k, True), fx[tag + "_ids_prompt"])


@pytest.mark.parametrize("tag", QM.TAGS)
def test_qwen2moe_production_routing(K, fx, base, tag):
    """production attention, same rows: the selected set of experts equals the fixture's in every row, and their order
    too in every row whose smallest gap among the first k+1 probabilities exceeds 2 x own_dp, the largest move of a
    recorded probability between the reference's own runs (the factor the logit bars give an implementation)"""
    hp = QM.tag_hp(tag)
    k, NL = hp["n_expert_used"], hp["n_layer"]
    prompt = [int(t) for t in fx[tag + "_prompt"]]
    _, last_ids, trace = base[tag]
    got = np.concatenate([trace.reshape(-1, k), last_ids[0][None], _layer0_prompt_ids(K, tag, prompt, k, False)])
    want = np.concatenate([fx[tag + "_ids"][1:].reshape(-1, k), fx[tag + "_ids"][0, NL - 1][None], fx[tag + "_ids_prompt"]])
    probs = np.concatenate([fx[tag + "_probs"][1:].reshape(-1, hp["n_expert"]), fx[tag + "_probs"][0, NL - 1][None],
                            fx[tag + "_probs_prompt"]]).astype(np.float64)
    top = np.sort(probs, axis=1)[:, ::-1][:, :k + 1]
    clear = (top[:, :-1] - top[:, 1:]).min(axis=1) > 2 * float(fx[tag + "_own_dp"])
    print("%s production: %d of %d rows ordered unlike the fixture, %d rows clear of 2 x own_dp = %.3g" % (
        tag, int((got != want).any(axis=1).sum()), len(got), int(clear.sum()), 2 * float(fx[tag + "_own_dp"])))
    assert np.array_equal(np.sort(got, axis=1), np.sort(want, axis=1))
    assert np.array_equal(got[clear], want[clear])


@pytest.mark.parametrize("tag", QM.TAGS)
def test_qwen2moe_self_consistency(K, fx, base, tag):
    b = base[tag][0]
    d = np.abs(b - run_forced(K, tag, fx, fused=False))
    print("%s fused vs unfused: max %.3g median %.3g" % (tag, d.max(), np.median(d)))
    assert d.max() < TOL_MAX and np.median(d) < 1e-5, (d.max(), np.median(d))
    assert np.array_equal(b, run_forced(K, tag, fx, graphs=False))
    np.testing.assert_allclose(b, run_forced(K, tag, fx, ub=8), rtol=0, atol=TOL_MAX)
    np.testing.assert_allclose(b, run_forced(K, tag, fx, grouped=False), rtol=0, atol=TOL_MAX)


def test_fixture_not_reachable_without_the_feature(K, fx, base):
    """normalised weights, another gate, or a shared expert that contributes nothing each move the logits past the
    bar.  No switch forces the gate to 1, so the gate row is negated instead (the gate becomes 1 - gate); the missing
    shared expert is ffn_down_shexp set to zero blocks, every other weight as the fixture's."""
    tag = "top2"
    L = fx[tag + "_logits"]
    bar_max, _ = _bars(fx, tag, False)
    assert np.abs(base[tag][0] - L).max() <= bar_max
    hp, ty = QM.tag_hp(tag), QM.tag_types(tag)
    shapes = QM.weight_shapes(hp)

    def negate_gate(m):
        for il in range(hp["n_layer"]):
            idx = 3 + QM.PER_LAYER * il + QM.J_GATE_VEC
            m.set_tensor(idx, np.ascontiguousarray(-QM.gate_vector(hp, il, ty[idx])))

    def zero_shexp(m):
        for il in range(hp["n_layer"]):
            idx = 3 + QM.PER_LAYER * il + 13
            k, n = shapes[idx]
            m.set_tensor(idx, np.zeros(R.row_bytes(ty[idx], k) * n, np.uint8))

    for what, kw in (("normalised weights", dict(hp=dict(hp, moe_norm_w=1))), ("negated gate row", dict(tweak=negate_gate)),
                     ("zero ffn_down_shexp", dict(tweak=zero_shexp))):
        d = np.abs(run_forced(K, tag, fx, **kw) - L).max()
        print("%s: max |dlogit| %.3g (bar %.3g)" % (what, d, bar_max))
        assert d > 2 * bar_max, what
