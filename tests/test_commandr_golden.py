"""The Command-R fixture (tests/golden/commandr_tiny.npz, from the reference ggml: tests/golden/make_commandr.py) is fit
for its purpose, checked without a GPU: LayerNorm matters for it (layer-input rows far from zero mean), enough steps pin
the greedy token against the reference's own noise, and the recorded ggml_norm + ggml_mul rows are what the documented
arithmetic gives -- the arithmetic kcpp_layer_norm and the PRO 3 prologue implement."""
import os

import numpy as np
import pytest

import commandr_gguf as C

FX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "commandr_tiny.npz")
LN_CASES = {"ln2048": (2048, 1), "ln1792": (1792, 9), "ln8192": (8192, 3)}
LN_EPS = 1e-5


@pytest.fixture(scope="module")
def fx():
    return np.load(FX)


def layer_norm_ref(x, w, eps):
    """ggml_compute_forward_norm_f32 (two passes, sequential double sums) then ggml_mul, in numpy"""
    x = np.asarray(x, np.float32)
    n = x.shape[-1]
    y = np.empty_like(x)
    for r in range(x.shape[0]):
        mean = np.float32(np.cumsum(x[r].astype(np.float64))[-1] / n)
        v = (x[r] - mean).astype(np.float32)
        var = np.float32(np.cumsum((v * v).astype(np.float32).astype(np.float64))[-1] / n)
        scale = np.float32(1.0) / np.sqrt(np.float32(var + np.float32(eps)))
        y[r] = ((v * scale).astype(np.float32) * w).astype(np.float32)
    return y


@pytest.mark.parametrize("tag", C.TAGS)
def test_fixture_shape_and_inputs(fx, tag):
    hp = C.tag_hp(tag)
    assert fx[tag + "_types"].tolist() == C.tag_types(tag)
    assert fx[tag + "_prompt"].tolist() == C.prompt_tokens(hp, int(fx["prompt_seed"]))
    assert len(fx[tag + "_prompt"]) == C.N_PROMPT == 17 and len(fx[tag + "_tokens"]) == C.N_GEN == 6
    assert fx[tag + "_logits"].shape == (1 + C.N_GEN, hp["n_vocab"])
    # greedy: each token is the argmax of the step before it
    assert fx[tag + "_tokens"].tolist() == np.argmax(fx[tag + "_logits"][:-1], axis=1).tolist()


@pytest.mark.parametrize("tag", C.TAGS)
def test_layer_inputs_are_far_from_zero_mean(fx, tag):
    """every layer sees prompt rows with |mean| / std >= 0.25: with a zero-mean input LayerNorm is RMS norm"""
    ms = fx[tag + "_lin_ms"]
    assert ms.shape == (2, C.N_PROMPT)
    assert (ms.max(axis=1) >= 0.25).all(), ms.max(axis=1)


@pytest.mark.parametrize("tag", C.TAGS)
def test_enough_steps_pin_the_token(fx, tag):
    """at least 4 of the 7 steps have a top-2 margin above 4 x the reference's own spread / flash-attention gap"""
    bar = 4.0 * max(float(fx[tag + "_spread_max"].max()), float(fx[tag + "_fagap_max"].max()))
    top2 = np.sort(fx[tag + "_logits"].astype(np.float64), axis=1)[:, -2:]
    assert int(((top2[:, 1] - top2[:, 0]) > bar).sum()) >= 4


@pytest.mark.parametrize("name", sorted(LN_CASES))
def test_numpy_layer_norm_equals_the_reference(fx, name):
    width, rows = LN_CASES[name]
    x, w, y = fx[name + "_x"], fx[name + "_w"], fx[name + "_y"]
    assert x.shape == y.shape == (rows, width)
    xs = x.astype(np.float64)
    if rows > 1:      # row means up to 3 x the std: the mean's subtraction cancels digits
        assert (np.abs(xs.mean(axis=1)) / xs.std(axis=1)).max() > 2.9
    assert np.array_equal(layer_norm_ref(x, w, LN_EPS).view(np.uint32), y.view(np.uint32))


def test_embedding_rows_have_an_offset():
    e = C.embedding_f32(C.TINY_CMDR).astype(np.float64)
    r = np.abs(e.mean(axis=1)) / e.std(axis=1)
    assert r.min() > 0.9 and r.max() < 2.2
