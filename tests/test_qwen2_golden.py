"""CPU checks of tests/golden/qwen2_tiny.npz (no GPU): every key is there with the right shape, the spreads are
finite and positive, the inputs the fixture is built from are what tests/qwen2_gguf.py makes today, and -- where the
reference build exists (oracle/_ref) -- one regenerated step equals the stored logits bit for bit, which pins the
fixture to the reference build as tests/test_oracle_golden.py pins the others."""
import os
import sys

import numpy as np
import pytest

import qwen2_gguf as Q

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "qwen2_tiny.npz"))


@pytest.mark.parametrize("tag", Q.TAGS)
def test_fixture_keys_and_shapes(fx, tag):
    hp = Q.tag_hp(tag)
    steps = 1 + Q.N_GEN
    assert [int(t) for t in fx[tag + "_types"]] == Q.tag_types(tag)
    assert [int(t) for t in fx[tag + "_prompt"]] == Q.prompt_tokens(hp) and len(fx[tag + "_prompt"]) == Q.N_PROMPT
    L = fx[tag + "_logits"]
    assert L.shape == (steps, hp["n_vocab"]) and L.dtype == np.float32 and np.all(np.isfinite(L))
    assert np.array_equal(fx[tag + "_tokens"], np.argmax(L, axis=1)[:Q.N_GEN])      # the reference's own greedy tokens
    for nm in ("spread", "fagap"):
        for st in ("max", "med"):
            v = fx["%s_%s_%s" % (tag, nm, st)]
            assert v.shape == (steps,) and np.all(np.isfinite(v)) and np.all(v > 0), (nm, st, v)
        assert np.all(fx["%s_%s_med" % (tag, nm)] <= fx["%s_%s_max" % (tag, nm)])


def test_fixture_types_and_widths():
    """what each tag can reach in the runtime's decode: q4k -- q|k|v all Q4_K in both layers (one fused k_gemv_rs launch
    per layer); q4km -- layer 1 keeps attn_v in Q6_K, which has no row-major layout at n_embd 1792 (1792 / 256 = 7), so
    that layer takes the unfused fallback; q4km_w -- the same types at n_embd 2048 (8 super-blocks per row), where that
    layer is the mixed Q4_K + Q6_K launch.  That the launches really agree with the unfused ops is the GPU tests' matter
    (tests/test_gpu_qwen2_model.py); this pins only the shapes they rely on."""
    import refharness as R
    a, b, w = Q.tag_types("q4km"), Q.tag_types("q4k"), Q.tag_types("q4km_w")
    assert [a[3 + 9 * 1 + j] for j in (1, 2, 3)] == [R.Q4_K, R.Q4_K, R.Q6_K] == [w[3 + 9 * 1 + j] for j in (1, 2, 3)]
    assert [a[3 + 9 * 0 + j] for j in (1, 2, 3)] == [R.Q4_K] * 3
    assert all([b[3 + 9 * il + j] for j in (1, 2, 3)] == [R.Q4_K] * 3 for il in range(2))
    assert Q.tag_hp("q4km")["n_embd"] // 256 % 8 != 0 and Q.tag_hp("q4km_w")["n_embd"] // 256 % 8 == 0
    assert Q.tag_hp("q4km_w")["n_embd"] // Q.tag_hp("q4km_w")["n_head"] == 128


def test_fixture_rope_and_kshift_cases(fx):
    hp = Q.TINY_QWEN2
    D = hp["n_embd"] // hp["n_head"]
    EKV = hp["n_head_kv"] * D
    p0, diff = (int(v) for v in fx["kshift_p0_diff"])
    n = Q.N_PROMPT + Q.N_GEN - p0 - diff
    assert fx["kshift_before"].shape == (n, EKV) == fx["kshift_after"].shape and fx["kshift_before"].dtype == np.uint16
    # the NeoX K-shift as rope_f16 states it: f32 products of the f16 pair (j, j + D/2), f16 result
    theta = (-diff) * np.float32(hp["rope_base"]) ** (-2.0 * np.arange(D // 2, dtype=np.float32) / D)
    c, s = np.cos(theta).astype(np.float32), np.sin(theta).astype(np.float32)
    k = fx["kshift_before"].view(np.float16).reshape(n, hp["n_head_kv"], D).astype(np.float32)
    x0, x1 = k[..., :D // 2], k[..., D // 2:]
    want = np.concatenate([x0 * c - x1 * s, x0 * s + x1 * c], axis=-1).astype(np.float16).astype(np.float32)
    got = fx["kshift_after"].view(np.float16).reshape(n, hp["n_head_kv"], D).astype(np.float32)
    assert np.abs(got - want).max() <= 2 * np.spacing(np.float16(np.abs(want).max())).astype(np.float32)
    for name, (T, H, HKV, Dc, pos) in Q.ROPE_CASES.items():
        assert fx[name + "_q"].shape == (T, H, Dc) and fx[name + "_k"].shape == (T, HKV, Dc)
        x = Q.rope_case_input(name)
        t0 = pos.index(0)                      # position 0 rotates by nothing
        assert np.array_equal(fx[name + "_q"][t0].reshape(-1), x[t0, :H * Dc])


def test_fixture_pinned_to_reference_build(fx):
    """one regenerated step (the prompt's logits of the q4k tag, AVX2 build, flash-attention graph) == the fixture"""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_qwen2 as M
    if not os.path.exists(M.REFLIB):
        pytest.skip("reference build (oracle/_ref) not present")
    out = M.run(M.REFLIB, "q4k", True, steps=1)
    assert np.array_equal(out["logits"][0].view(np.uint32), fx["q4k_logits"][0].view(np.uint32))
