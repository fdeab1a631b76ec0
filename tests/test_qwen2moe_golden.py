"""tests/golden/qwen2moe_tiny.npz (from tests/golden/make_qwen2moe.py: the reference ggml's build_qwen2moe graph) is what
the GPU tests take it for: complete, finite, greedy, built from the helper's inputs, with routing gaps that make an
exact comparison of expert ids fair and gates on both sides of one half.  Where the reference builds exist
(oracle/_ref), one regenerated prompt step of a27 equals the stored logits bit for bit."""
import os
import sys

import numpy as np
import pytest

import qwen2moe_gguf as QM
import refharness as R

HERE = os.path.dirname(os.path.abspath(__file__))
GAP = 1e-4          # ten times the bar tests/test_gpu_moe.py calls a clear routing decision


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "qwen2moe_tiny.npz"))


@pytest.mark.parametrize("tag", QM.TAGS)
def test_keys_shapes_finite(fx, tag):
    hp = QM.tag_hp(tag)
    NL, NE, k, V = hp["n_layer"], hp["n_expert"], hp["n_expert_used"], hp["n_vocab"]
    S = 1 + QM.N_GEN
    want = {"types": (3 + QM.PER_LAYER * NL,), "prompt_seed": (), "prompt": (QM.N_PROMPT,), "tokens": (QM.N_GEN,),
            "logits": (S, V), "ids_prompt": (QM.N_PROMPT, k), "probs_prompt": (QM.N_PROMPT, NE),
            "gate_prompt": (QM.N_PROMPT,), "ids": (S, NL, k), "probs": (S, NL, NE), "gate": (S, NL),
            "own_margin": (), "own_dp": (), "spread_max": (S,), "spread_med": (S,), "fagap_max": (S,), "fagap_med": (S,)}
    for name, shape in want.items():
        a = fx["%s_%s" % (tag, name)]
        assert a.shape == shape, (name, a.shape)
        assert np.isfinite(a).all(), name
    assert float(fx[tag + "_spread_max"].max()) > 0 and float(fx[tag + "_fagap_max"].max()) > 0


@pytest.mark.parametrize("tag", QM.TAGS)
def test_tokens_are_the_argmax_of_the_logits(fx, tag):
    assert np.array_equal(fx[tag + "_tokens"], np.argmax(fx[tag + "_logits"][:-1], axis=1))


@pytest.mark.parametrize("tag", QM.TAGS)
def test_helper_inputs_are_the_fixtures(fx, tag):
    hp = QM.tag_hp(tag)
    assert fx[tag + "_types"].tolist() == QM.tag_types(tag)
    assert fx[tag + "_prompt"].tolist() == QM.prompt_tokens(hp, int(fx[tag + "_prompt_seed"]))
    assert len(QM.weight_shapes(hp)) == len(QM.tag_types(tag))
    for il in range(hp["n_layer"]):
        idx = 3 + QM.PER_LAYER * il + QM.J_GATE_VEC
        g = QM.gate_vector(hp, il, QM.tag_types(tag)[idx])
        assert g.shape == (hp["n_embd"],) and np.abs(g.astype(np.float64)).max() < 1
        assert QM.synth_tensor(hp, QM.tag_types(tag)[idx], QM.SEED, idx).tobytes() == g.tobytes()
    # rows are whole blocks of their types (a27's ffn_down_exps, K = 1408, is Q5_0 / Q8_0 for that reason)
    for (k, n), t in zip(QM.weight_shapes(hp), QM.tag_types(tag)):
        assert k % R.BLOCK[t][0] == 0, (k, t)


@pytest.mark.parametrize("tag", QM.TAGS)
def test_routing_is_clear_and_ids_are_the_top_k(fx, tag):
    k = QM.tag_hp(tag)["n_expert_used"]
    for probs, ids in ((fx[tag + "_probs_prompt"], fx[tag + "_ids_prompt"]), (fx[tag + "_probs"], fx[tag + "_ids"])):
        p = probs.reshape(-1, probs.shape[-1]).astype(np.float64)
        i = ids.reshape(-1, k)
        s = np.sort(p, axis=1)[:, ::-1][:, :k + 1]
        assert (s[:, :-1] - s[:, 1:]).min() >= GAP
        assert np.array_equal(np.argsort(-p, axis=1, kind="stable")[:, :k], i)
        np.testing.assert_allclose(p.sum(1), 1.0, atol=1e-5)


@pytest.mark.parametrize("tag", QM.TAGS)
def test_gates_span_both_sides_of_one_half(fx, tag):
    g = np.concatenate([fx[tag + "_gate_prompt"].ravel(), fx[tag + "_gate"].ravel()])
    assert g.min() < 0.35 and g.max() > 0.65, (g.min(), g.max())
    assert g.min() > 0 and g.max() < 1


def test_fixture_is_small(fx):
    assert os.path.getsize(os.path.join(HERE, "golden", "qwen2moe_tiny.npz")) < 256 * 1024


def test_regenerated_prompt_step_equals_the_fixture(fx):
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_qwen2 as MQ
    if not os.path.exists(MQ.REFLIB):
        pytest.skip("oracle/_ref not built (no reference sources on this machine)")
    import make_qwen2moe as MM
    a = MM.run(MQ.REFLIB, "a27", True, steps=1, pseed=int(fx["a27_prompt_seed"]))
    assert np.array_equal(a["logits"][0].view(np.uint32), fx["a27_logits"][0].view(np.uint32))
    assert np.array_equal(a["ids_prompt"], fx["a27_ids_prompt"])
