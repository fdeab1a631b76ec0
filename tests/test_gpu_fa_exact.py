"""Strict-parity attention (csrc/attn_exact.hip, kcpp_flash_attn_exact): the reference CPU's
flash_attn_ext_f16 arithmetic order with its f16 V accumulator (ggml.c:15667-15875).

* kernel vs the reference build's own outputs (tests/golden/ops.npz fa_*, from oracle/_ref): equal up to
  the rounding of exp (the reference calls glibc expf, the kernel rounds a double exp -- both correctly
  rounded except in rare ties); measured bit-exact on these fixtures, asserted within 1 f32 ulp of the
  output scale;
* both forms of the kernel -- the runtime's (f16 q, causal window, n_past by value or from a device word) and the
  graph's (kcpp_flash_attn_ext_exact: f32 strided q, explicit mask and mask_ld) -- under the same bar on the cases
  of refharness.FA_CASES: past the EX_CH = 512 chunk loop (512, 513, 1024, 1537, 3840 keys, 701 live of 768),
  head dim 64, GQA 1 / 4 / 8, masked ranges, finite mask values, NaN in masked cells; expected values from the
  reference build (tests/golden/fa_long.npz) or from the oracle's strict restatement, which
  tests/test_fa_strict_oracle.py pins to the reference bit for bit;
* end to end, a model in this mode vs the reference golden logits: within the reference's own AVX2-vs-scalar
  build spread (tests/golden/ref_spread.npz) -- tiny models here, full width in test_gpu_fullwidth.py."""
import numpy as np
import pytest

import refharness as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    import koboldcpp_amd.lib as K
    return torch, K


@pytest.mark.parametrize("key", ["fa_1_256", "fa_5_300"])
def test_fa_exact_vs_reference_golden(env, golden_ops, key):
    torch, K = env
    q, k, v = (golden_ops[key + s] for s in ("_q", "_k", "_v"))
    T, H, D = q.shape
    n_kv, HKV, _ = k.shape
    qd = torch.from_numpy(q.astype(np.float16).view(np.int16)).cuda()
    kd = torch.from_numpy(np.ascontiguousarray(k).view(np.int16)).cuda()
    vd = torch.from_numpy(np.ascontiguousarray(v).view(np.int16)).cuda()
    out = torch.full((T, H, D), float("nan"), device="cuda")
    K.call("kcpp_flash_attn_exact", qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(), T, H, HKV, D,
           n_kv - T, None, float(np.float32(1) / np.sqrt(np.float32(D))),   # 1.0f / sqrtf(D), as ref_llama
           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got, ref = out.cpu().numpy(), golden_ops[key + "_y"]
    n_diff = int((got.view(np.uint32) != ref.view(np.uint32)).sum())
    print("%s: %d of %d outputs differ in any bit" % (key, n_diff, got.size))
    assert np.abs(got - ref).max() <= np.spacing(np.abs(ref).max())


_FA_LONG = {}


def _case(name):
    """(inputs, expected) of refharness.FA_CASES[name], made once: expected is the reference build's own output
    (tests/golden/fa_long.npz) where the case has one, else R.flash_attn_strict, which test_fa_strict_oracle.py pins
    to the reference bit for bit"""
    if name not in _FA_LONG:
        c = R.fa_case(name)
        if c.get("fixture", True):
            fx = np.load(R.ROOT + "/tests/golden/fa_long.npz")
            assert c["crc"] == int(fx[name + "_crc"])
            ref = fx[name + "_y"]
        else:
            ref = R.flash_attn_strict(c["q"], c["k"], c["v"], c["mask"])
        # NaN in every K / V cell that no query row may read
        dead = np.all(np.isneginf(c["mask"].astype(np.float32)), axis=0)
        c["k_nan"], c["v_nan"] = c["k"].copy(), c["v"].copy()
        c["k_nan"][dead] = np.nan
        c["v_nan"][dead] = np.nan
        c["n_dead"] = int(dead.sum())
        _FA_LONG[name] = (c, ref)
    return _FA_LONG[name]


def _check(tag, got, ref):
    n_diff = int((got.view(np.uint32) != ref.view(np.uint32)).sum())
    print("%s: %d of %d outputs differ in any bit, max |d| %.3g" % (tag, n_diff, got.size, np.abs(got - ref).max()))
    assert np.abs(got - ref).max() <= np.spacing(np.abs(ref).max())


def _scale(D):
    return float(np.float32(1) / np.sqrt(np.float32(D)))       # 1.0f / sqrtf(D), as ref_llama


@pytest.mark.parametrize("mask_pad", [0, 64], ids=["ld_nkv", "ld_nkv64"])
@pytest.mark.parametrize("q_layout", ["THD", "HTD"])
@pytest.mark.parametrize("name", list(R.FA_CASES))
def test_fa_exact_ext_form_long(env, name, q_layout, mask_pad):
    """the graph form (kcpp_flash_attn_ext_exact, what the ggml backend plugin dispatches) past the kernel's 512-key
    chunk: f32 q by byte strides -- [T][H][D], and [H][T][D] as the graph's permuted view -- under an explicit
    f16 mask of 32 padded rows with row stride n_kv or n_kv + 64 (the padding NaN), NaN in every masked K / V cell"""
    torch, K = env
    c, ref = _case(name)
    T, H, HKV, D, n_kv = (c[n] for n in ("T", "H", "HKV", "D", "n_kv"))
    if q_layout == "THD":
        qd, nb1, nb2 = torch.from_numpy(c["q"]).cuda(), H * D * 4, D * 4
    else:
        qd, nb1, nb2 = torch.from_numpy(np.ascontiguousarray(c["q"].transpose(1, 0, 2))).cuda(), D * 4, T * D * 4
    ld = n_kv + mask_pad
    mask = np.full((32, ld), np.nan, np.float16)
    mask[:T, :n_kv] = c["mask"]
    md = torch.from_numpy(mask.view(np.int16)).cuda()
    kd = torch.from_numpy(c["k_nan"].view(np.int16)).cuda()
    vd = torch.from_numpy(c["v_nan"].view(np.int16)).cuda()
    out = torch.full((T, H, D), float("nan"), device="cuda")
    K.call("kcpp_flash_attn_ext_exact", qd.data_ptr(), nb1, nb2, kd.data_ptr(), vd.data_ptr(), md.data_ptr(), ld,
           out.data_ptr(), T, H, HKV, D, n_kv, _scale(D), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _check("%s ext %s ld=%d (%d NaN cells)" % (name, q_layout, ld, c["n_dead"]), out.cpu().numpy(), ref)


@pytest.mark.parametrize("n_past_from", ["value", "device"])
@pytest.mark.parametrize("name", R.FA_CAUSAL_CASES)
def test_fa_exact_runtime_form_long(env, name, n_past_from):
    """the runtime's form (kcpp_flash_attn_exact: f16 q, implicit causal window) on the causal cases, n_past by value
    and read from a device word (the captured decode graph's way) with the by-value argument 0"""
    torch, K = env
    c, ref = _case(name)
    T, H, HKV, D, n_past = (c[n] for n in ("T", "H", "HKV", "D", "n_past"))
    qd = torch.from_numpy(c["q"].astype(np.float16).view(np.int16)).cuda()
    kd = torch.from_numpy(c["k_nan"].view(np.int16)).cuda()
    vd = torch.from_numpy(c["v_nan"].view(np.int16)).cuda()
    out = torch.full((T, H, D), float("nan"), device="cuda")
    npd = torch.tensor([n_past], dtype=torch.int32, device="cuda")
    by_value = n_past_from == "value"
    K.call("kcpp_flash_attn_exact", qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(), T, H, HKV, D,
           n_past if by_value else 0, None if by_value else npd.data_ptr(), _scale(D),
           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _check("%s runtime n_past by %s" % (name, n_past_from), out.cpu().numpy(), ref)


def _forced(K, hp, types, prompt, forced, exact):
    m = K.Model(hp, types)
    m.set_fa_exact(exact)
    m.synth(1234)
    out = [m.decode(prompt, 0)]
    n = len(prompt)
    for tok in forced:
        out.append(m.decode([int(tok)], n))
        n += 1
    m.close()
    return np.array(out)


@pytest.mark.parametrize("tag", ["q4km", "q8_0"])
def test_e2e_exact_within_reference_spread(env, golden_e2e, tag):
    """strict mode end to end (prefill + teacher-forced decode) vs the reference golden: per step within the
    reference's own AVX2-vs-scalar spread on the same fixture (max over steps, x1.5: the GPU sums the
    quantized dots in a third order, so its distance to the AVX2 build is a spread of the same class)"""
    torch, K = env
    sp = np.load(R.ROOT + "/tests/golden/ref_spread.npz")
    types = [int(t) for t in golden_e2e[tag + "_types"]]
    L = golden_e2e[tag + "_logits"]
    got = _forced(K, R.TINY, types, golden_e2e[tag + "_prompt"], golden_e2e[tag + "_tokens"][:-1], True)
    d = np.abs(got - L)
    print(tag, "exact-mode vs ref max", d.max(axis=1), "median", np.median(d, axis=1))
    assert np.all(d.max(axis=1) <= 1.5 * sp["tiny_%s_max" % tag].max())
    assert np.all(np.median(d, axis=1) <= 1.5 * sp["tiny_%s_median" % tag].max())


def test_exact_mode_graph_replay_equals_eager(env):
    """the strict kernel reads n_past from the device in the captured decode graph"""
    torch, K = env
    types = R.q4_k_m_types(R.TINY["n_layer"])
    prompt = list(range(3, 40))
    outs = []
    for graphs in (True, False):
        m = K.Model(R.TINY, types)
        m.set_fa_exact(True)
        m.set_graphs(graphs)
        m.synth(1234)
        lg = [m.decode(prompt, 0)]
        n = len(prompt)
        for tok in (5, 9, 200):
            lg.append(m.decode([tok], n))
            n += 1
        m.close()
        outs.append(np.array(lg))
    assert np.array_equal(outs[0], outs[1])
