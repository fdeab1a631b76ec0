"""The MFMA prefill attention (attn_mfma.hip k_fa_prefill_mfma3 + k_fa_split_merge) at every GQA ratio 1..8, D = 128.

A workgroup has four slots of (one head, 16 queries): 4, 2 or 1 heads x 1, 2 or 4 consecutive 16-query blocks by ratio
(csrc/fa_plan.h).  So beside the planted-key conditions of test_gpu_attn_reach.py (whose cases, reference, metric and
2e-3 bar this file imports) the inputs must tell slots apart: `_exchange`, asserted on the float64 reference alone before
any GPU result is read, requires the reference with any two heads exchanged, or any two complete 16-query blocks of one
head exchanged, to be >= 10 bars from itself on its worst row -- a kernel that hands a slot the wrong head or query block
cannot pass.  Plain Gaussian inputs meet it at every shape here (least 1.28 over all of them).  Planted inputs do
not: their needles carry most of every row's mass, so rows of one kv head resemble each other -- exchanging two
heads moves the planted references by 0.036 at the least at (70, 0), (70, 130) and (65, 4090) but by 0.013 at (33, 0),
and exchanging two query blocks of a head by 0.011 to 0.041, on both sides of the 0.02 required.  So every shape runs
with both kinds of input: the planted case carries `_conditions` (no stretch of the context dropped), its Gaussian
twin `_exchange` (no slot confused), each against float64 at the same bar; the planted figure is printed.

Shapes: H = 2 G over 2 kv heads unless stated; T = 70 has a second 64-query group of 6 rows, 65 one of 1 row, 17 one
block of 16 + 1 row (slots wholly past T), n_past 4090 crosses 4096 and 32760 crosses 32768; (64, 200) gives the early
query blocks of a workgroup a whole key split with no visible key."""
import numpy as np
import pytest

import qwen2_gguf as Q
from test_gpu_attn_reach import BAR_MFMA, PAD_ROWS, _check, _conditions, case, ref64, regions
from test_gpu_kernels import dev, host, sptr
from test_gpu_model import TOL_MAX

pytestmark = pytest.mark.gpu
D = 128
SCALE = float(1.0 / np.sqrt(D))
RATIOS = list(range(1, 9))


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import koboldcpp_amd.lib as K
    return torch, K


_GAUSS = {}


def gauss(H, HKV, T, n_past):
    """plain Gaussian q, K, V in f16 and their float64 attention, made once and left unchanged"""
    key = (H, HKV, T, n_past)
    if key not in _GAUSS:
        rng = np.random.default_rng(7919 * n_past + 131 * T + 17 * H + HKV)
        n_keys = n_past + T
        q = rng.standard_normal((T, H, D)).astype(np.float16)
        k = rng.standard_normal((n_keys + PAD_ROWS, HKV, D)).astype(np.float16)
        v = rng.standard_normal((n_keys + PAD_ROWS, HKV, D)).astype(np.float16)
        v[n_keys:] = 100                                  # rows no query may see: fatal if attended
        ref, _, _ = ref64(q, k[:n_keys], v[:n_keys], n_past, regions(n_past + 1))
        _GAUSS[key] = dict(q=q, k=k, v=v, ref=ref, n_keys=n_keys, e_orc=float("nan"))
    return _GAUSS[key]


def _exchange(c, bar=BAR_MFMA):
    """on the reference alone: exchanging two heads, or two complete 16-query blocks of a head, moves it >= 10 bars"""
    c["exchange"] = _exchange_least(c)
    assert c["exchange"] >= 10 * bar, ("two heads or two query blocks exchanged stay within 10 bars", c["exchange"])


def _exchange_least(c):
    """the least worst-row distance of the reference from itself over every such exchange"""
    if "exchange" not in c:
        ref = c["ref"]
        T, H, _ = ref.shape
        amax = np.abs(ref).max(axis=-1)                   # [T][H]
        least = np.inf
        for i in range(H - 1):                            # heads i <-> j: rows of both heads change
            d = np.abs(ref[:, i + 1:] - ref[:, i:i + 1]).max(axis=-1)
            e = np.maximum(d / amax[:, i + 1:], d / amax[:, i:i + 1]).max(axis=0)
            least = min(least, e.min())
        nb = T // 16
        for a in range(nb - 1):                           # blocks a <-> b of one head
            for b in range(a + 1, nb):
                ra, rb = slice(16 * a, 16 * a + 16), slice(16 * b, 16 * b + 16)
                d = np.abs(ref[ra] - ref[rb]).max(axis=-1)
                e = np.maximum(d / amax[ra], d / amax[rb]).max(axis=0)
                least = min(least, e.min())
        c["exchange"] = float(least)
    return c["exchange"]


def _inputs(kind, H, HKV, T, n_past):
    """the case and its input condition, on the reference alone"""
    if kind == "planted":
        c = case(D, H, HKV, T, n_past)
        _conditions(c, BAR_MFMA)
        print("planted T %d n_past %d H %d: least exchange distance %.3g" % (T, n_past, H, _exchange_least(c)))
    else:
        c = gauss(H, HKV, T, n_past)
        _exchange(c)
    return c


def _unsplit(torch, K, c, T, H, HKV, n_past):
    q16, kd, vd = dev(torch, c["q"]), dev(torch, c["k"]), dev(torch, c["v"])
    out = torch.full((T, H, D), float("nan"), dtype=torch.float32, device="cuda")
    rc = K.raw().kcpp_flash_attn_prefill_mfma(q16.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(), T, H, HKV, D,
                                              n_past, SCALE, sptr(torch))
    assert rc == 0, ("kcpp_flash_attn_prefill_mfma refused a GQA ratio", rc, H, HKV)
    return host(torch, out, np.float32).reshape(T, H, D)


def _ta_of(torch, K, out, E, T):
    """kcpp_quantize_act(KT_Q8_0_TA) of the host array out [T][E]"""
    qr = torch.zeros(K.act_bytes(K.Q8_0_T, E, T), dtype=torch.uint8, device="cuda")
    od = dev(torch, np.ascontiguousarray(out, np.float32).reshape(T, E))
    K.call("kcpp_quantize_act", K.Q8_0_TA, od.data_ptr(), E, qr.data_ptr(), E, T, sptr(torch))
    return host(torch, qr, np.uint8)


# ---------------------------------------------------------------- 1, 2: unsplit against float64
@pytest.mark.parametrize("G", RATIOS)
@pytest.mark.parametrize("kind", ["planted", "gauss"])
@pytest.mark.parametrize("T,n_past", [(70, 0), (70, 130), (65, 4090)])
def test_unsplit_vs_float64(env, G, T, n_past, kind):
    """kcpp_flash_attn_prefill_mfma (k_fa_prefill_mfma3<8, false, false, G>) at the MFMA bar"""
    torch, K = env
    H, HKV = 2 * G, 2
    c = _inputs(kind, H, HKV, T, n_past)
    _check(c, _unsplit(torch, K, c, T, H, HKV, n_past), "k_fa_prefill_mfma3", "%s T %d G %d" % (kind, T, G), BAR_MFMA)


# ---------------------------------------------------------------- 3: key-split + merge, the TA output
@pytest.mark.parametrize("G", [g for g in RATIOS if g != 4])
@pytest.mark.parametrize("kind", ["planted", "gauss"])
@pytest.mark.parametrize("T,n_past", [(17, 4090), (64, 200), (33, 0)])
def test_key_split(env, G, T, n_past, kind):
    """kcpp_flash_attn_prefill_mfma_ex with a workspace (k_fa_prefill_mfma3<8, true, false, G> + k_fa_split_merge<G>;
    (33, 0) has one key tile and stays unsplit) writing out and the KT_Q8_0_TA activation"""
    torch, K = env
    H, HKV = 2 * G, 2
    E = H * D
    c = _inputs(kind, H, HKV, T, n_past)
    q16, kd, vd = dev(torch, c["q"]), dev(torch, c["k"]), dev(torch, c["v"])
    ws = torch.zeros(K.fa_workspace_bytes(16, H, c["n_keys"]), dtype=torch.uint8, device="cuda")
    assert ws.numel() >= K.raw().kcpp_fa_split_ws_bytes(H)
    outs, qtas = [], []
    for _ in range(2):
        out = torch.full((T, H, D), float("nan"), dtype=torch.float32, device="cuda")
        qta = torch.zeros(K.act_bytes(K.Q8_0_T, E, T), dtype=torch.uint8, device="cuda")
        rc = K.raw().kcpp_flash_attn_prefill_mfma_ex(q16.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(),
                                                     qta.data_ptr(), ws.data_ptr(), T, H, HKV, D, n_past, SCALE, sptr(torch))
        assert rc == 0, rc
        outs.append(host(torch, out, np.float32).reshape(T, H, D))
        qtas.append(host(torch, qta, np.uint8))
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), "two runs on one workspace differ"
    assert np.array_equal(qtas[0], qtas[1])
    assert not ws[:2048].any().item(), "the workspace header was written"
    _check(c, outs[0], "k_fa_prefill_mfma3 split", "%s T %d G %d" % (kind, T, G), BAR_MFMA)
    un = _unsplit(torch, K, c, T, H, HKV, n_past)
    err = np.abs(outs[0] - un).max()
    print("T %d n_past %d G %d: split vs unsplit max |d| %.3g (max |ref| %.3g)" % (T, n_past, G, err, np.abs(c["ref"]).max()))
    assert err <= 2e-3 * np.abs(c["ref"]).max() + 1e-5
    assert np.array_equal(qtas[0], _ta_of(torch, K, outs[0], E, T)), "TA bytes != kcpp_quantize_act of the same output"


@pytest.mark.parametrize("G", [g for g in RATIOS if g != 4])
def test_unsplit_ta_epilogue(env, G):
    """T = 80 (no split), out = NULL: the TA epilogue alone equals kcpp_quantize_act of the plain launch's output"""
    torch, K = env
    H, HKV, T, n_past = 2 * G, 2, 80, 500
    E = H * D
    c = gauss(H, HKV, T, n_past)
    _exchange(c)
    un = _unsplit(torch, K, c, T, H, HKV, n_past)
    _check(c, un, "k_fa_prefill_mfma3", "gauss T %d G %d" % (T, G), BAR_MFMA)
    q16, kd, vd = dev(torch, c["q"]), dev(torch, c["k"]), dev(torch, c["v"])
    ws = torch.zeros(K.fa_workspace_bytes(16, H, c["n_keys"]), dtype=torch.uint8, device="cuda")
    qta = torch.zeros(K.act_bytes(K.Q8_0_T, E, T), dtype=torch.uint8, device="cuda")
    rc = K.raw().kcpp_flash_attn_prefill_mfma_ex(q16.data_ptr(), kd.data_ptr(), vd.data_ptr(), None, qta.data_ptr(),
                                                 ws.data_ptr(), T, H, HKV, D, n_past, SCALE, sptr(torch))
    assert rc == 0, rc
    assert np.array_equal(host(torch, qta, np.uint8), _ta_of(torch, K, un, E, T))


# ---------------------------------------------------------------- 4: past 32768 keys
@pytest.mark.parametrize("H,T,split", [(14, 65, False), (14, 64, True), (16, 65, False)])
def test_reach(env, H, T, split):
    """G = 7 and 8 at n_past = 32760, planted keys in all four regions of the context (the conditions alone: these
    shapes' slots are told apart at 4090 keys above).  On the reference: least region mass 0.0142, 0.0191 and 0.0120 of
    a row, a masked region moves it by 0.85, 0.62 and 0.67 at the least -- clear of the 1 % and 10-bar lines of
    `_conditions` (H = 2 at this depth sits at 0.010 and is not used)"""
    torch, K = env
    HKV, n_past = 2, 32760
    c = case(D, H, HKV, T, n_past)
    _conditions(c, BAR_MFMA)
    if split:
        q16, kd, vd = dev(torch, c["q"]), dev(torch, c["k"]), dev(torch, c["v"])
        ws = torch.zeros(K.fa_workspace_bytes(16, H, c["n_keys"]), dtype=torch.uint8, device="cuda")
        out = torch.full((T, H, D), float("nan"), dtype=torch.float32, device="cuda")
        rc = K.raw().kcpp_flash_attn_prefill_mfma_ex(q16.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(), None,
                                                     ws.data_ptr(), T, H, HKV, D, n_past, SCALE, sptr(torch))
        assert rc == 0, rc
        got = host(torch, out, np.float32)
    else:
        got = _unsplit(torch, K, c, T, H, HKV, n_past)
    _check(c, got, "k_fa_prefill_mfma3 split" if split else "k_fa_prefill_mfma3", "T %d G %d" % (T, H // HKV), BAR_MFMA)


# ---------------------------------------------------------------- 5: head layouts of real models
@pytest.mark.parametrize("H,HKV", [(28, 4), (40, 8), (56, 8), (64, 8), (8, 8)])
def test_model_head_layouts(env, H, HKV):
    """Qwen2.5-7B (28 / 4: kv heads not a multiple of 8), Qwen2.5-14B, G = 7 over 8, Llama-3-70B, G = 1 over 8: both
    branches of the workgroup order"""
    torch, K = env
    T, n_past = 70, 130
    c = gauss(H, HKV, T, n_past)
    _exchange(c)
    _check(c, _unsplit(torch, K, c, T, H, HKV, n_past), "k_fa_prefill_mfma3", "gauss H %d HKV %d" % (H, HKV), BAR_MFMA)


# ---------------------------------------------------------------- 6: dispatch
@pytest.mark.parametrize("G", RATIOS)
def test_dispatch(env, G):
    """kcpp_flash_attn: force_path 3 is the direct entry; the auto path runs the MFMA kernel where the plan's table has
    the ratio on and k_fa_prefill<128> (force_path 2) where it has it off -- bit for bit"""
    torch, K = env
    H, HKV, T, n_past = 2 * G, 2, 70, 130
    c = gauss(H, HKV, T, n_past)
    _exchange(c)
    q16, kd, vd = dev(torch, c["q"]), dev(torch, c["k"]), dev(torch, c["v"])
    ws = torch.zeros(K.fa_workspace_bytes(16, H, 64), dtype=torch.uint8, device="cuda")

    def run(path):
        out = torch.full((T, H, D), float("nan"), dtype=torch.float32, device="cuda")
        rc = K.raw().kcpp_flash_attn(q16.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(), None, ws.data_ptr(), T,
                                     H, HKV, D, n_past, None, c["n_keys"] + PAD_ROWS, SCALE, path, sptr(torch))
        assert rc == 0, (rc, path)
        return host(torch, out, np.float32).reshape(T, H, D).view(np.uint32)

    direct = _unsplit(torch, K, c, T, H, HKV, n_past).view(np.uint32)
    forced = run(3)
    assert np.array_equal(forced, direct)
    on = K.fa_prefill_plan(T, H, HKV, D, n_past)["kernel"] != "fma"
    print("G %d: the auto path takes %s" % (G, "the MFMA kernel" if on else "k_fa_prefill<128>"))
    assert np.array_equal(run(0), forced if on else run(2))


# ---------------------------------------------------------------- 7: the model
def _logits(K, types, prompt, ub):
    hp = Q.TINY_QWEN2
    m = K.Model(hp, types, max_ubatch=ub)
    m.synth(Q.SEED)
    m.set_rope_mode(2)
    for il in range(hp["n_layer"]):
        m.set_qkv_bias(il, *Q.qkv_bias(hp, il))
    lg = np.array(m.decode(prompt, 0))
    m.close()
    return lg


@pytest.mark.parametrize("tag", ["q8_0", "q4k"])
def test_qwen2_prompt_in_ubatches(env, tag):
    """TINY_QWEN2 (G = 7), 150-token prompt: ubatch 512 (one unsplit launch per layer) and ubatch 48 (q8_0: the model's
    Q8_0-tile branch, keys split from the second ubatch on) against ubatch 8 (the f32 chunk kernels), at the bar the
    same comparison has for Llama"""
    torch, K = env
    types = Q.tag_types(tag)
    prompt = [int(t) for t in np.random.default_rng(150).integers(1, Q.TINY_QWEN2["n_vocab"], 150)]
    base = _logits(K, types, prompt, 8)
    for ub in (512, 48):
        d = np.abs(_logits(K, types, prompt, ub) - base)
        print("qwen2 %s ubatch %d vs 8: max %.3g median %.3g (bar %.3g)" % (tag, ub, d.max(), np.median(d), TOL_MAX))
        assert d.max() <= TOL_MAX, (ub, d.max())
