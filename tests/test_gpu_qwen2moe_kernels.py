"""The two device pieces build_qwen2moe (src/llama.cpp:12248-12392) adds to the MoE FFN:

* the router's options (kcpp_moe_route_ex / kcpp_moe_route_norm_ex): top-k softmax probabilities taken as they are
  (llm_build_moe_ffn with norm_w = false) and the shared expert's gate row dotted in the same launch,
  gate = silu(z) / z -- against a numpy restatement (test_gpu_moe._route_ref's arithmetic without the division);
  with both options off the bits are kcpp_moe_route's; the _norm_ex form is kcpp_rms_norm + _ex bit for bit;
* k_moe_combine_shexp: x = (((s0 + s1) + ...) + gate * sh) + x, bit-equal to numpy f32 in that order."""
import numpy as np
import pytest

import refharness as R

pytestmark = pytest.mark.gpu

E, T = 512, 37
CASES = [(60, 4), (64, 8), (12, 4), (8, 2)]


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    import koboldcpp_amd.lib as K
    return torch, K


def _inputs(NE, k, wtype, gtype=None):
    gtype = wtype if gtype is None else gtype
    rng = np.random.default_rng(NE * 10 + k)
    x = rng.standard_normal((T, E)).astype(np.float32)
    w = (0.05 * rng.standard_normal((NE, E))).astype(np.float16 if wtype == R.F16 else np.float32)
    g = (0.05 * rng.standard_normal(E)).astype(np.float16 if gtype == R.F16 else np.float32)
    return x, w, g


def _act(x, wtype):
    return (x.astype(np.float16) if wtype == R.F16 else x).astype(np.float64)


def route_raw_ref(x, w, wtype, k):
    """test_gpu_moe._route_ref without the division: ids in top-k order, the selected probabilities, and whether every
    adjacent gap among the first k+1 sorted probabilities exceeds 1e-5 (near-ties may swap under fp32 sum order)"""
    lg = (_act(x, wtype) @ w.astype(np.float64).T).astype(np.float32)
    ids, wts, clear = [], [], []
    for p in lg:
        e = np.exp((p - p.max()).astype(np.float32)).astype(np.float32)
        pr = (e * np.float32(1.0 / e.astype(np.float64).sum())).astype(np.float32)
        sel = sorted(range(len(pr)), key=lambda i: (-pr[i], i))[:k]
        srt = np.sort(pr)[::-1][:k + 1].astype(np.float64)
        clear.append(bool((srt[:-1] - srt[1:] > 1e-5).all()))
        ids.append(sel)
        wts.append(pr[sel])
    return np.array(ids), np.array(wts, np.float32), np.array(clear)


def gate_ref(x, g, gtype):
    z = (_act(x, gtype) @ g.astype(np.float64)).astype(np.float32).astype(np.float64)
    return 1.0 / (1.0 + np.exp(-z))


def _dev(torch, a):
    return torch.from_numpy(a.view(np.uint8).copy()).cuda()


def _route_ex(env, x, w, wtype, k, moe_norm_w, g=None, gtype=0):
    torch, K = env
    NE = w.shape[0]
    xd, wd = torch.from_numpy(x).cuda(), _dev(torch, w)
    gd = _dev(torch, g) if g is not None else None
    ids = torch.full((T, k), -1, dtype=torch.int32, device="cuda")
    wts = torch.zeros((T, k), device="cuda")
    gate = torch.full((T,), float("nan"), device="cuda")
    K.call("kcpp_moe_route_ex", xd.data_ptr(), E, wd.data_ptr(), wtype, E, NE, k, moe_norm_w,
           gd.data_ptr() if gd is not None else None, gtype, ids.data_ptr(), wts.data_ptr(), gate.data_ptr(), T,
           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), wts.cpu().numpy(), gate.cpu().numpy()


@pytest.mark.parametrize("wtype", [R.F16, R.F32], ids=["f16", "f32"])
@pytest.mark.parametrize("NE,k", CASES)
def test_route_raw_weights_and_gate_vs_restatement(env, wtype, NE, k):
    x, w, g = _inputs(NE, k, wtype)
    gid, gw, gg = _route_ex(env, x, w, wtype, k, 0, g, wtype)
    rid, rw, clear = route_raw_ref(x, w, wtype, k)
    want_g = gate_ref(x, g, wtype)
    print("NE %d k %d wtype %d: clear %d/%d, max|dw| %.3g, gate %.3f..%.3f, max|dgate| %.3g" % (
        NE, k, wtype, clear.sum(), T, np.abs(gw[clear] - rw[clear]).max(), gg.min(), gg.max(), np.abs(gg - want_g).max()))
    assert clear.sum() >= 36
    np.testing.assert_array_equal(gid[clear], rid[clear])
    np.testing.assert_allclose(gw[clear], rw[clear], rtol=2e-5, atol=1e-6)
    assert (gw.sum(1) < 1.0).all()                       # raw probabilities: NE > k, never the normalised sum
    np.testing.assert_allclose(gg, want_g, rtol=2e-5, atol=1e-6)
    assert want_g.min() < 0.35 and want_g.max() > 0.65   # a saturated gate would hide a wrong one


@pytest.mark.parametrize("NE,k", [(12, 4), (8, 2)])
def test_route_gate_row_of_the_other_type(env, NE, k):
    """F16 router rows with an F32 gate row (the activation rounded for the router only), and the reverse"""
    for wtype, gtype in ((R.F16, R.F32), (R.F32, R.F16)):
        x, w, g = _inputs(NE, k, wtype, gtype)
        gid, gw, gg = _route_ex(env, x, w, wtype, k, 0, g, gtype)
        rid, rw, clear = route_raw_ref(x, w, wtype, k)
        assert clear.sum() >= 36
        np.testing.assert_array_equal(gid[clear], rid[clear])
        np.testing.assert_allclose(gw[clear], rw[clear], rtol=2e-5, atol=1e-6)
        np.testing.assert_allclose(gg, gate_ref(x, g, gtype), rtol=2e-5, atol=1e-6)


@pytest.mark.parametrize("wtype", [R.F16, R.F32], ids=["f16", "f32"])
@pytest.mark.parametrize("NE,k", CASES)
def test_route_ex_options_off_is_moe_route(env, wtype, NE, k):
    torch, K = env
    x, w, g = _inputs(NE, k, wtype)
    xd, wd = torch.from_numpy(x).cuda(), _dev(torch, w)
    ids = torch.full((T, k), -1, dtype=torch.int32, device="cuda")
    wts = torch.zeros((T, k), device="cuda")
    K.call("kcpp_moe_route", xd.data_ptr(), E, wd.data_ptr(), wtype, E, NE, k, ids.data_ptr(), wts.data_ptr(), T,
           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    gid, gw, _ = _route_ex(env, x, w, wtype, k, 1)
    assert np.array_equal(gid, ids.cpu().numpy())
    assert np.array_equal(gw.view(np.uint32), wts.cpu().numpy().view(np.uint32))
    # the gate changes neither: same ids, and the raw weights are the normalised ones times their sum
    gid2, gw2, _ = _route_ex(env, x, w, wtype, k, 1, g, wtype)
    assert np.array_equal(gid2, gid) and np.array_equal(gw2.view(np.uint32), gw.view(np.uint32))
    gid3, gw3, _ = _route_ex(env, x, w, wtype, k, 0)
    assert np.array_equal(gid3, gid)
    np.testing.assert_allclose(gw3 / gw3.astype(np.float64).sum(1, keepdims=True), gw, rtol=1e-6)


@pytest.mark.parametrize("wtype,gtype", [(R.F16, R.F16), (R.F32, R.F32), (R.F16, R.F32)], ids=["f16", "f32", "f16_f32"])
@pytest.mark.parametrize("Ek", [4096, 2048, 768])        # kcpp_rms_norm takes multiples of 256
def test_route_norm_ex_is_norm_then_route_ex(env, wtype, gtype, Ek):
    """ffn_norm folded into the router launch (NE <= 8, K <= 4096) == kcpp_rms_norm then kcpp_moe_route_ex, bit for bit"""
    torch, K = env
    NE, k, Tn = 8, 2, 5
    s = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(Ek)
    x = rng.standard_normal((Tn, Ek)).astype(np.float32)
    nw = (1 + 0.1 * rng.standard_normal(Ek)).astype(np.float32)
    w = (0.05 * rng.standard_normal((NE, Ek))).astype(np.float16 if wtype == R.F16 else np.float32)
    g = (0.05 * rng.standard_normal(Ek)).astype(np.float16 if gtype == R.F16 else np.float32)
    xd, nd, wd, gd = torch.from_numpy(x).cuda(), torch.from_numpy(nw).cuda(), _dev(torch, w), _dev(torch, g)
    xn = torch.zeros((Tn, Ek), device="cuda")
    out = []
    for fused in (True, False):
        ids = torch.full((Tn, k), -1, dtype=torch.int32, device="cuda")
        wts = torch.zeros((Tn, k), device="cuda")
        gate = torch.full((Tn,), float("nan"), device="cuda")
        if fused:
            K.call("kcpp_moe_route_norm_ex", xd.data_ptr(), Ek, nd.data_ptr(), 1e-5, wd.data_ptr(), wtype, Ek, NE, k, 0,
                   gd.data_ptr(), gtype, ids.data_ptr(), wts.data_ptr(), gate.data_ptr(), Tn, s)
        else:
            K.call("kcpp_rms_norm", xd.data_ptr(), Ek, nd.data_ptr(), xn.data_ptr(), Ek, None, Ek, Tn, 1e-5, s)
            K.call("kcpp_moe_route_ex", xn.data_ptr(), Ek, wd.data_ptr(), wtype, Ek, NE, k, 0, gd.data_ptr(), gtype,
                   ids.data_ptr(), wts.data_ptr(), gate.data_ptr(), Tn, s)
        torch.cuda.synchronize()
        out.append((ids.cpu().numpy(), wts.cpu().numpy(), gate.cpu().numpy()))
    assert np.array_equal(out[0][0], out[1][0])
    assert np.array_equal(out[0][1].view(np.uint32), out[1][1].view(np.uint32))
    assert np.array_equal(out[0][2].view(np.uint32), out[1][2].view(np.uint32))
    assert np.isfinite(out[0][2]).all() and (out[0][1].sum(1) < 1.0).all()


def test_route_ex_rejects_what_it_does_not_cover(env):
    torch, K = env
    raw = K.raw()
    assert raw.kcpp_moe_route_ex(None, 512, None, R.F16, 512, 65, 2, 0, None, 0, None, None, None, 1, None) != 0
    assert raw.kcpp_moe_route_ex(None, 512, None, R.F16, 512, 8, 9, 0, None, 0, None, None, None, 1, None) != 0
    buf = torch.zeros(512, device="cuda")
    p = buf.data_ptr()
    # a gate row that is neither F32 nor F16, and a gate row without an output
    assert raw.kcpp_moe_route_ex(p, 512, p, R.F32, 512, 8, 2, 0, p, R.Q8_0, p, p, p, 1, None) == -3
    assert raw.kcpp_moe_route_ex(p, 512, p, R.F32, 512, 8, 2, 0, p, R.F32, p, p, None, 1, None) != 0
    # the folded norm keeps kcpp_moe_route_norm's limits
    assert raw.kcpp_moe_route_norm_ex(p, 8192, p, 1e-5, p, R.F32, 8192, 8, 2, 0, None, 0, p, p, None, 1, None) == -3
    assert raw.kcpp_moe_route_norm_ex(p, 512, p, 1e-5, p, R.F32, 512, 12, 4, 0, None, 0, p, p, None, 1, None) == -3
    torch.cuda.synchronize()


@pytest.mark.parametrize("Tn", [1, 37])
@pytest.mark.parametrize("k", [2, 8])
def test_combine_shexp_order(env, Tn, k):
    torch, K = env
    Ee = 1024
    rng = np.random.default_rng(100 * Tn + k)
    x = rng.standard_normal((Tn, Ee)).astype(np.float32)
    slots = rng.standard_normal((k, Tn, Ee)).astype(np.float32)
    sh = rng.standard_normal((Tn, Ee)).astype(np.float32)
    gate = rng.random(Tn).astype(np.float32)
    xd, sd = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(slots).cuda()
    hd, gd = torch.from_numpy(sh).cuda(), torch.from_numpy(gate).cuda()
    K.call("kcpp_moe_combine_shexp", xd.data_ptr(), sd.data_ptr(), Tn * Ee, k, gd.data_ptr(), hd.data_ptr(), Ee, Tn,
           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    acc = slots[0].copy()
    for j in range(1, k):
        acc = acc + slots[j]
    want = (acc + gate[:, None] * sh) + x
    assert want.dtype == np.float32
    assert np.array_equal(xd.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_combine_shexp_rejects_unaligned_rows(env):
    torch, K = env
    assert K.raw().kcpp_moe_combine_shexp(None, None, 1022, 2, None, None, 1022, 1, None) != 0
