"""The kernels of the Command-R graph (LayerNorm, its prologue in the fused decode mat-vecs, the logit scale).

* kcpp_layer_norm == the reference's ggml_norm + ggml_mul rows (tests/golden/commandr_tiny.npz ln_*: widths 2048, 1792,
  8192, row means up to 3 x the std), bit for bit; its Q8_K output and kcpp_layer_norm_q80's Q8_0 output == the norm
  followed by kcpp_quantize_act, byte for byte;
* the fused PRO 3 launches (gemv_rs.hip: mode 2 q|k|v, mode 1 the 8-wave gate|up, mode 0 the head, the mixed Q4_K + Q6_K
  q|k + v launch) == the unfused path on the same weights (kcpp_layer_norm -> Q8_K, PRO 0 of the same kernel, for q|k|v
  then kcpp_rope_kv_ex), bit for bit, for each row-major type at K 2048 (one prologue chunk) and K 8192 (two: the
  smallest shape at which the two-chunk reductions can go wrong), on an input row whose mean is 3 x its std;
* kcpp_scale is one f32 multiply per element, and a model's head with set_logit_scale(s) writes the unscaled head's
  logits times s, bit for bit, with the device argmax reading the scaled values."""
import ctypes
import os

import numpy as np
import pytest

import commandr_gguf as C
from test_gpu_kernels import dev, host, sptr
from test_gpu_qwen2_kernels import rope_table

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LN_CASES = ("ln2048", "ln1792", "ln8192")
EPS = 1e-5


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    import koboldcpp_amd.lib as K
    return torch, K


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "commandr_tiny.npz"))


@pytest.mark.parametrize("name", LN_CASES)
def test_layer_norm_vs_reference(env, fx, name):
    torch, K = env
    sp = sptr(torch)
    x, w, want = fx[name + "_x"], fx[name + "_w"], fx[name + "_y"]
    rows, E = x.shape
    xd, wd = dev(torch, x), dev(torch, w)
    y = torch.zeros(rows * E, dtype=torch.float32, device="cuda")
    nk, n0 = K.act_bytes(K.Q4_K, E, rows), K.act_bytes(K.Q8_0, E, rows)
    q8k, q8k_ref = (torch.zeros(nk, dtype=torch.uint8, device="cuda") for _ in range(2))
    q80, q80_ref = (torch.zeros(n0, dtype=torch.uint8, device="cuda") for _ in range(2))
    K.call("kcpp_layer_norm", xd.data_ptr(), E, wd.data_ptr(), y.data_ptr(), E, q8k.data_ptr(), E, rows, EPS, sp)
    got = host(torch, y, np.float32).reshape(rows, E)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), int((got != want).sum())
    # not the RMS norm: the rows' means are far from zero
    rms = torch.zeros(rows * E, dtype=torch.float32, device="cuda")
    K.call("kcpp_rms_norm", xd.data_ptr(), E, wd.data_ptr(), rms.data_ptr(), E, None, E, rows, EPS, sp)
    assert np.abs(host(torch, rms, np.float32).reshape(rows, E) - want).max() > 0.5
    # the quantizing epilogues == norm, then kcpp_quantize_act
    K.call("kcpp_quantize_act", K.Q8_K, y.data_ptr(), E, q8k_ref.data_ptr(), E, rows, sp)
    assert np.array_equal(host(torch, q8k, np.uint8), host(torch, q8k_ref, np.uint8))
    K.call("kcpp_layer_norm_q80", xd.data_ptr(), E, wd.data_ptr(), q80.data_ptr(), E, rows, EPS, 0, sp)
    K.call("kcpp_quantize_act", K.Q8_0, y.data_ptr(), E, q80_ref.data_ptr(), E, rows, sp)
    assert np.array_equal(host(torch, q80, np.uint8), host(torch, q80_ref, np.uint8))
    # the quantized output alone (no f32 row), as the runtime calls it
    q8k2 = torch.zeros(nk, dtype=torch.uint8, device="cuda")
    K.call("kcpp_layer_norm", xd.data_ptr(), E, wd.data_ptr(), None, E, q8k2.data_ptr(), E, rows, EPS, sp)
    assert np.array_equal(host(torch, q8k2, np.uint8), host(torch, q8k_ref, np.uint8))


def test_layer_norm_refuses_bad_widths(env):
    torch, K = env
    d = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
    for E in (2000, 16640):
        assert K.raw().kcpp_layer_norm(d.data_ptr(), E, d.data_ptr(), d.data_ptr(), E, None, E, 1, ctypes.c_float(EPS),
                                       ctypes.c_void_p(sptr(torch))) == -1


def _inputs(torch, K, tys, ns, E, seed):
    """weights of the given row-major types, an input row with mean 3 x std, a norm weight near 1"""
    sp = sptr(torch)
    ws = []
    for i, (ty, n) in enumerate(zip(tys, ns)):
        w = torch.empty(K.row_bytes(ty, E) * n, dtype=torch.uint8, device="cuda")
        K.call("kcpp_weight_synth", ty, 23, seed + i + 1, w.data_ptr(), E, n, sp)
        ws.append(w)
    rng = np.random.default_rng(seed + E)
    x = dev(torch, (3.0 + rng.standard_normal(E)).astype(np.float32))
    nw = dev(torch, (1.0 + 0.1 * rng.standard_normal(E)).astype(np.float32))
    act = torch.zeros(K.act_bytes(K.Q4_K, E, 1), dtype=torch.uint8, device="cuda")
    K.call("kcpp_layer_norm", x.data_ptr(), E, nw.data_ptr(), None, E, act.data_ptr(), E, 1, EPS, sp)
    return ws, x, nw, act


def _qkv_fused_vs_unfused(torch, K, E, qtype, vtype, H=2, HKV=1, D=128, pos=5):
    NQ, EKV = H * D, HKV * D
    LQ, n_ctx = NQ + 2 * EKV, pos + 3
    sp = sptr(torch)
    tys, ns = [qtype, qtype, vtype], [NQ, EKV, EKV]
    ws, x, nw, act = _inputs(torch, K, tys, ns, E, 100)
    rt = dev(torch, rope_table(K, n_ctx, D, base=8000000.0))
    posd = dev(torch, np.array([pos], np.int32))

    def bufs():
        return (torch.zeros(NQ, dtype=torch.int16, device="cuda"), torch.zeros(n_ctx * EKV, dtype=torch.int16, device="cuda"),
                torch.zeros(n_ctx * EKV, dtype=torch.int16, device="cuda"))
    q16, kc, vc = bufs()
    a = K.DecArgs()
    a.K, a.x, a.nw, a.eps = E, x.data_ptr(), nw.data_ptr(), EPS
    a.q16, a.kc, a.vc, a.ekv, a.D, a.pos, a.rope_tab = q16.data_ptr(), kc.data_ptr(), vc.data_ptr(), EKV, D, \
        posd.data_ptr(), rt.data_ptr()
    for i in range(3):
        a.W[i], a.N[i], a.role[i] = ws[i].data_ptr(), ns[i], i
    a.nseg = 3
    if vtype == qtype:
        rc = K.raw().kcpp_gemv_rs(qtype, ctypes.byref(a), 2, 3, ctypes.c_void_p(sp))
    else:
        rc = K.raw().kcpp_gemv_rs_qkv_mixed_pro(ctypes.byref(a), 3, ctypes.c_void_p(sp))
    assert rc == 0
    fused = [host(torch, t, np.int16).copy() for t in (q16, kc, vc)]
    qkv = torch.zeros(LQ, dtype=torch.float32, device="cuda")
    off = 0
    for i in range(3):
        b = K.DecArgs()
        b.K, b.act, b.nseg = E, act.data_ptr(), 1
        b.W[0], b.N[0], b.Y[0] = ws[i].data_ptr(), ns[i], qkv.data_ptr() + 4 * off
        assert K.raw().kcpp_gemv_rs(tys[i], ctypes.byref(b), 0, 0, ctypes.c_void_p(sp)) == 0
        off += ns[i]
    q16, kc, vc = bufs()
    K.call("kcpp_rope_kv_ex", qkv.data_ptr(), LQ, None, q16.data_ptr(), kc.data_ptr(), vc.data_ptr(), 1, H, HKV, D, pos,
           None, rt.data_ptr(), 0, None, None, None, sp)
    unfused = [host(torch, t, np.int16).copy() for t in (q16, kc, vc)]
    for nm, f, u in zip(("q16", "kc", "vc"), fused, unfused):
        assert np.array_equal(f, u), (nm, int((f != u).sum()))
    assert np.abs(fused[0]).max() > 0 and np.abs(fused[1][pos * EKV:(pos + 1) * EKV]).max() > 0
    assert np.abs(fused[2][pos * EKV:(pos + 1) * EKV]).max() > 0


RS_TYPES = ("Q4_K_RS", "Q5_K_RS", "Q6_K_RS")


@pytest.mark.parametrize("E", (2048, 8192))
@pytest.mark.parametrize("ty", RS_TYPES)
def test_pro3_qkv_equals_unfused(env, ty, E):
    """mode 2 (R 2, 4 waves): 256 + 128 + 128 rows"""
    torch, K = env
    _qkv_fused_vs_unfused(torch, K, E, getattr(K, ty), getattr(K, ty))


@pytest.mark.parametrize("E", (2048, 8192))
def test_pro3_mixed_qkv_equals_unfused(env, E):
    """q, k Q4_K_RS + v Q6_K_RS in one launch (k_gemv_rs_qkv) with the LayerNorm prologue"""
    torch, K = env
    _qkv_fused_vs_unfused(torch, K, E, K.Q4_K_RS, K.Q6_K_RS)


@pytest.mark.parametrize("E", (2048, 8192))
@pytest.mark.parametrize("ty", RS_TYPES)
def test_pro3_glu_equals_unfused(env, ty, E):
    """mode 1 (8 waves, prefetch): 384 gate + 384 up rows"""
    torch, K = env
    t, N = getattr(K, ty), 384
    sp = sptr(torch)
    ws, x, nw, act = _inputs(torch, K, [t, t], [N, N], E, 200)
    out = []
    for pro in (3, 0):
        h = torch.zeros(N, dtype=torch.float32, device="cuda")
        a = K.DecArgs()
        a.K, a.nseg, a.eps = E, 1, EPS
        a.W[0], a.W2, a.N[0], a.Y[0] = ws[0].data_ptr(), ws[1].data_ptr(), N, h.data_ptr()
        if pro == 3:
            a.x, a.nw = x.data_ptr(), nw.data_ptr()
        else:
            a.act = act.data_ptr()
        assert K.raw().kcpp_gemv_rs(t, ctypes.byref(a), 1, pro, ctypes.c_void_p(sp)) == 0
        out.append(host(torch, h, np.float32).copy())
    assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32)), int((out[0] != out[1]).sum())
    assert np.abs(out[0]).max() > 0


@pytest.mark.parametrize("E", (2048, 8192))
@pytest.mark.parametrize("ty", RS_TYPES)
def test_pro3_head_equals_unfused(env, ty, E):
    """mode 0 at the head's row count (the plan takes the LayerNorm prologue above 16384 rows only): 16384 + 320 rows"""
    torch, K = env
    t, N = getattr(K, ty), 16384 + 320
    sp = sptr(torch)
    ws, x, nw, act = _inputs(torch, K, [t], [N], E, 300)
    out = []
    for pro in (3, 0):
        y = torch.zeros(N, dtype=torch.float32, device="cuda")
        a = K.DecArgs()
        a.K, a.nseg, a.eps = E, 1, EPS
        a.W[0], a.N[0], a.Y[0] = ws[0].data_ptr(), N, y.data_ptr()
        if pro == 3:
            a.x, a.nw = x.data_ptr(), nw.data_ptr()
        else:
            a.act = act.data_ptr()
        assert K.raw().kcpp_gemv_rs(t, ctypes.byref(a), 0, pro, ctypes.c_void_p(sp)) == 0
        out.append(host(torch, y, np.float32).copy())
    assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32)), int((out[0] != out[1]).sum())
    assert np.abs(out[0]).max() > 0
    # below the head's row count there is no instance: -3, nothing launched
    a.N[0] = 4096
    assert K.raw().kcpp_gemv_rs(t, ctypes.byref(a), 0, 3, ctypes.c_void_p(sp)) == -3


def test_scale_kernel(env):
    torch, K = env
    x = (np.random.default_rng(5).standard_normal(70001) * 7).astype(np.float32)
    for s in (0.0625, 0.3):
        d = dev(torch, x)
        K.call("kcpp_scale", d.data_ptr(), s, x.size, sptr(torch))
        want = (x * np.float32(s)).astype(np.float32)
        assert np.array_equal(host(torch, d, np.float32).view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("scale", (0.0625, 0.3))
def test_logit_scale_on_the_head(env, fx, scale):
    """prefill head and graph-replayed decode head: scaled logits == unscaled x scale bit for bit; the device argmax,
    read after the step, is the argmax of the scaled logits"""
    torch, K = env
    tag = "q4k"
    hp = C.tag_hp(tag)
    prompt = [int(t) for t in fx[tag + "_prompt"]]
    outs = []
    for s in (0.0, scale):
        m = C.setup_model(K.Model(C.model_hp(hp), C.tag_types(tag)), hp, logit_scale=s)
        lg = [m.decode(prompt, 0)]
        am = [m.argmax()]
        lg.append(m.decode([int(fx[tag + "_tokens"][0])], len(prompt)))
        am.append(m.argmax())
        m.close()
        outs.append((np.array(lg), am))
    want = (outs[0][0] * np.float32(scale)).astype(np.float32)
    assert np.array_equal(outs[1][0].view(np.uint32), want.view(np.uint32))
    assert outs[1][1] == [int(v) for v in np.argmax(outs[1][0], axis=1)]
