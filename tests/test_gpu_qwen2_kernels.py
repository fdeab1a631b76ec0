"""The kernels of the Qwen2 graph (q / k / v bias, NeoX rope pairs, GQA ratios 3, 5, 6, 7).

* the fused decode q|k|v launch with DecArgs.bias / rope_neox (gemv_rs.hip EX instances: k_gemv_rs mode 2 and the
  Q4_K + Q6_K mixed launch) == the unfused sequence on the same weights (kcpp_rms_norm -> Q8_K, mode-0 mat-vecs,
  kcpp_rope_kv_ex), bit for bit in q16 and the K / V cache rows;
* kcpp_rope_kv_ex / kcpp_rope_qk_inplace_ex in NeoX mode == the reference's ggml_rope_ext mode 2
  (tests/golden/qwen2_tiny.npz rope*), under the bar test_gpu_kernels.test_rope_kv holds the NORM kernel to
  (np.array_equal: bit for bit), and the NeoX K-shift == the reference's build_k_shift rows, as test_kshift_golden;
* the fused mode-2 implementations without the feature (kcpp_gemv_q4k, kcpp_gemv_dec on non-RS types) answer -3 when a
  bias or rope_neox is set, where the same arguments without them launch;
* decode attention at H / HKV = 3, 5, 6, 7 against refharness.flash_attn under test_gpu_kernels.
  test_flash_attn_vs_oracle's bar (rtol = atol = 4e-3), its Q8_K output == kcpp_quantize_act of the f32 output, and
  the strict-order kernel at G = 7 past one 512-key chunk == refharness.flash_attn_strict bit for bit.

The mixed launch exists only where Q6_K_RS does (K / 256 a multiple of 8, kcpp_rs_supported), so its smallest shape
is K = 2048; at the narrower shapes of the single-type test it answers -3, which is asserted too."""
import ctypes
import os

import numpy as np
import pytest

import qwen2_gguf as Q
import refharness as R
from test_gpu_kernels import dev, host, sptr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    import koboldcpp_amd.lib as K
    return torch, K


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "qwen2_tiny.npz"))


def rope_table(K, n_pos, D, base=1000000.0):
    tab = np.zeros((n_pos, D // 2, 2), np.float32)
    K.raw().kcpp_rope_table(tab.ctypes.data_as(ctypes.c_void_p), n_pos, D, ctypes.c_float(base), ctypes.c_float(1.0), None,
                            ctypes.c_float(0.0), ctypes.c_float(1.0), ctypes.c_float(32.0), ctypes.c_float(1.0), n_pos)
    return tab


def _biases(E, EKV, seed):
    rng = np.random.default_rng(seed)
    bq = rng.standard_normal(E).astype(np.float32)
    bk = rng.standard_normal(EKV).astype(np.float32)
    bk[3::29] = 50.0
    bk[7::31] = -50.0
    bv = rng.standard_normal(EKV).astype(np.float32)
    return bq, bk, bv


def _fused_vs_unfused(torch, K, Kin, H, HKV, D, pos, bias, neox, vtype, qtype=None):
    """q, k in qtype (Q4_K_RS by default), v in vtype (== qtype: one kcpp_gemv_rs launch; Q4_K_RS + Q6_K_RS: the mixed
    launch); weights [Kin][H D], [Kin][HKV D], [Kin][HKV D]"""
    qtype = K.Q4_K_RS if qtype is None else qtype
    E, NQ = Kin, H * D
    EKV = HKV * D
    LQ = NQ + 2 * EKV
    n_ctx = pos + 4
    sp = sptr(torch)
    ws, tys, ns = [], [qtype, qtype, vtype], [NQ, EKV, EKV]
    for i, (ty, n) in enumerate(zip(tys, ns)):
        w = torch.empty(K.row_bytes(ty, E) * n, dtype=torch.uint8, device="cuda")
        K.call("kcpp_weight_synth", ty, 11, i + 1, w.data_ptr(), E, n, sp)
        ws.append(w)
    rng = np.random.default_rng(E + 7 * pos + H)
    x = dev(torch, rng.standard_normal(E).astype(np.float32))
    nw = dev(torch, (1.0 + 0.1 * rng.standard_normal(E)).astype(np.float32))
    rt = dev(torch, rope_table(K, n_ctx, D))
    posd = dev(torch, np.array([pos], np.int32))
    bd = [dev(torch, b) for b in _biases(NQ, EKV, E + H)] if bias else [None] * 3
    bp = [b.data_ptr() if b is not None else None for b in bd]
    eps = 1e-6

    def bufs():
        return (torch.zeros(NQ, dtype=torch.int16, device="cuda"), torch.zeros(n_ctx * EKV, dtype=torch.int16, device="cuda"),
                torch.zeros(n_ctx * EKV, dtype=torch.int16, device="cuda"))
    # fused
    q16, kc, vc = bufs()
    a = K.DecArgs()
    a.K, a.x, a.nw, a.eps = E, x.data_ptr(), nw.data_ptr(), eps
    a.q16, a.kc, a.vc, a.ekv, a.D, a.pos, a.rope_tab = q16.data_ptr(), kc.data_ptr(), vc.data_ptr(), EKV, D, \
        posd.data_ptr(), rt.data_ptr()
    for i in range(3):
        a.W[i], a.N[i], a.role[i], a.bias[i] = ws[i].data_ptr(), ns[i], i, bp[i]
    a.nseg, a.rope_neox = 3, int(neox)
    if vtype == qtype:
        rc = K.raw().kcpp_gemv_rs(qtype, ctypes.byref(a), 2, 1, ctypes.c_void_p(sp))
    else:
        rc = K.raw().kcpp_gemv_rs_qkv_mixed(ctypes.byref(a), ctypes.c_void_p(sp))
    if rc != 0:
        return rc, None, None
    fused = [host(torch, t, np.int16).copy() for t in (q16, kc, vc)]
    # unfused: rms_norm -> Q8_K, one mode-0 mat-vec per segment into the f32 staging row, kcpp_rope_kv_ex
    act = torch.zeros(K.act_bytes(K.Q4_K, E, 1), dtype=torch.uint8, device="cuda")
    K.call("kcpp_rms_norm", x.data_ptr(), E, nw.data_ptr(), None, E, act.data_ptr(), E, 1, eps, sp)
    qkv = torch.zeros(LQ, dtype=torch.float32, device="cuda")
    off = 0
    for i in range(3):
        b = K.DecArgs()
        b.K, b.act, b.nseg = E, act.data_ptr(), 1
        b.W[0], b.N[0], b.Y[0] = ws[i].data_ptr(), ns[i], qkv.data_ptr() + 4 * off
        assert K.gemv_dec(tys[i], b, 0, 0, 1, sp) == 0
        off += ns[i]
    q16, kc, vc = bufs()
    K.call("kcpp_rope_kv_ex", qkv.data_ptr(), LQ, None, q16.data_ptr(), kc.data_ptr(), vc.data_ptr(), 1, H, HKV, D, pos,
           None, rt.data_ptr(), 2 if neox else 0, bp[0], bp[1], bp[2], sp)
    unfused = [host(torch, t, np.int16).copy() for t in (q16, kc, vc)]
    return 0, fused, unfused


VARIANTS = [(True, True), (False, True), (True, False)]     # (bias, neox)


@pytest.mark.parametrize("pos", [0, 37])
@pytest.mark.parametrize("E,H,HKV,D", [(512, 6, 2, 128), (1792, 14, 2, 128), (256, 4, 2, 64)])
def test_fused_qkv_equals_unfused(env, E, H, HKV, D, pos):
    """kcpp_gemv_rs mode 2 / pro 1 (q|k|v all Q4_K_RS) with bias and / or NeoX pairs; input width E, H x D query rows"""
    torch, K = env
    for bias, neox in VARIANTS:
        rc, fused, unfused = _fused_vs_unfused(torch, K, E, H, HKV, D, pos, bias, neox, K.Q4_K_RS)
        assert rc == 0
        for nm, a, b in zip(("q16", "kc", "vc"), fused, unfused):
            assert np.array_equal(a, b), (nm, bias, neox, int((a != b).sum()))
        EKV = HKV * D
        assert np.abs(fused[0]).max() > 0 and np.abs(fused[1][pos * EKV:(pos + 1) * EKV]).max() > 0
        assert np.abs(fused[2][pos * EKV:(pos + 1) * EKV]).max() > 0


@pytest.mark.parametrize("pos", [0, 37])
@pytest.mark.parametrize("E,H,HKV,D", [(2048, 6, 2, 128), (2048, 14, 2, 128), (2048, 4, 2, 64)])
def test_fused_qkv_mixed_equals_unfused(env, E, H, HKV, D, pos):
    """kcpp_gemv_rs_qkv_mixed (q, k Q4_K_RS + v Q6_K_RS) with bias and / or NeoX pairs: the head layouts of the
    single-type test at the narrowest input width the mixed launch takes (K = 2048)"""
    torch, K = env
    for bias, neox in VARIANTS:
        rc, fused, unfused = _fused_vs_unfused(torch, K, E, H, HKV, D, pos, bias, neox, K.Q6_K_RS)
        assert rc == 0
        for nm, a, b in zip(("q16", "kc", "vc"), fused, unfused):
            assert np.array_equal(a, b), (nm, bias, neox, int((a != b).sum()))


@pytest.mark.parametrize("ty", ["Q5_K_RS", "Q6_K_RS"])
def test_fused_qkv_other_rs_types(env, ty):
    """the single-type launch in the other two row-major layouts (one instance list serves all three) at K = 2048, the
    narrowest width Q6_K_RS exists at: (14, 2) heads of 128, position 37, the three bias / NeoX variants"""
    torch, K = env
    t = getattr(K, ty)
    for bias, neox in VARIANTS:
        rc, fused, unfused = _fused_vs_unfused(torch, K, 2048, 14, 2, 128, 37, bias, neox, t, qtype=t)
        assert rc == 0
        for nm, a, b in zip(("q16", "kc", "vc"), fused, unfused):
            assert np.array_equal(a, b), (nm, bias, neox, int((a != b).sum()))


def test_fused_qkv_refusals(env):
    """the mixed launch where Q6_K_RS does not exist (K / 256 not a multiple of 8) and NeoX over a segment that is
    not whole heads answer -3; they never ignore the fields"""
    torch, K = env
    sp = sptr(torch)
    dummy = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    a = K.DecArgs()                              # the issue's (14, 2) shape at K = 1792: no launch may happen
    a.K, a.nseg, a.rope_neox, a.D = 1792, 3, 1, 128
    for i, n in enumerate((1792, 256, 256)):
        a.W[i], a.N[i], a.role[i] = dummy.data_ptr(), n, i
    assert K.raw().kcpp_gemv_rs_qkv_mixed(ctypes.byref(a), ctypes.c_void_p(sp)) == -3
    E = 512
    w = torch.zeros(K.row_bytes(K.Q4_K_RS, E) * E, dtype=torch.uint8, device="cuda")
    a = K.DecArgs()
    a.K, a.nseg, a.rope_neox, a.D = E, 1, 1, 128
    a.W[0], a.N[0], a.role[0] = w.data_ptr(), 192, 0             # 1.5 heads
    assert K.raw().kcpp_gemv_rs(K.Q4_K_RS, ctypes.byref(a), 2, 1, ctypes.c_void_p(sp)) == -3


@pytest.mark.parametrize("case", sorted(Q.ROPE_CASES))
def test_rope_ex_neox_vs_reference(env, fx, case):
    """NeoX mode of both rope kernels == ggml_rope_ext mode 2 of the reference build, bit for bit (the bar of
    test_gpu_kernels.test_rope_kv: np.array_equal); with biases == the same kernels on rows with the bias already
    added; the two kernels' f32 results agree bit for bit"""
    torch, K = env
    T, H, HKV, D, pos = Q.ROPE_CASES[case]
    EKV, LQ = HKV * D, (H + 2 * HKV) * D
    n_ctx = max(pos) + 1
    sp = sptr(torch)
    x = Q.rope_case_input(case)
    rt = dev(torch, rope_table(K, n_ctx, D))
    posd = dev(torch, np.asarray(pos, np.int32))
    want_q, want_k = fx[case + "_q"], fx[case + "_k"]
    bq, bk, bv = _biases(H * D, EKV, 5)
    bcat = np.concatenate([bq, bk, bv])

    def run_kv(rows, b):
        qd = dev(torch, rows)
        qo = torch.zeros((T, H, D), dtype=torch.float32, device="cuda")
        q16 = torch.zeros((T, H, D), dtype=torch.float16, device="cuda")
        kc = torch.zeros((n_ctx, EKV), dtype=torch.float16, device="cuda")
        vc = torch.zeros((n_ctx, EKV), dtype=torch.float16, device="cuda")
        bd = [dev(torch, v) for v in b] if b else [None] * 3
        K.call("kcpp_rope_kv_ex", qd.data_ptr(), LQ, qo.data_ptr(), q16.data_ptr(), kc.data_ptr(), vc.data_ptr(), T, H, HKV,
               D, 0, posd.data_ptr(), rt.data_ptr(), 2, *[v.data_ptr() if v is not None else None for v in bd], sp)
        return (host(torch, qo, np.float32).reshape(T, H, D), host(torch, q16, np.float16).reshape(T, H, D),
                host(torch, kc, np.float16)[pos].reshape(T, HKV, D), host(torch, vc, np.float16)[pos])

    qo, q16, kc, vc = run_kv(x, None)
    assert np.array_equal(qo, want_q)
    assert np.array_equal(q16, want_q.astype(np.float16))
    assert np.array_equal(kc, want_k.astype(np.float16))
    assert np.array_equal(vc, x[:, (H + HKV) * D:].astype(np.float16))
    xb = (x + bcat[None, :]).astype(np.float32)             # the f32 ggml_add in front of the rope
    got_b, want_b = run_kv(x, (bq, bk, bv)), run_kv(xb, None)
    for a, b in zip(got_b, want_b):
        assert np.array_equal(a, b)
    # the in-place kernel (quantized-KV path): positions n_past + t, so one launch per row
    for b in (None, (bq, bk, bv)):
        rows = x.copy()
        for t in range(T):
            rd = dev(torch, rows[t])
            bd = [dev(torch, v) for v in b] if b else [None] * 3
            K.call("kcpp_rope_qk_inplace_ex", rd.data_ptr(), LQ, 1, H, HKV, D, pos[t], None, rt.data_ptr(), 2,
                   *[v.data_ptr() if v is not None else None for v in bd], sp)
            rows[t] = host(torch, rd, np.float32)
        ref = want_b if b else (qo, None, None, None)
        assert np.array_equal(rows[:, :H * D].reshape(T, H, D), ref[0])
        if b is None:
            assert np.array_equal(rows[:, H * D:(H + HKV) * D].reshape(T, HKV, D), want_k)
            assert np.array_equal(rows[:, (H + HKV) * D:], x[:, (H + HKV) * D:])
        else:
            assert np.array_equal(rows[:, (H + HKV) * D:], xb[:, (H + HKV) * D:])
            assert np.array_equal(rows[:, H * D:(H + HKV) * D].astype(np.float16).reshape(T, HKV, D), want_b[2])


def test_rope_ex_mode0_is_rope_kv(env):
    """mode 0 with null biases is kcpp_rope_kv (the old entry is a wrapper); another mode is refused"""
    torch, K = env
    T, H, HKV, D, n_past = 3, 4, 2, 128, 9
    LQ = (H + 2 * HKV) * D
    sp = sptr(torch)
    x = dev(torch, np.random.default_rng(1).standard_normal((T, LQ)).astype(np.float32))
    rt = dev(torch, rope_table(K, 16, D))
    outs = []
    for ex in (False, True):
        q16 = torch.zeros(T * H * D, dtype=torch.int16, device="cuda")
        kc = torch.zeros(16 * HKV * D, dtype=torch.int16, device="cuda")
        vc = torch.zeros(16 * HKV * D, dtype=torch.int16, device="cuda")
        if ex:
            K.call("kcpp_rope_kv_ex", x.data_ptr(), LQ, None, q16.data_ptr(), kc.data_ptr(), vc.data_ptr(), T, H, HKV, D,
                   n_past, None, rt.data_ptr(), 0, None, None, None, sp)
        else:
            K.call("kcpp_rope_kv", x.data_ptr(), LQ, None, q16.data_ptr(), kc.data_ptr(), vc.data_ptr(), T, H, HKV, D,
                   n_past, None, rt.data_ptr(), sp)
        outs.append([host(torch, t, np.int16).copy() for t in (q16, kc, vc)])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    assert K.raw().kcpp_rope_kv_ex(None, LQ, None, None, None, None, T, H, HKV, D, 0, None, None, 1, None, None, None,
                                   ctypes.c_void_p(sp)) == -1


def test_kv_shift_neox_vs_reference(env, fx):
    """kcpp_kv_shift_rows_ex mode 2 == the reference's build_k_shift on NeoX pairs (ggml_rope_ext_inplace mode 2 on
    the f16 cache rows at position -diff), bit for bit, as test_kshift_golden for NORM"""
    torch, K = env
    before, after = fx["kshift_before"], fx["kshift_after"]
    diff = int(fx["kshift_p0_diff"][1])
    hp = Q.TINY_QWEN2
    D = hp["n_embd"] // hp["n_head"]
    n = before.shape[0] * before.shape[1] // D
    row = np.zeros(D, np.float32)
    K.call("kcpp_rope_row", row.ctypes.data, -diff, D, float(hp["rope_base"]), 1.0, 0.0, 1.0, 32.0, 1.0, hp["n_ctx"])
    kd = torch.from_numpy(before.view(np.int16).copy()).cuda()
    vd = torch.from_numpy(np.arange(kd.numel(), dtype=np.int16).reshape(kd.shape)).cuda()
    ks, vs = torch.zeros_like(kd), torch.zeros_like(vd)
    csd = dev(torch, row)
    K.call("kcpp_kv_shift_rows_ex", kd.data_ptr(), vd.data_ptr(), ks.data_ptr(), vs.data_ptr(), n, D, csd.data_ptr(), 2,
           sptr(torch))
    assert np.array_equal(host(torch, ks, np.uint16).reshape(after.shape), after)
    assert np.array_equal(host(torch, vs, np.int16), host(torch, vd, np.int16))
    assert not np.array_equal(before, after)


def test_other_fused_kernels_refuse_bias_and_neox(env):
    """mode-2 implementations without the feature answer -3 with bias[] or rope_neox set (never ignore them):
    kcpp_gemv_q4k and kcpp_gemv_dec on non-RS types, at a shape where the same arguments without the fields launch
    (rc 0), so the -3 is the new guard's.  kcpp_gemv_stream is called too, but proves nothing about its guard: it has
    no mode-2 launch at any shape (only K = 14336, mode 0, pro 2), so it answered -3 before as well."""
    torch, K = env
    E, H, HKV, D = 4096, 32, 8, 128
    EKV = HKV * D
    sp = sptr(torch)
    rng = np.random.default_rng(3)
    x = dev(torch, rng.standard_normal(E).astype(np.float32))
    nw = dev(torch, np.ones(E, np.float32))
    rt = dev(torch, rope_table(K, 8, D))
    posd = dev(torch, np.array([2], np.int32))
    q16 = torch.zeros(E, dtype=torch.int16, device="cuda")
    kc = torch.zeros(8 * EKV, dtype=torch.int16, device="cuda")
    vc = torch.zeros(8 * EKV, dtype=torch.int16, device="cuda")
    bq = dev(torch, np.ones(E, np.float32))

    def args(w, which):
        a = K.DecArgs()
        a.K, a.x, a.nw, a.eps = E, x.data_ptr(), nw.data_ptr(), 1e-5
        a.q16, a.kc, a.vc, a.ekv, a.D, a.pos, a.rope_tab = q16.data_ptr(), kc.data_ptr(), vc.data_ptr(), EKV, D, \
            posd.data_ptr(), rt.data_ptr()
        a.W[0], a.N[0], a.role[0], a.nseg = w.data_ptr(), E, 0, 1
        if which == "bias":
            a.bias[0] = bq.data_ptr()
        elif which == "neox":
            a.rope_neox = 1
        return a
    for ty in (R.Q4_K, R.Q8_0, R.Q6_K):
        w = torch.empty(K.row_bytes(ty, E) * E, dtype=torch.uint8, device="cuda")
        K.call("kcpp_weight_synth", ty, 5, 1, w.data_ptr(), E, E, sp)
        assert K.gemv_dec(ty, args(w, None), 2, 1, 2, sp) == 0
        for which in ("bias", "neox"):
            a = args(w, which)
            assert K.gemv_dec(ty, a, 2, 1, 2, sp) == -3
            if ty == R.Q4_K:
                assert K.raw().kcpp_gemv_q4k(ctypes.byref(a), 2, 1, ctypes.c_void_p(sp)) == -3
                assert K.raw().kcpp_gemv_stream(ty, ctypes.byref(a), 2, 1, ctypes.c_void_p(sp)) == -3
    torch.cuda.synchronize()


# ---------------------------------------------------------------- attention ratios
_FA = {}


def _fa_inputs(H, HKV):
    """q / K / V of one (H, HKV), made once; the references per key count are added as they are first needed"""
    if (H, HKV) not in _FA:
        D, n_ctx = 128, 704
        rng = np.random.default_rng(100 * H + HKV)
        q = rng.standard_normal((5, H, D)).astype(np.float32)
        k = (rng.standard_normal((n_ctx, HKV, D)) * 0.5).astype(np.float16)
        v = rng.standard_normal((n_ctx, HKV, D)).astype(np.float16)
        _FA[(H, HKV)] = dict(q=q, k=k, v=v, ref={})
    return _FA[(H, HKV)]


def _fa_ref(c, T, n_kv):
    if (T, n_kv) not in c["ref"]:
        n_past = n_kv - T
        mask = np.zeros((T, n_kv), np.float16)
        for t in range(T):
            mask[t, n_past + t + 1:] = -np.inf
        c["ref"][(T, n_kv)] = R.flash_attn(c["q"][:T].astype(np.float16).astype(np.float32), c["k"][:n_kv], c["v"][:n_kv],
                                           mask)
    return c["ref"][(T, n_kv)]


@pytest.mark.parametrize("H,HKV", [(6, 2), (10, 2), (12, 2), (14, 2)])
def test_decode_attention_ratios(env, H, HKV):
    """kcpp_flash_attn at T = 1 (the split pair, force_path 1, and the one-launch short form, 7; n_past by value and
    from a device word) at 1, 64, 65 and 700 keys, the Q8_K output of the split pair, and T = 5 through the 64-key
    chunk kernel, against refharness.flash_attn at rtol = atol = 4e-3 (test_flash_attn_vs_oracle's bar)"""
    torch, K = env
    D, n_ctx = 128, 704
    c = _fa_inputs(H, HKV)
    sp = sptr(torch)
    kd, vd = dev(torch, c["k"]), dev(torch, c["v"])
    ws = torch.zeros(K.fa_workspace_bytes(16, H, n_ctx), dtype=torch.uint8, device="cuda")
    scale = 1.0 / np.sqrt(D)
    for n_kv in (1, 64, 65, 700):
        want = _fa_ref(c, 1, n_kv)
        q16 = dev(torch, c["q"][:1].astype(np.float16))
        npd = dev(torch, np.array([n_kv - 1], np.int32))
        for path in (1, 7):
            for use_dev in (False, True):
                out = torch.full((1, H, D), float("nan"), dtype=torch.float32, device="cuda")
                rc = K.raw().kcpp_flash_attn(q16.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(), None, ws.data_ptr(),
                                             1, H, HKV, D, 0 if use_dev else n_kv - 1, npd.data_ptr() if use_dev else None,
                                             n_ctx, scale, path, sp)
                assert rc == 0, (n_kv, path, use_dev, rc)
                got = host(torch, out, np.float32).reshape(1, H, D)
                print("H %d HKV %d keys %d path %d dev %d: max |d| %.3g" % (H, HKV, n_kv, path, use_dev, np.abs(got - want).max()))
                np.testing.assert_allclose(got, want, rtol=4e-3, atol=4e-3)
        # Q8_K output of the split pair == kcpp_quantize_act of its f32 output, bit for bit
        nb = K.act_bytes(R.Q4_K, H * D, 1)
        out = torch.zeros((1, H, D), dtype=torch.float32, device="cuda")
        qo = torch.zeros(nb, dtype=torch.uint8, device="cuda")
        assert K.raw().kcpp_flash_attn(q16.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(), qo.data_ptr(),
                                       ws.data_ptr(), 1, H, HKV, D, n_kv - 1, None, n_ctx, scale, 1, sp) == 0
        qr = torch.zeros(nb, dtype=torch.uint8, device="cuda")
        K.call("kcpp_quantize_act", R.Q8_K, out.data_ptr(), H * D, qr.data_ptr(), H * D, 1, sp)
        assert np.array_equal(host(torch, qo, np.uint8), host(torch, qr, np.uint8))
    # T = 5: the 64-key-chunk kernel (1 < T <= 16), rows end at 296..300 keys
    T, n_kv = 5, 300
    want = _fa_ref(c, T, n_kv)
    q16 = dev(torch, c["q"][:T].astype(np.float16))
    out = torch.full((T, H, D), float("nan"), dtype=torch.float32, device="cuda")
    assert K.raw().kcpp_flash_attn(q16.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(), None, ws.data_ptr(), T, H,
                                   HKV, D, n_kv - T, None, n_ctx, scale, 0, sp) == 0
    np.testing.assert_allclose(host(torch, out, np.float32).reshape(T, H, D), want, rtol=4e-3, atol=4e-3)
    # kcpp_fa_decode_ex: the production pair (5), the short form (8) and the chunk kernel (0) on the same views
    want = _fa_ref(c, 1, 65)
    q16 = dev(torch, c["q"][:1].astype(np.float16))
    for variant in (5, 8, 0):
        out = torch.full((1, H, D), float("nan"), dtype=torch.float32, device="cuda")
        assert K.raw().kcpp_fa_decode_ex(q16.data_ptr(), kd.data_ptr(), vd.data_ptr(), HKV * D, D, out.data_ptr(), None,
                                         ws.data_ptr(), H, HKV, 64, None, n_ctx, scale, variant, sp) == 0, variant
        np.testing.assert_allclose(host(torch, out, np.float32).reshape(1, H, D), want, rtol=4e-3, atol=4e-3)


def test_fa_exact_g7_513_keys(env):
    """the strict-order kernel at G = 7, one key into the second 512-key chunk == refharness.flash_attn_strict, bit for
    bit (the restatement is pinned to the reference build by tests/test_fa_strict_oracle.py)"""
    torch, K = env
    H, HKV, D, n_kv = 14, 2, 128, 513
    c = _fa_inputs(H, HKV)
    q = c["q"][:1]
    mask = np.zeros((1, n_kv), np.float16)
    want = R.flash_attn_strict(q.astype(np.float16).astype(np.float32), c["k"][:n_kv], c["v"][:n_kv], mask)
    q16 = dev(torch, q.astype(np.float16))
    kd, vd = dev(torch, c["k"]), dev(torch, c["v"])
    out = torch.full((1, H, D), float("nan"), dtype=torch.float32, device="cuda")
    K.call("kcpp_flash_attn_exact", q16.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(), 1, H, HKV, D, n_kv - 1,
           None, float(np.float32(1) / np.sqrt(np.float32(D))), sptr(torch))
    got = host(torch, out, np.float32).reshape(1, H, D)
    print("differing outputs:", int((got.view(np.uint32) != want.view(np.uint32)).sum()), "of", got.size)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
