"""Attention past 4096 keys, across 64-key chunk boundaries, and at every GQA ratio of every kernel that serves it
(koboldcpp_amd/csrc/attn.hip, attn_mfma.hip, attn_kvq.hip).

Inputs carry PLANTED KEYS.  With Gaussian K the softmax over n keys is nearly flat, the output shrinks like 1/sqrt(n)
and a kernel that dropped a whole stretch of the context would stay inside any absolute bar.  Here every kv head has a
direction u (|u| = sqrt(D)); q = 0.7 u + 0.7 N(0, 1), K = 0.5 N(0, 1), V = N(0, 1), and the first and the last key
of each region of the context -- [0, 64), [64, 4096), [4096, 32768), [32768, ...) : one 64-key chunk, what the suite
covered before, k_fa_combine's chunks 64..511, its chunks past 511 -- hold k = u and v = 4 N(0, 1).  The regions cut
[0, n_past + 1), the keys every row of the case sees.  Two conditions are asserted on the float64 reference alone,
before any GPU result is looked at (`_conditions`):

  1. every region holds >= 1 % of the softmax mass of every row;
  2. the reference with any one region masked out is >= 10 bars away from the full one (same metric as the test).

Reference: numpy float64 softmax(q k^T scale + causal mask) v on the f16-rounded inputs.  Metric: max |got - ref| /
max |ref| per (token, head) row, worst row.

Bars.  FMA kernels (k_fa_dec4 / k_fa_dec5 + k_fa_comb4, k_fa_decode + k_fa_combine, k_fa_prefill<128> / <64>):
max(2e-5, 4 e_orc), e_orc the error of the CPU oracle with f32 accumulation (R.flash_attn under
orc_set_fa_f32_accum(1), a serial online softmax that shares nothing with the kernels) against the same float64
reference; 2e-5 is the suite's bar against that oracle, the factor 4 covers another f32 summation order of the same
terms.  MFMA kernels round P to f16: 2e-3 (2^-11 per weight, times 4), independent of the key count.  Quantized caches:
R.flash_attn_q at test_gpu_kvq.test_flash_attn_q_vs_oracle's bar.  A Q8_K output is byte-equal to kcpp_quantize_act of
the same launch's f32 output.  Every case prints "reach <kernel> keys <n>: e_orc .. err .. bar .." (DESIGN.md's table).
"""
import numpy as np
import pytest

import refharness as R
from test_gpu_kernels import dev, host, sptr
from test_gpu_kvq import attend, soa_to_blocks, store

pytestmark = pytest.mark.gpu

EDGES = (0, 64, 4096, 32768)
BAR_MFMA = 2e-3
PAD_ROWS = 64         # cache rows past the keys: k = u (the needle direction), v = 100 -- finite, and fatal if attended


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import koboldcpp_amd.lib as K
    return torch, K


def regions(n):
    """[0, n) cut at 64, 4096 and 32768"""
    e = [x for x in EDGES if x < n] + [n]
    return list(zip(e[:-1], e[1:]))


def planted(seed, T, H, HKV, D, n_past, n_rows=None, gain=0.7):
    """q f16 [T][H][D], k / v f16 [n_rows][HKV][D] (keys [0, n_past + T), then padding rows no query may see)"""
    rng = np.random.default_rng(seed)
    G = H // HKV
    n_keys = n_past + T
    n_rows = n_rows or n_keys + PAD_ROWS
    assert n_rows >= n_keys
    u = rng.standard_normal((HKV, D))
    u *= np.sqrt(D) / np.linalg.norm(u, axis=1, keepdims=True)
    q = (gain * u[np.arange(H) // G][None] + 0.7 * rng.standard_normal((T, H, D))).astype(np.float16)
    k = (0.5 * rng.standard_normal((n_rows, HKV, D))).astype(np.float16)
    v = rng.standard_normal((n_rows, HKV, D)).astype(np.float16)
    for lo, hi in regions(n_past + 1):
        for p in (lo, hi - 1):
            k[p] = u.astype(np.float16)
            v[p] = (4 * rng.standard_normal((HKV, D))).astype(np.float16)
    k[n_keys:] = u.astype(np.float16)
    v[n_keys:] = 100
    return q, k, v


def ref64(q, k, v, n_past, regs):
    """float64 causal attention of q [T][H][D] over k / v [n_keys][HKV][D] (any float dtype), head by head.  Returns
    out [T][H][D], mass [region][T][H] (softmax mass of each region) and drop [region][T][H][D] (the output with that
    region masked out)."""
    T, H, D = q.shape
    n_keys, HKV, _ = k.shape
    G = H // HKV
    scale = float(np.float32(1) / np.sqrt(np.float32(D)))
    out = np.empty((T, H, D))
    mass = np.empty((len(regs), T, H))
    drop = np.empty((len(regs), T, H, D))
    dead = np.arange(n_keys)[None, :] > (n_past + np.arange(T))[:, None]
    for h in range(H):
        kk, vv = k[:, h // G].astype(np.float64), v[:, h // G].astype(np.float64)
        s = q[:, h].astype(np.float64) @ kk.T * scale
        s[dead] = -np.inf
        p = np.exp(s - s.max(axis=1, keepdims=True))
        p /= p.sum(axis=1, keepdims=True)
        out[:, h] = p @ vv
        for r, (lo, hi) in enumerate(regs):
            mass[r, :, h] = p[:, lo:hi].sum(axis=1)
            with np.errstate(divide="ignore", invalid="ignore"):
                drop[r, :, h] = (out[:, h] - p[:, lo:hi] @ vv[lo:hi]) / (1 - mass[r, :, h])[:, None]
    return out, mass, drop


def rel_err(got, ref):
    """max |got - ref| / max |ref| per (token, head) row, the worst row"""
    got = np.asarray(got, np.float64).reshape(ref.shape)
    assert np.isfinite(got).all()
    return float((np.abs(got - ref).max(axis=-1) / np.abs(ref).max(axis=-1)).max())


def causal_mask(T, n_past, n_kv, rows=None):
    m = np.zeros((rows or T, n_kv), np.float16)
    for t in range(T):
        m[t, n_past + t + 1:] = -np.inf
    m[T:] = -np.inf
    return m


_CASES = {}


def case(D, H, HKV, T, n_past, n_rows=None, gain=0.7, seed=0):
    """inputs, float64 reference and oracle error of one case, made once and left unchanged"""
    key = (D, H, HKV, T, n_past, n_rows, gain, seed)
    if key not in _CASES:
        q, k, v = planted(1000003 * seed + 7919 * n_past + 131 * T + 17 * H + HKV + D, T, H, HKV, D, n_past, n_rows, gain)
        n_keys = n_past + T
        regs = regions(n_past + 1)
        ref, mass, drop = ref64(q, k[:n_keys], v[:n_keys], n_past, regs)
        R.lib().orc_set_fa_f32_accum(1)
        try:
            orc = R.flash_attn(q.astype(np.float32), k[:n_keys], v[:n_keys], causal_mask(T, n_past, n_keys))
        finally:
            R.lib().orc_set_fa_f32_accum(0)
        e_orc = rel_err(orc, ref)
        _CASES[key] = dict(q=q, k=k, v=v, ref=ref, mass=mass, drop=drop, regs=regs, e_orc=e_orc, n_keys=n_keys,
                           bar=max(2e-5, 4 * e_orc))
    return _CASES[key]


def _conditions(c, bar):
    """the two input conditions, on the reference alone"""
    assert c["mass"].min() >= 0.01, ("a region below 1 % of a row's softmax mass", c["regs"], c["mass"].min(axis=(1, 2)))
    if len(c["regs"]) > 1:          # (with one region there is nothing left to attend once it is masked)
        for r, reg in enumerate(c["regs"]):
            d = rel_err(c["drop"][r], c["ref"])
            assert d >= 10 * bar, ("masking region %s moves the reference by %.3g < 10 bars" % (reg, d), bar)


def _check(c, got, kernel, note, bar=None):
    e_orc = c["e_orc"]
    bar = c["bar"] if bar is None else bar
    err = rel_err(got, c["ref"])
    print("reach %s keys %d: e_orc %.3g err %.3g bar %.3g  [%s, max |ref| %.3g]" %
          (kernel, c["n_keys"], e_orc, err, bar, note, np.abs(c["ref"]).max()))
    assert err <= bar, (kernel, note, err, bar)


def _q8k_of(torch, K, out, E, T):
    """kcpp_quantize_act(Q8_K) of the device tensor out [T][E]"""
    qr = torch.zeros(K.act_bytes(R.Q4_K, E, T), dtype=torch.uint8, device="cuda")
    K.call("kcpp_quantize_act", R.Q8_K, out.data_ptr(), E, qr.data_ptr(), E, T, sptr(torch))
    return host(torch, qr, np.uint8)


def _flash_attn(torch, K, c, T, H, HKV, D, n_past, path, use_dev, want_q, ws, kd, vd, n_ctx):
    """one kcpp_flash_attn launch; returns (out [T][H][D], Q8_K bytes or None, kcpp_quantize_act(Q8_K) of out or None)"""
    q16 = dev(torch, c["q"])
    out = torch.full((T, H, D), float("nan"), dtype=torch.float32, device="cuda")
    qo = torch.zeros(K.act_bytes(R.Q4_K, H * D, T), dtype=torch.uint8, device="cuda") if want_q else None
    npd = dev(torch, np.array([n_past], np.int32)) if use_dev else None
    rc = K.raw().kcpp_flash_attn(q16.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(),
                                 qo.data_ptr() if want_q else None, ws.data_ptr(), T, H, HKV, D, 0 if use_dev else n_past,
                                 npd.data_ptr() if use_dev else None, n_ctx, float(1.0 / np.sqrt(D)), path, sptr(torch))
    assert rc == 0, ("kcpp_flash_attn refused a shape the loader accepts", rc, T, H, HKV, D, n_past, path)
    got = host(torch, out, np.float32).reshape(T, H, D)
    if not want_q:
        return got, None, None
    return got, host(torch, qo, np.uint8), _q8k_of(torch, K, out, H * D, T)


# ---------------------------------------------------------------- 1: single-token decode, the split pair
# G = 1..8 (H even: odd ratios over 2 kv heads), 64 splits; G = 4 over 2 kv heads (64 splits); G = 1 over 8 (32 splits)
SPLIT_PAIR = [(H, HKV, 4097) for H, HKV in ((2, 2), (2, 1), (6, 2), (4, 1), (10, 2), (6, 1), (14, 2), (8, 1), (8, 2), (8, 8))]
SPLIT_PAIR += [(H, HKV, 33000) for H, HKV in ((2, 2), (4, 1), (14, 2), (8, 1))]


@pytest.mark.parametrize("H,HKV,n_kv", SPLIT_PAIR)
def test_decode_split_pair(env, H, HKV, n_kv):
    """kcpp_flash_attn, T = 1, force_path 1 (k_fa_dec5 + k_fa_comb4), n_past by value and from a device word: one key
    into the 65th 64-key chunk, and 33000 keys"""
    torch, K = env
    G, D = H // HKV, 128
    n_ctx = n_kv + PAD_ROWS
    c = case(D, H, HKV, 1, n_kv - 1)
    _conditions(c, c["bar"])
    kd, vd = dev(torch, c["k"]), dev(torch, c["v"])
    ws = torch.zeros(K.fa_workspace_bytes(16, H, 64), dtype=torch.uint8, device="cuda")
    for use_dev in (False, True):
        got, _, _ = _flash_attn(torch, K, c, 1, H, HKV, D, n_kv - 1, 1, use_dev, False, ws, kd, vd, n_ctx)
        _check(c, got, "k_fa_dec5+k_fa_comb4", "G %d HKV %d dev %d" % (G, HKV, use_dev))


# ---------------------------------------------------------------- 2: 2..16 tokens, the chunk kernel + k_fa_combine
# (16, 56), (2, 63), (16, 4090): the batch straddles a 64-key boundary (a chunk empty for the early tokens, live for the
# late ones); (5, 4200): combine's c0 loop (more than 64 chunks); (16, 32760), (2, 33000): its r + 512 loops
@pytest.mark.parametrize("H,HKV", [(2, 2), (2, 1), (4, 1), (14, 2), (8, 1)])
@pytest.mark.parametrize("T,n_past", [(16, 56), (2, 63), (16, 4090), (5, 4200), (16, 32760), (2, 33000)])
def test_chunk_decode_and_combine(env, H, HKV, T, n_past):
    """kcpp_flash_attn, auto path, 2 <= T <= 16 (k_fa_decode<128, G> + k_fa_combine<QUANT>), with and without the Q8_K
    output, n_past by value and from a device word"""
    torch, K = env
    G, D = H // HKV, 128
    c = case(D, H, HKV, T, n_past)
    _conditions(c, c["bar"])
    n_ctx = c["n_keys"] + PAD_ROWS
    kd, vd = dev(torch, c["k"]), dev(torch, c["v"])
    ws = torch.zeros(K.fa_workspace_bytes(16, H, n_ctx), dtype=torch.uint8, device="cuda")
    for use_dev in (False, True):
        for want_q in (False, True):
            ws.fill_(0xFF)              # partials of chunks a query does not use must not be read (NaN bytes)
            got, qo, qr = _flash_attn(torch, K, c, T, H, HKV, D, n_past, 0, use_dev, want_q, ws, kd, vd, n_ctx)
            _check(c, got, "k_fa_decode+k_fa_combine", "T %d G %d HKV %d dev %d qout %d" % (T, G, HKV, use_dev, want_q))
            if want_q:
                assert np.array_equal(qo, qr), "Q8_K output != kcpp_quantize_act of the same launch's f32 output"


# ---------------------------------------------------------------- 3: tiled prefill, D = 128, every ratio but 4
TILED_128 = [(H, T, n_past) for H in (2, 4, 6, 10, 12, 14, 16) for T, n_past in ((70, 0), (70, 130), (65, 4090))]
TILED_128 += [(14, 65, 32760)]


@pytest.mark.parametrize("H,T,n_past", TILED_128)
def test_tiled_prefill_128(env, H, T, n_past):
    """kcpp_flash_attn force_path 2 (k_fa_prefill<128>, what every model with G != 4 runs for a ubatch over 16 tokens):
    two query tiles with a ragged second one, n_past = 0 and > 0, past 4096 keys; G = 7 also past 32768"""
    torch, K = env
    HKV, D = 2, 128
    c = case(D, H, HKV, T, n_past)
    _conditions(c, c["bar"])
    n_ctx = c["n_keys"] + PAD_ROWS
    kd, vd = dev(torch, c["k"]), dev(torch, c["v"])
    ws = torch.zeros(K.fa_workspace_bytes(16, H, 64), dtype=torch.uint8, device="cuda")
    got, _, _ = _flash_attn(torch, K, c, T, H, HKV, D, n_past, 2, False, False, ws, kd, vd, n_ctx)
    _check(c, got, "k_fa_prefill<128>", "T %d G %d" % (T, H // HKV))


# ---------------------------------------------------------------- 4: 64-dim heads
@pytest.mark.parametrize("H,HKV", [(4, 4), (8, 2), (32, 4)])
@pytest.mark.parametrize("T,n_past,use_dev,want_q", [(1, 0, True, False), (1, 64, True, False), (1, 4096, True, False),
                                                     (5, 295, False, True), (70, 130, False, False),
                                                     (65, 4090, False, False)])
def test_head_dim_64(env, H, HKV, T, n_past, use_dev, want_q):
    """kcpp_flash_attn at D = 64 (k_fa_prefill<64>: decode from a device word, small batches and prefill alike), the
    Q8_K output at (5, 295)"""
    torch, K = env
    D = 64
    c = case(D, H, HKV, T, n_past)
    _conditions(c, c["bar"])
    n_ctx = c["n_keys"] + PAD_ROWS
    kd, vd = dev(torch, c["k"]), dev(torch, c["v"])
    ws = torch.zeros(K.fa_workspace_bytes(16, H, 64), dtype=torch.uint8, device="cuda")
    got, qo, qr = _flash_attn(torch, K, c, T, H, HKV, D, n_past, 0, use_dev, want_q, ws, kd, vd, n_ctx)
    _check(c, got, "k_fa_prefill<64>", "T %d H %d HKV %d dev %d" % (T, H, HKV, use_dev))
    if want_q:
        assert np.array_equal(qo, qr), "Q8_K output != kcpp_quantize_act of the same launch's f32 output"


# ---------------------------------------------------------------- 5: MFMA prefill, unsplit and key-split
@pytest.mark.parametrize("H,HKV", [(4, 1), (8, 2)])
@pytest.mark.parametrize("T,n_past,split", [(17, 4090, True), (64, 32760, True), (65, 4090, False), (65, 32760, False)])
def test_mfma_prefill(env, H, HKV, T, n_past, split):
    """kcpp_flash_attn_prefill_mfma (unsplit) and kcpp_flash_attn_prefill_mfma_ex with a workspace (T <= 64: keys split
    over the grid, k_fa_split_merge) past 4096 and past 32768 keys, at the MFMA bar"""
    torch, K = env
    D = 128
    c = case(D, H, HKV, T, n_past)
    _conditions(c, BAR_MFMA)
    q16, kd, vd = dev(torch, c["q"]), dev(torch, c["k"]), dev(torch, c["v"])
    out = torch.full((T, H, D), float("nan"), dtype=torch.float32, device="cuda")
    scale = float(1.0 / np.sqrt(D))
    if split:
        ws = torch.zeros(K.fa_workspace_bytes(16, H, c["n_keys"]), dtype=torch.uint8, device="cuda")
        assert ws.numel() >= K.raw().kcpp_fa_split_ws_bytes(H)
        rc = K.raw().kcpp_flash_attn_prefill_mfma_ex(q16.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(), None,
                                                     ws.data_ptr(), T, H, HKV, D, n_past, scale, sptr(torch))
    else:
        rc = K.raw().kcpp_flash_attn_prefill_mfma(q16.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.data_ptr(), T, H, HKV,
                                                  D, n_past, scale, sptr(torch))
    assert rc == 0, rc
    _check(c, host(torch, out, np.float32), "k_fa_prefill_mfma3 split" if split else "k_fa_prefill_mfma3",
           "T %d HKV %d" % (T, HKV), BAR_MFMA)


# ---------------------------------------------------------------- 6: the ggml-op form
@pytest.mark.parametrize("D,H,HKV", [(128, 2, 1), (128, 14, 2), (64, 4, 1)])
@pytest.mark.parametrize("T", [5, 17])
@pytest.mark.parametrize("n_past,n_kv", [(4100, 4352), (32800, 33024)])
def test_ggml_op_form(env, D, H, HKV, T, n_past, n_kv):
    """kcpp_flash_attn_ext: q f32, an explicit f16 mask of 32 padded rows over n_kv keys padded to 256, every row's
    causal window past key 4100 / 32800.  D = 128: T = 5 runs k_fa_decode + k_fa_combine in the masked form (every
    chunk of n_kv: 68 and 516), T = 17 k_fa_prefill<128> under the mask; D = 64: k_fa_prefill<64>"""
    torch, K = env
    # D = 64 past 32768 keys: at the gain 0.7 a needle scores 0.7 * 64 / 8 = 5.6 and the four needles of the first and the
    # last region stay below 1 % of the 32800-key softmax; gain 1.0 gives the score D = 128 has at 0.7 (7.9)
    c = case(D, H, HKV, T, n_past, n_rows=n_kv, gain=1.0 if (D == 64 and n_past > 32768) else 0.7)
    _conditions(c, c["bar"])
    mask = causal_mask(T, n_past, n_kv, rows=32)
    qd = dev(torch, c["q"].astype(np.float32))
    kd, vd, md = dev(torch, c["k"]), dev(torch, c["v"]), dev(torch, mask)
    out = torch.full((T, H, D), float("nan"), dtype=torch.float32, device="cuda")
    ws = torch.zeros(K.fa_ext_workspace_bytes(T, H, n_kv, D), dtype=torch.uint8, device="cuda")
    rc = K.raw().kcpp_flash_attn_ext(qd.data_ptr(), H * D * 4, D * 4, kd.data_ptr(), vd.data_ptr(), md.data_ptr(), n_kv,
                                     out.data_ptr(), ws.data_ptr(), T, H, HKV, D, n_kv, float(1.0 / np.sqrt(D)),
                                     sptr(torch))
    assert rc == 0, rc
    kernel = "k_fa_prefill<64> masked" if D == 64 else ("k_fa_decode+k_fa_combine masked" if T <= 16 else
                                                         "k_fa_prefill<128> masked")
    _check(c, host(torch, out, np.float32), kernel, "T %d G %d" % (T, H // HKV))


# ---------------------------------------------------------------- 7: quantized caches (Q8_0 K, Q4_0 V)
@pytest.mark.parametrize("H,HKV,D", [(14, 2, 128), (8, 2, 64)])
@pytest.mark.parametrize("T,n_past", [(1, 4200), (70, 4090)])
def test_quantized_cache(env, H, HKV, D, T, n_past):
    """kcpp_flash_attn_q over caches filled by kcpp_kv_store_q, against R.flash_attn_q at test_flash_attn_q_vs_oracle's
    bar; the planted-key conditions on the float64 attention of the dequantized q (Q8_0), K and V.

    At 4160 keys R.flash_attn_q (the reference's loop: f32, one key after another) is itself 4.5e-6 max |want| from the
    float64 attention of the same inputs, above the 2e-6 bar, so the bar holds only for a kernel that sums in the
    reference's order: keys ascending, the row sum carried per key.  k_fa_q does; before it did,
    [70-4090-14-2-128] failed at 3.2e-6 max |want|.  Measured on an MI355X: 2.6e-7, 2.4e-7, 6.4e-7 and 4.0e-7 max |want|;
    kernel and oracle both 2.7e-6 to 5.9e-6 from float64 in the row metric."""
    torch, K = env
    tk, tv = R.Q8_0, R.Q4_0
    q16, k16, v16 = planted(31 * n_past + T + H + D, T, H, HKV, D, n_past, n_rows=n_past + T)
    n_keys, ekv, n_ctx = n_past + T, HKV * D, n_past + T + PAD_ROWS
    q = q16.astype(np.float32)
    kf, vf = k16.astype(np.float32).reshape(n_keys, ekv), v16.astype(np.float32).reshape(n_keys, ekv)
    kc, vc = store(torch, K, tk, tv, kf, vf, n_ctx, 0)
    kb, vb = soa_to_blocks(tk, kc, n_ctx, ekv)[:n_keys], soa_to_blocks(tv, vc, n_ctx, ekv)[:n_keys]
    assert np.array_equal(kb, np.stack([R.quantize(tk, r) for r in kf]))
    assert np.array_equal(vb, np.stack([R.quantize(tv, r) for r in vf]))
    want = R.flash_attn_q(q, kb, vb, tk, tv, causal_mask(T, n_past, n_keys))
    # float64 attention of what the kernel is given: q as Q8_0 (K's vec_dot_type), K and V dequantized
    qq = np.stack([R.dequant(R.Q8_0, R.quantize(R.Q8_0, r), D) for r in q.reshape(T * H, D)]).reshape(T, H, D)
    kq = np.stack([R.dequant(tk, r, ekv) for r in kb]).reshape(n_keys, HKV, D)
    vq = np.stack([R.dequant(tv, r, ekv) for r in vb]).reshape(n_keys, HKV, D)
    regs = regions(n_past + 1)
    ref, mass, drop = ref64(qq, kq, vq, n_past, regs)
    c = dict(ref=ref, mass=mass, drop=drop, regs=regs, n_keys=n_keys, e_orc=rel_err(want, ref))
    _conditions(c, 2e-6)
    got = attend(torch, K, tk, tv, q, kb, vb, n_ctx, n_past, dev_pos=(T == 1))
    d = np.abs(got - want).max()
    print("reach k_fa_q<%d> keys %d: e_orc %.3g err %.3g (vs oracle %.3g of max |want| %.3g) [T %d G %d]" %
          (D, n_keys, c["e_orc"], rel_err(got, ref), d, np.abs(want).max(), T, H // HKV))
    assert d <= 2e-6 * np.abs(want).max(), d
