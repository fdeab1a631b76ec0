"""The ggml backend plugin on the nodes of the Gemma-2 graph (reference src/llama.cpp build_gemma2, llm_build_kqv):
FLASH_ATTN_EXT at head dim 256 and with the logit soft-cap, UNARY GELU and TANH.

As tests/test_gpu_ggml_backend.py: the graphs are built by the reference ggml library (oracle/_ref/libggml_ref.so),
allocated in this backend's buffer type, computed through its vtable, and the same graph on the reference CPU backend
is the expected result (computed once per case and shared by the modes that are compared with it).

Bars.  GELU: bit-equal (the same f16 table, filled by the same libm).  TANH: the device tanhf against libm, 2 x the
measured maximum, never above 9.5e-7 (8 ulp at |y| <= 1).  Attention at D = 256, strict-parity mode without a cap:
bit-equal; with the cap (tanhf differs): 2 x the measured error, and below the production kernels' error of the same
case; production kernels: within 2 x the error of the unchanged D = 128 production path on the same case (same
arithmetic, the dot twice as long, the f16 P.V rounding independent of D).  A Gemma-2-shaped layer: LAYER_PROD."""
import ctypes
import os

import numpy as np
import pytest

import refharness as R

pytestmark = pytest.mark.gpu

REFLIB = os.path.join(R.ROOT, "oracle", "_ref", "libggml_ref.so")
P, I, I64, F, SZ = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t

LAYER_PROD = 2e-2                      # tests/test_gpu_ggml_backend.py: the production attention's layer bar
ATTN_NOFA = 7e-7                       # tests/test_gpu_ggml_backend.py: f32 attention on both sides, summation order only
# measured on the MI355X (printed by the tests below); every bar is 2 x its figure
TANH_MEASURED = 1.192e-7               # max |device tanhf - libm tanhf| over test 3's inputs (3,740 of 65,540 differ)
TANH_BAR = None if TANH_MEASURED is None else min(2 * TANH_MEASURED, 9.5e-7)
STRICT_CAP_MEASURED = 4.81e-4          # strict mode with cap 50: max over the cases of tests 4 / 5, relative to max |ref|
#                                        (8.9e-8 at 37 keys .. 4.8e-4 at 333: the f16 accumulator amplifies tanhf's ulps)
LAYER_STRICT_MEASURED = 6.55e-3        # the Gemma-2 layer in strict mode: max over its four cases (decode 1.6e-7, 33 tokens 6.5e-3)


class InitParams(ctypes.Structure):
    _fields_ = [("mem_size", SZ), ("mem_buffer", P), ("no_alloc", ctypes.c_bool)]


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    if not os.path.exists(REFLIB):
        pytest.skip("reference ggml build not shipped")
    import koboldcpp_amd.lib as K
    G = ctypes.CDLL(REFLIB)
    sigs = {"ggml_init": ([InitParams], P), "ggml_free": ([P], None),
            "ggml_new_tensor_1d": ([P, I, I64], P), "ggml_new_tensor_2d": ([P, I, I64, I64], P),
            "ggml_new_tensor_3d": ([P, I, I64, I64, I64], P),
            "ggml_mul_mat": ([P, P, P], P), "ggml_rms_norm": ([P, P, F], P), "ggml_mul": ([P, P, P], P),
            "ggml_add": ([P, P, P], P), "ggml_gelu": ([P, P], P), "ggml_tanh": ([P, P], P), "ggml_silu": ([P, P], P),
            "ggml_scale": ([P, P, F], P), "ggml_cpy": ([P, P, P], P), "ggml_soft_max_ext": ([P, P, P, F, F], P),
            "ggml_rope_ext": ([P, P, P, P, I, I, I, F, F, F, F, F, F], P),
            "ggml_flash_attn_ext": ([P, P, P, P, P, F, F, F], P), "ggml_flash_attn_ext_set_prec": ([P, I], None),
            "ggml_view_1d": ([P, P, I64, SZ], P), "ggml_view_2d": ([P, P, I64, I64, SZ, SZ], P),
            "ggml_cont_2d": ([P, P, I64, I64], P), "ggml_view_3d": ([P, P, I64, I64, I64, SZ, SZ, SZ], P),
            "ggml_reshape_2d": ([P, P, I64, I64], P), "ggml_reshape_3d": ([P, P, I64, I64, I64], P),
            "ggml_permute": ([P, P, I, I, I, I], P), "ggml_new_graph": ([P], P),
            "ggml_build_forward_expand": ([P, P], None), "ggml_graph_compute_with_ctx": ([P, P, I], I),
            "ggml_get_data": ([P], P), "ggml_nbytes": ([P], SZ),
            "ggml_graph_n_nodes": ([P], I), "ggml_graph_node": ([P, I], P),
            "ggml_backend_alloc_ctx_tensors": ([P, P], P), "ggml_backend_tensor_set": ([P, P, SZ, SZ], None),
            "ggml_backend_tensor_get": ([P, P, SZ, SZ], None), "ggml_backend_graph_compute": ([P, P], I),
            "ggml_backend_buffer_free": ([P], None), "ggml_backend_supports_op": ([P, P], ctypes.c_bool),
            "ggml_backend_free": ([P], None)}
    for n, (a, r) in sigs.items():
        fn = getattr(G, n)
        fn.argtypes, fn.restype = a, r
    G.ggml_init(InitParams(1 << 20, None, False))      # fp16 / GELU tables
    L = K.raw()
    L.ggml_backend_cuda_init.argtypes, L.ggml_backend_cuda_init.restype = [I], P
    L.kcpp_ggml_backend_last_error.restype = ctypes.c_char_p
    be = L.ggml_backend_cuda_init(0)
    assert be
    yield G, L, be
    G.ggml_backend_free(be)


def run_graph(env, build, data, on_gpu, exact=False, all_supported=False):
    """build(ctx) -> (input tensors, out tensor, nodes to expand before out); data: one array per input.  One run on
    this backend (strict-parity attention when exact) or on the reference CPU; the output as flat f32"""
    G, L, be = env
    ctx = G.ggml_init(InitParams(256 << 20, None, on_gpu))
    ins, out, pre = build(ctx)
    g = G.ggml_new_graph(ctx)
    for p_ in pre:
        G.ggml_build_forward_expand(g, p_)
    G.ggml_build_forward_expand(g, out)
    n_out = G.ggml_nbytes(out) // 4
    if on_gpu:
        if all_supported:
            for i in range(G.ggml_graph_n_nodes(g)):
                assert G.ggml_backend_supports_op(be, G.ggml_graph_node(g, i)), "node %d is not supported" % i
        buf = G.ggml_backend_alloc_ctx_tensors(ctx, be)
        assert buf
        for t, arr in zip(ins, data):
            a = np.ascontiguousarray(arr)
            assert a.nbytes == G.ggml_nbytes(t), (a.nbytes, G.ggml_nbytes(t))
            G.ggml_backend_tensor_set(t, a.ctypes.data, 0, a.nbytes)
        L.kcpp_ggml_backend_set_fa_exact(ctypes.c_void_p(be), int(exact))
        try:
            st = G.ggml_backend_graph_compute(be, g)
        finally:
            L.kcpp_ggml_backend_set_fa_exact(ctypes.c_void_p(be), 0)
        assert st == 0, L.kcpp_ggml_backend_last_error()
        res = np.empty(n_out, np.float32)
        G.ggml_backend_tensor_get(out, res.ctypes.data, 0, res.nbytes)
        G.ggml_backend_buffer_free(buf)
    else:
        for t, arr in zip(ins, data):
            a = np.ascontiguousarray(arr)
            assert a.nbytes == G.ggml_nbytes(t), (a.nbytes, G.ggml_nbytes(t))
            ctypes.memmove(G.ggml_get_data(t), a.ctypes.data, a.nbytes)
        assert G.ggml_graph_compute_with_ctx(ctx, g, 8) == 0
        res = np.ctypeslib.as_array((ctypes.c_float * n_out).from_address(G.ggml_get_data(out))).copy()
    G.ggml_free(ctx)
    return res


def rel(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def bits_differ(a, b):
    return int((a.view(np.uint32) != b.view(np.uint32)).sum())


def within(value, measured, what):
    """the bar 2 x the figure measured on the MI355X (a module constant above)"""
    print("%s: %.4g (recorded %s)" % (what, value, measured))
    assert measured is not None, "no recorded figure for %s: measured now %.4g" % (what, value)
    assert value <= 2 * measured, (what, value, measured)


# ---------------------------------------------------------------- 1. placement
def test_placement_of_gemma2_nodes(env):
    """supports_op: FLASH_ATTN_EXT at D = 256, the soft-cap at D = 128 / 256, UNARY GELU / TANH; still refused: another
    head dim, D = 64 with a cap, quantized K/V at D = 256, ALiBi"""
    G, L, be = env
    ctx = G.ggml_init(InitParams(4 << 20, None, True))

    def fa(D, cap=0.0, max_bias=0.0, kvt=R.F16, H=8, HKV=4, T=1, n_kv=256):
        q = G.ggml_permute(ctx, G.ggml_new_tensor_3d(ctx, R.F32, D, H, T), 0, 2, 1, 3)
        if kvt == R.F16:
            kc, vc = (G.ggml_new_tensor_1d(ctx, R.F16, n_kv * HKV * D) for _ in range(2))
            k, v = (G.ggml_view_3d(ctx, c, D, n_kv, HKV, HKV * D * 2, D * 2, 0) for c in (kc, vc))
        else:
            k, v = (G.ggml_new_tensor_3d(ctx, kvt, D, n_kv, HKV) for _ in range(2))
        m = G.ggml_new_tensor_2d(ctx, R.F16, n_kv, (T + 31) // 32 * 32)
        return G.ggml_backend_supports_op(be, G.ggml_flash_attn_ext(ctx, q, k, v, m, 1.0 / np.sqrt(D), max_bias, cap))
    assert fa(256) and fa(256, T=33)
    assert fa(128, cap=50.0) and fa(256, cap=50.0)
    assert fa(128) and fa(64)                      # as before
    x = G.ggml_new_tensor_2d(ctx, R.F32, 96, 3)
    assert G.ggml_backend_supports_op(be, G.ggml_gelu(ctx, x))
    assert G.ggml_backend_supports_op(be, G.ggml_tanh(ctx, x))
    assert not fa(80)
    assert not fa(64, cap=50.0)
    assert not fa(256, kvt=R.Q8_0)
    assert not fa(128, cap=50.0, kvt=R.Q8_0)
    assert fa(128, kvt=R.Q8_0)                     # as before
    assert not fa(256, max_bias=8.0) and not fa(128, max_bias=8.0)
    G.ggml_free(ctx)


# ---------------------------------------------------------------- 2. GELU
def _unary_both(env, fn, x, view=None):
    """fn(ctx, X) (or of a row-strided view of X) on this backend and on the reference CPU"""
    G = env[0]

    def build(ctx):
        X = G.ggml_new_tensor_2d(ctx, R.F32, x.shape[1], x.shape[0])
        src = X if view is None else G.ggml_view_2d(ctx, X, view[0], x.shape[0], x.shape[1] * 4, view[1] * 4)
        return [X], getattr(G, fn)(ctx, src), []
    return run_graph(env, build, [x], True, all_supported=True), run_graph(env, build, [x], False)


def test_gelu_bit_equal_to_reference_cpu(env):
    """ggml_vec_gelu_f32's table form (ggml.c:2564-2578): every finite f16 value widened to f32; f32 values that are
    not f16-representable (rounded to the table index) with the +-10 switch points and +-0; a row-strided source"""
    codes = np.arange(1 << 16, dtype=np.uint16)
    allf16 = codes.view(np.float16)
    allf16 = allf16[np.isfinite(allf16)].astype(np.float32)
    assert allf16.size == 63488
    ours, ref = _unary_both(env, "ggml_gelu", allf16.reshape(1, -1))
    assert bits_differ(ours, ref) == 0, "%d of %d finite f16 inputs differ" % (bits_differ(ours, ref), ours.size)
    rng = np.random.default_rng(5)
    x = rng.uniform(-12, 12, 8192).astype(np.float32)
    x = x[x.astype(np.float16).astype(np.float32) != x][:4096]
    assert x.size == 4096
    x = np.concatenate([x, np.float32([0.0, -0.0, 10.0, -10.0])])
    ours, ref = _unary_both(env, "ggml_gelu", x.reshape(1, -1))
    assert bits_differ(ours, ref) == 0, "%d of %d f32 inputs differ" % (bits_differ(ours, ref), ours.size)
    assert ours[-2] == 10.0 and ours[-1] == 0.0
    xs = rng.uniform(-11, 11, (3, 128)).astype(np.float32)
    ours, ref = _unary_both(env, "ggml_gelu", xs, view=(96, 16))
    assert ours.size == 3 * 96 and bits_differ(ours, ref) == 0


# ---------------------------------------------------------------- 3. TANH
def test_tanh_vs_reference_cpu(env):
    """the device tanhf against libm's: not bit-equal, both a few ulp.  Measured on the MI355X: max |d| 1.192e-7 (two f32
    ulp below 1) over 65,536 values in (-9, 9), so the bar is 2.384e-7 (the cap of 9.5e-7 does not bind)"""
    rng = np.random.default_rng(6)
    x = np.concatenate([rng.uniform(-9, 9, 65536).astype(np.float32), np.float32([0.0, -0.0, 20.0, -20.0])])
    ours, ref = _unary_both(env, "ggml_tanh", x.reshape(1, -1))
    d = float(np.abs(ours.astype(np.float64) - ref).max())
    print("tanh: max |d| %.4g over %d values, %d differ in any bit" % (d, x.size, bits_differ(ours, ref)))
    assert np.array_equal(ours[-4:], ref[-4:])        # +-0 and the saturated ends
    assert TANH_BAR is not None, "no recorded figure: measured now %.4g" % d
    assert d <= TANH_BAR, (d, TANH_BAR)


# ---------------------------------------------------------------- 4. / 5. the FLASH_ATTN_EXT node
def fa_inputs(D, H, HKV, T, n_past, window, seed):
    """q ~ N(0,1) [T][H][D]; K / V caches padded to a multiple of 256 rows, the padding NaN and masked -inf; the mask
    f16 [PAD(T, 32)][n_kv]: causal, or a sliding window of `window` keys (whole leading key tiles and whole decode
    splits dead); every query row keeps at least one live key"""
    live = n_past + T
    n_kv = (live + 255) // 256 * 256
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((T, H, D)).astype(np.float32)
    kc = (rng.standard_normal((n_kv, HKV * D)) * 0.5).astype(np.float16)
    vc = rng.standard_normal((n_kv, HKV * D)).astype(np.float16)
    kc[live:] = np.nan
    vc[live:] = np.nan
    mask = np.full(((T + 31) // 32 * 32, n_kv), -np.inf, np.float16)
    for t in range(T):
        pos = n_past + t
        mask[t, (max(0, pos - window + 1) if window else 0):pos + 1] = 0
    return n_kv, [q, kc, vc, mask]


def fa_build(G, D, H, HKV, T, n_kv, cap):
    def build(ctx):
        Q = G.ggml_new_tensor_3d(ctx, R.F32, D, H, T)
        KC, VC = (G.ggml_new_tensor_1d(ctx, R.F16, n_kv * HKV * D) for _ in range(2))
        Mk = G.ggml_new_tensor_2d(ctx, R.F16, n_kv, (T + 31) // 32 * 32)
        k, v = (G.ggml_view_3d(ctx, c, D, n_kv, HKV, HKV * D * 2, D * 2, 0) for c in (KC, VC))
        fa = G.ggml_flash_attn_ext(ctx, G.ggml_permute(ctx, Q, 0, 2, 1, 3), k, v, Mk, 1.0 / np.sqrt(D), 0.0, cap)
        return [Q, KC, VC, Mk], fa, []
    return build


_fa_cache = {}


def fa_errors(env, D, H, HKV, T, n_past, window, cap, seed):
    """(production error, strict error, differing bits in strict mode) of the node against the reference CPU, per
    (case, D, cap) computed once"""
    key = (D, H, HKV, T, n_past, window, cap, seed)
    if key not in _fa_cache:
        n_kv, data = fa_inputs(D, H, HKV, T, n_past, window, seed)
        build = fa_build(env[0], D, H, HKV, T, n_kv, cap)
        ref = run_graph(env, build, data, False)
        assert np.isfinite(ref).all()
        prod = run_graph(env, build, data, True, all_supported=True)
        strict = run_graph(env, build, data, True, exact=True)
        assert np.isfinite(prod).all(), "%d production outputs are not finite" % (~np.isfinite(prod)).sum()
        assert np.isfinite(strict).all(), "%d strict outputs are not finite" % (~np.isfinite(strict)).sum()
        _fa_cache[key] = (rel(prod, ref), rel(strict, ref), bits_differ(strict, ref))
    return _fa_cache[key]


# (H, HKV, T, n_past, window (0 = causal), cap)
FA256_CASES = (
    [(8, 4, 1, n - 1, 0, 0.0) for n in (1, 37, 256, 701)]       # 701 keys cross the strict kernel's 512-key chunk
    + [(8, 4, 1, 36, 0, 50.0), (8, 4, 1, 700, 0, 50.0), (8, 4, 1, 700, 16, 0.0),
       (2, 2, 1, 700, 0, 0.0), (8, 2, 1, 700, 0, 50.0), (8, 1, 1, 700, 0, 0.0), (8, 1, 1, 36, 0, 50.0)]
    + [(8, 4, T, 300, w, 0.0) for T in (5, 33, 65) for w in (0, 16)]
    + [(8, 4, 33, 300, 0, 50.0), (8, 4, 5, 300, 16, 50.0), (8, 4, 65, 300, 16, 50.0),
       (2, 2, 33, 300, 0, 0.0), (8, 2, 65, 300, 16, 50.0), (8, 1, 5, 300, 0, 50.0), (8, 1, 33, 300, 16, 0.0),
       (8, 2, 5, 300, 16, 0.0)])


def _check_fa(env, D, case):
    H, HKV, T, n_past, window, cap = case
    seed = 1000 + 7 * H + HKV + 13 * T + n_past + window
    prod, strict, nbits = fa_errors(env, D, H, HKV, T, n_past, window, cap, seed)
    # the yardstick: the same case at D = 128 without a cap through the production path this work leaves unchanged
    base, _, _ = fa_errors(env, 128, H, HKV, T, n_past, window, 0.0, seed)
    print("FA D=%d %s: production %.4g (D = 128 production %.4g), strict %.4g, %d strict outputs differ in a bit" % (
        D, case, prod, base, strict, nbits))
    assert prod <= 2 * base, (prod, base)
    if cap == 0.0:
        assert nbits == 0, "strict mode: %d outputs differ from the reference, rel err %.3g" % (nbits, strict)
    else:
        assert strict < prod, (strict, prod)      # only tanhf differs: far below the production kernels' f32 / f16 gap
        within(strict, STRICT_CAP_MEASURED, "strict mode with the cap")


@pytest.mark.parametrize("case", FA256_CASES, ids=lambda c: "H%d_HKV%d_T%d_past%d_w%d_cap%g" % c)
def test_flash_attn_d256_vs_reference_cpu(env, case):
    """the node at head dim 256: one query on the split decode pair (1, 37, 256, 701 keys), 5 queries on the same pair
    per query, 33 and 65 on the MFMA tile kernel (a second tile of queries), causal and 16-key-window masks 300 keys
    into the cache, GQA ratios 1, 2, 4, 8, with and without the cap; the strict-parity kernel on the same inputs"""
    _check_fa(env, 256, case)


FA128_CAP_CASES = [(8, 4, 1, 700, 0, 50.0), (8, 4, 5, 300, 0, 50.0), (8, 4, 33, 300, 0, 50.0), (8, 2, 33, 300, 16, 50.0)]


@pytest.mark.parametrize("case", FA128_CAP_CASES, ids=lambda c: "H%d_HKV%d_T%d_past%d_w%d_cap%g" % c)
def test_flash_attn_d128_softcap_vs_reference_cpu(env, case):
    """the cap on the D = 128 paths: k_fa_dec5<GRAPH> (one query), k_fa_decode (5), the masked k_fa_prefill (33), and
    the strict kernel"""
    _check_fa(env, 128, case)


@pytest.mark.parametrize("T,n_past", [(1, 700), (5, 300), (33, 300)])
def test_softcap_entry_points_without_a_cap_are_the_old_ones(env, T, n_past):
    """kcpp_flash_attn_ext_sc / _dec_sc / _exact_sc with cap 0 at D = 128: bitwise the old entry points' output"""
    import torch
    import koboldcpp_amd.lib as K
    D, H, HKV = 128, 8, 4
    n_kv, (q, kc, vc, mask) = fa_inputs(D, H, HKV, T, n_past, 0, 77)
    qd = torch.from_numpy(q).cuda()
    kd, vd, md = (torch.from_numpy(a.view(np.int16)).cuda() for a in (kc, vc, mask))     # the f16 bytes
    ws = torch.zeros(K.fa_ext_workspace_bytes(T, H, n_kv, D), dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    scale = float(1.0 / np.sqrt(D))

    def run(name, *args):
        out = torch.full((T, H, D), float("nan"), device="cuda")
        K.call(name, *[out.data_ptr() if a is Ellipsis else a for a in args])
        torch.cuda.synchronize()
        return out.cpu().numpy()
    common = (qd.data_ptr(), H * D * 4, D * 4, kd.data_ptr(), vd.data_ptr(), md.data_ptr(), n_kv)
    old = run("kcpp_flash_attn_ext", *common, ..., ws.data_ptr(), T, H, HKV, D, n_kv, scale, st)
    new = run("kcpp_flash_attn_ext_sc", *common, ..., ws.data_ptr(), T, H, HKV, D, n_kv, scale, st, 0.0)
    assert np.isfinite(old).all() and bits_differ(old, new) == 0
    old = run("kcpp_flash_attn_ext_exact", *common, ..., T, H, HKV, D, n_kv, scale, st)
    new = run("kcpp_flash_attn_ext_exact_sc", *common, ..., T, H, HKV, D, n_kv, scale, st, 0.0)
    assert np.isfinite(old).all() and bits_differ(old, new) == 0
    if T == 1:
        L = K.raw()
        L.kcpp_flash_attn_ext_dec.argtypes = [P, I64, P, P, I64, I64, P, P, P, I, I, I, I, F, P]
        dec = (qd.data_ptr(), D * 4, kd.data_ptr(), vd.data_ptr(), HKV * D, D, md.data_ptr())
        old = run("kcpp_flash_attn_ext_dec", *dec, ..., ws.data_ptr(), H, HKV, D, n_kv, scale, st)
        new = run("kcpp_flash_attn_ext_dec_sc", *dec, ..., ws.data_ptr(), H, HKV, D, n_kv, scale, st, 0.0)
        assert np.isfinite(old).all() and bits_differ(old, new) == 0


# ---------------------------------------------------------------- 6. a Gemma-2-shaped layer
_layer_ref = {}


@pytest.mark.parametrize("exact", [False, True], ids=["production", "strict"])
@pytest.mark.parametrize("T,n_past,window", [(1, 700, 0), (1, 700, 16), (33, 300, 0), (33, 300, 16)],
                         ids=["decode_global", "decode_window16", "prefill_global", "prefill_window16"])
def test_gemma2_layer_vs_reference_cpu(env, T, n_past, window, exact):
    """one build_gemma2 layer (src/llama.cpp:13700-13784) with flash attention on: RMS_NORM . w, q / k / v MUL_MAT, NeoX
    ROPE, the Q SCALE, CPY into the F16 cache, FLASH_ATTN_EXT with cap 50 over the padded cache view, wo, post-norm,
    ADD, ffn norm, gate MUL_MAT, GELU, up MUL_MAT, MUL, down, post-norm, ADD.  n_embd 512, 4 / 2 heads x 256 (so
    H * D != n_embd), n_ff 1024, Q4_K weights with Q6_K v and down"""
    G, L, be = env
    E, H, HKV, D, Fd = 512, 4, 2, 256, 1024
    EKV, live = HKV * D, n_past + T
    n_kv = (live + 255) // 256 * 256
    n_ctx = n_kv
    rng = np.random.default_rng(21 + T + window)
    tys = [R.Q4_K, R.Q4_K, R.Q6_K, R.Q4_K, R.Q4_K, R.Q4_K, R.Q6_K]
    shapes = [(E, H * D), (E, EKV), (E, EKV), (H * D, E), (E, Fd), (E, Fd), (Fd, E)]
    ws = [R.synth(t, 9, 500 + i, k, n) for i, (t, (k, n)) in enumerate(zip(tys, shapes))]
    norms = [(1 + 0.05 * rng.standard_normal(E)).astype(np.float32) for _ in range(4)]
    x = rng.standard_normal((T, E)).astype(np.float32)
    kc = (rng.standard_normal((n_ctx, EKV)) * 0.5).astype(np.float16)
    vc = rng.standard_normal((n_ctx, EKV)).astype(np.float16)
    kc[live:] = np.nan
    vc[live:] = np.nan
    pos = np.arange(n_past, live, dtype=np.int32)
    mask = np.full((32 * ((T + 31) // 32), n_kv), -np.inf, np.float16)
    for t in range(T):
        p = n_past + t
        mask[t, (max(0, p - window + 1) if window else 0):p + 1] = 0

    def build(ctx):
        W = [G.ggml_new_tensor_2d(ctx, t, k, n) for t, (k, n) in zip(tys, shapes)]
        N = [G.ggml_new_tensor_1d(ctx, R.F32, E) for _ in range(4)]
        X = G.ggml_new_tensor_2d(ctx, R.F32, E, T)
        KC, VC = G.ggml_new_tensor_1d(ctx, R.F16, n_ctx * EKV), G.ggml_new_tensor_1d(ctx, R.F16, n_ctx * EKV)
        Pz = G.ggml_new_tensor_1d(ctx, 26, T)
        Mk = G.ggml_new_tensor_2d(ctx, R.F16, n_kv, mask.shape[0])
        rope = lambda t_, nh: G.ggml_rope_ext(ctx, G.ggml_reshape_3d(ctx, t_, D, nh, T), Pz, None, D, 2, n_ctx, 10000.0,
                                              1.0, 0.0, 1.0, 32.0, 1.0)
        cur = G.ggml_mul(ctx, G.ggml_rms_norm(ctx, X, 1e-6), N[0])
        qc, kcur, vcur = (G.ggml_mul_mat(ctx, W[i], cur) for i in range(3))
        q = G.ggml_scale(ctx, rope(qc, H), 1.0 / np.sqrt(D))
        k = rope(kcur, HKV)
        st_k = G.ggml_cpy(ctx, k, G.ggml_view_1d(ctx, KC, T * EKV, n_past * EKV * 2))
        st_v = G.ggml_cpy(ctx, vcur, G.ggml_view_1d(ctx, VC, T * EKV, n_past * EKV * 2))
        kview, vview = (G.ggml_view_3d(ctx, c, D, n_kv, HKV, EKV * 2, D * 2, 0) for c in (KC, VC))
        fa = G.ggml_flash_attn_ext(ctx, G.ggml_permute(ctx, q, 0, 2, 1, 3), kview, vview, Mk, 1.0, 0.0, 50.0)
        G.ggml_flash_attn_ext_set_prec(fa, 1)            # GGML_PREC_F32, as llm_build_kqv asks for Gemma-2
        att = G.ggml_mul_mat(ctx, W[3], G.ggml_reshape_2d(ctx, fa, H * D, T))
        att = G.ggml_mul(ctx, G.ggml_rms_norm(ctx, att, 1e-6), N[1])
        sa_out = G.ggml_add(ctx, att, X)
        h = G.ggml_mul(ctx, G.ggml_rms_norm(ctx, sa_out, 1e-6), N[2])
        h = G.ggml_mul(ctx, G.ggml_gelu(ctx, G.ggml_mul_mat(ctx, W[4], h)), G.ggml_mul_mat(ctx, W[5], h))
        h = G.ggml_mul(ctx, G.ggml_rms_norm(ctx, G.ggml_mul_mat(ctx, W[6], h), 1e-6), N[3])
        return W + N + [X, KC, VC, Pz, Mk], G.ggml_add(ctx, h, sa_out), [st_k, st_v]
    data = ws + norms + [x, kc, vc, pos, mask]
    key = (T, n_past, window)
    if key not in _layer_ref:
        _layer_ref[key] = run_graph(env, build, data, False)
    ref = _layer_ref[key]
    assert np.isfinite(ref).all()
    ours = run_graph(env, build, data, True, exact=exact, all_supported=True)
    assert np.isfinite(ours).all()
    e = rel(ours, ref)
    print("gemma-2 layer %s exact=%d: rel err max %.4g" % (key, exact, e))
    assert e <= LAYER_PROD, e
    if exact:
        within(e, LAYER_STRICT_MEASURED, "gemma-2 layer in strict mode")
        assert 2 * LAYER_STRICT_MEASURED <= LAYER_PROD


# ---------------------------------------------------------------- 7. the non-flash form
@pytest.mark.parametrize("case", [(8, 4, 256, 1, 41, 64, 64), (8, 4, 256, 33, 31, 64, 96)],
                         ids=lambda c: "H%d_HKV%d_D%d_T%d_past%d_kv%d_ctx%d" % c)
def test_attention_without_flash_attn_softcap_vs_reference_cpu(env, case):
    """llm_build_kqv's else branch for Gemma-2 (src/llama.cpp:9578-9627): K . Q MUL_MAT, SCALE(1/50), TANH, SCALE(50),
    SOFT_MAX under the F32 mask, MUL_MAT with the transposed V cache view, permute + cont_2d; q arrives pre-scaled"""
    G, L, be = env
    H, HKV, D, T, n_past, n_kv, n_ctx = case
    EKV = HKV * D
    rng = np.random.default_rng(H + D + T)
    q = (rng.standard_normal((T, H, D)) / np.sqrt(D)).astype(np.float32)
    kc = (rng.standard_normal((n_ctx, EKV)) * 0.5).astype(np.float16)
    vc = rng.standard_normal((EKV, n_ctx)).astype(np.float16)
    mask = np.full(((T + 31) // 32 * 32, n_kv), -np.inf, np.float32)
    for t in range(T):
        mask[t, :n_past + t + 1] = 0
    mask[T - 1, 1] = -np.inf

    def build(ctx):
        Q = G.ggml_new_tensor_3d(ctx, R.F32, D, H, T)
        KC, VC = G.ggml_new_tensor_1d(ctx, R.F16, n_ctx * EKV), G.ggml_new_tensor_1d(ctx, R.F16, n_ctx * EKV)
        Mk = G.ggml_new_tensor_2d(ctx, R.F32, n_kv, mask.shape[0])
        k = G.ggml_view_3d(ctx, KC, D, n_kv, HKV, EKV * 2, D * 2, 0)
        kq = G.ggml_mul_mat(ctx, k, G.ggml_permute(ctx, Q, 0, 2, 1, 3))
        kq = G.ggml_scale(ctx, G.ggml_tanh(ctx, G.ggml_scale(ctx, kq, 1.0 / 50.0)), 50.0)
        kq = G.ggml_soft_max_ext(ctx, kq, Mk, 1.0, 0.0)
        v = G.ggml_view_3d(ctx, VC, n_kv, D, HKV, n_ctx * 2, n_ctx * D * 2, 0)
        kqv = G.ggml_mul_mat(ctx, v, kq)
        return [Q, KC, VC, Mk], G.ggml_cont_2d(ctx, G.ggml_permute(ctx, kqv, 0, 2, 1, 3), D * H, T), []
    data = [q, kc, vc, mask]
    ref = run_graph(env, build, data, False)
    ours = run_graph(env, build, data, True, all_supported=True)
    assert np.isfinite(ref).all() and np.isfinite(ours).all()
    e = rel(ours, ref)
    print("attention without flash attention, soft-cap %s: rel err max %.4g" % (case, e))
    assert e <= ATTN_NOFA, e


# ---------------------------------------------------------------- 8. the final logit cap
def test_final_logit_softcap_vs_reference_cpu(env):
    """build_gemma2's SCALE(1/30), TANH, SCALE(30) over the logits [n_vocab 1000, 3 tokens]: test 3's bar x 30"""
    G = env[0]
    x = (np.random.default_rng(8).standard_normal((3, 1000)) * 20).astype(np.float32)

    def build(ctx):
        X = G.ggml_new_tensor_2d(ctx, R.F32, 1000, 3)
        return [X], G.ggml_scale(ctx, G.ggml_tanh(ctx, G.ggml_scale(ctx, X, 1.0 / 30.0)), 30.0), []
    ours, ref = run_graph(env, build, [x], True, all_supported=True), run_graph(env, build, [x], False)
    d = float(np.abs(ours.astype(np.float64) - ref).max())
    print("final logit cap: max |d| %.4g" % d)
    assert TANH_BAR is not None, "no recorded figure: measured now %.4g" % d
    assert d <= 30 * TANH_BAR, (d, 30 * TANH_BAR)
