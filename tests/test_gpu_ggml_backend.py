"""The ggml backend plugin (include/kcpp_ggml_backend.h, csrc/ggml_backend.cpp) driven by the REFERENCE host.

The graphs are built by the reference ggml library itself (oracle/_ref/libggml_ref.so: ggml.c graph builder,
ggml-alloc.c allocator, ggml-backend.cpp dispatch), allocated by ggml_backend_alloc_ctx_tensors in OUR buffer
type, filled by ggml_backend_tensor_set, computed by ggml_backend_graph_compute(our backend) and read back by
ggml_backend_tensor_get -- every call crossing the plugin boundary through the vtables, as llama.cpp would.  The
same graph computed by the reference CPU backend is the expected result.

Bars: quantized and F16 mat-mul: exact integer dots, fp32 combination order only -> max |d| <= 3e-6 x max |ref|.
Elementwise / norm / rope ops: 2e-6 relative.  A whole Llama layer (norm, q/k/v, rope, f16 KV-cache stores into
cache views, masked flash attention over the cache, wo, residual, norm, gate/up/silu, down, residual): 2e-5
with the strict-parity attention (kcpp_ggml_backend_set_fa_exact) while its inputs are bit-equal to the CPU run's
(its FA node is held bit-equal to the reference's on the same inputs at every length), 2e-2 with the production
one (the reference accumulates attention in f16, ggml.c:15788, this backend in f32).  The graph llama.cpp builds with
flash attention OFF (koboldcpp's default: mul_mat / soft_max_ext / mul_mat over the K view and the transposed V
cache, the transposed V store): the attention alone 7e-7, the whole layer 1.6e-6 (f32 attention on both sides)."""
import ctypes
import os

import numpy as np
import pytest

import refharness as R

pytestmark = pytest.mark.gpu

REFLIB = os.path.join(R.ROOT, "oracle", "_ref", "libggml_ref.so")
P, I, I64, F, SZ = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t


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
            "ggml_add": ([P, P, P], P), "ggml_silu": ([P, P], P), "ggml_scale": ([P, P, F], P),
            "ggml_get_rows": ([P, P, P], P), "ggml_cpy": ([P, P, P], P),
            "ggml_soft_max_ext": ([P, P, P, F, F], P),
            "ggml_rope_ext": ([P, P, P, P, I, I, I, F, F, F, F, F, F], P),
            "ggml_flash_attn_ext": ([P, P, P, P, P, F, F, F], P),
            "ggml_view_1d": ([P, P, I64, SZ], P), "ggml_view_2d": ([P, P, I64, I64, SZ, SZ], P),
            "ggml_transpose": ([P, P], P), "ggml_cont_2d": ([P, P, I64, I64], P), "ggml_view_3d": ([P, P, I64, I64, I64, SZ, SZ, SZ], P),
            "ggml_reshape_2d": ([P, P, I64, I64], P), "ggml_reshape_3d": ([P, P, I64, I64, I64], P),
            "ggml_permute": ([P, P, I, I, I, I], P), "ggml_new_graph": ([P], P),
            "ggml_build_forward_expand": ([P, P], None), "ggml_graph_compute_with_ctx": ([P, P, I], I),
            "ggml_get_data": ([P], P), "ggml_nbytes": ([P], SZ), "ggml_row_size": ([I, I64], SZ),
            "ggml_graph_n_nodes": ([P], I), "ggml_graph_node": ([P, I], P),
            "ggml_backend_alloc_ctx_tensors": ([P, P], P), "ggml_backend_tensor_set": ([P, P, SZ, SZ], None),
            "ggml_backend_tensor_get": ([P, P, SZ, SZ], None), "ggml_backend_graph_compute": ([P, P], I),
            "ggml_backend_buffer_free": ([P], None), "ggml_backend_buft_get_alignment": ([P], SZ),
            "ggml_backend_buft_get_alloc_size": ([P, P], SZ), "ggml_backend_buft_alloc_buffer": ([P, SZ], P),
            "ggml_backend_buffer_clear": ([P, ctypes.c_uint8], None), "ggml_backend_buffer_get_base": ([P], P),
            "ggml_backend_buffer_set_usage": ([P, I], None), "ggml_backend_tensor_alloc": ([P, P, P], None),
            "ggml_backend_supports_op": ([P, P], ctypes.c_bool), "ggml_backend_name": ([P], ctypes.c_char_p),
            "ggml_backend_dev_name": ([P], ctypes.c_char_p), "ggml_backend_get_device": ([P], P),
            "ggml_backend_dev_type": ([P], I), "ggml_backend_free": ([P], None),
            "ggml_backend_get_default_buffer_type": ([P], P)}
    for n, (a, r) in sigs.items():
        fn = getattr(G, n)
        fn.argtypes, fn.restype = a, r
    G.ggml_init(InitParams(1 << 20, None, False))      # fp16 tables
    L = K.raw()
    L.ggml_backend_cuda_init.argtypes, L.ggml_backend_cuda_init.restype = [I], P
    L.ggml_backend_cuda_buffer_type.argtypes, L.ggml_backend_cuda_buffer_type.restype = [I], P
    L.ggml_backend_cuda_reg.restype = P
    L.kcpp_ggml_backend_last_error.restype = ctypes.c_char_p
    be = L.ggml_backend_cuda_init(0)
    assert be
    yield G, L, be
    G.ggml_backend_free(be)


def run_both(G, be, build, inputs_fn, nthreads=8):
    """build(ctx) -> (inputs [(tensor, np.ndarray)], out tensor); returns (ours, reference CPU)"""
    outs = []
    for on_gpu in (True, False):
        ctx = G.ggml_init(InitParams(512 << 20, None, on_gpu))
        ins, out = build(ctx)
        g = G.ggml_new_graph(ctx)
        G.ggml_build_forward_expand(g, out)
        data = inputs_fn()
        if on_gpu:
            buf = G.ggml_backend_alloc_ctx_tensors(ctx, be)
            assert buf
            for t, arr in zip(ins, data):
                a = np.ascontiguousarray(arr)
                assert a.nbytes == G.ggml_nbytes(t)
                G.ggml_backend_tensor_set(t, a.ctypes.data, 0, a.nbytes)
            st = G.ggml_backend_graph_compute(be, g)
            assert st == 0, st
            res = np.empty(G.ggml_nbytes(out) // 4, np.float32)
            G.ggml_backend_tensor_get(out, res.ctypes.data, 0, res.nbytes)
            G.ggml_backend_buffer_free(buf)
        else:
            for t, arr in zip(ins, data):
                a = np.ascontiguousarray(arr)
                ctypes.memmove(G.ggml_get_data(t), a.ctypes.data, a.nbytes)
            assert G.ggml_graph_compute_with_ctx(ctx, g, nthreads) == 0
            res = np.ctypeslib.as_array((ctypes.c_float * (G.ggml_nbytes(out) // 4)).from_address(G.ggml_get_data(out))).copy()
        G.ggml_free(ctx)
        outs.append(res)
    return outs


# whole layer vs the reference CPU (relative to max |ref|): strict-parity attention reproduces the reference's
# f16-accumulating order, leaving only the fp32 combination order of the quantized dots (measured 6.2e-6 max,
# 3.6e-8 median); the production f32-accumulating attention differs by the reference's own f16 rounding
# (measured 7.0e-3 max, 1.2e-3 median)
LAYER_EXACT = 2e-5
LAYER_PROD = 2e-2


def rel(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def test_registry_device_and_buffer_rules(env):
    """ROCm registry / GPU_FULL device through the reference accessors; alignment 128; quantized rows padded to
    512 elements in get_alloc_size and the pad zeroed by init_tensor (not for compute buffers)
    (ggml-cuda.cu:443-461, 567-586)"""
    G, L, be = env
    assert G.ggml_backend_name(be) == b"ROCm0"
    dev = G.ggml_backend_get_device(be)
    assert G.ggml_backend_dev_name(dev) == b"ROCm0" and G.ggml_backend_dev_type(dev) == 3   # GPU_FULL
    buft = G.ggml_backend_get_default_buffer_type(be)
    assert buft == L.ggml_backend_cuda_buffer_type(0)
    assert G.ggml_backend_buft_get_alignment(buft) == 128
    ctx = G.ggml_init(InitParams(1 << 20, None, True))
    t = G.ggml_new_tensor_2d(ctx, R.Q4_K, 2304, 3)                # 9 super-blocks per row: 2304 % 512 = 256
    nb = G.ggml_nbytes(t)
    assert nb == 3 * 9 * 144
    assert G.ggml_backend_buft_get_alloc_size(buft, t) == nb + G.ggml_row_size(R.Q4_K, 256)
    f = G.ggml_new_tensor_2d(ctx, R.F32, 100, 3)
    assert G.ggml_backend_buft_get_alloc_size(buft, f) == G.ggml_nbytes(f)
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [P, P, SZ, I]
    for usage, zeroed in ((1, True), (2, False)):                 # WEIGHTS, COMPUTE
        buf = G.ggml_backend_buft_alloc_buffer(buft, 8192)
        G.ggml_backend_buffer_set_usage(buf, usage)
        G.ggml_backend_buffer_clear(buf, 0xFF)
        base = G.ggml_backend_buffer_get_base(buf)
        t = G.ggml_new_tensor_2d(ctx, R.Q4_K, 2304, 3)            # a fresh tensor: tensor_alloc asserts buffer == NULL
        G.ggml_backend_tensor_alloc(buf, t, base)
        host = np.empty(nb + 144, np.uint8)
        assert hip.hipMemcpy(host.ctypes.data, base, host.nbytes, 2) == 0
        assert np.all(host[:nb] == 0xFF)
        assert np.all(host[nb:] == 0) if zeroed else np.all(host[nb:] == 0xFF)
        G.ggml_backend_buffer_free(buf)
    G.ggml_free(ctx)


MM_CASES = [(R.Q4_K, 4096, 512, 1), (R.Q4_K, 4096, 384, 7), (R.Q4_K, 2048, 256, 40), (R.Q6_K, 4096, 256, 1),
            (R.Q6_K, 2048, 256, 33), (R.Q5_K, 4096, 256, 1), (R.Q5_K, 2048, 128, 20), (R.Q8_0, 4096, 256, 1),
            (R.Q8_0, 2048, 256, 24), (R.Q4_0, 4096, 256, 1), (R.Q4_0, 2048, 256, 40), (R.F16, 1024, 96, 5),
            (R.F16, 1024, 96, 1), (R.F16, 1024, 96, 2),
            (R.Q2_K, 4096, 256, 1), (R.Q2_K, 2048, 256, 24), (R.Q3_K, 4096, 256, 1), (R.Q3_K, 2048, 384, 40),
            (R.Q5_0, 4096, 256, 1), (R.Q5_0, 2048, 256, 24), (R.Q4_1, 4096, 256, 1), (R.Q4_1, 2048, 256, 24),
            (R.Q5_1, 4096, 256, 3), (R.Q5_1, 2048, 256, 40), (R.IQ4_NL, 4096, 256, 1), (R.IQ4_NL, 2048, 256, 24),
            (R.IQ4_XS, 4096, 256, 1), (R.IQ4_XS, 2048, 256, 40),
            (R.IQ2_XXS, 4096, 256, 1), (R.IQ2_XS, 2048, 256, 24), (R.IQ2_S, 4096, 256, 3), (R.IQ3_XXS, 2048, 256, 40),
            (R.IQ3_S, 4096, 256, 1), (R.IQ1_S, 2048, 256, 24), (R.IQ1_M, 4096, 256, 2)]


@pytest.mark.parametrize("case", MM_CASES, ids=lambda c: "t%d_%dx%d_m%d" % c)
def test_mul_mat_vs_reference_cpu(env, case):
    G, L, be = env
    t, Kd, N, M = case
    rng = np.random.default_rng(Kd + N + M + t)
    w = R.synth(t, 5, 100 + t, Kd, N) if t != R.F16 else (rng.standard_normal((N, Kd)) * 0.05).astype(np.float16)
    x = rng.standard_normal((M, Kd)).astype(np.float32)
    probe = t == R.F16 and M <= 2
    if probe:
        # F16 weights at one and two tokens: the reference rounds src1 to f16 at one token (vec_dot_f16: tinyBLAS
        # refuses n < 2, llamafile/sgemm.cpp:1033) and leaves it in f32 from two on (tinyBLAS); on these inputs the two
        # results lie more than 100 bars apart on every output, so the backend must pick the same route
        w, x, want_r, want_u = R.mm_rounding_probe(rng, M, Kd, N)
        assert np.abs(want_r - want_u).min() >= 100 * 3e-6 * max(np.abs(want_r).max(), np.abs(want_u).max())

    def build(ctx):
        W = G.ggml_new_tensor_2d(ctx, t, Kd, N)
        X = G.ggml_new_tensor_2d(ctx, R.F32, Kd, M)
        return [W, X], G.ggml_mul_mat(ctx, W, X)
    ours, ref = run_both(G, be, build, lambda: [w, x])
    if probe:
        assert rel(ref, (want_r if M == 1 else want_u).ravel()) <= 3e-6       # the route the reference took
    assert rel(ours, ref) <= 3e-6, rel(ours, ref)
    assert L.kcpp_ggml_backend_last_nodes() == 1


def test_elementwise_ops_vs_reference_cpu(env):
    """rms_norm * w + x, silu, scale, soft_max with an f16 mask, rope (NORM, base 500000) on a [128, 8, 6] view"""
    G, L, be = env
    rng = np.random.default_rng(3)
    x = rng.standard_normal((6, 1024)).astype(np.float32)
    w = (1 + 0.1 * rng.standard_normal(1024)).astype(np.float32)
    msk = np.where(rng.random((6, 1024)) < 0.2, -np.inf, 0).astype(np.float16)
    pos = np.arange(6, dtype=np.int32) * 37

    def build(ctx):
        X = G.ggml_new_tensor_2d(ctx, R.F32, 1024, 6)
        Wt = G.ggml_new_tensor_1d(ctx, R.F32, 1024)
        Mk = G.ggml_new_tensor_2d(ctx, R.F16, 1024, 6)
        Pz = G.ggml_new_tensor_1d(ctx, 26, 6)                     # I32
        h = G.ggml_add(ctx, G.ggml_mul(ctx, G.ggml_rms_norm(ctx, X, 1e-5), Wt), X)
        h = G.ggml_scale(ctx, G.ggml_silu(ctx, h), 0.5)
        h = G.ggml_soft_max_ext(ctx, h, Mk, 0.125, 0.0)
        r = G.ggml_rope_ext(ctx, G.ggml_reshape_3d(ctx, X, 128, 8, 6), Pz, None, 128, 0, 4096, 500000.0, 1.0, 0.0,
                            1.0, 32.0, 1.0)
        out = G.ggml_add(ctx, G.ggml_reshape_2d(ctx, r, 1024, 6), h)
        return [X, Wt, Mk, Pz], out
    ours, ref = run_both(G, be, build, lambda: [x, w, msk, pos])
    assert rel(ours, ref) <= 2e-6, rel(ours, ref)


@pytest.mark.parametrize("t", [R.Q4_K, R.Q6_K, R.Q8_0, R.Q4_0, R.Q5_0, R.Q2_K, R.Q3_K, R.Q4_1, R.Q5_1, R.IQ4_NL, R.IQ4_XS,
                               R.IQ2_XXS, R.IQ2_XS, R.IQ2_S, R.IQ3_XXS, R.IQ3_S, R.IQ1_S, R.IQ1_M, R.F16])
def test_get_rows_vs_reference_cpu(env, t):
    """token embedding gather (get_rows of a quantized or f16 table): dequantization is exact on both sides"""
    G, L, be = env
    Kd, N = 2048, 50
    rng = np.random.default_rng(t)
    tab = R.synth(t, 4, 40 + t, Kd, N) if t != R.F16 else rng.standard_normal((N, Kd)).astype(np.float16)
    ids = rng.integers(0, N, size=9).astype(np.int32)

    def build(ctx):
        Tb = G.ggml_new_tensor_2d(ctx, t, Kd, N)
        Ix = G.ggml_new_tensor_1d(ctx, 26, 9)
        return [Tb, Ix], G.ggml_get_rows(ctx, Tb, Ix)
    ours, ref = run_both(G, be, build, lambda: [tab, ids])
    assert np.array_equal(ours.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("exact,n_past,T,n_ctx,pad", [(True, 37, 5, 64, 0), (False, 37, 5, 64, 0), (False, 37, 1, 64, 0),
                                                     (True, 37, 1, 64, 0), (False, 700, 1, 1024, 256),
                                                     (True, 700, 1, 1024, 256)],
                         ids=["fa_exact", "production", "decode", "decode_exact", "decode_ctx700_pad256",
                              "decode_ctx700_exact"])
def test_llama_layer_vs_reference_cpu(env, exact, n_past, T, n_ctx, pad):
    """one build_llama layer (src/llama.cpp:10453-10620) at n_embd 1024, 8/2 heads x 128, n_ff 2816, Q4_K_M-like
    weights, 5 new tokens after 37 cached positions; and single tokens (decode: MUL_MAT on the fused mat-vec with its
    quantize prologue, FLASH_ATTN_EXT on the split decode kernel under the graph's mask), also with the KV view padded
    to 256 cells as llama_kv_cache does for flash attention (masked cells past n_past hold NaN, never read into V)"""
    G, L, be = env
    E, H, HKV, D, Fd = 1024, 8, 2, 128, 2816
    EKV = HKV * D
    n_kv = n_past + T if not pad else (n_past + T + pad - 1) // pad * pad
    rng = np.random.default_rng(11)
    tys = [R.Q4_K, R.Q4_K, R.Q6_K, R.Q4_K, R.Q4_K, R.Q4_K, R.Q6_K]
    shapes = [(E, E), (E, EKV), (E, EKV), (E, E), (E, Fd), (E, Fd), (Fd, E)]
    ws = [R.synth(t, 9, 300 + i, k, n) for i, (t, (k, n)) in enumerate(zip(tys, shapes))]
    nw1 = (1 + 0.05 * rng.standard_normal(E)).astype(np.float32)
    nw2 = (1 + 0.05 * rng.standard_normal(E)).astype(np.float32)
    x = rng.standard_normal((T, E)).astype(np.float32)
    kc = (rng.standard_normal((n_ctx, EKV)) * 0.5).astype(np.float16)
    vc = rng.standard_normal((n_ctx, EKV)).astype(np.float16)
    if pad:
        kc[n_past + T:] = np.nan
        vc[n_past + T:] = np.nan
    pos = np.arange(n_past, n_past + T, dtype=np.int32)
    T_pad = 32
    mask = np.full((T_pad, n_kv), -np.inf, np.float16)
    for t in range(T):
        mask[t, :n_past + t + 1] = 0

    def build(ctx):
        W = [G.ggml_new_tensor_2d(ctx, t, k, n) for t, (k, n) in zip(tys, shapes)]
        N1, N2 = G.ggml_new_tensor_1d(ctx, R.F32, E), G.ggml_new_tensor_1d(ctx, R.F32, E)
        X = G.ggml_new_tensor_2d(ctx, R.F32, E, T)
        KC, VC = G.ggml_new_tensor_1d(ctx, R.F16, n_ctx * EKV), G.ggml_new_tensor_1d(ctx, R.F16, n_ctx * EKV)
        Pz = G.ggml_new_tensor_1d(ctx, 26, T)
        Mk = G.ggml_new_tensor_2d(ctx, R.F16, n_kv, T_pad)
        cur = G.ggml_mul(ctx, G.ggml_rms_norm(ctx, X, 1e-5), N1)
        q = G.ggml_rope_ext(ctx, G.ggml_reshape_3d(ctx, G.ggml_mul_mat(ctx, W[0], cur), D, H, T), Pz, None, D, 0, n_ctx,
                            500000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
        k = G.ggml_rope_ext(ctx, G.ggml_reshape_3d(ctx, G.ggml_mul_mat(ctx, W[1], cur), D, HKV, T), Pz, None, D, 0, n_ctx,
                            500000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
        v = G.ggml_mul_mat(ctx, W[2], cur)
        kv = G.ggml_view_1d(ctx, KC, T * EKV, n_past * EKV * 2)
        vv = G.ggml_view_1d(ctx, VC, T * EKV, n_past * EKV * 2)
        st_k = G.ggml_cpy(ctx, k, kv)
        st_v = G.ggml_cpy(ctx, v, vv)
        kview = G.ggml_view_3d(ctx, KC, D, n_kv, HKV, EKV * 2, D * 2, 0)
        vview = G.ggml_view_3d(ctx, VC, D, n_kv, HKV, EKV * 2, D * 2, 0)
        fa = G.ggml_flash_attn_ext(ctx, G.ggml_permute(ctx, q, 0, 2, 1, 3), kview, vview, Mk, 1.0 / np.sqrt(D), 0.0, 0.0)
        att = G.ggml_mul_mat(ctx, W[3], G.ggml_reshape_2d(ctx, fa, E, T))
        ffn_in = G.ggml_add(ctx, att, X)
        h = G.ggml_mul(ctx, G.ggml_rms_norm(ctx, ffn_in, 1e-5), N2)
        h = G.ggml_mul(ctx, G.ggml_silu(ctx, G.ggml_mul_mat(ctx, W[4], h)), G.ggml_mul_mat(ctx, W[5], h))
        out = G.ggml_add(ctx, G.ggml_mul_mat(ctx, W[6], h), ffn_in)
        # the cache stores must precede attention (llm_build_kv: ggml_build_forward_expand of the cpy nodes first)
        build.pre = [st_k, st_v]
        build.keep = [q, KC, VC, fa]        # the attention node's inputs and output, read back in the strict mode
        return W + [N1, N2, X, KC, VC, Pz, Mk], out

    def inputs():
        return ws + [nw1, nw2, x, kc, vc, pos, mask]

    def fa_only_cpu(qv, kcb, vcb):
        """the reference CPU's ggml_flash_attn_ext alone, on the given q [T][H][D] f32 and cache bytes"""
        ctx = G.ggml_init(InitParams(64 << 20, None, False))
        Q = G.ggml_new_tensor_3d(ctx, R.F32, D, H, T)
        KC, VC = G.ggml_new_tensor_1d(ctx, R.F16, n_ctx * EKV), G.ggml_new_tensor_1d(ctx, R.F16, n_ctx * EKV)
        Mk = G.ggml_new_tensor_2d(ctx, R.F16, n_kv, T_pad)
        for t, a in ((Q, qv), (KC, kcb), (VC, vcb), (Mk, mask)):
            a = np.ascontiguousarray(a)
            assert a.nbytes == G.ggml_nbytes(t)
            ctypes.memmove(G.ggml_get_data(t), a.ctypes.data, a.nbytes)
        kview = G.ggml_view_3d(ctx, KC, D, n_kv, HKV, EKV * 2, D * 2, 0)
        vview = G.ggml_view_3d(ctx, VC, D, n_kv, HKV, EKV * 2, D * 2, 0)
        fa = G.ggml_flash_attn_ext(ctx, G.ggml_permute(ctx, Q, 0, 2, 1, 3), kview, vview, Mk, 1.0 / np.sqrt(D), 0.0, 0.0)
        g = G.ggml_new_graph(ctx)
        G.ggml_build_forward_expand(g, fa)
        assert G.ggml_graph_compute_with_ctx(ctx, g, 8) == 0
        res = np.ctypeslib.as_array((ctypes.c_float * (T * H * D)).from_address(G.ggml_get_data(fa))).copy()
        G.ggml_free(ctx)
        return res

    def grab(t, dtype, on_gpu):
        a = np.empty(G.ggml_nbytes(t) // np.dtype(dtype).itemsize, dtype)
        if on_gpu:
            G.ggml_backend_tensor_get(t, a.ctypes.data, 0, a.nbytes)
        else:
            ctypes.memmove(a.ctypes.data, G.ggml_get_data(t), a.nbytes)
        return a

    L.kcpp_ggml_backend_set_fa_exact(ctypes.c_void_p(be), int(exact))
    outs, kept = [], []
    for on_gpu in (True, False):
        ctx = G.ggml_init(InitParams(256 << 20, None, on_gpu))
        ins, out = build(ctx)
        g = G.ggml_new_graph(ctx)
        for p_ in build.pre:
            G.ggml_build_forward_expand(g, p_)
        G.ggml_build_forward_expand(g, out)
        if on_gpu:
            for i in range(G.ggml_graph_n_nodes(g)):
                assert G.ggml_backend_supports_op(be, G.ggml_graph_node(g, i))
            buf = G.ggml_backend_alloc_ctx_tensors(ctx, be)
            for t, a in zip(ins, inputs()):
                a = np.ascontiguousarray(a)
                G.ggml_backend_tensor_set(t, a.ctypes.data, 0, a.nbytes)
            assert G.ggml_backend_graph_compute(be, g) == 0, L.kcpp_ggml_backend_last_error()
            res = np.empty(T * E, np.float32)
            G.ggml_backend_tensor_get(out, res.ctypes.data, 0, res.nbytes)
            # (ggml_backend_alloc_ctx_tensors gives every tensor its own memory, and a fused launch writes every
            # node's output, the roped q included -- fuse_mv_rope -- so the readback needs no unfused run)
            if exact:
                kept.append([grab(t, dt, True) for t, dt in zip(build.keep, (np.float32, np.uint16, np.uint16, np.float32))])
            G.ggml_backend_buffer_free(buf)
        else:
            for t, a in zip(ins, inputs()):
                a = np.ascontiguousarray(a)
                ctypes.memmove(G.ggml_get_data(t), a.ctypes.data, a.nbytes)
            assert G.ggml_graph_compute_with_ctx(ctx, g, 8) == 0
            res = np.ctypeslib.as_array((ctypes.c_float * (T * E)).from_address(G.ggml_get_data(out))).copy()
            if exact:
                kept.append([grab(t, dt, False) for t, dt in zip(build.keep, (np.float32, np.uint16, np.uint16, np.float32))])
        G.ggml_free(ctx)
        outs.append(res)
    L.kcpp_ggml_backend_set_fa_exact(ctypes.c_void_p(be), 0)
    e = rel(outs[0], outs[1])
    med = float(np.median(np.abs(outs[0] - outs[1])) / np.abs(outs[1]).max())
    print("layer exact=%d rel err max %.3g median %.3g" % (exact, e, med))
    n_flipped = 0
    if exact:
        (q_g, kc_g, vc_g, fa_g), (q_c, kc_c, vc_c, fa_c) = kept
        # 1. the instrument: the strict kernel's FA node against the reference CPU's ggml_flash_attn_ext ALONE on the
        # GPU run's own q, cache bytes and mask -- the op-level bar of test_gpu_fa_exact.py (bit-equal up to an exp tie)
        fa_r = fa_only_cpu(q_g, kc_g, vc_g)
        n_bits = int((fa_g.view(np.uint32) != fa_r.view(np.uint32)).sum())
        print("FA node on the GPU run's inputs, %d keys: %d of %d outputs differ in any bit, max |d| %.3g" % (
            n_past + T, n_bits, fa_g.size, np.abs(fa_g - fa_r).max()))
        assert np.abs(fa_g - fa_r).max() <= np.spacing(np.abs(fa_r).max())
        # 2. the inputs: f16 codes of q (as attention rounds it) and of the new cache rows that differ between the runs
        rows = slice(n_past * EKV, (n_past + T) * EKV)
        flips = [int((q_g.astype(np.float16).view(np.uint16) != q_c.astype(np.float16).view(np.uint16)).sum()),
                 int((kc_g[rows] != kc_c[rows]).sum()), int((vc_g[rows] != vc_c[rows]).sum())]
        n_flipped = sum(flips)
        fa_e = rel(fa_g, fa_c)
        n_q8 = int((R.quantize(R.Q8_K, fa_g) != R.quantize(R.Q8_K, fa_c)).sum())      # wo's activation (vec_dot_type)
        print("attention inputs: %d f16 codes differ GPU vs CPU (q %d of %d, new K rows %d, new V rows %d of %d); "
              "FA node GPU vs CPU run rel err %.3g, %d bytes of its Q8_K image differ" % (
                  n_flipped, flips[0], q_g.size, flips[1], flips[2], T * EKV, fa_e, n_q8))
        # rows the graph does not store must be the uploaded bytes on both sides
        assert np.array_equal(kc_g[:rows.start], kc_c[:rows.start]) and np.array_equal(vc_g[:rows.start], vc_c[:rows.start])
    # What the 700-key case's 3.99e-3 max / 8.7e-4 median is (measured): NOT the kernel -- the FA node is bit-equal
    # to the reference CPU's on the same inputs at 38, 42 and 701 keys (0 differing bits, assertion 1.).  Its INPUTS
    # differ: q and the new K row reach attention through a quantized mat-mul and RoPE that agree with the CPU only to
    # ~3e-6, which flips f16 codes (2 at 701 keys: one in q, one in the new K row; 2 at 38 keys; 10 of 7680 at 42 keys,
    # 5 rows).  The strict order is chaotic in its inputs -- one f16 ulp of q moves every output of the head, by ~1e-3
    # of the head's maximum over 701 keys -- so the FA nodes of the two runs differ by 1.3e-4 ..
    # 3.9e-4, and wo's Q8_K rounding of that activation (a flipped code is 1/127 of its block's maximum) and the FFN's
    # two further activation roundings carry a difference of this class into the layer output, or do not: the same
    # two flips leave the 38-key layer at 2.5e-7.  So the 2e-5 layer bar is a statement about bit-equal attention
    # inputs: it holds whenever no code flipped, and below 100 keys as before; with flipped inputs assertion 1. carries
    # the exactness claim and LAYER_PROD stays the sanity bound.  (The strict mode is also pinned end to end at 3840
    # keys by test_gpu_deep.py.)
    assert e <= (LAYER_EXACT if exact and (n_past < 100 or n_flipped == 0) else LAYER_PROD), e


def test_unsupported_ops_are_refused(env):
    """placement: supports_op is false where this backend has no kernel (ggml-cuda.cu:2959-3185 decides placement;
    ggml_backend_sched then keeps such nodes on the CPU backend)"""
    G, L, be = env
    ctx = G.ggml_init(InitParams(1 << 20, None, True))
    w = G.ggml_new_tensor_2d(ctx, 15, 256, 4)                     # GGML_TYPE_Q8_K weights: no kernel here
    x = G.ggml_new_tensor_2d(ctx, R.F32, 256, 2)
    assert not G.ggml_backend_supports_op(be, G.ggml_mul_mat(ctx, w, x))
    w2 = G.ggml_new_tensor_2d(ctx, R.Q4_K, 256, 4)
    assert G.ggml_backend_supports_op(be, G.ggml_mul_mat(ctx, w2, x))
    G.ggml_free(ctx)


def _moe_sigs(G):
    for n, a in {"ggml_mul_mat_id": [P, P, P, P], "ggml_top_k": [P, P, I], "ggml_soft_max": [P, P],
                 "ggml_sum_rows": [P, P], "ggml_div": [P, P, P], "ggml_view_2d": [P, P, I64, I64, SZ, SZ]}.items():
        fn = getattr(G, n)
        fn.argtypes, fn.restype = a, P


MMID_CASES = [(R.Q4_K, 1), (R.Q4_K, 3), (R.Q4_K, 24), (R.Q5_K, 1), (R.Q5_K, 24), (R.Q6_K, 2), (R.Q6_K, 24),
              (R.Q8_0, 1), (R.Q8_0, 24), (R.Q4_0, 3), (R.Q2_K, 1), (R.Q3_K, 24), (R.Q4_1, 2), (R.Q5_1, 24),
              (R.IQ4_NL, 2), (R.IQ4_XS, 24), (R.IQ2_XXS, 1), (R.IQ2_S, 24), (R.IQ3_XXS, 3), (R.IQ1_M, 2)]


@pytest.mark.parametrize("case", MMID_CASES, ids=lambda c: "t%d_T%d" % c)
def test_mul_mat_id_vs_reference_cpu(env, case):
    """GGML_OP_MUL_MAT_ID (ggml_cuda_mul_mat_id, ggml-cuda.cu:2003-2139) with 8 experts, 2 used: src1 broadcast over
    the used slots (ne11 = 1, the up / gate form) and one column per slot (ne11 = 2, the down form); T <= 8 runs the
    device-routed expert mat-vecs, T = 24 the host-grouped GEMMs (one kcpp_gemm_grouped launch over all experts for
    Q4_K / Q5_K / Q6_K, one GEMM per expert for the other types)"""
    G, L, be = env
    _moe_sigs(G)
    t, T = case
    Kd, N, E, k = 1024, 512, 8, 2
    rng = np.random.default_rng(t * 100 + T)
    w = np.concatenate([R.synth(t, 6, 500 + e, Kd, N) for e in range(E)])
    ids = np.stack([rng.permutation(E)[:k] for _ in range(T)]).astype(np.int32)       # [T][k]
    for ne11 in (1, k):
        x = rng.standard_normal((T, ne11, Kd)).astype(np.float32)

        def build(ctx):
            W = G.ggml_new_tensor_3d(ctx, t, Kd, N, E)
            X = G.ggml_new_tensor_3d(ctx, R.F32, Kd, ne11, T)
            Ix = G.ggml_new_tensor_2d(ctx, 26, k, T)
            return [W, X, Ix], G.ggml_mul_mat_id(ctx, W, X, Ix)
        ours, ref = run_both(G, be, build, lambda: [w, x, ids])
        assert rel(ours, ref) <= 3e-6, (ne11, rel(ours, ref))


@pytest.mark.parametrize("T", [1, 5, 40])
def test_moe_ffn_graph_vs_reference_cpu(env, T):
    """llm_build_moe_ffn (src/llama.cpp:9416-9514) at Mixtral's shape ratios (n_embd 1024, n_ff 1536, 8 experts,
    top-2; Q5_K gate / up, Q6_K down, F32 router): router mul_mat, soft_max, top_k (argsort + view), get_rows of the
    probabilities, sum_rows + div normalisation, MUL_MAT_ID x 3, silu, mul, weighting, slot views summed --
    every node supported by this backend, the result equal to the reference CPU backend's"""
    G, L, be = env
    _moe_sigs(G)
    E_, Fd, NE, k = 1024, 1536, 8, 2
    rng = np.random.default_rng(T)
    router = (rng.standard_normal((NE, E_)) * 0.05).astype(np.float32)
    up = np.concatenate([R.synth(R.Q5_K, 7, 600 + e, E_, Fd) for e in range(NE)])
    gate = np.concatenate([R.synth(R.Q5_K, 7, 700 + e, E_, Fd) for e in range(NE)])
    down = np.concatenate([R.synth(R.Q6_K, 7, 800 + e, Fd, E_) for e in range(NE)])
    x = rng.standard_normal((T, E_)).astype(np.float32)

    def build(ctx):
        Rt = G.ggml_new_tensor_2d(ctx, R.F32, E_, NE)
        Up = G.ggml_new_tensor_3d(ctx, R.Q5_K, E_, Fd, NE)
        Gt = G.ggml_new_tensor_3d(ctx, R.Q5_K, E_, Fd, NE)
        Dn = G.ggml_new_tensor_3d(ctx, R.Q6_K, Fd, E_, NE)
        X = G.ggml_new_tensor_2d(ctx, R.F32, E_, T)
        logits = G.ggml_mul_mat(ctx, Rt, X)
        probs = G.ggml_soft_max(ctx, logits)
        sel = G.ggml_top_k(ctx, probs, k)
        wts = G.ggml_get_rows(ctx, G.ggml_reshape_3d(ctx, probs, 1, NE, T), sel)
        wts = G.ggml_reshape_2d(ctx, wts, k, T)
        wts = G.ggml_div(ctx, wts, G.ggml_sum_rows(ctx, wts))
        wts = G.ggml_reshape_3d(ctx, wts, 1, k, T)
        cur = G.ggml_reshape_3d(ctx, X, E_, 1, T)
        u = G.ggml_mul_mat_id(ctx, Up, cur, sel)
        g = G.ggml_silu(ctx, G.ggml_mul_mat_id(ctx, Gt, cur, sel))
        ex = G.ggml_mul(ctx, G.ggml_mul_mat_id(ctx, Dn, G.ggml_mul(ctx, u, g), sel), wts)
        nb1 = E_ * 4
        out = G.ggml_view_2d(ctx, ex, E_, T, nb1 * k, 0)
        for i in range(1, k):
            out = G.ggml_add(ctx, out, G.ggml_view_2d(ctx, ex, E_, T, nb1 * k, i * nb1))
        build.graph_out = out
        return [Rt, Up, Gt, Dn, X], out

    ctx = G.ggml_init(InitParams(64 << 20, None, True))
    _, out = build(ctx)
    g = G.ggml_new_graph(ctx)
    G.ggml_build_forward_expand(g, out)
    unsupported = [i for i in range(G.ggml_graph_n_nodes(g)) if not G.ggml_backend_supports_op(be, G.ggml_graph_node(g, i))]
    G.ggml_free(ctx)
    assert not unsupported, unsupported
    ours, ref = run_both(G, be, build, lambda: [router, up, gate, down, x])
    assert rel(ours, ref) <= 2e-5, rel(ours, ref)


LAYER_CASES = [  # (name, n_embd, H, HKV, D, kv type, weight type, strict attention)
    ("d64_f16_exact", 1024, 16, 4, 64, R.F16, R.Q4_0, True),
    ("d64_f16_prod", 1024, 16, 4, 64, R.F16, R.Q4_0, False),
    ("d128_kv_q8_0", 1024, 8, 2, 128, R.Q8_0, R.Q4_K, False),
    ("d128_kv_q4_0", 1024, 8, 2, 128, R.Q4_0, R.Q4_K, False),
    ("d64_kv_q8_0", 1024, 16, 4, 64, R.Q8_0, R.Q4_0, False),
]


@pytest.mark.parametrize("case", LAYER_CASES, ids=lambda c: c[0])
def test_llama_layer_variants_vs_reference_cpu(env, case):
    """one build_llama layer with 64-dim heads (TinyLlama class, BASELINE config 1) and with --quantkv caches (K / V
    stored by ggml_cpy into Q8_0 / Q4_0 cache views, attention over the quantized views, fattn.cu:210-218): every
    node supported by this backend, the output equal to the reference CPU backend's (F16 production attention: the
    reference's f16 accumulation bound, as the 128-dim layer test)"""
    G, L, be = env
    name, E, H, HKV, D, kvt, wt, exact = case
    Fd, n_ctx, n_past, T = 2816, 64, 37, 5
    EKV = HKV * D
    n_kv = n_past + T
    rng = np.random.default_rng(len(name))
    tys = [wt] * 7
    shapes = [(E, E), (E, EKV), (E, EKV), (E, E), (E, Fd), (E, Fd), (Fd, E)]
    ws = [R.synth(t, 9, 300 + i, k, n) for i, (t, (k, n)) in enumerate(zip(tys, shapes))]
    nw1 = (1 + 0.05 * rng.standard_normal(E)).astype(np.float32)
    nw2 = (1 + 0.05 * rng.standard_normal(E)).astype(np.float32)
    x = rng.standard_normal((T, E)).astype(np.float32)
    if kvt == R.F16:
        kc = (rng.standard_normal((n_ctx, EKV)) * 0.5).astype(np.float16)
        vc = rng.standard_normal((n_ctx, EKV)).astype(np.float16)
    else:
        kc, vc = R.synth(kvt, 3, 11, EKV, n_ctx), R.synth(kvt, 3, 12, EKV, n_ctx)
    pos = np.arange(n_past, n_past + T, dtype=np.int32)
    T_pad = 32
    mask = np.full((T_pad, n_kv), -np.inf, np.float16)
    for t in range(T):
        mask[t, :n_past + t + 1] = 0
    rs = G.ggml_row_size(kvt, EKV)

    def build(ctx):
        W = [G.ggml_new_tensor_2d(ctx, t, k, n) for t, (k, n) in zip(tys, shapes)]
        N1, N2 = G.ggml_new_tensor_1d(ctx, R.F32, E), G.ggml_new_tensor_1d(ctx, R.F32, E)
        X = G.ggml_new_tensor_2d(ctx, R.F32, E, T)
        KC, VC = G.ggml_new_tensor_1d(ctx, kvt, n_ctx * EKV), G.ggml_new_tensor_1d(ctx, kvt, n_ctx * EKV)
        Pz = G.ggml_new_tensor_1d(ctx, 26, T)
        Mk = G.ggml_new_tensor_2d(ctx, R.F16, n_kv, T_pad)
        cur = G.ggml_mul(ctx, G.ggml_rms_norm(ctx, X, 1e-5), N1)
        q = G.ggml_rope_ext(ctx, G.ggml_reshape_3d(ctx, G.ggml_mul_mat(ctx, W[0], cur), D, H, T), Pz, None, D, 0, n_ctx,
                            10000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
        k = G.ggml_rope_ext(ctx, G.ggml_reshape_3d(ctx, G.ggml_mul_mat(ctx, W[1], cur), D, HKV, T), Pz, None, D, 0, n_ctx,
                            10000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
        v = G.ggml_mul_mat(ctx, W[2], cur)
        st_k = G.ggml_cpy(ctx, k, G.ggml_view_1d(ctx, KC, T * EKV, n_past * rs))
        st_v = G.ggml_cpy(ctx, v, G.ggml_view_1d(ctx, VC, T * EKV, n_past * rs))
        kview = G.ggml_view_3d(ctx, KC, D, n_kv, HKV, rs, G.ggml_row_size(kvt, D), 0)
        vview = G.ggml_view_3d(ctx, VC, D, n_kv, HKV, rs, G.ggml_row_size(kvt, D), 0)
        fa = G.ggml_flash_attn_ext(ctx, G.ggml_permute(ctx, q, 0, 2, 1, 3), kview, vview, Mk, 1.0 / np.sqrt(D), 0.0, 0.0)
        att = G.ggml_mul_mat(ctx, W[3], G.ggml_reshape_2d(ctx, fa, E, T))
        ffn_in = G.ggml_add(ctx, att, X)
        h = G.ggml_mul(ctx, G.ggml_rms_norm(ctx, ffn_in, 1e-5), N2)
        h = G.ggml_mul(ctx, G.ggml_silu(ctx, G.ggml_mul_mat(ctx, W[4], h)), G.ggml_mul_mat(ctx, W[5], h))
        out = G.ggml_add(ctx, G.ggml_mul_mat(ctx, W[6], h), ffn_in)
        return W + [N1, N2, X, KC, VC, Pz, Mk], out, [st_k, st_v]

    L.kcpp_ggml_backend_set_fa_exact(ctypes.c_void_p(be), int(exact))
    outs = []
    for on_gpu in (True, False):
        ctx = G.ggml_init(InitParams(256 << 20, None, on_gpu))
        ins, out, pre = build(ctx)
        g = G.ggml_new_graph(ctx)
        for p_ in pre:
            G.ggml_build_forward_expand(g, p_)
        G.ggml_build_forward_expand(g, out)
        if on_gpu:
            bad = [i for i in range(G.ggml_graph_n_nodes(g)) if not G.ggml_backend_supports_op(be, G.ggml_graph_node(g, i))]
            assert not bad, bad
            buf = G.ggml_backend_alloc_ctx_tensors(ctx, be)
            for t, a in zip(ins, ws + [nw1, nw2, x, kc, vc, pos, mask]):
                a = np.ascontiguousarray(a)
                assert a.nbytes == G.ggml_nbytes(t)
                G.ggml_backend_tensor_set(t, a.ctypes.data, 0, a.nbytes)
            assert G.ggml_backend_graph_compute(be, g) == 0, L.kcpp_ggml_backend_last_error()
            res = np.empty(T * E, np.float32)
            G.ggml_backend_tensor_get(out, res.ctypes.data, 0, res.nbytes)
            G.ggml_backend_buffer_free(buf)
        else:
            for t, a in zip(ins, ws + [nw1, nw2, x, kc, vc, pos, mask]):
                a = np.ascontiguousarray(a)
                ctypes.memmove(G.ggml_get_data(t), a.ctypes.data, a.nbytes)
            assert G.ggml_graph_compute_with_ctx(ctx, g, 8) == 0
            res = np.ctypeslib.as_array((ctypes.c_float * (T * E)).from_address(G.ggml_get_data(out))).copy()
        G.ggml_free(ctx)
        outs.append(res)
    L.kcpp_ggml_backend_set_fa_exact(ctypes.c_void_p(be), 0)
    e = rel(outs[0], outs[1])
    print("%s rel err max %.3g" % (name, e))
    # F16 caches: the attention bounds as in the 128-dim test.  Quantized caches: the cache store turns a 1-ulp
    # difference of a k / v value (the q|k|v mat-mul's fp32 order) into a whole Q8_0 / Q4_0 quantum of that row
    # (measured up to 4.9e-3 here; the per-op tests below pin the store and the attention exactly)
    bar = LAYER_KVQ if kvt != R.F16 else (LAYER_EXACT if exact else LAYER_PROD)
    assert e <= bar, e


LAYER_KVQ = 1e-2


# ---- attention WITHOUT flash attention: koboldcpp's default (no --flashattention), llm_build_kqv's else branch
def nofa_attention(G, ctx, q_cur, KC, VC, Mk, H, HKV, D, T, n_kv, n_ctx):
    """llm_build_kqv without flash attention (src/llama.cpp:9543-9628) on q_cur f32 [D, H, T], the K cache f16
    [n_ctx][HKV * D] and the TRANSPOSED V cache f16 [HKV * D][n_ctx]: kqv_merged_cont f32 [D * H, T]"""
    EKV = HKV * D
    q = G.ggml_permute(ctx, q_cur, 0, 2, 1, 3)
    k = G.ggml_view_3d(ctx, KC, D, n_kv, HKV, EKV * 2, D * 2, 0)
    kq = G.ggml_mul_mat(ctx, k, q)
    kq = G.ggml_soft_max_ext(ctx, kq, Mk, 1.0 / np.sqrt(D), 0.0)
    v = G.ggml_view_3d(ctx, VC, n_kv, D, HKV, n_ctx * 2, n_ctx * D * 2, 0)
    kqv = G.ggml_mul_mat(ctx, v, kq)
    return G.ggml_cont_2d(ctx, G.ggml_permute(ctx, kqv, 0, 2, 1, 3), D * H, T)


def nofa_mask(T, n_past, n_kv):
    """llama.cpp's KQ_mask without flash attention (src/llama.cpp:10293, filled at :16660-16703): F32
    [n_kv, PAD(T, 32)], 0 inside the causal window, -inf elsewhere -- the cells from n_past + T to n_kv and every padded
    row included -- and one hole inside the last token's window"""
    mask = np.full(((T + 31) // 32 * 32, n_kv), -np.inf, np.float32)
    for t in range(T):
        mask[t, :n_past + t + 1] = 0
    mask[T - 1, 1] = -np.inf
    return mask


# attention sub-graph vs the reference CPU: both sides round q (and, at one token, the probabilities) to f16 alike and
# accumulate in f32, in different orders (measured 5.8e-8, 1.6e-7, 1.8e-7, 1.8e-7 over the four cases; before the mask
# row and the one-token rounding were put right: NaN in three of them)
ATTN_NOFA = 7e-7

ATTN_NOFA_CASES = [(8, 2, 128, 1, 41, 64, 64), (8, 2, 128, 5, 37, 64, 64), (16, 4, 64, 33, 0, 64, 96),
                   (4, 4, 128, 32, 10, 64, 64)]


@pytest.mark.parametrize("case", ATTN_NOFA_CASES, ids=lambda c: "H%d_HKV%d_D%d_T%d_past%d_kv%d_ctx%d" % c)
def test_attention_without_flash_attn_vs_reference_cpu(env, case):
    """the attention of the graph llama.cpp builds when flash attention is off: mul_mat of the K-cache view with the
    permuted q, soft_max_ext under the F32 mask padded to 32 rows, mul_mat of the transposed-V-cache view with the
    probabilities, permute + cont_2d.  One token (the padded mask rows must stay unread: ggml takes mask row
    flat_row % T, ggml.c:13965; and the probabilities are rounded to f16 as the reference's vec_dot_f16 route does),
    5 tokens with 4 q heads per K / V head, 33 tokens (a second block of 32 mask rows, D = 64, V's row stride n_ctx
    longer than n_kv) and exactly 32 tokens (the one count where the mask's row count and T coincide).  Cache cells no
    query may see hold ordinary finite values: reading one moves the result."""
    G, L, be = env
    H, HKV, D, T, n_past, n_kv, n_ctx = case
    EKV = HKV * D
    rng = np.random.default_rng(H + D + T)
    q = rng.standard_normal((T, H, D)).astype(np.float32)
    kc = (rng.standard_normal((n_ctx, EKV)) * 0.5).astype(np.float16)
    vc = rng.standard_normal((EKV, n_ctx)).astype(np.float16)
    mask = nofa_mask(T, n_past, n_kv)

    def build(ctx):
        Q = G.ggml_new_tensor_3d(ctx, R.F32, D, H, T)
        KC, VC = G.ggml_new_tensor_1d(ctx, R.F16, n_ctx * EKV), G.ggml_new_tensor_1d(ctx, R.F16, n_ctx * EKV)
        Mk = G.ggml_new_tensor_2d(ctx, R.F32, n_kv, mask.shape[0])
        return [Q, KC, VC, Mk], nofa_attention(G, ctx, Q, KC, VC, Mk, H, HKV, D, T, n_kv, n_ctx)
    ours, ref = run_both(G, be, build, lambda: [q, kc, vc, mask])
    assert np.isfinite(ref).all()
    e = rel(ours, ref)
    print("attention without flash attention %s: rel err max %.3g" % (case, e))
    assert np.isfinite(ours).all(), "%d of %d outputs are not finite" % ((~np.isfinite(ours)).sum(), ours.size)
    assert e <= ATTN_NOFA, e


# whole layer without flash attention vs the reference CPU: the attention is f32 on both sides here, so only the fp32
# combination order of the quantized dots remains, well inside LAYER_EXACT (measured 4.0e-7, 1.3e-7, 2.3e-7 over the
# three cases; 0.36, 0.13, 0.26 before the fixes).  The T stored V columns, as f32, against the reference's: the v
# mat-mul's one-ulp f32 differences move an f16 code here and there (measured 2.0e-6, 2.2e-6, 6.4e-5: one code of 1280,
# 256 and 256 differs, by one f16 ulp)
LAYER_NOFA = 1.6e-6
VSTORE_NOFA = 2.5e-4

# (the third case: one token on a weight layout whose mat-vec fuses the cache store -- a transposed single-token v is
# contiguous by ggml's rule, its strided destination is not, so the V store must run as a plain CPY)
LAYER_NOFA_CASES = [("nofa_d128", 1024, 8, 2, 128, R.Q4_K, 5, 37), ("nofa_d64_decode", 1024, 16, 4, 64, R.Q4_0, 1, 41),
                    ("nofa_d128_decode", 1024, 8, 2, 128, R.Q4_K, 1, 41)]


@pytest.mark.parametrize("case", LAYER_NOFA_CASES, ids=lambda c: c[0])
def test_llama_layer_without_flash_attn_vs_reference_cpu(env, case):
    """one build_llama layer as llama.cpp builds it with flash attention off: K stored through ggml_view_1d, V stored
    TRANSPOSED (llm_build_kv_store: cpy(transpose(v_cur), view_2d(v_cache, T, n_embd_v_gqa, n_ctx * 2, kv_head * 2))),
    attention from mul_mat / soft_max_ext / mul_mat / permute / cont_2d nodes.  Every node supported by this backend,
    the output equal to the reference CPU backend's; the V cache afterwards holds the T new columns and, everywhere
    else, the uploaded bytes."""
    G, L, be = env
    name, E, H, HKV, D, wt, T, n_past = case
    Fd, n_ctx, n_kv = 2816, 64, 64
    EKV = HKV * D
    rng = np.random.default_rng(len(name))
    shapes = [(E, E), (E, EKV), (E, EKV), (E, E), (E, Fd), (E, Fd), (Fd, E)]
    ws = [R.synth(wt, 9, 300 + i, k, n) for i, (k, n) in enumerate(shapes)]
    nw1 = (1 + 0.05 * rng.standard_normal(E)).astype(np.float32)
    nw2 = (1 + 0.05 * rng.standard_normal(E)).astype(np.float32)
    x = rng.standard_normal((T, E)).astype(np.float32)
    kc = (rng.standard_normal((n_ctx, EKV)) * 0.5).astype(np.float16)
    vc = rng.standard_normal((EKV, n_ctx)).astype(np.float16)
    pos = np.arange(n_past, n_past + T, dtype=np.int32)
    mask = nofa_mask(T, n_past, n_kv)
    data = ws + [nw1, nw2, x, kc, vc, pos, mask]

    def build(ctx):
        W = [G.ggml_new_tensor_2d(ctx, wt, k, n) for k, n in shapes]
        N1, N2 = G.ggml_new_tensor_1d(ctx, R.F32, E), G.ggml_new_tensor_1d(ctx, R.F32, E)
        X = G.ggml_new_tensor_2d(ctx, R.F32, E, T)
        KC, VC = G.ggml_new_tensor_1d(ctx, R.F16, n_ctx * EKV), G.ggml_new_tensor_1d(ctx, R.F16, n_ctx * EKV)
        Pz = G.ggml_new_tensor_1d(ctx, 26, T)
        Mk = G.ggml_new_tensor_2d(ctx, R.F32, n_kv, mask.shape[0])
        cur = G.ggml_mul(ctx, G.ggml_rms_norm(ctx, X, 1e-5), N1)
        q = G.ggml_rope_ext(ctx, G.ggml_reshape_3d(ctx, G.ggml_mul_mat(ctx, W[0], cur), D, H, T), Pz, None, D, 0, n_ctx,
                            10000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
        k = G.ggml_rope_ext(ctx, G.ggml_reshape_3d(ctx, G.ggml_mul_mat(ctx, W[1], cur), D, HKV, T), Pz, None, D, 0, n_ctx,
                            10000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
        v = G.ggml_mul_mat(ctx, W[2], cur)
        st_k = G.ggml_cpy(ctx, k, G.ggml_view_1d(ctx, KC, T * EKV, n_past * EKV * 2))
        st_v = G.ggml_cpy(ctx, G.ggml_transpose(ctx, v), G.ggml_view_2d(ctx, VC, T, EKV, n_ctx * 2, n_past * 2))
        att = nofa_attention(G, ctx, q, KC, VC, Mk, H, HKV, D, T, n_kv, n_ctx)
        att = G.ggml_mul_mat(ctx, W[3], att)
        ffn_in = G.ggml_add(ctx, att, X)
        h = G.ggml_mul(ctx, G.ggml_rms_norm(ctx, ffn_in, 1e-5), N2)
        h = G.ggml_mul(ctx, G.ggml_silu(ctx, G.ggml_mul_mat(ctx, W[4], h)), G.ggml_mul_mat(ctx, W[5], h))
        out = G.ggml_add(ctx, G.ggml_mul_mat(ctx, W[6], h), ffn_in)
        return W + [N1, N2, X, KC, VC, Pz, Mk], out, [st_k, st_v], VC

    outs, vcs = [], []
    for on_gpu in (True, False):
        ctx = G.ggml_init(InitParams(256 << 20, None, on_gpu))
        ins, out, pre, VC = build(ctx)
        g = G.ggml_new_graph(ctx)
        for p_ in pre:      # the cache stores precede attention (llm_build_kv expands the cpy nodes first)
            G.ggml_build_forward_expand(g, p_)
        G.ggml_build_forward_expand(g, out)
        res, vres = np.empty(T * E, np.float32), np.empty((EKV, n_ctx), np.float16)
        if on_gpu:
            bad = [i for i in range(G.ggml_graph_n_nodes(g)) if not G.ggml_backend_supports_op(be, G.ggml_graph_node(g, i))]
            assert not bad, bad
            buf = G.ggml_backend_alloc_ctx_tensors(ctx, be)
            for t, a in zip(ins, data):
                a = np.ascontiguousarray(a)
                assert a.nbytes == G.ggml_nbytes(t)
                G.ggml_backend_tensor_set(t, a.ctypes.data, 0, a.nbytes)
            assert G.ggml_backend_graph_compute(be, g) == 0, L.kcpp_ggml_backend_last_error()
            G.ggml_backend_tensor_get(out, res.ctypes.data, 0, res.nbytes)
            G.ggml_backend_tensor_get(VC, vres.ctypes.data, 0, vres.nbytes)
            G.ggml_backend_buffer_free(buf)
        else:
            for t, a in zip(ins, data):
                a = np.ascontiguousarray(a)
                ctypes.memmove(G.ggml_get_data(t), a.ctypes.data, a.nbytes)
            assert G.ggml_graph_compute_with_ctx(ctx, g, 8) == 0
            ctypes.memmove(res.ctypes.data, G.ggml_get_data(out), res.nbytes)
            ctypes.memmove(vres.ctypes.data, G.ggml_get_data(VC), vres.nbytes)
        G.ggml_free(ctx)
        outs.append(res)
        vcs.append(vres)
    cols = slice(n_past, n_past + T)
    for vres in vcs:        # every byte outside the T new columns is the uploaded one, on both sides
        kept = vres.copy()
        kept[:, cols] = vc[:, cols]
        assert np.array_equal(kept.view(np.uint16), vc.view(np.uint16))
    assert not np.array_equal(vcs[1][:, cols].view(np.uint16), vc[:, cols].view(np.uint16))   # the store happened
    ev = rel(vcs[0][:, cols].astype(np.float32), vcs[1][:, cols].astype(np.float32))
    n_codes = int((vcs[0][:, cols].view(np.uint16) != vcs[1][:, cols].view(np.uint16)).sum())
    e = rel(outs[0], outs[1])
    print("%s rel err max %.3g; stored V columns rel err max %.3g, %d of %d f16 codes differ" % (name, e, ev, n_codes,
                                                                                              T * EKV))
    assert ev <= VSTORE_NOFA, ev
    assert e <= LAYER_NOFA, e


@pytest.mark.parametrize("kvt", [R.Q8_0, R.Q4_0])
def test_cpy_f32_to_quantized_cache_vs_reference_cpu(env, kvt):
    """the --quantkv cache store (ggml_cpy f32 -> Q8_0 / Q4_0 view of the cache, quantize_row_q8_0 AVX2 /
    quantize_row_q4_0_ref): the same bytes as the reference CPU's, including zero blocks and rounding ties"""
    G, L, be = env
    n_ctx, EKV, T, off = 16, 1024, 5, 7
    rng = np.random.default_rng(kvt)
    x = rng.standard_normal((T, EKV)).astype(np.float32)
    x[0, :32] = 0.0                                               # an all-zero block
    x[1, :32] = np.arange(32) - 15.5                              # exact .5 ties after scaling
    cache = R.synth(kvt, 2, 5, EKV, n_ctx)
    rs = G.ggml_row_size(kvt, EKV)

    def build(ctx):
        X = G.ggml_new_tensor_2d(ctx, R.F32, EKV, T)
        C = G.ggml_new_tensor_1d(ctx, kvt, n_ctx * EKV)
        st = G.ggml_cpy(ctx, X, G.ggml_view_1d(ctx, C, T * EKV, off * rs))
        build.cache = C
        return [X, C], st
    outs = []
    for on_gpu in (True, False):
        ctx = G.ggml_init(InitParams(16 << 20, None, on_gpu))
        ins, st = build(ctx)
        g = G.ggml_new_graph(ctx)
        G.ggml_build_forward_expand(g, st)
        res = np.empty(n_ctx * rs, np.uint8)
        if on_gpu:
            assert G.ggml_backend_supports_op(be, G.ggml_graph_node(g, 0))
            buf = G.ggml_backend_alloc_ctx_tensors(ctx, be)
            for t, a in zip(ins, [x, cache]):
                G.ggml_backend_tensor_set(t, np.ascontiguousarray(a).ctypes.data, 0, a.nbytes)
            assert G.ggml_backend_graph_compute(be, g) == 0, L.kcpp_ggml_backend_last_error()
            G.ggml_backend_tensor_get(build.cache, res.ctypes.data, 0, res.nbytes)
            G.ggml_backend_buffer_free(buf)
        else:
            for t, a in zip(ins, [x, cache]):
                ctypes.memmove(G.ggml_get_data(t), np.ascontiguousarray(a).ctypes.data, a.nbytes)
            assert G.ggml_graph_compute_with_ctx(ctx, g, 4) == 0
            ctypes.memmove(res.ctypes.data, G.ggml_get_data(build.cache), res.nbytes)
        G.ggml_free(ctx)
        outs.append(res)
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("case", [(128, R.Q8_0, R.Q8_0, 1), (128, R.Q4_0, R.Q4_0, 7), (128, R.Q8_0, R.Q4_0, 3),
                                  (64, R.Q8_0, R.Q8_0, 5), (64, R.Q4_0, R.Q8_0, 1)], ids=lambda c: "d%d_k%d_v%d_T%d" % c)
def test_flash_attn_quantized_views_vs_reference_cpu(env, case):
    """GGML_OP_FLASH_ATTN_EXT over Q8_0 / Q4_0 K and V cache views (fattn.cu:210-218) on identical inputs: q quantized
    to Q8_0, exact integer block dots, V dequantized and accumulated in f32 as the reference CPU does"""
    G, L, be = env
    D, tk, tv, T = case
    H, HKV, n_ctx, n_kv = 8, 2, 96, 70
    EKV = HKV * D
    rng = np.random.default_rng(D + T)
    q = rng.standard_normal((T, H, D)).astype(np.float32)
    kc, vc = R.synth(tk, 4, 21, EKV, n_ctx), R.synth(tv, 4, 22, EKV, n_ctx)
    T_pad = 32
    mask = np.full((T_pad, n_kv), -np.inf, np.float16)
    for t in range(T):
        mask[t, :n_kv - T + t + 1] = 0
    mask[0, 3] = -np.inf                                          # a hole inside the window

    def build(ctx):
        Q = G.ggml_new_tensor_3d(ctx, R.F32, D, H, T)
        KC, VC = G.ggml_new_tensor_1d(ctx, tk, n_ctx * EKV), G.ggml_new_tensor_1d(ctx, tv, n_ctx * EKV)
        Mk = G.ggml_new_tensor_2d(ctx, R.F16, n_kv, T_pad)
        kv = G.ggml_view_3d(ctx, KC, D, n_kv, HKV, G.ggml_row_size(tk, EKV), G.ggml_row_size(tk, D), 0)
        vv = G.ggml_view_3d(ctx, VC, D, n_kv, HKV, G.ggml_row_size(tv, EKV), G.ggml_row_size(tv, D), 0)
        fa = G.ggml_flash_attn_ext(ctx, G.ggml_permute(ctx, Q, 0, 2, 1, 3), kv, vv, Mk, 1.0 / np.sqrt(D), 0.0, 0.0)
        return [Q, KC, VC, Mk], fa
    ours, ref = run_both(G, be, build, lambda: [q, kc, vc, mask])
    assert rel(ours, ref) <= 2e-6, rel(ours, ref)


@pytest.mark.parametrize("t", [R.Q4_K, R.Q6_K, R.Q8_0, R.Q4_0, R.Q5_K])
def test_weight_buffer_holds_one_copy(env, t):
    """weights in a buffer marked WEIGHTS (llama.cpp's model buffers, src/llama.cpp:8982) are converted to the
    device layout in place: no separate image is allocated, the mat-mul equals the reference CPU before and after,
    and reading the tensor back through the buffer interface returns the original ggml bytes (the layout is restored
    first); a later write is honoured"""
    G, L, be = env
    L.kcpp_ggml_backend_image_bytes.restype = I64
    Kd, N, M = 2048, 384, 3
    rng = np.random.default_rng(t)
    w = R.synth(t, 8, 70 + t, Kd, N)
    w2 = R.synth(t, 8, 71 + t, Kd, N)
    x = rng.standard_normal((M, Kd)).astype(np.float32)
    ctx_w = G.ggml_init(InitParams(1 << 20, None, True))
    W = G.ggml_new_tensor_2d(ctx_w, t, Kd, N)
    bw = G.ggml_backend_alloc_ctx_tensors(ctx_w, be)
    G.ggml_backend_buffer_set_usage(bw, 1)                         # GGML_BACKEND_BUFFER_USAGE_WEIGHTS
    G.ggml_backend_tensor_set(W, w.ctypes.data, 0, w.nbytes)
    base = L.kcpp_ggml_backend_image_bytes()

    def run(wbytes):
        ctx = G.ggml_init(InitParams(1 << 20, None, True))
        X = G.ggml_new_tensor_2d(ctx, R.F32, Kd, M)
        out = G.ggml_mul_mat(ctx, W, X)
        g = G.ggml_new_graph(ctx)
        G.ggml_build_forward_expand(g, out)
        bx = G.ggml_backend_alloc_ctx_tensors(ctx, be)
        G.ggml_backend_tensor_set(X, x.ctypes.data, 0, x.nbytes)
        assert G.ggml_backend_graph_compute(be, g) == 0, L.kcpp_ggml_backend_last_error()
        res = np.empty(M * N, np.float32)
        G.ggml_backend_tensor_get(out, res.ctypes.data, 0, res.nbytes)
        G.ggml_backend_buffer_free(bx)
        G.ggml_free(ctx)
        # the reference CPU on the same bytes
        cctx = G.ggml_init(InitParams(64 << 20, None, False))
        Wc = G.ggml_new_tensor_2d(cctx, t, Kd, N)
        Xc = G.ggml_new_tensor_2d(cctx, R.F32, Kd, M)
        oc = G.ggml_mul_mat(cctx, Wc, Xc)
        gc = G.ggml_new_graph(cctx)
        G.ggml_build_forward_expand(gc, oc)
        ctypes.memmove(G.ggml_get_data(Wc), wbytes.ctypes.data, wbytes.nbytes)
        ctypes.memmove(G.ggml_get_data(Xc), x.ctypes.data, x.nbytes)
        assert G.ggml_graph_compute_with_ctx(cctx, gc, 4) == 0
        ref = np.ctypeslib.as_array((ctypes.c_float * (M * N)).from_address(G.ggml_get_data(oc))).copy()
        G.ggml_free(cctx)
        return res, ref
    for _ in range(2):
        ours, ref = run(w)
        assert rel(ours, ref) <= 3e-6
        assert L.kcpp_ggml_backend_image_bytes() == base           # no second copy of the weight
    back = np.empty_like(w)
    G.ggml_backend_tensor_get(W, back.ctypes.data, 0, back.nbytes)
    assert np.array_equal(back, w)
    G.ggml_backend_tensor_set(W, w2.ctypes.data, 0, w2.nbytes)
    ours, ref = run(w2)
    assert rel(ours, ref) <= 3e-6
    G.ggml_backend_buffer_free(bw)
    G.ggml_free(ctx_w)


@pytest.mark.parametrize("case", [(R.Q4_K, 4096, 1024, 1), (R.Q6_K, 4096, 768, 5), (R.Q4_0, 2048, 640, 24),
                                  (R.Q8_0, 2048, 512, 40), (R.Q4_K, 2048, 1280, 33)], ids=lambda c: "t%d_%dx%d_m%d" % c)
def test_split_buffer_mul_mat_vs_reference_cpu(env, case, monkeypatch):
    """ggml_backend_cuda_split_buffer_type (ggml-cuda.cu:625-955, llama.cpp's --rowsplit buffers): the weight's rows
    spread over 3 lanes by tensor_split 1:2:1 (KCPP_VIRTUAL_DEVICES=3 puts the lanes on the one test GPU), each slice
    held in the device layout; MUL_MAT on the main device's backend with peer copies of the activation and of the
    result rows equals the reference CPU; the weight reads back byte-exact; only MUL_MAT may read a split tensor"""
    G, L, be = env
    monkeypatch.setenv("KCPP_VIRTUAL_DEVICES", "3")
    t, Kd, N, M = case
    for n, a in {"ggml_backend_alloc_ctx_tensors_from_buft": ([P, P], P)}.items():
        fn = getattr(G, n)
        fn.argtypes, fn.restype = a
    L.ggml_backend_cuda_split_buffer_type.argtypes, L.ggml_backend_cuda_split_buffer_type.restype = [P], P
    ts = (ctypes.c_float * 16)(1.0, 2.0, 1.0)
    sbt = L.ggml_backend_cuda_split_buffer_type(ts)
    assert sbt
    rng = np.random.default_rng(N + M)
    w = R.synth(t, 12, 90 + t, Kd, N)
    x = rng.standard_normal((M, Kd)).astype(np.float32)
    ctx_w = G.ggml_init(InitParams(1 << 20, None, True))
    W = G.ggml_new_tensor_2d(ctx_w, t, Kd, N)
    bw = G.ggml_backend_alloc_ctx_tensors_from_buft(ctx_w, sbt)
    assert bw
    G.ggml_backend_tensor_set(W, w.ctypes.data, 0, w.nbytes)
    back = np.empty_like(w)
    G.ggml_backend_tensor_get(W, back.ctypes.data, 0, back.nbytes)
    assert np.array_equal(back, w)
    ctx = G.ggml_init(InitParams(1 << 20, None, True))
    X = G.ggml_new_tensor_2d(ctx, R.F32, Kd, M)
    out = G.ggml_mul_mat(ctx, W, X)
    assert G.ggml_backend_supports_op(be, out)
    Ix = G.ggml_new_tensor_1d(ctx, 26, 2)
    assert not G.ggml_backend_supports_op(be, G.ggml_get_rows(ctx, W, Ix))
    g = G.ggml_new_graph(ctx)
    G.ggml_build_forward_expand(g, out)
    bx = G.ggml_backend_alloc_ctx_tensors(ctx, be)
    G.ggml_backend_tensor_set(X, x.ctypes.data, 0, x.nbytes)
    assert G.ggml_backend_graph_compute(be, g) == 0, L.kcpp_ggml_backend_last_error()
    ours = np.empty(M * N, np.float32)
    G.ggml_backend_tensor_get(out, ours.ctypes.data, 0, ours.nbytes)
    G.ggml_backend_buffer_free(bx)
    G.ggml_free(ctx)
    G.ggml_backend_buffer_free(bw)
    G.ggml_free(ctx_w)
    cctx = G.ggml_init(InitParams(64 << 20, None, False))
    Wc = G.ggml_new_tensor_2d(cctx, t, Kd, N)
    Xc = G.ggml_new_tensor_2d(cctx, R.F32, Kd, M)
    oc = G.ggml_mul_mat(cctx, Wc, Xc)
    gc = G.ggml_new_graph(cctx)
    G.ggml_build_forward_expand(gc, oc)
    ctypes.memmove(G.ggml_get_data(Wc), w.ctypes.data, w.nbytes)
    ctypes.memmove(G.ggml_get_data(Xc), x.ctypes.data, x.nbytes)
    assert G.ggml_graph_compute_with_ctx(cctx, gc, 4) == 0
    ref = np.ctypeslib.as_array((ctypes.c_float * (M * N)).from_address(G.ggml_get_data(oc))).copy()
    G.ggml_free(cctx)
    assert rel(ours, ref) <= 3e-6, rel(ours, ref)


FUSION_CASES = [("q4k_q6k", R.Q4_K, R.Q6_K, "ctx"), ("q4k_q6k_gallocr", R.Q4_K, R.Q6_K, "gallocr"),
                ("q8_0", R.Q8_0, R.Q8_0, "ctx"), ("q5k_gallocr", R.Q5_K, R.Q5_K, "gallocr")]


@pytest.mark.parametrize("case", FUSION_CASES, ids=lambda c: c[0])
def test_decode_node_fusion_matches_node_by_node(env, case):
    """the plugin's decode node fusion (ggml_backend.cpp fuse_at: RMS_NORM+MUL, MUL_MAT+ADD, the SiLU GLU quadruple,
    MUL_MAT + ROPE, ROPE / MUL_MAT + CPY into the F16 cache)
    against the same graph run node by node (kcpp_ggml_backend_set_fusion(be, 0)) on one token of a build_llama
    layer: bit for bit on the layer output, and -- each tensor in its own allocation (ggml_backend_alloc_ctx_tensors)
    -- on EVERY node's output, the fused launches writing the intermediate nodes' tensors too.  Allocated by
    ggml_gallocr (ggml-alloc.c, the allocator llama.cpp's scheduler uses) the intermediates share bytes in place, which
    the fusion must leave as the node sequence does.  The mat-vec fusions need an RS layout (Q4_K / Q5_K / Q6_K): the
    Q8_0 case fuses the norms only."""
    G, L, be = env
    name, wt, wdown, alloc = case
    for n, (a, r) in {"ggml_gallocr_new": ([P], P), "ggml_gallocr_alloc_graph": ([P, P], ctypes.c_bool),
                      "ggml_gallocr_free": ([P], None), "ggml_set_input": ([P], None),
                      "ggml_set_output": ([P], None)}.items():
        fn = getattr(G, n)
        fn.argtypes, fn.restype = a, r
    L.kcpp_ggml_backend_set_fusion.argtypes = [P, I]
    E, H, HKV, D, Fd, n_ctx, n_past, T = 1024, 8, 2, 128, 2816, 64, 37, 1
    EKV, n_kv = HKV * D, n_past + T
    rng = np.random.default_rng(5)
    tys = [wt] * 6 + [wdown]
    shapes = [(E, E), (E, EKV), (E, EKV), (E, E), (E, Fd), (E, Fd), (Fd, E)]
    ws = [R.synth(t, 9, 400 + i, k, n) for i, (t, (k, n)) in enumerate(zip(tys, shapes))]
    nw1 = (1 + 0.05 * rng.standard_normal(E)).astype(np.float32)
    nw2 = (1 + 0.05 * rng.standard_normal(E)).astype(np.float32)
    x = rng.standard_normal((T, E)).astype(np.float32)
    kc = (rng.standard_normal((n_ctx, EKV)) * 0.5).astype(np.float16)
    vc = rng.standard_normal((n_ctx, EKV)).astype(np.float16)
    pos = np.array([n_past], np.int32)
    mask = np.full((32, n_kv), -np.inf, np.float16)
    mask[0, :n_kv] = 0
    data = ws + [nw1, nw2, x, kc, vc, pos, mask]

    ctx = G.ggml_init(InitParams(256 << 20, None, True))
    W = [G.ggml_new_tensor_2d(ctx, t, k, n) for t, (k, n) in zip(tys, shapes)]
    N1, N2 = G.ggml_new_tensor_1d(ctx, R.F32, E), G.ggml_new_tensor_1d(ctx, R.F32, E)
    X = G.ggml_new_tensor_2d(ctx, R.F32, E, T)
    KC, VC = G.ggml_new_tensor_1d(ctx, R.F16, n_ctx * EKV), G.ggml_new_tensor_1d(ctx, R.F16, n_ctx * EKV)
    Pz = G.ggml_new_tensor_1d(ctx, 26, T)
    Mk = G.ggml_new_tensor_2d(ctx, R.F16, n_kv, 32)
    ins = W + [N1, N2, X, KC, VC, Pz, Mk]
    for t in ins:
        G.ggml_set_input(t)
    cur = G.ggml_mul(ctx, G.ggml_rms_norm(ctx, X, 1e-5), N1)
    q = G.ggml_rope_ext(ctx, G.ggml_reshape_3d(ctx, G.ggml_mul_mat(ctx, W[0], cur), D, H, T), Pz, None, D, 0, n_ctx,
                        500000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
    k = G.ggml_rope_ext(ctx, G.ggml_reshape_3d(ctx, G.ggml_mul_mat(ctx, W[1], cur), D, HKV, T), Pz, None, D, 0, n_ctx,
                        500000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
    v = G.ggml_mul_mat(ctx, W[2], cur)
    st_k = G.ggml_cpy(ctx, k, G.ggml_view_1d(ctx, KC, T * EKV, n_past * EKV * 2))
    st_v = G.ggml_cpy(ctx, v, G.ggml_view_1d(ctx, VC, T * EKV, n_past * EKV * 2))
    kview = G.ggml_view_3d(ctx, KC, D, n_kv, HKV, EKV * 2, D * 2, 0)
    vview = G.ggml_view_3d(ctx, VC, D, n_kv, HKV, EKV * 2, D * 2, 0)
    fa = G.ggml_flash_attn_ext(ctx, G.ggml_permute(ctx, q, 0, 2, 1, 3), kview, vview, Mk, 1.0 / np.sqrt(D), 0.0, 0.0)
    att = G.ggml_mul_mat(ctx, W[3], G.ggml_reshape_2d(ctx, fa, E, T))
    ffn_in = G.ggml_add(ctx, att, X)
    h = G.ggml_mul(ctx, G.ggml_rms_norm(ctx, ffn_in, 1e-5), N2)
    h = G.ggml_mul(ctx, G.ggml_silu(ctx, G.ggml_mul_mat(ctx, W[4], h)), G.ggml_mul_mat(ctx, W[5], h))
    out = G.ggml_add(ctx, G.ggml_mul_mat(ctx, W[6], h), ffn_in)
    G.ggml_set_output(out)
    g = G.ggml_new_graph(ctx)
    G.ggml_build_forward_expand(g, st_k)
    G.ggml_build_forward_expand(g, st_v)
    G.ggml_build_forward_expand(g, out)
    nodes = [G.ggml_graph_node(g, i) for i in range(G.ggml_graph_n_nodes(g))]
    assert all(G.ggml_backend_supports_op(be, n) for n in nodes)
    if alloc == "ctx":
        buf, galloc = G.ggml_backend_alloc_ctx_tensors(ctx, be), None
        assert buf
    else:
        galloc = G.ggml_gallocr_new(L.ggml_backend_cuda_buffer_type(0))
        assert G.ggml_gallocr_alloc_graph(galloc, g)
    # every node with its own bytes (ctx allocation): the F32 node outputs compared too
    probe = [n for n in nodes if alloc == "ctx" and ctypes.c_int.from_address(n).value == R.F32]
    runs = []
    try:
        for fused in (1, 0):
            assert L.kcpp_ggml_backend_set_fusion(ctypes.c_void_p(be), fused) == 0
            for t, a in zip(ins, data):
                a = np.ascontiguousarray(a)
                G.ggml_backend_tensor_set(t, a.ctypes.data, 0, a.nbytes)
            assert G.ggml_backend_graph_compute(be, g) == 0, L.kcpp_ggml_backend_last_error()
            nf = (L.kcpp_ggml_backend_last_fused(), L.kcpp_ggml_backend_last_fused_launches())
            got = []
            for t in [out] + probe:
                r = np.empty(G.ggml_nbytes(t) // 4, np.float32)
                G.ggml_backend_tensor_get(t, r.ctypes.data, 0, r.nbytes)
                got.append(r)
            runs.append((nf, got))
    finally:
        L.kcpp_ggml_backend_set_fusion(ctypes.c_void_p(be), 1)
        if galloc:
            G.ggml_gallocr_free(galloc)
        else:
            G.ggml_backend_buffer_free(buf)
        G.ggml_free(ctx)
    ((nf1, nl1), a), ((nf0, nl0), b) = runs
    L.kcpp_rs_supported.argtypes = [I, I64]
    rs = [bool(L.kcpp_rs_supported(t, k)) for t, (k, n) in zip(tys, shapes)]      # ggml type ids = KT_ codes
    # 2 norms (+ MUL); on RS layouts q's MUL_MAT + RESHAPE + ROPE, k's MUL_MAT + RESHAPE + ROPE + VIEW + CPY into the
    # cache (otherwise its ROPE + VIEW + CPY), v's MUL_MAT + VIEW + CPY, wo + ADD, the GLU quadruple, down + ADD
    want = 2 * 2 + 3 * rs[0] + (5 if rs[1] else 3) + 3 * rs[2] + 2 * rs[3] + 4 * rs[4] + 2 * rs[6]
    # launches: the attention norm inside k's chain (RS k; otherwise its own launch and k's ROPE + CPY), q's chain, v,
    # wo + ADD, the ffn norm inside the GLU (RS gate / up; otherwise its own launch), down + ADD
    want_l = (1 if rs[1] else 2) + rs[0] + rs[2] + rs[3] + 1 + rs[6]
    print("%s: %d nodes fused of %d in %d launches (expected %d in %d)" % (name, nf1, len(nodes), nl1, want, want_l))
    assert nf0 == 0 and nf1 == want, (nf1, want)
    # (under ggml_gallocr the norm weights are graph tensors whose bytes the allocator may hand to a mat-vec output
    # once the MUL has read them; a norm fused into that mat-vec's prologue would race with it, so the norm then runs
    # as its own launch -- llama.cpp keeps the weights in their own buffer)
    assert nl1 == want_l if alloc == "ctx" else want_l <= nl1 <= want_l + 2, (nl1, want_l)
    assert rs[4] == (wt != R.Q8_0)
    for i, (u, w_) in enumerate(zip(a, b)):
        assert np.array_equal(u.view(np.uint32), w_.view(np.uint32)), (i, rel(u, w_))


@pytest.mark.parametrize("wt,mode,ext,ff", [(R.Q4_K, 0, 0.0, False), (R.Q4_K, 0, 1.0, True), (R.Q4_K, 2, 0.0, False),
                                            (R.Q6_K, 0, 1.0, False), (R.Q8_0, 0, 0.0, True)],
                         ids=["q4k_norm", "q4k_norm_yarn_ff", "q4k_neox", "q6k_norm_yarn", "q8_0_norm_ff"])
def test_mv_rope_cpy_fusion(env, wt, mode, ext, ff):
    """the k path of a token graph -- MUL_MAT -> RESHAPE -> ROPE -> VIEW -> CPY into an F16 cache view -- fused
    (NORM rope on RS layouts: one mat-vec launch with the rope pairs in its epilogue; NEOX rope or other layouts: the
    ROPE + CPY pair) against node by node, bitwise on the product, the roped tensor and the cache bytes, with YaRN
    (ext_factor, freq_scale 0.25) and freq factors; and the fused result against the reference CPU backend"""
    G, L, be = env
    L.kcpp_ggml_backend_set_fusion.argtypes = [P, I]
    Kd, D, HKV, n_ctx, n_past = 4096, 128, 8, 64, 21
    EKV = D * HKV
    w = R.synth(wt, 9, 77, Kd, EKV)
    rng = np.random.default_rng(3)
    x = rng.standard_normal(Kd).astype(np.float32)
    kc = (rng.standard_normal((n_ctx, EKV)) * 0.5).astype(np.float16)
    pos = np.array([n_past], np.int32)
    fq = (1.0 + 0.5 * rng.random(D // 2)).astype(np.float32)
    fscale = 0.25 if ext else 1.0

    def build(ctx):
        Wt = G.ggml_new_tensor_2d(ctx, wt, Kd, EKV)
        X = G.ggml_new_tensor_2d(ctx, R.F32, Kd, 1)
        KC = G.ggml_new_tensor_1d(ctx, R.F16, n_ctx * EKV)
        Pz = G.ggml_new_tensor_1d(ctx, 26, 1)
        FF = G.ggml_new_tensor_1d(ctx, R.F32, D // 2) if ff else None
        mm = G.ggml_mul_mat(ctx, Wt, X)
        k = G.ggml_rope_ext(ctx, G.ggml_reshape_3d(ctx, mm, D, HKV, 1), Pz, FF, D, mode, 4096, 500000.0, fscale, ext,
                            1.0, 32.0, 1.0)
        st = G.ggml_cpy(ctx, k, G.ggml_view_1d(ctx, KC, EKV, n_past * EKV * 2))
        ins = [Wt, X, KC, Pz] + ([FF] if ff else [])
        return ins, [mm, k], st, KC

    data = [w, x, kc, pos] + ([fq] if ff else [])
    outs = {}
    for tag in ("fused", "nodes", "cpu"):
        ctx = G.ggml_init(InitParams(64 << 20, None, tag != "cpu"))
        ins, probes, st, KC = build(ctx)
        g = G.ggml_new_graph(ctx)
        G.ggml_build_forward_expand(g, st)
        if tag != "cpu":
            assert L.kcpp_ggml_backend_set_fusion(ctypes.c_void_p(be), int(tag == "fused")) == 0
            buf = G.ggml_backend_alloc_ctx_tensors(ctx, be)
            for t, a in zip(ins, data):
                a = np.ascontiguousarray(a)
                G.ggml_backend_tensor_set(t, a.ctypes.data, 0, a.nbytes)
            try:
                assert G.ggml_backend_graph_compute(be, g) == 0, L.kcpp_ggml_backend_last_error()
                nf = L.kcpp_ggml_backend_last_fused()
            finally:
                L.kcpp_ggml_backend_set_fusion(ctypes.c_void_p(be), 1)
            got = []
            for t in probes:
                r = np.empty(G.ggml_nbytes(t) // 4, np.float32)
                G.ggml_backend_tensor_get(t, r.ctypes.data, 0, r.nbytes)
                got.append(r)
            c = np.empty(n_ctx * EKV, np.float16)
            G.ggml_backend_tensor_get(KC, c.ctypes.data, 0, c.nbytes)
            got.append(c)
            G.ggml_backend_buffer_free(buf)
            outs[tag] = (nf, got)
        else:
            for t, a in zip(ins, data):
                a = np.ascontiguousarray(a)
                ctypes.memmove(G.ggml_get_data(t), a.ctypes.data, a.nbytes)
            assert G.ggml_graph_compute_with_ctx(ctx, g, 8) == 0
            got = [np.ctypeslib.as_array((ctypes.c_float * (G.ggml_nbytes(t) // 4)).from_address(G.ggml_get_data(t))).copy()
                   for t in probes]
            got.append(np.ctypeslib.as_array((ctypes.c_uint16 * (n_ctx * EKV)).from_address(G.ggml_get_data(KC))).copy()
                       .view(np.float16))
            outs[tag] = (0, got)
        G.ggml_free(ctx)
    L.kcpp_rs_supported.argtypes = [I, I64]
    rs = bool(L.kcpp_rs_supported(wt, Kd))
    (nf1, a), (nf0, b), (_, c) = outs["fused"], outs["nodes"], outs["cpu"]
    assert nf0 == 0 and nf1 == (5 if rs and mode == 0 else 3), nf1
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.uint16 if u.dtype == np.float16 else np.uint32),
                              v.view(np.uint16 if v.dtype == np.float16 else np.uint32))
    assert rel(a[0], c[0]) <= 3e-6, rel(a[0], c[0])                  # the product: exact dots, fp32 order
    assert rel(a[1], c[1]) <= 1e-5, rel(a[1], c[1])                  # roped
    kcache = a[2].astype(np.float32).reshape(n_ctx, EKV)
    assert np.array_equal(kcache[:n_past], c[2].astype(np.float32).reshape(n_ctx, EKV)[:n_past])   # untouched rows
    assert np.abs(kcache[n_past] - a[1]).max() <= np.abs(a[1]).max() * 2e-3       # the stored row: f16 of the roped
