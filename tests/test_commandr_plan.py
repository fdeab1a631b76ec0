"""The LayerNorm prologue (pro 3) in the decode mat-vec launch plan (gemv_plan.h through kcpp_gemv_dec_plan, no GPU):
exactly the instances built for the Command-R launches -- q|k|v, the 8-wave gate|up, the head and the mixed q|k + v
launch over the row-major K-quant layouts -- with their pro 1 counterparts' R / waves / grid, and -3 everywhere else."""
import pytest

RS = ("Q4_K_RS", "Q5_K_RS", "Q6_K_RS")
SAME = ("kernel", "type", "mode", "NI", "R", "MC", "PF", "waves", "XL", "ROUTE", "EX", "block", "nblk", "lds_bytes")
# (mode, N): q|k|v of Aya-8B-like / MHA shapes, gate|up, the head (more than 16384 rows)
@pytest.fixture(scope="module")
def K():
    # inside a fixture, as the other plan tests do: a whole-suite collection must not load the native library (and
    # with it a HIP runtime) before the GPU tests' own first import of torch
    import koboldcpp_amd.lib as K
    return K


LAUNCHES = ((2, (4096, 1024, 1024)), (2, (2048, 2048, 2048)), (2, (8192, 1024)), (1, (14336,)), (1, (1024,)),
            (0, (256000,)), (0, (16896,)))


@pytest.mark.parametrize("wtype", RS)
@pytest.mark.parametrize("Kw", (2048, 4096, 8192))
@pytest.mark.parametrize("mode,N", LAUNCHES)
def test_pro3_is_the_pro1_plan(K, wtype, Kw, mode, N):
    wtype = getattr(K, wtype)
    rpw = 4 if mode == 0 else (2 if mode == 2 else 1)
    for entry in ("dec", "rs"):
        p1 = K.gemv_dec_plan(entry, wtype, Kw, N, mode, 1, rpw)
        p3 = K.gemv_dec_plan(entry, wtype, Kw, N, mode, 3, rpw)
        assert isinstance(p1, dict) and isinstance(p3, dict), (p1, p3)
        assert p3["pro"] == 3 and p3["kernel"] == "rs"
        assert {k: p3[k] for k in SAME} == {k: p1[k] for k in SAME}
        # the built PRO 3 instances (gemv_rs.hip KCPP_RS_INSTANCES)
        inst = (p3["R"], p3["mode"], p3["PF"], p3["waves"], p3["XL"], p3["ROUTE"], p3["EX"])
        assert inst == {2: (2, 2, 0, 4, 0, 0, 0), 1: (1, 1, 1, 8, 0, 0, 0), 0: (2, 0, 0, 4, 0, 0, 0)}[mode]
        assert p3["MC"] == (Kw + 4095) // 4096


@pytest.mark.parametrize("Kw,nia,nib,mc", ((2048, 1, 1, 1), (4096, 2, 1, 1), (8192, 4, 2, 2)))
def test_pro3_mixed_launch(K, Kw, nia, nib, mc):
    N = (Kw, 1024, 1024)
    p1 = K.gemv_qkv_mixed_plan(Kw, N, pro=1)
    p3 = K.gemv_qkv_mixed_plan(Kw, N, pro=3)
    assert p1["PRO"] == 1 and p3["PRO"] == 3
    assert (p3["NIA"], p3["NIB"], p3["MC"], p3["EX"]) == (nia, nib, mc, 0)
    assert {k: v for k, v in p3.items() if k != "PRO"} == {k: v for k, v in p1.items() if k != "PRO"}
    assert {k: v for k, v in p1.items() if k != "PRO"} == K.gemv_qkv_mixed_plan(Kw, N)
    # no LayerNorm instance carries a bias or NeoX pairs
    assert K.gemv_qkv_mixed_plan(Kw, N, flags=("ex",), pro=3) == -3
    assert K.gemv_qkv_mixed_plan(Kw, N, flags=("ex", "neox"), D=128, pro=3) == -3
    assert K.gemv_qkv_mixed_plan(6144, (6144, 1024, 1024), pro=3) == -3     # no mixed instance at this width


def test_pro3_refusals(K):
    q = (4096, 1024, 1024)
    # every other family: the unit kernels (Q8_0, Q4_0, the IQ types, Q6_K / Q4_K in the block order), Q4K, STREAM
    for t in (K.Q8_0, K.Q4_0, K.Q4_K, K.Q5_K, K.Q6_K, K.Q3_K, K.Q2_K, K.IQ4_NL, K.IQ4_XS, K.IQ2_XS, K.IQ3_S):
        for mode, N, rpw in ((2, q, 2), (1, (14336,), 1), (0, (256000,), 4), (0, (4096,), 1)):
            assert K.gemv_dec_plan("dec", t, 4096, N, mode, 3, rpw) == -3, (t, mode)
    for entry, t in (("unit", K.Q8_0), ("q4k", K.Q4_K), ("stream", K.Q4_K)):
        assert K.gemv_dec_plan(entry, t, 4096, (14336,), 1, 3, 1) == -3
    assert K.gemv_dec_plan("stream", K.Q4_K, 14336, (4096,), 0, 3, 1) == -3
    # no AUX instance has the LayerNorm prologue
    fl = ("aux", "aux_p0h0", "aux_glu", "nw")
    assert isinstance(K.gemv_dec_plan("rs_aux", K.Q4_K_RS, 4096, (14336,), 1, 1, 1, flags=fl), dict)
    assert K.gemv_dec_plan("rs_aux", K.Q4_K_RS, 4096, (14336,), 1, 3, 1, flags=fl) == -3
    for t in (getattr(K, n) for n in RS):
        # XL widths: Q4_K / Q5_K past NI 7 (K 16384), Q6_K past NI 4 (K 18432 has nsb 72 = 8 x 9)
        kxl = 18432
        assert isinstance(K.gemv_dec_plan("rs", t, kxl, (4096,), 1, 1, 1), dict)
        for mode, N in ((2, q), (1, (4096,)), (0, (32000,))):
            assert K.gemv_dec_plan("rs", t, kxl, N, mode, 3, 2) == -3
        # mode 0 below the head's row count, mode 3, two-segment gate|up, experts, a router, bias / NeoX
        assert K.gemv_dec_plan("rs", t, 4096, (4096,), 0, 3, 1) == -3
        assert K.gemv_dec_plan("rs", t, 4096, (16384,), 0, 3, 1) == -3
        assert K.gemv_dec_plan("rs", t, 4096, (20000, 20000), 0, 3, 1) == -3
        assert K.gemv_dec_plan("rs", t, 14336, (4096,), 3, 3, 1, flags=("eid", "eid1", "escale")) == -3
        assert K.gemv_dec_plan("rs", t, 4096, (1024, 1024), 1, 3, 1, flags=("eid", "eid1")) == -3
        assert K.gemv_dec_plan("rs", t, 4096, (1024,), 1, 3, 1, flags=("eid",)) == -3
        assert K.gemv_dec_plan("rs", t, 4096, (1024, 1024), 1, 3, 1, flags=("route_w", "route_out"), route_wt=K.F32,
                               route_ne=8) == -3
        assert K.gemv_dec_plan("rs", t, 4096, q, 2, 3, 2, flags=("ex",)) == -3
        assert K.gemv_dec_plan("rs", t, 4096, q, 2, 3, 2, flags=("ex", "neox"), D=128) == -3
        assert K.gemv_dec_plan("rs", t, 4096, q, 2, 4, 2) == -3
    # a segment that is no whole number of R-row groups keeps its own code
    assert K.gemv_dec_plan("rs", K.Q4_K_RS, 4096, (4097, 1024, 1024), 2, 3, 2) == -5
