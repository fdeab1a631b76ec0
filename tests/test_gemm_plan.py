"""kcpp_gemm's launch plan (csrc/gemm_plan.h through kcpp_gemm_plan) against a table worked out by hand from the
dispatcher it replaced, and kcpp_gemm_workspace_bytes against the byte counts that dispatcher's library returned.
Host only: the plan decides the split-K factor (which changes output bits) and the tile (which changes speed), so it is
pinned here on both sides of every rule's threshold and for the variants the tests and tools use.

How the expected rows were derived (Mp = M rounded up to 128, nsb = K / 256, nt = ceil(N / 128)):
  cols   Q4_1 / Q5_1 / IQ4_NL / IQ4_XS / IQ1-3 at M <= 16 (variant 20: every M)
  q80s   Q8_0 at M <= 32; ks = max(min(ceil(384 / nt), max(1, K / 32 / 16)), ceil(K / 32 / 48)), nwg = nt ks
  v4     Q4_K (+RS) -- and Q5_K (+RS) where ks would be 2, or GLU with Mp <= 256 -- with aligned bsums and M > 32;
         ks = 2 iff mode 0, nsb even, nt <= 32; TPW 4 iff Q4_K, ks 1 and Mp / 128 * ceil(N / 256) >= 224;
         nwg = Mp / 128 * (TPW 4: ceil(N / 256), else nt) * ks * (GLU: 2, gate and up in one launch); 8 waves
  q4v3   what v4 leaves of Q4_K (+RS): big = Mp / 128 * nt >= 384: BMT 4, 8 waves, else BMT 2, 4 waves;
         ks = 2 iff mode 0, nsb even, not big, and nt < 16 or nsb >= 32; nwg = Mp / (32 BMT) * nt * ks
  q6v3   Q6_K_RS: BMT 4, 8 waves iff big or (nsb >= 32 even, mode 0, Mp / 128 * nt * 2 >= 256); ks and nwg as q4v3
  v2     the other Q4_K / Q5_K / Q6_K (+RS): TM 2 iff Q4_K, Mp % 256 == 0, N >= 8192; nwg = Mp / (128 TM) * ceil(N / 64)
  v1     everything else: ks doubles from 1 while ks < 8, ceil(N / 64) * 4 * 2 ks <= 1024 and nsb % 2 ks == 0;
         nwg = ceil(N / 64) * Mp / 128 * ks
Variants: 2 (and unknown numbers) v2; 3 v3 unsplit; 4 v3 split wherever mode 0 and nsb even; 5 / 6 / 7 v3 unsplit with
PF 2 / PF 2 + 4 waves / 4 waves; 8-10 v3 unsplit XG 2 / 4 / 8; 11 v4 forced (else v3 unsplit), 12 with XG 2, 13 v4
unsplit; 14 TPW 4 forced (Q5_K TPW 2; else v2); 15-17 v3 by rule with q6v3 (BMT, waves) (4, 4) / (4, 8) / (2, 8);
20 as 2 + cols at every M; 21 as 2 + v1 unsplit."""
import pytest

Q4_0, Q4_1, Q8_0, Q2_K, Q4_K, Q5_K, Q6_K, IQ2_XS, IQ4_XS = 2, 3, 8, 10, 12, 13, 14, 17, 23
Q4_K_RS, Q5_K_RS, Q6_K_RS = 112, 113, 114


def P(family, ks, nwg, **kw):
    return dict(family=family, ks=ks, nwg=nwg, **kw)


# (variant, type, K, N, M, mode, bs_aligned) -> the fields the old dispatcher fixed for that family
ROWS = [
    # ---- variant 0, M = 512: the Llama-3-8B / Mixtral shapes of tools/gemm_ab.py
    (0, Q4_K_RS, 4096, 28672, 512, 0, 1, P("v4", 1, 448, rs=1, tile=4, waves=8, xg=1)),
    (0, Q4_K_RS, 4096, 6144, 512, 0, 1, P("v4", 1, 192, rs=1, tile=2, waves=8)),
    (0, Q4_K_RS, 4096, 4096, 512, 0, 1, P("v4", 2, 256, rs=1, tile=2)),
    (0, Q4_K_RS, 14336, 4096, 512, 0, 1, P("v4", 2, 256, rs=1, tile=2)),
    (0, Q4_K_RS, 4096, 14336, 512, 1, 1, P("v4", 1, 448, rs=1, tile=4)),          # GLU in one launch: 2 x 224
    (0, Q6_K_RS, 14336, 4096, 512, 0, 1, P("q6v3", 2, 256, rs=1, tile=4, waves=8)),
    (0, Q6_K_RS, 4096, 1024, 512, 0, 1, P("q6v3", 2, 128, rs=1, tile=2, waves=4)),
    # ---- v4's split: 32 / 33 row tiles; an odd super-block count
    (0, Q4_K, 4096, 4096, 512, 0, 1, P("v4", 2, 256, rs=0, tile=2)),
    (0, Q4_K, 4096, 4224, 512, 0, 1, P("v4", 1, 132, rs=0, tile=2)),
    (0, Q4_K, 768, 4096, 512, 0, 1, P("v4", 1, 128, rs=0, tile=2)),
    # ---- v5 (TPW 4) at 224 / 220 workgroups, GLU
    (0, Q4_K, 4096, 14336, 512, 1, 1, P("v4", 1, 448, tile=4)),
    (0, Q4_K, 4096, 14080, 512, 1, 1, P("v4", 1, 880, tile=2)),
    # ---- v4 needs aligned bsums and M > 32: else v3
    (0, Q4_K_RS, 4096, 4096, 512, 0, 0, P("q4v3", 1, 256, rs=1, tile=2, waves=4, xg=1, pf=1)),
    (0, Q4_K_RS, 14336, 4096, 512, 0, 0, P("q4v3", 2, 512, tile=2, waves=4)),   # long K: split
    (0, Q4_K_RS, 4096, 1920, 512, 0, 0, P("q4v3", 2, 240, tile=2, waves=4)),    # 15 row tiles: split
    (0, Q4_K_RS, 4096, 2048, 512, 0, 0, P("q4v3", 1, 128, tile=2, waves=4)),    # 16 row tiles: not
    (0, Q4_K_RS, 4096, 4096, 32, 0, 1, P("q4v3", 1, 64, tile=2, waves=4)),
    (0, Q4_K_RS, 4096, 4096, 33, 0, 1, P("v4", 2, 64, tile=2)),
    # ---- v3's big grid: 384 / 380 workgroups of 128 x 128
    (0, Q4_K_RS, 4096, 12288, 512, 0, 0, P("q4v3", 1, 384, tile=4, waves=8)),
    (0, Q4_K_RS, 4096, 12160, 512, 0, 0, P("q4v3", 1, 760, tile=2, waves=4)),
    (0, Q4_K_RS, 16384, 12288, 512, 0, 0, P("q4v3", 1, 384, tile=4, waves=8)),  # big: never split
    # ---- Q5_K: v4 where it splits (<= 32 row tiles), GLU up to Mp = 256; else v2
    (0, Q5_K, 4096, 4096, 512, 0, 1, P("v4", 2, 256, rs=0, tile=2)),
    (0, Q5_K, 4096, 4224, 512, 0, 1, P("v2", 1, 264, rs=0, tile=1, waves=4)),
    (0, Q5_K, 14336, 4096, 128, 0, 1, P("v4", 2, 64, tile=2)),
    (0, Q5_K_RS, 4096, 14336, 256, 1, 1, P("v4", 1, 448, rs=1, tile=2)),
    (0, Q5_K_RS, 4096, 14336, 257, 1, 1, P("v2", 1, 672, rs=1, tile=1)),
    (0, Q5_K, 4096, 4096, 512, 0, 0, P("v2", 1, 256, tile=1)),
    # ---- Q6_K in the base layout: v2
    (0, Q6_K, 4096, 4096, 512, 0, 1, P("v2", 1, 256, rs=0, tile=1)),
    # ---- q6v3 tiles: long K needs 256 workgroups after the split (M = 512: 256, M = 384: 192)
    (0, Q6_K_RS, 14336, 4096, 384, 0, 1, P("q6v3", 2, 384, tile=2, waves=4)),
    (0, Q6_K_RS, 4096, 4096, 512, 1, 1, P("q6v3", 1, 256, tile=2, waves=4)),
    # ---- variant 2: v2's TM
    (2, Q4_K_RS, 4096, 8192, 256, 0, 1, P("v2", 1, 128, rs=1, tile=2, waves=4)),
    (2, Q4_K_RS, 4096, 8192, 128, 0, 1, P("v2", 1, 128, rs=1, tile=1)),
    (2, Q4_K_RS, 4096, 8128, 256, 0, 1, P("v2", 1, 254, tile=1)),
    (2, Q6_K_RS, 4096, 1024, 512, 0, 1, P("v2", 1, 64, rs=1, tile=1)),
    (99, Q4_K_RS, 4096, 4096, 512, 0, 1, P("v2", 1, 256, tile=1)),               # unknown numbers: as 2
    (1, Q6_K_RS, 4096, 1024, 512, 0, 1, P("v2", 1, 64, tile=1)),
    # ---- Q8_0 small batch
    (0, Q8_0, 4096, 4096, 32, 0, 1, P("q80s", 8, 256)),
    (0, Q8_0, 4096, 4096, 33, 0, 1, P("v1", 4, 256)),
    (0, Q8_0, 14336, 4096, 8, 1, 1, P("q80s", 12, 384)),
    # ---- the mat-vec types: 16 / 17 columns
    (0, Q4_1, 4096, 4096, 16, 0, 1, P("cols", 1, 0)),
    (0, Q4_1, 4096, 4096, 17, 0, 1, P("v1", 4, 256)),
    (0, IQ4_XS, 4096, 4096, 16, 0, 1, P("cols", 1, 0)),
    (0, IQ4_XS, 4096, 4096, 17, 0, 1, P("v1", 4, 256)),
    (0, IQ2_XS, 4096, 4096, 16, 1, 1, P("cols", 1, 0)),
    (0, IQ2_XS, 4096, 4096, 17, 1, 1, P("v1", 4, 256)),
    (20, Q4_1, 4096, 4096, 512, 0, 1, P("cols", 1, 0)),
    (20, Q4_K_RS, 4096, 4096, 512, 0, 1, P("v2", 1, 256)),
    # ---- v1's split: 8 / 4 / 2 / 1 by the row-tile count, 1 on an odd super-block count
    (0, Q4_0, 4096, 2048, 512, 0, 1, P("v1", 8, 1024)),
    (0, Q4_0, 4096, 2112, 512, 0, 1, P("v1", 4, 528)),
    (0, Q2_K, 4096, 4096, 512, 0, 1, P("v1", 4, 1024)),
    (0, Q2_K, 4096, 4160, 512, 0, 1, P("v1", 2, 520)),
    (0, Q4_0, 4096, 8192, 512, 1, 1, P("v1", 2, 1024)),
    (0, Q4_0, 4096, 8256, 512, 0, 1, P("v1", 1, 516)),
    (0, Q2_K, 768, 2048, 512, 0, 1, P("v1", 1, 128)),
    (0, Q2_K, 1536, 2048, 100, 0, 1, P("v1", 2, 64)),
    (21, Q4_0, 4096, 2048, 512, 0, 1, P("v1", 1, 128)),
    # ---- variants 3 / 4: v3 without / with the split
    (3, Q4_K_RS, 14336, 4096, 512, 0, 1, P("q4v3", 1, 256, tile=2, waves=4, pf=1, xg=1)),
    (3, Q6_K_RS, 4096, 1024, 512, 0, 1, P("q6v3", 1, 64, tile=2, waves=4)),
    (3, Q6_K, 4096, 1024, 512, 0, 1, P("v2", 1, 64)),
    (3, Q5_K, 4096, 4096, 512, 0, 1, P("v2", 1, 256)),
    (4, Q4_K_RS, 4096, 6144, 512, 0, 1, P("q4v3", 2, 768, tile=2, waves=4)),
    (4, Q4_K_RS, 4096, 14336, 512, 1, 1, P("q4v3", 1, 448, tile=4, waves=8)),
    (4, Q4_K_RS, 768, 4096, 512, 0, 1, P("q4v3", 1, 256, tile=2)),
    (4, Q6_K_RS, 4096, 4096, 512, 0, 1, P("q6v3", 2, 512, tile=2, waves=4)),
    # ---- variants 5 - 10: v3's PF / waves / XG
    (5, Q4_K_RS, 4096, 28672, 512, 0, 1, P("q4v3", 1, 896, tile=4, waves=8, pf=2, xg=1)),
    (6, Q4_K_RS, 4096, 28672, 512, 0, 1, P("q4v3", 1, 896, tile=4, waves=4, pf=2)),
    (7, Q4_K_RS, 4096, 28672, 512, 0, 1, P("q4v3", 1, 896, tile=4, waves=4, pf=1)),
    (7, Q6_K_RS, 14336, 4096, 512, 0, 1, P("q6v3", 1, 128, tile=4, waves=8)),
    (8, Q4_K, 4096, 4096, 512, 0, 1, P("q4v3", 1, 256, tile=2, waves=4, xg=2)),
    (9, Q4_K, 4096, 4096, 512, 0, 1, P("q4v3", 1, 256, xg=4)),
    (10, Q4_K, 4096, 4096, 512, 0, 1, P("q4v3", 1, 256, xg=8)),
    # ---- variants 11 - 14: v4 / v5 forced
    (11, Q4_K_RS, 4096, 4096, 512, 0, 1, P("v4", 2, 256, tile=2, xg=1)),
    (11, Q4_K_RS, 4096, 28672, 512, 0, 1, P("v4", 1, 896, tile=2)),
    (11, Q5_K, 4096, 4224, 512, 0, 1, P("v4", 1, 132, tile=2)),
    (11, Q6_K_RS, 14336, 4096, 512, 0, 1, P("q6v3", 1, 128, tile=4, waves=8)),
    (11, Q4_K_RS, 4096, 4096, 512, 0, 0, P("q4v3", 1, 256, tile=2)),
    (12, Q4_K_RS, 4096, 4096, 512, 0, 1, P("v4", 2, 256, tile=2, xg=2)),
    (13, Q4_K_RS, 4096, 4096, 512, 0, 1, P("v4", 1, 128, tile=2)),
    (13, Q5_K_RS, 14336, 4096, 100, 0, 1, P("v4", 1, 32, tile=2)),
    (14, Q4_K_RS, 4096, 6144, 512, 0, 1, P("v4", 1, 96, tile=4)),
    (14, Q4_K_RS, 4096, 4096, 512, 0, 1, P("v4", 2, 128, tile=4)),
    (14, Q5_K_RS, 4096, 4096, 512, 0, 1, P("v4", 2, 256, rs=1, tile=2)),
    (14, Q4_K_RS, 4096, 4096, 512, 0, 0, P("v2", 1, 256, tile=1)),
    (14, Q6_K_RS, 4096, 1024, 512, 0, 1, P("v2", 1, 64)),
    # ---- variants 15 - 17: q6v3's tile; Q4_K on v3 by its split rule
    (15, Q6_K_RS, 4096, 1024, 512, 0, 1, P("q6v3", 2, 64, tile=4, waves=4)),
    (16, Q6_K_RS, 4096, 1024, 512, 0, 1, P("q6v3", 2, 64, tile=4, waves=8)),
    (17, Q6_K_RS, 14336, 4096, 512, 0, 1, P("q6v3", 2, 512, tile=2, waves=8)),
    (15, Q4_K_RS, 4096, 4096, 512, 0, 1, P("q4v3", 1, 256, tile=2, waves=4)),
    (16, Q4_K_RS, 14336, 4096, 512, 0, 1, P("q4v3", 2, 512, tile=2, waves=4)),
    (17, Q5_K, 4096, 4096, 512, 0, 1, P("v2", 1, 256)),
]

# kcpp_gemm_workspace_bytes(type, K, N, M) of the library built from the dispatcher this plan replaced
WS_BYTES = {
    (2, 4096, 2048, 512): 42467328,
    (2, 4096, 2112, 512): 26345472,
    (2, 4096, 8192, 512): 55050240,
    (2, 4096, 8256, 512): 38535168,
    (3, 4096, 4096, 16): 9830400,
    (3, 4096, 4096, 17): 9846784,
    (3, 4096, 4096, 512): 46661632,
    (8, 4096, 4096, 32): 18481152,
    (8, 4096, 4096, 33): 18497536,
    (8, 14336, 4096, 8): 25231360,
    (10, 768, 2048, 512): 9230336,
    (10, 1536, 2048, 100): 3337216,
    (10, 4096, 4096, 512): 46432256,
    (10, 4096, 4160, 512): 30048256,
    (12, 768, 4096, 512): 26007552,
    (12, 4096, 4096, 512): 29655040,
    (12, 4096, 4224, 512): 30441472,
    (12, 4096, 14080, 512): 90996736,
    (12, 4096, 14336, 512): 92569600,
    (13, 4096, 4096, 512): 46432256,
    (13, 4096, 4224, 512): 30441472,
    (13, 14336, 4096, 128): 14413824,
    (14, 4096, 1024, 512): 23363584,
    (14, 4096, 4096, 512): 46432256,
    (17, 4096, 4096, 16): 9773056,
    (17, 4096, 4096, 17): 9789440,
    (23, 4096, 4096, 16): 9773056,
    (23, 4096, 4096, 17): 9789440,
    (112, 768, 4096, 512): 26007552,
    (112, 4096, 1920, 512): 16285696,
    (112, 4096, 2048, 512): 17072128,
    (112, 4096, 4096, 32): 5840896,
    (112, 4096, 4096, 33): 5857280,
    (112, 4096, 4096, 512): 29655040,
    (112, 4096, 6144, 512): 42237952,
    (112, 4096, 8128, 256): 27213824,
    (112, 4096, 8192, 128): 13705216,
    (112, 4096, 8192, 256): 27410432,
    (112, 4096, 12160, 512): 79200256,
    (112, 4096, 12288, 512): 79986688,
    (112, 4096, 14336, 512): 92569600,
    (112, 4096, 28672, 512): 180649984,
    (112, 14336, 4096, 512): 40878080,
    (112, 16384, 12288, 512): 93454336,
    (113, 4096, 4096, 512): 46432256,
    (113, 4096, 14336, 256): 46284800,
    (113, 4096, 14336, 257): 62144512,
    (113, 14336, 4096, 100): 13955072,
    (114, 4096, 1024, 512): 10780672,
    (114, 4096, 4096, 512): 29655040,
    (114, 14336, 4096, 384): 30658560,
    (114, 14336, 4096, 512): 40878080,
}


@pytest.fixture(scope="module")
def K():
    import koboldcpp_amd.lib as K
    yield K
    K.raw().kcpp_gemm_set_variant(0)


@pytest.mark.parametrize("row", ROWS, ids=lambda r: "v%d-t%d-%dx%d-M%d-m%d-a%d" % r[:7])
def test_plan_matches_hand_table(K, row):
    variant, t, Kd, N, M, mode, aligned, want = row
    K.raw().kcpp_gemm_set_variant(variant)
    try:
        got = K.gemm_plan(t, Kd, N, M, mode, aligned)
    finally:
        K.raw().kcpp_gemm_set_variant(0)
    assert {k: got[k] for k in want} == want, got


def test_variant_numbers_keep_their_meaning(K):
    raw = K.raw()
    assert raw.kcpp_gemm_set_variant(-1) == 0
    assert raw.kcpp_gemm_set_variant(13) == 0            # -1 reads back as 0, the default
    assert raw.kcpp_gemm_set_variant(0) == 13
    assert K.gemm_plan(Q4_K_RS, 4096, 4096, 512)["family"] == "v4"


def test_plan_rejects_what_kcpp_gemm_rejects(K):
    import ctypes
    out = (ctypes.c_int32 * 8)()
    assert K.raw().kcpp_gemm_plan(Q4_K, 4000, 4096, 512, 0, 1, out) == -1      # K % 256, as kcpp_gemm
    assert K.raw().kcpp_gemm_plan(Q4_K, 4096, 4096, 512, 2, 1, out) == -1
    assert K.raw().kcpp_gemm_plan(115, 4096, 4096, 512, 0, 1, out) == -3       # Q8_0_T: planned in gemm_q80t.hip


def test_workspace_bytes_unchanged(K):
    shapes = sorted({r[1:5] for r in ROWS})
    assert set(shapes) == set(WS_BYTES)
    got = {s: int(K.raw().kcpp_gemm_workspace_bytes(*s)) for s in shapes}
    assert got == WS_BYTES
