"""The launch plan of the decode attention and of the ggml-op forms (csrc/fa_plan.h fa_decode_plan through
kcpp_fa_decode_plan), host only.

`rules` below restates, independently of the C++, which kernel each entry of attn.hip runs and with which return code
(the comment block on fa_decode_plan); the sweeps hold the plan to it, and re-derive the split count, the grids and the
workspace layout: the partials (and the ggml-op form's f16 copy of Q) lie behind the 2048-byte header, do not overlap and
end inside what kcpp_fa_workspace_bytes / kcpp_fa_ext_workspace_bytes reserve."""
import itertools
import os
import subprocess
import sys

import pytest

GS_ = range(1, 9)
HKVS = (1, 2, 4, 8, 32, 64)
TS = (1, 2, 16, 17)
NKVS = (1, 63, 64, 65, 4096, 131072, 131073)
FORCE_PATHS = (0, 1, 2, 3, 4, 6, 7)          # 4: no path of its own (runs the tiles past the decode family)
VARIANTS = (0, 1, 3, 5, 6, 7, 8)             # 1: no such variant
HEADER = 2048
ENV4 = os.environ.get("KCPP_FA_DEC", "").strip() == "4"


@pytest.fixture(scope="module")
def K():
    import koboldcpp_amd.lib as K
    return K


def cdiv(a, b):
    return -(-a // b)


def splits(HKV):
    """256 / HKV rounded down to a power of two, within [4, 64]"""
    ns = 1
    while 2 * ns <= 256 // HKV:
        ns *= 2
    return min(64, max(4, ns))


def split_pair(G, n_rows, qkind, have_out, want5):
    if not qkind and not have_out:
        return -1
    if G in (3, 5, 6, 7):
        return "split5" if n_rows >= 1 else -1
    return "split5" if want5 and n_rows >= 1 else "split4"


def chunk_pair(nkv):
    return "chunk" if cdiv(nkv, 64) <= 2048 else -4


def rules(K, form, T, H, HKV, D, nkv, n_rows, qkind, sel, cap, have_out, env4=ENV4):
    """the kernel's name, or the error code"""
    G = H // HKV
    if form == "runtime":
        if D not in (64, 128) or H % HKV or H % 2:
            return -1
        if D == 64:
            return "tile" if have_out else -2
        if G > 8:
            return -1
        if sel == 7:
            return "short" if T == 1 and have_out and not qkind else -1
        if sel in (1, 6) or (sel == 0 and T <= 16):
            if T == 1 and sel != 6 and (not qkind or G >= 2):
                return split_pair(G, n_rows, qkind, have_out, not env4)
            return chunk_pair(nkv)
        if not have_out:
            return -2
        if sel == 3:
            return "mfma"
        if sel == 0 and K.fa_prefill_plan(64, H, HKV)["kernel"] != "fma":
            return "mfma"
        return "tile"
    if form == "ex":
        if H % HKV or not 1 <= G <= 8 or H % 2 or HKV > 64 or (qkind and G < 2):
            return -1
        if sel in (3, 5, 6, 7):
            return split_pair(G, n_rows, qkind, have_out, sel != 3)
        if sel == 8:
            return "short" if have_out and not qkind else -1
        return chunk_pair(nkv) if sel == 0 else -1
    if form == "graph1":
        if D != 128 or H % HKV or H % 2 or nkv < 1 or G not in (1, 2, 4, 8):
            return -3
        return "split5"
    assert form == "grapht"
    if D not in (64, 128) or H % HKV or G > 8 or H % 2 or nkv < 1 or (cap and D != 128):
        return -1
    if D == 64 or T > 16:
        return "tile"
    return chunk_pair(nkv)


def check_geometry(K, p, form, T, H, HKV, D, nkv, qkind):
    """grids, split count and the workspace layout of a planned launch"""
    if form in ("ex", "graph1"):
        T = 1
    kern = p["kernel"]
    regions = []
    if kern in ("split4", "split5"):
        ns = splits(HKV)
        assert (p["ns"], p["nch"], p["waves"]) == (ns, 0, 4)
        assert p["grid"] == (ns, HKV, 1) and p["cgrid"] == (H // 2, 1) and p["cthreads"] == 256
        assert p["cquant"] == qkind
        regions = [(p["part_o"], H * ns * 128 * 4), (p["part_ml"], H * ns * 8)]
    elif kern == "chunk":
        nch = cdiv(nkv, 64)
        assert (p["ns"], p["nch"], p["waves"]) == (0, nch, 4)
        assert p["grid"] == (nch, HKV, T) and p["cgrid"] == (H // 2, T) and p["cthreads"] == 1024
        assert p["cquant"] == (1 if qkind else 0)
        regions = [(p["part_o"], T * H * nch * 128 * 4), (p["part_ml"], T * H * nch * 8)]
    elif kern == "short":
        assert (p["ns"], p["nch"], p["waves"]) == (1, 0, 8)
        assert p["grid"] == (1, HKV, 1) and p["cgrid"] == (0, 0) and p["cthreads"] == 0 and p["cquant"] == 0
    else:
        assert p["grid"] == (cdiv(T, 64), H, 1) and p["waves"] == 4        # the tiles (the MFMA entry's fall-back)
        assert p["cgrid"] == (0, 0) and p["cthreads"] == 0 and p["cquant"] == 0
    if not regions:
        assert (p["part_o"], p["part_ml"]) == (0, 0)
    if form == "grapht":
        regions.append((p["q16"], T * H * D * 2))
    else:
        assert p["q16"] == 0
    end = HEADER
    for off, size in regions:            # in order, disjoint, behind the header
        assert off >= end, (p, regions)
        end = off + size
    assert p["ws_bytes"] == (end if regions else 0)
    if form in ("graph1", "grapht"):
        assert end <= K.fa_ext_workspace_bytes(T, H, nkv, D)
    else:
        assert end <= K.fa_workspace_bytes(T, H, nkv)


def sweep(K, form, sels, qkinds, Ds=(128,), caps=(False,)):
    n = 0
    for G, HKV, D in itertools.product(GS_, HKVS, Ds):
        H = G * HKV
        ns_seen = set()
        for T, nkv, sel, qkind, cap in itertools.product(TS, NKVS, sels, qkinds, caps):
            for n_rows, have_out in ((nkv, True), (0, True), (nkv, False)):
                want = rules(K, form, T, H, HKV, D, nkv, n_rows, qkind, sel, cap, have_out)
                p = K.fa_decode_plan(form, T, H, HKV, D, nkv, n_rows, qkind, sel, cap, have_out)
                got = p if isinstance(p, int) else p["kernel"]
                assert got == want, (form, T, H, HKV, D, nkv, n_rows, qkind, sel, cap, have_out)
                if not isinstance(p, int):
                    check_geometry(K, p, form, T, H, HKV, D, nkv, qkind)
                    if p["kernel"] in ("split4", "split5"):
                        ns_seen.add(p["ns"])
                    n += 1
        assert len(ns_seen) <= 1, (form, H, HKV)        # the split count depends on HKV alone: not on T, not on the keys
    assert n


def test_runtime_form(K):
    sweep(K, "runtime", FORCE_PATHS, (0, 1), Ds=(128, 64))


def test_runtime_form_with_the_ta_combine(K):
    """kcpp_flash_attn_dec_ta: force_path 1, one query, the KT_Q8_0_TA combine"""
    sweep(K, "runtime", (1,), (2,))


def test_decode_ex_form(K):
    sweep(K, "ex", VARIANTS, (0, 1))


def test_graph_forms(K):
    sweep(K, "graph1", (0,), (0,), Ds=(128, 64), caps=(False, True))
    sweep(K, "grapht", (0,), (0,), Ds=(128, 64), caps=(False, True))


def test_split_count_is_a_power_of_two_per_cu(K):
    for HKV, ns in ((1, 64), (2, 64), (4, 64), (8, 32), (16, 16), (32, 8), (64, 4), (3, 64), (6, 32), (48, 4)):
        assert splits(HKV) == ns
        for form, nkv, T in (("runtime", 1, 1), ("runtime", 131072, 1), ("graph1", 4096, 1), ("ex", 65, 17)):
            assert K.fa_decode_plan(form, T, 2 * HKV, HKV, 128, nkv, nkv, 0, 5 if form == "ex" else 0)["ns"] == ns


def test_named_cases(K):
    # one query with a quantized output at G = 1: the split pair's combine quantizes head pairs of one kv head only
    # from G = 2 on, so this runs the chunk pair
    p = K.fa_decode_plan("runtime", 1, 8, 8, 128, 700, 700, 1, 0)
    assert p["kernel"] == "chunk" and p["cquant"] == 1 and p["grid"] == (11, 8, 1)
    pair = "split4" if ENV4 else "split5"
    assert K.fa_decode_plan("runtime", 1, 8, 8, 128, 700, 700, 0, 0)["kernel"] == pair
    assert K.fa_decode_plan("runtime", 1, 16, 8, 128, 700, 700, 1, 0)["kernel"] == pair
    # G in {3, 5, 6, 7}: k_fa_dec5 whatever is asked for, and an error without the views' row count
    for G in (3, 5, 6, 7):
        assert K.fa_decode_plan("ex", 1, 2 * G, 2, 128, 700, 700, 0, 3)["kernel"] == "split5"
        assert K.fa_decode_plan("ex", 1, 2 * G, 2, 128, 700, 700, 0, 5)["kernel"] == "split5"
        assert K.fa_decode_plan("ex", 1, 2 * G, 2, 128, 700, 0, 0, 5) == -1
        assert K.fa_decode_plan("runtime", 1, 2 * G, 2, 128, 700, 0, 0, 1) == -1
        assert K.fa_decode_plan("graph1", 1, 2 * G, 2, 128, 700, 700) == -3
        assert K.fa_decode_plan("grapht", 5, 2 * G, 2, 128, 700, 700)["kernel"] == "chunk"
        assert K.fa_decode_plan("runtime", 1, 2 * G, 2, 128, 700, 700, 0, 7)["kernel"] == "short"
    for G in (1, 2, 4, 8):
        assert K.fa_decode_plan("ex", 1, 2 * G, 2, 128, 700, 700, 0, 3)["kernel"] == "split4"
        assert K.fa_decode_plan("ex", 1, 2 * G, 2, 128, 700, 0, 0, 5)["kernel"] == "split4"      # no row count
        assert K.fa_decode_plan("graph1", 1, 2 * G, 2, 128, 700, 700)["kernel"] == "split5"
    # 2048 chunks of 64 keys are k_fa_combine's table: one key more is -4, in every form that runs the chunk pair
    for form, T, sel in (("runtime", 2, 0), ("runtime", 1, 6), ("ex", 1, 0), ("grapht", 16, 0)):
        assert K.fa_decode_plan(form, T, 8, 2, 128, 131072, 131072, 0, sel)["nch"] == 2048
        assert K.fa_decode_plan(form, T, 8, 2, 128, 131073, 131073, 0, sel) == -4
    assert K.fa_decode_plan("runtime", 1, 8, 2, 128, 131073, 131073)["kernel"] in ("split4", "split5")   # no such bound
    # neither output; the prefill without out; the short form's conditions; a cap at D = 64
    assert K.fa_decode_plan("runtime", 1, 8, 2, 128, 9, 9, 0, 0, have_out=False) == -1
    assert K.fa_decode_plan("runtime", 17, 8, 2, 128, 17, 1, 1, 0, have_out=False) == -2
    assert K.fa_decode_plan("runtime", 1, 8, 2, 64, 9, 9, 1, 0, have_out=False) == -2
    assert K.fa_decode_plan("runtime", 2, 8, 2, 128, 9, 9, 0, 7) == -1
    assert K.fa_decode_plan("runtime", 1, 8, 2, 128, 9, 9, 1, 7) == -1
    assert K.fa_decode_plan("grapht", 1, 8, 2, 64, 9, 9, cap=True) == -1
    assert K.fa_decode_plan("grapht", 1, 8, 2, 128, 9, 9, cap=True)["kernel"] == "chunk"
    assert K.fa_decode_plan("runtime", 1, 18, 2, 128, 9, 9) == -1          # G = 9
    assert K.fa_decode_plan("runtime", 1, 18, 2, 64, 9, 9)["kernel"] == "tile"


def test_env_selects_the_legacy_split_kernel_where_it_is_built():
    """KCPP_FA_DEC=4 (read once, so in a child process): the runtime form plans k_fa_dec4 at G in {1, 2, 4, 8}; G in
    {3, 5, 6, 7} still plans k_fa_dec5; kcpp_fa_decode_ex's variants do not ask the environment"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import koboldcpp_amd.lib as K\n"
            "print([K.fa_decode_plan('runtime', 1, 2 * G, 2, 128, 700, 700)['kernel'] for G in range(1, 9)])\n"
            "print([K.fa_decode_plan('runtime', 1, 2 * G, 2, 128, 700, 700, 2, 1)['kernel'] for G in range(2, 9)])\n"
            "print([K.fa_decode_plan('ex', 1, 2 * G, 2, 128, 700, 700, 0, 5)['kernel'] for G in range(1, 9)])\n")
    env = dict(os.environ, KCPP_FA_DEC="4", PYTHONPATH=root)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout
    run, ta, ex = (eval(ln) for ln in out.strip().splitlines()[-3:])
    want = ["split4", "split4", "split5", "split4", "split5", "split5", "split5", "split4"]
    assert run == want and ta == want[1:]
    assert ex == ["split5"] * 8
