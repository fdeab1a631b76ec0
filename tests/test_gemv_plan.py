"""The launch plan of the fused single-token mat-vec (csrc/gemv_plan.h through kcpp_gemv_dec_plan), host only.

`expect` below restates, independently of the C++, which of the five kernels each entry runs for a call, with which
instance parameters and with which return code (the rules block at the top of gemv_plan.h); the sweeps hold the plan to
it, re-derive every grid and LDS size, and check that every plan names an instance its kernel file builds."""
import itertools

import pytest

Q4_0, Q4_1, Q5_0, Q5_1, Q8_0, Q2_K, Q3_K, Q4_K, Q5_K, Q6_K = 2, 3, 6, 7, 8, 10, 11, 12, 13, 14
IQ2_XXS, IQ2_XS, IQ3_XXS, IQ1_S, IQ4_NL, IQ3_S, IQ2_S, IQ4_XS, IQ1_M = 16, 17, 18, 19, 20, 21, 22, 23, 29
F32, F16 = 0, 1
Q4_K_RS, Q5_K_RS, Q6_K_RS = 112, 113, 114
RS_TYPES = (Q4_K_RS, Q5_K_RS, Q6_K_RS)
UNIT32 = (Q4_0, Q5_0, Q8_0, IQ4_NL)                     # 32 elements per unit, Q8_0 activation
UNIT64 = (Q4_K, Q5_K, Q6_K, Q3_K, Q2_K, IQ4_XS, IQ2_XXS, IQ2_XS, IQ2_S, IQ3_XXS, IQ3_S, IQ1_S, IQ1_M)
UNIT_TYPES = UNIT32 + UNIT64                            # every type kcpp_gemv_dec switches on
KS = (256, 2048, 4096, 4352, 8192, 14336, 14592, 20480, 20736, 28672, 28928, 32768, 33024)
NS = (2, 3, 4096, 16384, 16386, 128256)
RS_NSB_MAX = {Q4_K_RS: 112, Q5_K_RS: 80, Q6_K_RS: 128, Q4_K: 112, Q5_K: 80, Q6_K: 128}
# the instances the kernel files build (their KCPP_*_INSTANCES lists)
UNIT_BUILT = {(2, 2, 1, 1), (2, 2, 1, 2), (2, 1, 1, 1), (2, 1, 1, 2), (1, 1, 1, 1), (1, 1, 1, 2), (4, 0, 0, 1), (2, 0, 0, 1),
              (1, 0, 0, 1), (2, 0, 1, 1), (2, 0, 1, 2), (1, 0, 1, 1), (1, 0, 1, 2), (1, 0, 2, 2), (1, 0, 2, 4), (1, 0, 2, 8)}
Q4K_BUILT = {(1, 2, 1, 1, 1, 1), (1, 2, 2, 1, 1, 0), (1, 1, 0, 0, 1, 0), (1, 2, 0, 1, 1, 1), (4, 1, 0, 2, 4, 0), (4, 1, 0, 0, 4, 0)}
RS_BUILT = ({(R, m, p, pf, 4, 0, 0) for p in (0, 1, 2) for (R, m, pf) in
             ((1, 1, 1), (1, 1, 0), (2, 2, 0), (2, 0, 1), (2, 0, 0), (1, 0, 1), (1, 0, 0))} |
            {(1, 1, 1, 1, 8, 0, 0), (1, 0, 2, 0, 8, 0, 0), (2, 2, 1, 0, 4, 0, 1)})
RS_AUX_BUILT = {(2, 0, 2, 0, 4), (2, 0, 1, 0, 4), (1, 0, 2, 0, 8), (1, 1, 2, 1, 4), (1, 1, 1, 1, 8)}
RS_XL_BUILT = {(1, 0, 2), (1, 0, 1), (1, 0, 0), (1, 1, 1), (1, 1, 0), (2, 2, 1)}
RS_CLASSES = {Q4_K_RS: {(1, 1, 0), (2, 1, 0), (3, 2, 0), (4, 2, 0), (5, 3, 0), (6, 3, 0), (7, 4, 0), (10, 5, 1), (12, 6, 1), (14, 7, 1)},
              Q5_K_RS: {(1, 1, 0), (2, 1, 0), (3, 2, 0), (4, 2, 0), (5, 3, 0), (6, 3, 0), (7, 4, 0), (10, 5, 1)},
              Q6_K_RS: {(1, 1, 0), (2, 2, 0), (3, 3, 0), (4, 4, 0), (6, 6, 1), (8, 8, 1)}}


@pytest.fixture(scope="module")
def K():
    import koboldcpp_amd.lib as K
    return K


def cdiv(a, b):
    return -(-a // b)


def q8k_bytes(K_):
    return K_ + K_ // 256 * 4 + K_ // 16 * 2


def slot_grid(groups, wpg, cap, slots=64):
    """at most `cap` workgroups, but never more than `slots` groups for a wave to park"""
    return max(min(cdiv(groups, wpg), cap), cdiv(groups, slots * wpg))


def rs_supported(t, K_):
    nsb = K_ // 256
    if K_ % 256 or K_ < 256 or t not in RS_NSB_MAX or nsb > RS_NSB_MAX[t]:
        return False
    return nsb % 8 == 0 if t in (Q6_K, Q6_K_RS) else True


def rs_class(t, K_):
    """(NI, MC, XL) of a supported (type, K)"""
    pieces = K_ // 256 * (4 if t == Q6_K_RS else 8)
    ni, mc = cdiv(pieces, 64), cdiv(K_, 4096)
    if ni <= (4 if t == Q6_K_RS else 7):
        return ni, mc, 0
    ceil_ = min(c for c in {Q4_K_RS: (10, 12, 14), Q5_K_RS: (10,), Q6_K_RS: (6, 8)}[t] if c >= ni)
    return ceil_, (ceil_ if t == Q6_K_RS else ceil_ // 2), 1


def ex_ok(N, role, D, neox, segs):
    for i in segs:
        if not 0 <= role[i] <= 2:
            return False
        if neox and role[i] != 2 and (D < 2 or D % 2 or N[i] % D):
            return False
    return True


def expect_rs(t, K_, N, mode, pro, fl, role, D, route_wt, route_ne, aux):
    rows, nseg = sum(N), len(N)
    ex = "ex" in fl or "neox" in fl
    if aux:
        if "aux" not in fl or mode not in (0, 1):
            return -3
        if mode == 0 and not ({"aux_p0h0", "aux_rope"} & fl):
            return -3
        if mode == 1 and "aux_glu" not in fl:
            return -3
        if "aux_rope" in fl and (mode != 0 or "aux_rope_ok" not in fl):
            return -3
        pro = 1 if "nw" in fl else 2
        if pro == 1 and K_ > 4096:
            return -3
    if t not in RS_TYPES or not rs_supported(t, K_):
        return -3
    ni, mc, xl = rs_class(t, K_)
    d = dict(kernel="rs_aux" if aux else "rs", type=t, mode=mode, pro=pro, NI=ni, MC=mc, XL=xl, R=1, PF=0, waves=4, ROUTE=0,
             EX=0)
    if mode == 3:
        if pro != 2 or nseg != 1 or not {"eid", "eid1", "escale"} <= fl or K_ != 14336:
            return -3
        d.update(waves=8)
        cap = 256
    else:
        if mode == 1 and not (nseg == 1 or (nseg == 2 and ({"eid1", "route_w"} & fl))):
            return -3
        if mode == 2 and ex:
            if {"eid", "route_w"} & fl or not ex_ok(N, role, D, "neox" in fl, range(nseg)):
                return -3
            if aux or xl or pro != 1:
                return -3
        if xl:
            if aux or pro not in {0: (0, 1, 2), 1: (0, 1), 2: (1,)}[mode]:
                return -3
            if mode == 1 and ("route_w" in fl or (nseg == 2 and "eid1" not in fl)):
                return -3
            d.update(R=2 if mode == 2 else 1, waves=8)
            cap = 256
        elif aux:
            if "aux_rope" in fl:
                if rows > 16384 or rows % 2 or (pro == 1 and mc != 1):
                    return -3
                d.update(R=2)
                cap = 512
            elif mode == 0:
                if pro != 2 or rows > 16384:
                    return -3
                d.update(waves=8)
                cap = 256
            else:
                if nseg != 1 or {"eid", "route_w"} & fl or (pro == 1 and mc != 1):
                    return -3
                d.update(PF=1, waves=8 if pro == 1 else 4)
                cap = 256 if pro == 1 else 512
        else:
            if pro not in (0, 1, 2):
                return -3
            if mode == 2:
                d.update(R=2, EX=int(ex))
                cap = 512
            elif mode == 1:
                d.update(PF=1)
                cap = 512
                if pro == 1:
                    d.update(waves=8)
                    cap = 256
                    if "route_w" in fl:
                        if not (mc == 1 and nseg == 2 and 2 <= route_ne <= 8 and K_ <= 4096 and "route_out" in fl and
                                route_wt in (F32, F16)):
                            return -3
                        d.update(ROUTE=1)
            elif rows > 16384:
                d.update(R=2)
                cap = 512
            elif pro == 2:
                d.update(waves=8)
                cap = 256
            elif K_ > 8192:
                d.update(PF=int(t == Q4_K_RS))
                cap = 256 if t == Q4_K_RS else 512
            else:
                cap = 1024
    if any(n % d["R"] for n in N):
        return -5
    wpg = d["waves"] // 2 if mode == 3 else d["waves"]
    lds = 2 * ((q8k_bytes(K_) + 15) // 16 * 16) if mode == 3 else q8k_bytes(K_)
    d.update(nblk=slot_grid(rows // d["R"], wpg, cap), block=64 * d["waves"], lds_bytes=lds + 16)
    return d


def expect_q4k(K_, N, mode, pro, fl):
    table = {(4096, 1, 1): (1, 2, 1, 1), (4096, 2, 1): (1, 2, 1, 0), (4096, 0, 0): (1, 1, 1, 0), (4096, 0, 1): (1, 2, 1, 1),
             (14336, 0, 2): (4, 1, 4, 0), (14336, 0, 0): (4, 1, 4, 0)}            # (K, mode, pro) -> IT, R, MC, PF
    if (mode == 2 and {"ex", "neox"} & fl) or (K_, mode, pro) not in table:
        return -3
    it, R, mc, pf = table[(K_, mode, pro)]
    if any(n % R for n in N):
        return -5
    cap = 256 if mode == 1 and R == 2 else 512
    return dict(kernel="q4k", type=Q4_K, mode=mode, pro=pro, IT=it, R=R, MC=mc, PF=pf, waves=4, block=256,
                nblk=slot_grid(sum(N) // R, 4, cap), lds_bytes=q8k_bytes(K_) + 16)


def expect_stream(t, K_, N, mode, pro, fl):
    if t != Q4_K or "eid" in fl or (K_, mode, pro) != (14336, 0, 2):
        return -3
    nsb = K_ // 256
    return dict(kernel="stream", type=Q4_K, mode=0, pro=2, LPR=64, NI=8, MC=4, R=1, waves=4, block=256,
                nblk=slot_grid(sum(N), 4, 1024, slots=64), lds_bytes=(q8k_bytes(K_) + 15) // 16 * 16 + 4 * 1 * 1 * nsb * 20)


def expect_unit(t, K_, N, mode, pro, rpw):
    if t not in UNIT_TYPES:
        return -3
    if mode in (1, 2) and pro != 1:
        return -7
    chunks = cdiv(K_, 4096)
    if mode not in (1, 2):
        mode = 0
        pro = pro if pro in (0, 1) else 2
    if mode == 2:
        R = 2
    elif pro == 2:
        R = 1
    else:
        R = 4 if (mode, pro) == (0, 0) and rpw >= 4 else (2 if rpw >= 2 else 1)
    MC = 1 if pro == 0 else ((1 if chunks <= 1 else 2) if pro == 1 else (2 if chunks <= 2 else (4 if chunks <= 4 else 8)))
    slices = cdiv(K_ // (32 if t in UNIT32 else 64), 64)
    allowed = (2, 4, 8) if pro == 2 else (1, 2, 4)
    if slices > allowed[-1]:
        return -8
    IT = min(i for i in allowed if i >= slices)
    if any(n % R for n in N):
        return -5
    if pro != 0 and K_ > 4096 * MC:
        return -6
    act = K_ + K_ // 32 * 4 + K_ // 32 * 2 if t in UNIT32 else q8k_bytes(K_)
    return dict(kernel="unit", type=t, mode=mode, pro=pro, R=R, MC=MC, IT=IT, waves=4, block=256,
                nblk=min(cdiv(sum(N) // R, 4), 512 if K_ > 4096 else 1024), lds_bytes=act + 16 if pro else 0)


def expect(entry, t, K_, N, mode, pro, rpw=1, fl=frozenset(), role=(0, 1, 2), D=0, route_wt=0, route_ne=0):
    fl = frozenset(fl)
    if entry == "rs" or entry == "rs_aux" or (entry == "dec" and t in RS_TYPES):
        return expect_rs(t, K_, N, mode, pro, fl, role, D, route_wt, route_ne, entry == "rs_aux")
    if entry == "q4k":
        return expect_q4k(K_, N, mode, pro, fl)
    if entry == "stream":
        return expect_stream(t, K_, N, mode, pro, fl)
    if entry == "unit":
        return expect_unit(t, K_, N, mode, pro, rpw)
    if mode == 2 and {"ex", "neox"} & fl:
        return -3
    if t == Q4_K:
        r = expect_q4k(K_, N, mode, pro, fl)
        if r != -3:
            return r
    return expect_unit(t, K_, N, mode, pro, rpw)        # the stream kernel's one shape is the Q4_K kernel's first


def check(K, entry, t, K_, N, mode, pro, rpw=1, fl=(), **kw):
    got = K.gemv_dec_plan(entry, t, K_, N, mode, pro, rpw, tuple(fl), **kw)
    want = expect(entry, t, K_, N, mode, pro, rpw, fl, **kw)
    ctx = (entry, t, K_, N, mode, pro, rpw, tuple(fl), kw)
    if isinstance(want, int):
        assert got == want, ctx
        return got
    assert isinstance(got, dict), (got, ctx)
    for k, v in want.items():
        assert got[k] == v, (k, got[k], v, ctx)
    built(got, ctx)
    return got


def built(p, ctx):
    """the plan names an instance of its kernel file's list, and a wave never has more groups than result slots"""
    if p["kernel"] == "unit":
        assert (p["R"], p["mode"], p["pro"], p["MC"]) in UNIT_BUILT and p["IT"] in ((2, 4, 8) if p["pro"] == 2 else (1, 2, 4)), ctx
        return
    if p["kernel"] == "q4k":
        assert (p["IT"], p["R"], p["mode"], p["pro"], p["MC"], p["PF"]) in Q4K_BUILT, ctx
    elif p["kernel"] == "stream":
        assert (p["LPR"], p["NI"], p["mode"], p["pro"], p["MC"]) == (64, 8, 0, 2, 4), ctx
    else:
        assert (p["NI"], p["MC"], p["XL"]) in RS_CLASSES[p["type"]], ctx
        if p["mode"] == 3:
            assert (p["NI"], p["MC"], p["R"], p["pro"], p["waves"], p["XL"]) == (4 if p["type"] == Q6_K_RS else 7, 4, 1, 2, 8, 0), ctx
        elif p["XL"]:
            assert (p["R"], p["mode"], p["pro"]) in RS_XL_BUILT and (p["PF"], p["waves"], p["ROUTE"], p["EX"]) == (0, 8, 0, 0), ctx
            assert p["kernel"] == "rs", ctx
        elif p["kernel"] == "rs_aux":
            assert (p["R"], p["mode"], p["pro"], p["PF"], p["waves"]) in RS_AUX_BUILT, ctx
        elif p["ROUTE"]:
            assert (p["R"], p["mode"], p["pro"], p["PF"], p["waves"], p["EX"], p["MC"]) == (1, 1, 1, 1, 8, 0, 1), ctx
        else:
            assert (p["R"], p["mode"], p["pro"], p["PF"], p["waves"], p["ROUTE"], p["EX"]) in RS_BUILT, ctx
    rows = sum(ctx[3])
    wpg = p["waves"] // 2 if p["mode"] == 3 else p["waves"]
    assert cdiv(rows // p["R"], p["nblk"] * wpg) <= 64, ctx
    assert p["nblk"] >= 1 and p["lds_bytes"] <= 160 * 1024, ctx


def seg_lists():
    for n in NS:
        for nseg in (1, 2, 3):
            yield [n] * nseg
    yield [4096, 1024, 1024]
    yield [4096, 1024, 3]


def test_dec_entry_every_type(K):
    """kcpp_gemv_dec without flags: every type, K, segment list, mode, prologue and rows-per-wave"""
    kernels = set()
    for t in UNIT_TYPES + RS_TYPES + (Q4_1, Q5_1, F16):
        rpws = (1,) if t in RS_TYPES else (1, 2, 4)
        for K_, N, mode, pro, rpw in itertools.product(KS, seg_lists(), range(4), range(3), rpws):
            p = check(K, "dec", t, K_, N, mode, pro, rpw)
            if isinstance(p, dict):
                kernels.add(p["kernel"])
    assert kernels == {"rs", "q4k", "unit"}


FLAG_SETS = [("eid",), ("eid1",), ("escale",), ("route_w",), ("route_out",), ("ex",), ("ex", "neox"), ("nw",),
             ("eid", "eid1"), ("eid", "eid1", "escale"), ("eid", "escale"), ("route_w", "route_out"),
             ("route_w", "route_out", "eid"), ("ex", "eid"), ("ex", "neox", "route_w")]


@pytest.mark.parametrize("entry", ["dec", "rs"])
def test_flags_rs_types(K, entry):
    """each presence flag alone and the runtime's combinations over the RS types (and, through kcpp_gemv_rs, the -3 of
    every other type)"""
    routed = 0
    for t in RS_TYPES + ((Q4_K, Q8_0) if entry == "rs" else ()):
        for fl, K_, N, mode, pro in itertools.product(FLAG_SETS, KS, seg_lists(), range(4), range(3)):
            for ne, wt, D in ((8, F16, 128), (1, F32, 128), (8, Q8_0, 3), (9, F32, 0)) if {"route_w", "neox"} & set(fl) else ((0, 0, 128),):
                p = check(K, entry, t, K_, N, mode, pro, 1, fl, D=D, route_wt=wt, route_ne=ne)
                routed += isinstance(p, dict) and p["ROUTE"]
    assert routed
    # roles: out of range, and v in front (NeoX heads are checked on the q / k segments only)
    for role, D in (((0, 1, 3), 128), ((2, 2, 2), 3), ((-1, 1, 2), 128)):
        check(K, entry, Q4_K_RS, 4096, [4096, 1024, 1024], 2, 1, 1, ("ex", "neox"), role=role, D=D)


def test_flags_other_types(K):
    for t, fl, K_, N, mode, pro in itertools.product((Q4_K, Q6_K, Q8_0), FLAG_SETS, KS, seg_lists(), range(4), range(3)):
        check(K, "dec", t, K_, N, mode, pro, 2, fl)


def test_family_entries(K):
    """the single-family entries: the plan restricted to one kernel, with the -3 the tests of the entries assert"""
    seen = set()
    for fl, K_, N, mode, pro in itertools.product([(), ("eid",), ("ex",), ("ex", "neox")], KS, seg_lists(), range(4), range(3)):
        for entry, t in (("q4k", Q4_K), ("stream", Q4_K), ("stream", Q5_K), ("stream", Q4_K_RS)):
            p = check(K, entry, t, K_, N, mode, pro, 1, fl)
            if isinstance(p, dict):
                seen.add(p["kernel"])
        for t, rpw in itertools.product((Q4_K, Q4_0, IQ1_M, Q4_1, Q4_K_RS), (1, 2, 4)):
            check(K, "unit", t, K_, N, mode, pro, rpw, fl)
    assert seen == {"q4k", "stream"}


AUX_SETS = [(), ("aux",), ("aux", "aux_p0h0"), ("aux", "aux_glu"), ("aux", "aux_p0h0", "aux_glu"), ("aux", "aux_rope"),
            ("aux", "aux_rope", "aux_rope_ok"), ("aux", "aux_rope", "aux_rope_ok", "aux_p0h0"), ("aux", "aux_rope_ok", "aux_p0h0"),
            ("aux", "aux_glu", "aux_rope", "aux_rope_ok")]


def test_aux_entry(K):
    """kcpp_gemv_rs_aux: each aux kind, with and without the norm-in prologue, an expert id and a router"""
    kinds = set()
    for t in RS_TYPES + (Q4_K,):
        for aux, more, K_, N, mode in itertools.product(AUX_SETS, [(), ("nw",), ("eid",), ("route_w",), ("nw", "eid1")], KS,
                                                        seg_lists(), range(4)):
            p = check(K, "rs_aux", t, K_, N, mode, 0, 1, aux + more)
            if isinstance(p, dict):
                assert p["kernel"] == "rs_aux"
                kinds.add((p["R"], p["mode"], p["pro"], p["PF"], p["waves"]))
    assert kinds == RS_AUX_BUILT


def test_rs_supported(K):
    for t in RS_TYPES + UNIT_TYPES + (Q4_1, F16):
        for K_ in KS + (0, 128, 2304, 28672 + 256, 32768 + 2048):
            assert bool(K.raw().kcpp_rs_supported(t, K_)) == rs_supported(t, K_), (t, K_)


def test_mixed_plan(K):
    """q|k (Q4_K_RS) + v (Q6_K_RS): the RS mode-2 launch's grid at the same row count; instances at K 2048, 4096, 8192"""
    ok = 0
    for K_, N, fl in itertools.product(KS + (2304,), ([4096, 1024, 1024], [4096, 1024, 3], [2, 2, 2], [128256, 2, 2], [256, 128, 64]),
                                       [(), ("ex",), ("ex", "neox")]):
        for role, D in (((0, 1, 2), 128), ((0, 1, 2), 3), ((1, 0, 2), 128)):
            got = K.gemv_qkv_mixed_plan(K_, N, fl, role, D)
            ctx = (K_, N, fl, role, D)
            if K_ not in (2048, 4096, 8192) and not any(n % 2 for n in N) or K_ > 28672:
                assert got == -3, ctx
            if not (rs_supported(Q4_K_RS, K_) and rs_supported(Q6_K_RS, K_)):
                assert got == -3, ctx
            elif any(n % 2 for n in N):
                assert got == -5, ctx
            elif fl and (role != (0, 1, 2) or ("neox" in fl and (D % 2 or N[0] % D or N[1] % D))):
                assert got == -3, ctx
            elif K_ in (2048, 4096, 8192):
                rs = K.gemv_dec_plan("rs", Q4_K_RS, K_, [sum(N)], 2, 1)
                assert (got["NIA"], got["NIB"], got["MC"]) == {2048: (1, 1, 1), 4096: (2, 1, 1), 8192: (4, 2, 2)}[K_], ctx
                assert (got["nblk"], got["block"], got["lds_bytes"]) == (rs["nblk"], rs["block"], rs["lds_bytes"]), ctx
                assert got["nblk"] == slot_grid(sum(N) // 2, 4, 512) and got["EX"] == bool(fl), ctx
                ok += 1
    assert ok


def test_dual_plan(K):
    """q (RS) + k|v (Q8_0): the halves are the RS plan of q and the unit plan of k|v; instances at IT 2 with NI 2 / 1"""
    ok = 0
    for qt, K_, Na, Nb, fa, fb in itertools.product(RS_TYPES + (Q4_K,), (256, 2048, 2304, 4096, 4352, 8192), ([4096], [2], [3], [128256]),
                                                    ([1024, 1024], [1024, 3], [2]), [(), ("ex",), ("route_w",)], [(), ("neox",)]):
        got = K.gemv_qkv_dual_plan(qt, K_, Na, Nb, fa, fb)
        ctx = (qt, K_, Na, Nb, fa, fb)
        covered = qt in RS_TYPES and K_ <= 4096 and rs_supported(qt, K_) and not fa and not fb
        if not covered:
            assert got == -3, ctx
        elif any(n % 2 for n in Na + Nb):
            assert got == -5, ctx
        elif not (K_ > 2048 and (qt != Q6_K_RS or K_ == 4096)):
            assert got == -3, ctx
        else:
            a = K.gemv_dec_plan("rs", qt, K_, Na, 2, 1)
            b = K.gemv_dec_plan("unit", Q8_0, K_, Nb, 2, 1, 2)
            assert (got["a_nblk"], got["a_lds_bytes"], got["a_NI"]) == (a["nblk"], a["lds_bytes"], a["NI"]), ctx
            assert (got["b_nblk"], got["b_lds_bytes"], got["b_IT"]) == (b["nblk"], b["lds_bytes"], b["IT"]), ctx
            assert got["nblk"] == a["nblk"] + b["nblk"] and got["lds_bytes"] == max(a["lds_bytes"], b["lds_bytes"]), ctx
            assert (a["R"], a["waves"], a["MC"], a["XL"], b["R"], b["IT"]) == (2, 4, 1, 0, 2, 2), ctx
            ok += 1
    assert K.gemv_qkv_dual_plan(Q5_K_RS, 4096, [4096], [1024, 1024], Kb=2048) == -3
    assert ok
