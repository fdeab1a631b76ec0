"""Cells of the fused single-token mat-vec for tests/test_gpu_gemv_plan.py: the smallest call that reaches each (kernel,
instance) the launch plan (csrc/gemv_plan.h) can return and each refusal code, and the buffers such a call needs.

enumerate_cells is host only (it asks the plan).  run_cell builds every buffer a kernel of the cell's family may touch --
sized from the cell, never from what the plan says -- calls the real entry once and returns its return code and the
tensors it may have written."""
import ctypes
import itertools

Q4_0, Q5_0, Q8_0, Q2_K, Q3_K, Q4_K, Q5_K, Q6_K = 2, 6, 8, 10, 11, 12, 13, 14
IQ2_XXS, IQ2_XS, IQ3_XXS, IQ1_S, IQ4_NL, IQ3_S, IQ2_S, IQ4_XS, IQ1_M = 16, 17, 18, 19, 20, 21, 22, 23, 29
Q4_K_RS, Q5_K_RS, Q6_K_RS = 112, 113, 114
RS_TYPES = (Q4_K_RS, Q5_K_RS, Q6_K_RS)
UNIT_TYPES = (Q4_K, Q5_K, Q6_K, Q3_K, Q2_K, Q4_0, Q5_0, Q8_0, IQ4_NL, IQ4_XS, IQ2_XXS, IQ2_XS, IQ2_S, IQ3_XXS, IQ3_S, IQ1_S, IQ1_M)
BASE = {Q4_K_RS: Q4_K, Q5_K_RS: Q5_K, Q6_K_RS: Q6_K}
# K from the bottom of every NI / IT / MC class upward: 256, then each multiple of 2048 and one super-block past it
KC = (256,) + tuple(k + d for k in range(2048, 34817, 2048) for d in (0, 256))
P, I, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float


class RopeP(ctypes.Structure):
    _fields_ = [("out", P), ("pos", P), ("ff", P), ("D", I)] + [(n, Fl) for n in (
        "theta_scale", "freq_scale", "ext_factor", "attn_factor", "mscale_ext", "corr0", "corr1")]


class AuxOut(ctypes.Structure):
    """mirror of struct AuxOut (koboldcpp_amd/csrc/kcpp_internal.h)"""
    _fields_ = [("p0", P), ("p1", P), ("p2", P), ("h0", P), ("rope", RopeP), ("rn", P), ("yn", P)]


def cell(entry, t, K_, N, mode, pro, rpw=1, fl=(), D=2, ne=0, wt=0, pos=1):
    return dict(entry=entry, t=t, K=K_, N=list(N), mode=mode, pro=pro, rpw=rpw, fl=list(fl), D=D, ne=ne, wt=wt, pos=pos)


def plan_of(K, c):
    """the plan's answer for a cell: an rc, or the dict of lib.gemv_dec_plan / gemv_qkv_mixed_plan / gemv_qkv_dual_plan"""
    if c["entry"] == "mixed":
        return K.gemv_qkv_mixed_plan(c["K"], c["N"], c["fl"], (0, 1, 2), c["D"])
    if c["entry"] == "dual":
        return K.gemv_qkv_dual_plan(c["t"], c["K"], c["N"][:1], c["N"][1:], c["fl"], ())
    return K.gemv_dec_plan(c["entry"], c["t"], c["K"], c["N"], c["mode"], c["pro"], c["rpw"], c["fl"], (0, 1, 2), c["D"],
                           c["wt"], c["ne"])


def candidates():
    """small calls first, so that the first cell of a key is the cheapest"""
    moe, pair, routed = ("eid", "escale"), ("eid", "eid1", "escale"), ("route_w", "route_out")
    for t, K_, pro in itertools.product(RS_TYPES + UNIT_TYPES, KC, range(3)):
        rs = t in RS_TYPES
        for rpw in (1,) if rs else (1, 2, 4):
            yield cell("dec", t, K_, [4], 0, pro, rpw)
            yield cell("dec", t, K_, [3], 0, pro, rpw)
            yield cell("dec", t, K_, [4], 1, pro, rpw)
        yield cell("dec", t, K_, [4, 2, 2], 2, pro, 2)
        yield cell("dec", t, K_, [4, 3, 2], 2, pro, 2)
        yield cell("dec", t, K_, [4, 2, 2], 2, pro, 2, ("ex",))
        yield cell("dec", t, K_, [4, 2, 2], 2, pro, 2, ("ex", "neox"))
        yield cell("dec", t, K_, [4], 0, pro, 1, moe)
        if rs:
            yield cell("dec", t, K_, [2, 2], 1, pro, 1, ("eid", "eid1"))
            yield cell("dec", t, K_, [2, 2], 1, pro, 1, routed, ne=2)
            yield cell("dec", t, K_, [2, 2], 1, pro, 1, routed, ne=9)
            yield cell("dec", t, K_, [2], 3, pro, 1, pair)
            yield cell("dec", t, K_, [2], 3, pro, 1)
            for aux, mode, nw in itertools.product((("aux", "aux_p0h0"), ("aux", "aux_p0h0", "aux_glu"), ("aux", "aux_rope", "aux_rope_ok"),
                                                    ("aux", "aux_rope"), ("aux",)), (0, 1), ((), ("nw",))):
                yield cell("rs_aux", t, K_, [4], mode, 0, 1, aux + nw)
    for t, K_, pro in itertools.product(RS_TYPES, KC, range(3)):
        if K_ <= 12544:
            yield cell("dec", t, K_, [16386], 0, pro)             # the output head's shape: two rows per group
    for K_, mode, pro in itertools.product((2048, 4096, 14336), range(3), range(3)):
        N = [4, 2, 2] if mode == 2 else [4]
        yield cell("q4k", Q4_K, K_, N, mode, pro)
        yield cell("q4k", Q4_K, K_, [3] + N[1:], mode, pro)
        yield cell("stream", Q4_K, K_, N, mode, pro)
        yield cell("stream", Q5_K, K_, N, mode, pro)
    for K_, N, fl in itertools.product((2048, 4096, 6144, 8192), ([4, 2, 2], [4, 3, 2]), ((), ("ex",), ("ex", "neox"))):
        yield cell("mixed", Q4_K_RS, K_, N, 2, 1, 2, fl)
    for t, K_, N in itertools.product(RS_TYPES + (Q4_K,), (2048, 2304, 4096, 6144), ([4, 2, 2], [4, 3, 2])):
        yield cell("dual", t, K_, N, 2, 1, 2)


def enumerate_cells(K):
    """one cell per (kernel, instance parameters) and per (entry, type, mode, refusal code); each with its plan"""
    seen, out = set(), []
    for c in candidates():
        p = plan_of(K, c)
        if isinstance(p, int):
            key = (c["entry"], c["t"], c["mode"], p)
        elif c["entry"] in ("mixed", "dual"):
            key = (c["entry"], c["t"]) + tuple(v for k, v in sorted(p.items()) if k in ("NIA", "NIB", "MC", "EX", "a_NI", "b_IT"))
        else:
            key = tuple(p[k] for k in ("kernel", "type", "mode", "pro", "NI", "IT", "LPR", "R", "MC", "PF", "waves", "XL", "ROUTE", "EX"))
        if key not in seen:
            seen.add(key)
            out.append(dict(c, rc=p if isinstance(p, int) else 0))
    return out


def run_cell(torch, K, c, seed=3):
    """-> (rc, [tensors the call may have written])"""
    t, Kd, N, mode, pro, fl = c["t"], c["K"], c["N"], c["mode"], c["pro"], set(c["fl"])
    s = torch.cuda.current_stream().cuda_stream
    L = K.raw()
    L.kcpp_gemv_rs_aux.argtypes = [I, P, I, P, P]
    L.kcpp_gemv_rs_qkv_mixed.argtypes = [P, P]
    L.kcpp_gemv_qkv_dual.argtypes = [P, I, P, P]
    dev = "cuda"
    g = torch.Generator(device="cpu").manual_seed(seed)
    rows = sum(N)
    n_exp = max(2, c["ne"])          # the routed GLU's ids are below route_ne: every routable expert has its slice
    keep, outs = [], []

    def f32(n):
        v = torch.randn(n, generator=g).to(dev)
        keep.append(v)
        return v

    def out(n, dtype=torch.float32):
        v = torch.zeros(n, dtype=dtype, device=dev)
        outs.append(v)
        return v

    def weights(ty, n, tid):
        """n_exp expert slices of [n rows x Kd] of type ty"""
        w = torch.empty(K.row_bytes(ty, Kd) * n * n_exp, dtype=torch.uint8, device=dev)
        for e in range(n_exp):
            K.call("kcpp_weight_synth", ty, 7, tid * 8 + e, w.data_ptr() + e * K.row_bytes(ty, Kd) * n, Kd, n, s)
        keep.append(w)
        return w

    def args(ty, Ns, roles, tid0):
        a = K.DecArgs()
        a.K, a.nseg, a.eps, a.D = Kd, len(Ns), 1e-5, c["D"]
        x = f32(2 * Kd)                                    # mode 3 reads slot 1's row at x + K
        nw = 1 + 0.01 * f32(Kd)
        keep.append(nw)
        base = Q4_K if isinstance(ty, list) else BASE.get(ty, ty)
        act = torch.zeros(2 * K.act_bytes(base, Kd, 1) + 64, dtype=torch.uint8, device=dev)
        K.call("kcpp_quantize_act", K.vec_dot_type(base), x.data_ptr(), Kd, act.data_ptr(), Kd, 1, s)
        keep.append(act)
        a.x, a.nw, a.act = x.data_ptr(), nw.data_ptr(), act.data_ptr()
        for i, n in enumerate(Ns):
            w = weights(ty[i] if isinstance(ty, (list, tuple)) else ty, n, tid0 + i)
            a.W[i], a.N[i], a.role[i], a.Y[i] = w.data_ptr(), n, roles[i], out(n).data_ptr()
        return a

    def common(a, Ns, ty):
        n = sum(Ns)
        if mode == 1:
            a.W2 = weights(ty, max(Ns), 5).data_ptr()
        if mode in (0, 3) and len(Ns) == 1:
            a.res = f32(n).data_ptr()
        if mode == 2:
            ekv = max(Ns)
            a.q16, a.kc, a.vc = (out((c["pos"] + 1) * ekv, torch.int16).data_ptr() for _ in range(3))
            a.ekv = ekv
            posd = torch.tensor([c["pos"]], dtype=torch.int32, device=dev)
            keep.append(posd)
            tab = f32((c["pos"] + 1) * c["D"])             # (cos, sin) per position and pair
            a.pos, a.rope_tab = posd.data_ptr(), tab.data_ptr()
        if {"eid", "eid1", "route_w"} & fl:
            ids = torch.tensor([1, 0], dtype=torch.int32, device=dev)
            keep.append(ids)
            a.n_exp, a.ebytes = n_exp, K.row_bytes(ty, Kd) * Ns[0]
            if "eid" in fl:
                a.eid = ids.data_ptr()
            if "eid1" in fl:
                a.eid1 = ids.data_ptr() + 4
            if len(Ns) == 2:
                a.W[1] = a.W[0]                            # the two slots read the same expert tensors
        if "escale" in fl:
            a.escale = f32(2).data_ptr()
        if "route_w" in fl:
            a.route_w, a.route_wt, a.route_ne = f32(max(c["ne"], 2) * Kd).data_ptr(), c["wt"], c["ne"]
            if "route_out" in fl:
                a.route_ids, a.route_wts = out(2, torch.int32).data_ptr(), out(2).data_ptr()
        if "ex" in fl:
            for i, n in enumerate(Ns):
                a.bias[i] = f32(n).data_ptr()
        if "neox" in fl:
            a.rope_neox = 1

    if c["entry"] == "mixed":
        a = args([Q4_K_RS, Q4_K_RS, Q6_K_RS], N, (0, 1, 2), 1)
        common(a, N, Q4_K_RS)
        rc = L.kcpp_gemv_rs_qkv_mixed(ctypes.byref(a), s)
    elif c["entry"] == "dual":
        a = args(t, N[:1], (0,), 1)
        common(a, N[:1], t)
        b = args(Q8_0, N[1:], (1, 2), 2)
        common(b, N[1:], Q8_0)
        rc = L.kcpp_gemv_qkv_dual(ctypes.byref(a), t, ctypes.byref(b), s)
    else:
        a = args(t, N, (0, 1, 2), 1)
        common(a, N, t)
        if c["entry"] == "dec":
            rc = L.kcpp_gemv_dec(t, ctypes.byref(a), mode, pro, c["rpw"], s)
        elif c["entry"] == "q4k":
            rc = L.kcpp_gemv_q4k(ctypes.byref(a), mode, pro, s)
        elif c["entry"] == "stream":
            rc = L.kcpp_gemv_stream(t, ctypes.byref(a), mode, pro, s)
        elif c["entry"] == "rs":
            rc = L.kcpp_gemv_rs(t, ctypes.byref(a), mode, pro, s)
        else:
            assert c["entry"] == "rs_aux", c
            o = AuxOut()
            if "nw" not in fl:
                a.nw = None
            if "aux_p0h0" in fl:
                o.p0, o.h0 = out(rows).data_ptr(), out(rows, torch.int16).data_ptr()
            if "aux_glu" in fl:
                o.p1, o.p2 = out(rows).data_ptr(), out(rows).data_ptr()
            if "aux_rope" in fl:
                o.rope.out = out(rows).data_ptr()
            if "aux_rope_ok" in fl:
                posd = torch.tensor([c["pos"]], dtype=torch.int32, device=dev)
                keep.append(posd)
                o.rope.pos, o.rope.D = posd.data_ptr(), 2
                o.rope.theta_scale, o.rope.freq_scale, o.rope.attn_factor, o.rope.mscale_ext, o.rope.corr1 = 0.5, 1.0, 1.0, 1.0, 1.0
            o.rn, o.yn = out(Kd).data_ptr(), out(Kd).data_ptr()
            rc = L.kcpp_gemv_rs_aux(t, ctypes.byref(a), mode, ctypes.byref(o), s)
    torch.cuda.synchronize()
    return int(rc), outs
