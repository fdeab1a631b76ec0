"""Grammar-constrained sampling on the host (koboldcpp_amd/csrc/grammar.h through the kcpp_grammar_* test hooks), no GPU.

* Against tests/golden/grammar.npz (tests/golden/make_grammar.py: the reference's llama-grammar.cpp behind a driver):
  the parsed element arrays element for element, the initial stack count, and over scripted and seeded token walks on a
  synthetic vocabulary the reject bitmask bit for bit before every token, the stack count and the carried UTF-8 state
  after it.  The decoded-once vocabulary and the per-step decode must give the same mask.  Texts the reference makes no
  grammar of (a syntax error, an undefined rule, left recursion, no root) give none here.
* The sampled chain on a masked array: sample_grammar only writes -INFINITY before sample_dry, so the reference's
  SampleLogits on logits with -inf at the rejected ids (oracle/_ref/ref_sampler, built or skipped as
  tests/test_sampler_ref.py does) is the reference with that grammar state.  kcpp_sampler_probe on the same array and
  the masked front end's host path (kcpp_sampler_probe_front_masked: the masked CPU model of the device pass, then the
  bucket tail or the rebuild) must draw the same token.
* The masked CPU model itself against numpy."""
import ctypes
import os

import numpy as np
import pytest
import torch  # noqa: F401  (before the library, as tests/test_pipeline.py has it: this module is the first one collected
#               that loads the library, and loaded ahead of torch it brings up a HIP runtime of its own, apart from the
#               one torch ships, in which the process's later kernel launches find no device)

import koboldcpp_amd.lib as K
import test_sampler as TS
from test_sample_front import CTX, RESTARTS

HERE = os.path.dirname(os.path.abspath(__file__))
FX = np.load(os.path.join(HERE, "golden", "grammar.npz"))
L = K.raw()
P_ = ctypes.c_void_p
BLOB, OFF, EOS = np.ascontiguousarray(FX["vocab_blob"]), np.ascontiguousarray(FX["vocab_off"]), int(FX["eos"])
NV = len(OFF) - 1
NW = (NV + 31) // 32
CASES = list(range(int(FX["n_cases"])))
NAMES = [str(x) for x in FX["names"]]


def piece(i):
    return BLOB[OFF[i]:OFF[i + 1]].tobytes()


def create(i):
    return L.kcpp_grammar_create(FX["text_%d" % i].tobytes())


def reject(g, use_cache):
    m = np.zeros(NW, np.uint32)
    n = L.kcpp_grammar_reject(g, BLOB.ctypes.data_as(P_), OFF.ctypes.data_as(P_), NV, EOS, -1, int(use_cache), m.ctypes.data_as(P_))
    return n, m


def state(g):
    out = (ctypes.c_int64 * 2)()
    L.kcpp_grammar_partial(g, out)
    return [L.kcpp_grammar_n_stacks(g), out[0], out[1]]


def test_fixture_covers_what_it_should():
    good = {NAMES[i] for i in CASES if int(FX["ok_%d" % i])}
    bad = {NAMES[i] for i in CASES if not int(FX["ok_%d" % i])}
    assert len(good) >= 8 and {"bad_syntax", "bad_undefined", "bad_left_recursion"} <= bad
    assert 200 <= NV <= 1000 and piece(EOS) == b""
    ps = {piece(i) for i in range(NV)}
    assert {b"ye", b"s\n", b'{"', b"\x00", b"\xc3", b"\xa9", b"\xe6\x97", b"\xa5", b"\xf0\x9f", b"\x98\x80", b"\xc0\x80", b"\x80"} <= ps
    # some walk carries an unfinished character of each length across a token
    remain = set()
    for i in CASES:
        if int(FX["ok_%d" % i]):
            remain |= set(FX["state_%d" % i][:, 2].tolist())
    assert {0, 1, 2, 3} <= remain


@pytest.mark.parametrize("i", CASES, ids=["%s-%d" % (NAMES[i], i) for i in CASES])
def test_parse_mask_and_accept_equal_the_reference(i):
    g = create(i)
    if not int(FX["ok_%d" % i]):
        assert not g, "the reference makes no grammar of this text"
        return
    assert g
    try:
        want_e, want_len = FX["rules_%d" % i], FX["rule_len_%d" % i]
        elems, lens, ne = np.zeros(len(want_e) + 64, np.uint32), np.zeros(len(want_len) + 8, np.int32), ctypes.c_int(0)
        nr = L.kcpp_grammar_rules(g, elems.ctypes.data_as(P_), len(elems) // 2, lens.ctypes.data_as(P_), len(lens), ctypes.byref(ne))
        assert nr == len(want_len) and (lens[:nr] == want_len).all()
        assert 2 * ne.value == len(want_e) and (elems[:len(want_e)] == want_e).all()
        assert L.kcpp_grammar_n_stacks(g) == int(FX["stacks0_%d" % i])
        masks, toks, st = FX["masks_%d" % i], FX["toks_%d" % i], FX["state_%d" % i]
        for s in range(len(masks)):
            n1, m1 = reject(g, False)
            n2, m2 = reject(g, True)
            assert (m1 == masks[s]).all(), (s, np.flatnonzero(m1 != masks[s]))
            assert (m2 == m1).all() and n1 == n2 == int(sum(bin(int(w)).count("1") for w in m1))
            if s >= len(toks):
                break
            t = int(toks[s])
            p = piece(t)
            rc = L.kcpp_grammar_accept_piece(g, p, len(p), int(t == EOS))
            assert state(g) == st[s].tolist() or t == EOS
            assert rc == (0 if st[s][0] > 0 else -2)
    finally:
        L.kcpp_grammar_free(g)


def test_eos_needs_a_complete_grammar_and_limits_are_statuses():
    g = L.kcpp_grammar_create(b'root ::= "ab"')
    assert L.kcpp_grammar_accept_piece(g, b"", 0, 1) == -1           # EOS while no stack is empty: a status, no abort
    assert L.kcpp_grammar_accept_piece(g, b"ab", 2, 0) == 0 and L.kcpp_grammar_accept_piece(g, b"", 0, 1) == 0
    assert L.kcpp_grammar_accept_piece(g, b"x", 1, 0) == -2
    L.kcpp_grammar_free(g)
    # beyond the limits of grammar.h: no grammar, not a crash (the reference recurses without end on the first)
    for text in (b'root ::= opt root "a" | "b"\nopt ::= "x"?', b"root ::= " + b"(" * 5000 + b'"a"' + b")" * 5000,
                 b'root ::= "a"{99999999}', b'root ::= ("a"?){3000}'):
        assert not L.kcpp_grammar_create(text)
    assert not L.kcpp_grammar_create(b"") and not L.kcpp_grammar_create(None)


def _rules(g):
    elems, lens, ne = np.zeros(4096, np.uint32), np.zeros(64, np.int32), ctypes.c_int(0)
    nr = L.kcpp_grammar_rules(g, elems.ctypes.data_as(P_), len(elems) // 2, lens.ctypes.data_as(P_), len(lens), ctypes.byref(ne))
    return lens[:nr].tolist(), elems[:2 * ne.value].tolist()


def test_endless_expansion_and_huge_counts_give_no_grammar_at_once():
    """S ::= G S | with a G that is empty only through another rule passes the left-recursion check (here and in the
    reference) and re-enters S on both alternates at every level: the walk has to stop at the first limit it meets, not
    go on through 2^depth branches (before that, this load did not return).  Repetition counts past an int or past the
    limit are errors, not arithmetic on a narrowed value."""
    for text in (b'root ::= ((("a"?)?)?)* "b"', b'root ::= s\ns ::= g s |\ng ::= h\nh ::= "a" |',
                 b'root ::= "a"{2147483648,5}', b'root ::= "a"{4294967295}', b'root ::= "a"{18446744073709551615,}',
                 b'root ::= "a"{4294967298}', b'root ::= "a"{1048577}', b'root ::= "a"{2,4294967297}'):
        assert not L.kcpp_grammar_create(text), text
    # a maximum below the minimum: as if it were the minimum (the reference's loop over max - min runs no time)
    a, b = L.kcpp_grammar_create(b'root ::= "a"{3,2} "b"'), L.kcpp_grammar_create(b'root ::= "a"{3} "b"')
    assert a and b and _rules(a) == _rules(b) and _rules(a)[0] == [5]
    L.kcpp_grammar_free(a), L.kcpp_grammar_free(b)


# ---- the masked CPU model of the device pass
def _mask_of(n, allowed):
    rej = np.ones(n, bool)
    rej[np.asarray(allowed, np.int64)] = False
    bits = np.zeros(((n + 31) // 32) * 32, np.uint8)
    bits[:n] = rej
    return rej, np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1).copy()


def test_masked_cpu_model_against_numpy():
    from test_sample_front import buckets, cut_bucket, edited, make_input
    n = 20000
    raw, set_ids, adds, subs = make_input(n, "edges", 11)
    full = edited(raw, set_ids, adds, subs)
    rng = np.random.default_rng(3)
    for n_allowed in (50, 7000):
        allowed = np.sort(rng.choice(n, n_allowed, replace=False))
        rej, mask = _mask_of(n, allowed)
        h, ids, vals = K.candidates("ref", raw, 5000, set_ids, adds, subs, mask=mask)
        masked = np.where(rej, np.float32(-np.inf), full)
        ib = cut_bucket(masked)
        assert h.n_rej == n - n_allowed and h.h.n_bad == 0 and h.h.ib == ib
        assert list(h.h.hist) == np.bincount(buckets(masked), minlength=128).tolist()
        keep = np.flatnonzero(~rej & (buckets(masked) >= ib))
        assert h.h.nhave == len(keep) and (n_allowed == 50) == (ib == 0)
        assert (ids[:len(keep)] == keep).all() and (vals[:len(keep)].view(np.uint32) == full[keep].view(np.uint32)).all()
    # none rejected: the unmasked result; a raw NaN under a rejected bit still counts, a rejected finite logit does not
    h0, i0, v0 = K.candidates("ref", raw, 5000, set_ids, adds, subs)
    h1, i1, v1 = K.candidates("ref", raw, 5000, set_ids, adds, subs, mask=np.zeros((n + 31) // 32, np.uint32))
    assert bytes(h0) == bytes(h1.h) and h1.n_rej == 0 and (i0 == i1).all() and (v0.view(np.uint32) == v1.view(np.uint32)).all()
    raw2 = raw.copy()
    raw2[1234] = np.nan
    rej, mask = _mask_of(n, [i for i in range(0, n, 3) if i != 1234])
    assert K.candidates("ref", raw2, 5000, mask=mask)[0].h.n_bad == 1
    assert K.candidates("ref", raw, 5000, mask=mask)[0].h.n_bad == 0


# ---- the sampled chain on a masked array
def probe_front_masked(logits, P, order, ctx, last_n, restarts, seed, mu, mask):
    fp = (ctypes.c_float * 19)(P["top_k"], P["top_a"], P["top_p"], P["min_p"], P["typical"], P["tfs"], P["temp"],
                               P["rep_pen"], P["rep_slope"], P["presence"], P["miro_tau"], P["miro_eta"], P["dry_mult"],
                               P["dry_base"], P["xtc_thr"], P["xtc_prob"], P["dyn_range"], P["dyn_exp"], P["smoothing"])
    ip = (ctypes.c_int * 4)(P["rep_range"], P["mirostat"], P["dry_allowed"], P["dry_last_n"])
    rs = []
    for h, tails in restarts.items():
        for t in tails:
            rs += [h, len(t)] + list(t)
    arr = lambda v, t=ctypes.c_int: (t * max(1, len(v)))(*v)  # noqa: E731
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    mk = np.ascontiguousarray(mask, dtype=np.uint32)
    ids, ps = (ctypes.c_int * 8)(), (ctypes.c_float * 8)()
    n, status, m = ctypes.c_int(0), ctypes.c_int(-1), ctypes.c_float(mu)
    e_i, e_f = arr([]), arr([], ctypes.c_float)
    tok = L.kcpp_sampler_probe_front_masked(
        lg.ctypes.data_as(P_), len(lg), P["n_ctx"], fp, ip, arr(order), len(order), arr(ctx), len(ctx), arr(last_n),
        len(last_n), arr(rs), len(rs), seed, ctypes.byref(m), ids, ps, 8, ctypes.byref(n), e_i, 0, e_i, e_f, 0, e_i, e_f, 0,
        mk.ctypes.data_as(P_), ctypes.byref(status))
    return tok, status.value


# every sampler the issue names; each entry (name, parameter overrides, sampler order)
CHAINS = [
    ("top_k", dict(top_k=40, temp=0.8), TS.ORDER_DEFAULT),
    ("top_p_min_p", dict(top_p=0.9, min_p=0.05, temp=1.0), TS.ORDER_DEFAULT),
    ("top_a", dict(top_a=0.2, temp=1.1), TS.ORDER_DEFAULT),
    ("temperature_only", dict(temp=1.3), [5]),
    ("rep_pen", dict(rep_pen=1.3, rep_slope=0.7, presence=0.2, rep_range=64, temp=0.9, top_k=100), TS.ORDER_DEFAULT),
    ("dry", dict(temp=0.9, top_k=100, dry_mult=0.8, dry_base=1.75, dry_allowed=2, dry_last_n=0), TS.ORDER_DEFAULT),
    ("xtc", dict(temp=1.0, xtc_thr=0.05, xtc_prob=1.0), TS.ORDER_DEFAULT),
    ("mirostat2", dict(mirostat=2, temp=0.8, rep_pen=1.1), TS.ORDER_DEFAULT),
    ("greedy", dict(temp=0.0), TS.ORDER_DEFAULT),
    ("tail_free", dict(tfs=0.95, temp=1.0), TS.ORDER_DEFAULT),
    ("typical", dict(typical=0.9, temp=1.0), TS.ORDER_DEFAULT),
    ("mirostat1", dict(mirostat=1, temp=0.8), TS.ORDER_DEFAULT),
]
# (kind, what it must come out as): about 50 allowed (rebuild); about 5200 with the cut above bucket 0 (tail); about
# 5200 with every allowed logit below -10 (all in bucket 0: rebuild)
MASKS = ["few", "many_tail", "many_low"]


def masked_input(n, kind, seed):
    rng = np.random.default_rng(seed)
    raw = (rng.standard_normal(n) * 2.5).astype(np.float32)
    # the context's hot tokens (rep-pen / DRY act on ids < 40) stay allowed, so the penalties meet finite logits too
    hot = np.arange(40)
    if kind == "few":
        allowed = np.union1d(hot, rng.choice(n, 50, replace=False))
    else:
        allowed = np.union1d(hot, rng.choice(n, 5200, replace=False))
        if kind == "many_low":
            raw[allowed] = (-10.5 - np.abs(rng.standard_normal(len(allowed))) * 3).astype(np.float32)
    rej, mask = _mask_of(n, allowed)
    return raw, mask, np.where(rej, np.float32(-np.inf), raw).astype(np.float32)


@pytest.fixture(scope="module")
def ref():
    from test_sampler_ref import REF, ROOT
    import subprocess
    if not os.path.exists(REF):
        if not os.path.isdir("/root/reference"):
            pytest.skip("oracle/_ref/ref_sampler not built (reference sources absent)")
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "ref_sampler"])
    return REF


def _case(name, over, order, n, kind, seed):
    P = dict(TS.DEFAULT)
    P.update(over)
    last_n = ([0] * P["rep_range"] + CTX)[-P["rep_range"]:] if P["rep_range"] > 0 else []
    raw, mask, masked = masked_input(n, kind, 100 + seed)
    return P, list(order), last_n, raw, mask, masked


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("n", [6000, 20000])
def test_restated_chain_and_masked_front_end_agree_on_a_masked_array(n, kind):
    """no reference needed: the full chain on the array that carries the -inf and the front end's host path from the
    raw logits and the mask draw the same token; the path is the one the mask was built for"""
    for name, over, order in CHAINS:
        for seed in (1, 2):
            P, order_, last_n, raw, mask, masked = _case(name, over, order, n, kind, seed)
            mu = 2.0 * P["miro_tau"]
            want = TS.probe(masked, P, order_, CTX, last_n, RESTARTS, seed, mu)[0]
            got, status = probe_front_masked(raw, P, order_, CTX, last_n, RESTARTS, seed, mu, mask)
            assert status == (0 if kind == "many_tail" else 4), (name, status)
            assert got == want, (name, seed, got, want)


# samplers left out of the comparison with the reference (DESIGN.md 18 names each with the expression): none is needed
# so far -- an entry here must come with that expression
REF_EXCLUDED = set()

@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("n", [6000, 20000])
def test_chain_on_a_masked_array_matches_reference_samplelogits(ref, n, kind):
    from test_sampler_ref import pack, run_ref
    cases = []
    for name, over, order in CHAINS:
        if name in REF_EXCLUDED or name.startswith("mirostat"):       # mirostat: one process per case, below
            continue
        for seed in (1, 2):
            cases.append((name, seed) + _case(name, over, order, n, kind, seed))
    want = run_ref(ref, [pack(masked, P, order, CTX, last_n, RESTARTS, seed) for (_, seed, P, order, last_n, _, _, masked) in cases])
    assert len(want) == len(cases)
    for w, (name, seed, P, order, last_n, raw, mask, masked) in zip(want, cases):
        got = TS.probe(masked, P, order, CTX, last_n, RESTARTS, seed, 0.0)[0]
        front = probe_front_masked(raw, P, order, CTX, last_n, RESTARTS, seed, 0.0, mask)[0]
        print(name, seed, "reference", w, "chain", got, "front", front)
        assert got == w and front == w, (name, seed, got, front, w)


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("name", [m for m in ("mirostat1", "mirostat2") if m not in REF_EXCLUDED])
def test_mirostat_on_a_masked_array_matches_reference(ref, name, kind):
    """one process per case: the reference's mirostat mu is a function-static set to 2 tau on its first call"""
    from test_sampler_ref import pack, run_ref
    _, over, order = [c for c in CHAINS if c[0] == name][0]
    P, order_, last_n, raw, mask, masked = _case(name, over, order, 6000, kind, 7)
    want = run_ref(ref, [pack(masked, P, order_, CTX, last_n, RESTARTS, 7)])[0]
    mu = 2.0 * P["miro_tau"]
    got = TS.probe(masked, P, order_, CTX, last_n, RESTARTS, 7, mu)[0]
    front = probe_front_masked(raw, P, order_, CTX, last_n, RESTARTS, 7, mu, mask)[0]
    print(name, kind, "reference", want, "chain", got, "front", front)
    assert got == want and front == want
