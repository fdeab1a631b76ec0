"""The sampling front end's host side without a GPU (koboldcpp_amd/csrc/cand.h): kcpp_sampler_probe_front -- the CPU
model of the device pass (sparse logit edits, the bucket cut of top_k(5000), the survivors in id order), then
top_k_from_survivors and the rest of SampleLogits -- against kcpp_sampler_probe on logits that carry the same edits.
The drawn token, the candidate count, every candidate id in order and every probability must be equal bit for bit:
the front end is a faster way to the same 5000 candidates, the order of equal logits included."""
import ctypes

import numpy as np
import pytest

import koboldcpp_amd.lib as K
import test_sampler as TS

K_PRE = 5000


def buckets(l):
    """ksamp::top_k's bucket of each logit: int(6.4f * logit + 64.f) clamped to [0, 127], in float32"""
    f = (np.float32(6.4) * l.astype(np.float32)).astype(np.float32) + np.float32(64.0)
    return np.clip(np.trunc(f.astype(np.float64)), 0, 127).astype(np.int64)


def cut_bucket(l, k=K_PRE):
    h = np.bincount(buckets(l), minlength=128)
    have = 0
    for ib in range(127, -1, -1):
        have += h[ib]
        if have >= k:
            return ib
    raise AssertionError("k > n")


def edited(logits, set_ids, adds, subs):
    """what generate()'s full path does to the logits before SampleLogits, in float32 and in its order"""
    l = logits.astype(np.float32).copy()
    m = logits.min()
    low = np.float32(m - np.float32(8)) if m < 0 else np.float32(0)
    for i in set_ids:
        l[i] = low
    for i, v in adds:
        l[i] = np.float32(l[i] + np.float32(v))
    for i, v in subs:
        l[i] = np.float32(l[i] - np.float32(v))
    return l


def make_input(n, pattern, seed, k=K_PRE):
    """(raw logits, set-low ids, adds, subs).  "gauss": Gaussian logits alone.  "edges": exact ties (values copied
    between random ids, copies of the values on both sides of the cut bucket's upper edge, copies of the k-th largest
    value), values beyond +-10 (both clamps), and edits that touch id 0 and n - 1, repeat a bias id and bias a set-low id"""
    rng = np.random.default_rng(seed)
    l = (rng.standard_normal(n) * 2.5).astype(np.float32)
    if pattern == "gauss":
        return l, [], [], []
    src, dst = rng.integers(0, n, 40), rng.integers(0, n, 40)
    l[dst] = l[src]
    l[rng.integers(0, n, 6)] = np.array([11.0, 50.0, 1e4, -11.0, -50.0, -1e4], np.float32)
    order = np.argsort(-l, kind="stable")
    set_ids = [0, int(rng.integers(1, n - 1)), 7]
    adds = [(0, 1.5), (n - 1, 3.25), (9, 0.7), (9, 0.7), (9, -0.3), (7, 2.0), (int(order[10]), -4.0)]
    subs = [(n - 1, 0.5), (int(order[3]), 2.75), (11, 0.1)]
    touched = set(set_ids) | {i for i, _ in adds + subs}
    far = [i for i in order[min(n - 1, k + k // 12):] if i not in touched]   # ids well below the cut, left unedited
    if len(far) >= 12:
        pick = rng.choice(far, 12, replace=False)
        full = edited(l, set_ids, adds, subs)
        ib, b = cut_bucket(full, k), buckets(full)
        above, inside = full[b == ib + 1], full[b == ib]
        if len(above):
            l[pick[0:3]] = above.min()                   # ties just above bucket ib's upper edge
        l[pick[3:6]] = inside.max()                      # ... and just below it
        full = edited(l, set_ids, adds, subs)
        l[pick[6:12]] = np.sort(full)[::-1][k - 1]   # ties across the k-th position inside the cut bucket
    return l, set_ids, adds, subs


def probe_front(logits, P, order, ctx, last_n, restarts, seed, mu, set_ids, adds, subs):
    L = K.raw()
    fp = (ctypes.c_float * 19)(P["top_k"], P["top_a"], P["top_p"], P["min_p"], P["typical"], P["tfs"], P["temp"],
                               P["rep_pen"], P["rep_slope"], P["presence"], P["miro_tau"], P["miro_eta"], P["dry_mult"],
                               P["dry_base"], P["xtc_thr"], P["xtc_prob"], P["dyn_range"], P["dyn_exp"], P["smoothing"])
    ip = (ctypes.c_int * 4)(P["rep_range"], P["mirostat"], P["dry_allowed"], P["dry_last_n"])
    rs = []
    for h, tails in restarts.items():
        for t in tails:
            rs += [h, len(t)] + list(t)
    arr = lambda v, t=ctypes.c_int: (t * max(1, len(v)))(*v)
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    cap = len(logits)
    ids, ps = (ctypes.c_int * cap)(), (ctypes.c_float * cap)()
    n, status, m = ctypes.c_int(0), ctypes.c_int(-1), ctypes.c_float(mu)
    tok = L.kcpp_sampler_probe_front(
        lg.ctypes.data_as(ctypes.c_void_p), len(lg), P["n_ctx"], fp, ip, arr(order), len(order), arr(ctx), len(ctx),
        arr(last_n), len(last_n), arr(rs), len(rs), seed, ctypes.byref(m), ids, ps, cap, ctypes.byref(n),
        arr(set_ids), len(set_ids), arr([i for i, _ in adds]), arr([v for _, v in adds], ctypes.c_float), len(adds),
        arr([i for i, _ in subs]), arr([v for _, v in subs], ctypes.c_float), len(subs), ctypes.byref(status))
    return tok, [(ids[i], ps[i]) for i in range(n.value)], m.value, status.value


CTX = [int(x) for x in np.random.default_rng(7).integers(0, 40, 300)]
CTX += CTX[-25:-5] + CTX[-25:-12]                        # a repeated span for DRY / rep_pen
RESTARTS = {3: [[]], 11: [[12, 13]]}
SETTINGS = [
    ("prefilter", dict(), []),                           # n_order = 0: the 5000 candidates themselves come out
    ("defaults", dict(top_k=100, top_p=0.92, temp=0.7, rep_pen=1.1), TS.ORDER_DEFAULT),
    ("mirostat1", dict(mirostat=1, temp=0.7, rep_pen=1.1), TS.ORDER_DEFAULT),
    ("mirostat2", dict(mirostat=2, temp=0.7, rep_pen=1.1), TS.ORDER_DEFAULT),
    ("dry", dict(temp=0.9, top_k=100, dry_mult=0.8, dry_base=1.75, dry_allowed=2, dry_last_n=0), TS.ORDER_DEFAULT),
]
_INPUTS = {}


def _input(n, pattern):
    if (n, pattern) not in _INPUTS:
        raw, set_ids, adds, subs = make_input(n, pattern, 1000 + n % 997)
        _INPUTS[n, pattern] = (raw, set_ids, adds, subs, edited(raw, set_ids, adds, subs))
    return _INPUTS[n, pattern]


def both(raw, set_ids, adds, subs, full, over, order, seed=42):
    P = dict(TS.DEFAULT)
    P.update(over)
    last_n = ([0] * P["rep_range"] + CTX)[-P["rep_range"]:]
    mu = 2.0 * P["miro_tau"]
    want = TS.probe(full, P, order, CTX, last_n, RESTARTS, seed, mu)
    got = probe_front(raw, P, order, CTX, last_n, RESTARTS, seed, mu, set_ids, adds, subs)
    return want, got


@pytest.mark.parametrize("pattern", ["gauss", "edges"])
@pytest.mark.parametrize("n", [5001, 8229, 128256])
@pytest.mark.parametrize("name,over,order", SETTINGS, ids=[s[0] for s in SETTINGS])
def test_front_end_chain_equals_full_chain(name, over, order, n, pattern):
    raw, set_ids, adds, subs, full = _input(n, pattern)
    (tok, cands, mu), (ftok, fcands, fmu, status) = both(raw, set_ids, adds, subs, full, over, order)
    assert status == 0                                   # through the front end, not its fallback
    assert ftok == tok and len(fcands) == len(cands)
    assert [i for i, _ in fcands] == [i for i, _ in cands]
    assert [p for _, p in fcands] == [p for _, p in cands]             # float32 values: equal means bit-equal
    assert fmu == mu
    if name == "prefilter":
        assert len(cands) == K_PRE
    if name.startswith("mirostat"):
        assert mu != 2.0 * TS.DEFAULT["miro_tau"]        # the mirostat branch ran


def test_edges_input_has_the_ties_it_promises():
    """the "edges" inputs do tie across the k-th position and sit on both sides of the cut bucket's upper edge, after the
    edits too; and both clamps are hit"""
    for n in (8229, 128256):
        full = _input(n, "edges")[4]
        srt = np.sort(full)[::-1]
        assert srt[K_PRE - 1] == srt[K_PRE]              # equal logits across the k-th position
        ib, b = cut_bucket(full), buckets(full)
        for side in (ib, ib + 1):
            v = full[b == side]
            assert len(v) - len(np.unique(v)) >= 2
        assert (full > 10).any() and (full < -10).any()


def test_all_equal_logits_overflow_the_capacity_and_fall_back():
    """20000 equal logits: one bucket holds them all, so every id survives the cut -- more than the 16384 the front end
    carries.  The header says so and the hook draws the same token through its fallback."""
    raw = np.full(20000, 1.25, np.float32)
    hdr, ids, _ = K.candidates("ref", raw, K_PRE)
    assert hdr.nhave == 20000 and hdr.n_bad == 0 and hdr.hist[hdr.ib] == 20000
    assert (ids[:16384] == np.arange(16384)).all()
    for name, over, order in SETTINGS[:2]:
        (tok, cands, mu), (ftok, fcands, fmu, status) = both(raw, [], [], [], raw, over, order)
        assert status == 2
        assert ftok == tok and fcands == cands and fmu == mu


def test_front_ref_header_matches_numpy():
    """the CPU model's header against the numpy restatement: low, cut bucket, counts, the survivors in ascending id"""
    raw, set_ids, adds, subs, full = _input(128256, "edges")
    hdr, ids, vals = K.candidates("ref", raw, K_PRE, set_ids, adds, subs)
    b = buckets(full)
    assert list(hdr.hist) == list(np.bincount(b, minlength=128))
    assert hdr.ib == cut_bucket(full) and hdr.n_bad == 0
    assert np.float32(hdr.low) == np.float32(raw.min() - np.float32(8))
    keep = np.nonzero(b >= hdr.ib)[0]
    assert hdr.nhave == len(keep) <= 16384
    assert (ids[:len(keep)] == keep).all()
    assert (vals[:len(keep)].view(np.uint32) == full[keep].view(np.uint32)).all()
    assert (ids[len(keep):] == K.CAND_GUARD_ID).all()
