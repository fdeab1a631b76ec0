"""Grammar-constrained sampling on the GPU: the reject mask in the sampling front end's kernels
(koboldcpp_amd/csrc/cand.hip, against the CPU model kcpp_cand_front_ref_masked bit for bit), the masked argmax
(runtime.cpp, against numpy) and generate() with a GBNF grammar on the tiny synthetic model.

The tiny model's constrained steps allow a handful of tokens, so its sampled requests take the front end's rebuild (cut
in bucket 0); the bucket tail under a mask is driven through kcpp_logit_candidates_masked directly (the kernel tests)."""
import ctypes
import re

import numpy as np
import pytest

import gguf_writer as GW
import refharness as R

pytestmark = pytest.mark.gpu

CAP = 16384
SIZES = [5001, 8192, 40001]          # one past the pre-filter; whole 1024-slices; a ragged last slice and mask word
YESNO = b'root ::= ("yes" | "no") " " [0-9]{3}'
JSON = rb'''root   ::= value
value  ::= object | array | string | number | "true" | "false" | "null"
object ::= "{" ws ( pair ( "," ws pair )* )? "}"
pair   ::= string ws ":" ws value ws
array  ::= "[" ws ( value ws ( "," ws value ws )* )? "]"
string ::= "\"" ( [^"\\\x00-\x1f] | "\\" ( ["\\/bfnrt] | "u" [0-9a-fA-F]{4} ) )* "\""
number ::= "-"? ( "0" | [1-9] [0-9]* ) ( "." [0-9]+ )?
ws     ::= [ \t\n]*
'''


@pytest.fixture(scope="module")
def env():
    """torch first, then the library (see tests/test_gpu_sample_front.py)"""
    import torch
    assert torch.cuda.is_available()
    import koboldcpp_amd.lib as K
    return torch, K


def pack_mask(n, rejected):
    bits = np.zeros(((n + 31) // 32) * 32, np.uint8)
    bits[:n] = rejected
    return np.packbits(bits.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1).copy()


def on_device(env, raw, mask, set_ids=(), adds=(), subs=(), cap=CAP, guard=0):
    torch, K = env
    d = torch.from_numpy(np.ascontiguousarray(raw, dtype=np.float32)).cuda()
    torch.cuda.synchronize()
    out = K.candidates("dev", (d.data_ptr(), d.numel()), 5000, set_ids, adds, subs, cap, guard,
                       torch.cuda.current_stream().cuda_stream, mask=mask)
    assert (d.cpu().numpy().view(np.uint32) == np.asarray(raw, np.float32).view(np.uint32)).all()    # input untouched
    return out


def same(K, got, want, cap, have_low):
    (h, ids, vals), (rh, rids, rvals) = got, want
    assert (h.h.ib, h.h.nhave, h.h.n_bad, h.n_rej) == (rh.h.ib, rh.h.nhave, rh.h.n_bad, rh.n_rej)
    assert list(h.h.hist) == list(rh.h.hist)
    if have_low:
        assert np.float32(h.h.low).view(np.uint32) == np.float32(rh.h.low).view(np.uint32)
    have = min(h.h.nhave, cap)
    assert (ids[:have] == rids[:have]).all() and (np.diff(ids[:have]) > 0).all()
    assert (vals[:have].view(np.uint32) == rvals[:have].view(np.uint32)).all()
    assert (ids[have:] == K.CAND_GUARD_ID).all() and (vals[have:].view(np.uint32) == K.CAND_GUARD_BITS).all()


def masks_for(n, rng):
    """name -> rejected (bool per id)"""
    m = {"none": np.zeros(n, bool)}
    r = np.ones(n, bool)
    r[[1, n // 2, n - 2]] = False
    m["all_but_3"] = r
    r = np.ones(n, bool)
    r[rng.choice(n, min(6000, n - 1), replace=False)] = False
    m["about_6000"] = r
    r = np.zeros(n, bool)
    r[[0, 31, 32, 1023, 1024, n - 1]] = True
    m["edges"] = r
    return m


@pytest.mark.parametrize("edits", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_masked_kernels_equal_cpu_model(env, n, edits):
    _, K = env
    rng = np.random.default_rng(n)
    raw = (rng.standard_normal(n) * 2.5).astype(np.float32)
    for name, rej in masks_for(n, rng).items():
        allowed, gone = np.flatnonzero(~rej), np.flatnonzero(rej)
        set_ids, adds, subs = [], [], []
        if edits:                                    # edits that hit rejected and allowed ids, the first and last id
            set_ids = [int(allowed[0])] + ([int(gone[0])] if len(gone) else [])
            adds = [(int(allowed[1]), 1.5), (int(allowed[1]), -0.25), (n - 1, 2.0)] + ([(int(gone[-1]), 3.0)] if len(gone) else [])
            subs = [(int(allowed[2]), 0.75), (0, 0.5)]
        mask = pack_mask(n, rej)
        want = K.candidates("ref", raw, 5000, set_ids, adds, subs, mask=mask)
        got = on_device(env, raw, mask, set_ids, adds, subs)
        same(K, got, want, CAP, bool(set_ids))
        assert want[0].n_rej == len(gone) and want[0].h.n_bad == 0
        if name == "all_but_3":
            assert want[0].h.ib == 0 and want[0].h.nhave == 3 and list(got[1][:3]) == list(allowed)
        if name == "about_6000" and n > 6000:
            assert want[0].h.ib >= 1 and 5000 <= want[0].h.nhave <= 6000
        if name == "none":                           # also what the entry without a mask gives
            torch = env[0]
            d = torch.from_numpy(raw).cuda()
            h0, i0, v0 = K.candidates("dev", (d.data_ptr(), n), 5000, set_ids, adds, subs, CAP, 0,
                                      torch.cuda.current_stream().cuda_stream)
            assert (h0.ib, h0.nhave, h0.n_bad, list(h0.hist)) == (got[0].h.ib, got[0].h.nhave, got[0].h.n_bad, list(got[0].h.hist))
            assert (i0 == got[1]).all() and (v0.view(np.uint32) == got[2].view(np.uint32)).all()


def test_masked_overflow_is_a_status_and_writes_stop_at_cap(env):
    """20000 allowed, every logit below -10: the cut is bucket 0, n - n_rej exceeds the capacity"""
    _, K = env
    n = 40001
    rng = np.random.default_rng(9)
    raw = (-10.5 - np.abs(rng.standard_normal(n)) * 3).astype(np.float32)
    rej = np.ones(n, bool)
    allowed = np.sort(rng.choice(n, 20000, replace=False))
    rej[allowed] = False
    mask = pack_mask(n, rej)
    h, ids, vals = on_device(env, raw, mask, guard=256)
    assert h.h.ib == 0 and h.h.nhave == 20000 > CAP and h.n_rej == n - 20000 and h.h.n_bad == 0
    assert (ids[:CAP] == allowed[:CAP]).all() and (vals[:CAP].view(np.uint32) == raw[allowed[:CAP]].view(np.uint32)).all()
    assert (ids[CAP:] == K.CAND_GUARD_ID).all() and (vals[CAP:].view(np.uint32) == K.CAND_GUARD_BITS).all()
    same(K, (h, ids[:CAP], vals[:CAP]), K.candidates("ref", raw, 5000, mask=mask), CAP, False)
    h, ids, vals = on_device(env, raw, mask, cap=1000, guard=64)
    assert h.h.nhave == 20000 and (ids[:1000] == allowed[:1000]).all() and (ids[1000:] == K.CAND_GUARD_ID).all()


def test_raw_nan_under_a_rejected_bit_still_counts(env):
    _, K = env
    n = 8192
    raw = (np.random.default_rng(4).standard_normal(n) * 2.5).astype(np.float32)
    rej = np.zeros(n, bool)
    rej[[100, 4000]] = True
    mask = pack_mask(n, rej)
    assert on_device(env, raw, mask)[0].h.n_bad == 0             # rejected finite logits are not bad
    raw[100] = np.nan
    got = on_device(env, raw, mask)
    assert got[0].h.n_bad == 1 and got[0].n_rej == 2
    same(K, got, K.candidates("ref", raw, 5000, mask=mask), CAP, False)
    assert on_device(env, raw, mask, set_ids=[5])[0].h.n_bad == 1


def argmax_masked(env, raw, rej):
    torch, K = env
    d = torch.from_numpy(np.ascontiguousarray(raw, dtype=np.float32)).cuda()
    torch.cuda.synchronize()
    mask = pack_mask(len(raw), rej)
    tok, val = ctypes.c_int32(-5), ctypes.c_float(0)
    K.call("kcpp_logit_argmax_masked", ctypes.c_void_p(d.data_ptr()), len(raw), mask.ctypes.data_as(ctypes.c_void_p),
           ctypes.byref(tok), ctypes.byref(val), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return tok.value, val.value


@pytest.mark.parametrize("n", SIZES)
def test_masked_argmax_against_numpy(env, n):
    rng = np.random.default_rng(n + 1)
    raw = (rng.standard_normal(n) * 2.5).astype(np.float32)
    for frac in (0.0, 0.5, 0.99):
        rej = rng.random(n) < frac
        want = int(np.flatnonzero(~rej)[np.argmax(raw[~rej])])
        assert argmax_masked(env, raw, rej) == (want, raw[want])
    # ties: the lowest tied id is rejected, the next one wins; ids at the mask-word and slice seams
    tied = raw.copy()
    ids = [31, 32, 1023, 1024, n - 1]
    tied[ids] = 50.0
    rej = np.zeros(n, bool)
    rej[31] = True
    assert argmax_masked(env, tied, rej)[0] == 32
    rej[[32, 1023, 1024]] = True
    assert argmax_masked(env, tied, rej)[0] == n - 1
    rej = np.ones(n, bool)                           # all but one
    rej[n - 1] = False
    assert argmax_masked(env, raw, rej) == (n - 1, raw[n - 1])
    assert argmax_masked(env, raw, np.ones(n, bool))[0] == -1    # all rejected: the status, not a token


def test_model_entries_leave_the_logits_alone(env):
    _, K = env
    hp = dict(R.TINY, n_vocab=8192)
    m = K.Model(hp, R.q4_k_m_types(hp["n_layer"]))
    m.synth(1234)
    before = m.decode(list(range(1, 24)), 0)
    rng = np.random.default_rng(2)
    for n_allowed in (3, 6000):
        rej = np.ones(8192, bool)
        rej[rng.choice(8192, n_allowed, replace=False)] = False
        mask = pack_mask(8192, rej)
        got = K.candidates(m, None, 5000, [2, 17], [(0, 1.5), (8191, -2.0)], [(40, 0.25)], mask=mask)
        tok, val = ctypes.c_int32(-5), ctypes.c_float(0)
        K.call("kcpp_model_argmax_masked", m.m, mask.ctypes.data_as(ctypes.c_void_p), ctypes.byref(tok), ctypes.byref(val))
        after = np.empty(8192, np.float32)
        K.call("kcpp_model_read_logits", m.m, after.ctypes.data_as(ctypes.c_void_p))
        assert (after.view(np.uint32) == before.view(np.uint32)).all()
        same(K, got, K.candidates("ref", before, 5000, [2, 17], [(0, 1.5), (8191, -2.0)], [(40, 0.25)], mask=mask), CAP, True)
        assert tok.value == int(np.flatnonzero(~rej)[np.argmax(before[~rej])]) and val.value == before[tok.value]
    m.close()


# ---- generate() end to end
WORDS = GW.WORDS + ["yes", "no", '{"', "ye", "s", "▁1", "12", "tru", "e"]


@pytest.fixture(scope="module")
def engine(env, tmp_path_factory):
    from koboldcpp_amd import expose as X
    from test_gpu_sample_front import _load
    hp = dict(R.TINY, n_vocab=8192)
    path = str(tmp_path_factory.mktemp("gguf") / "grammar.gguf")
    toks = GW.llama_gguf(path, hp, R.q4_k_m_types(hp["n_layer"]), 1234, WORDS)
    h = X.init_library()
    _load(h, X, path)
    return h, X, toks


def _req(X, grammar, retain=False, **over):
    from test_gpu_sample_front import _request
    gi = _request(X, **over)
    gi.allow_eos_token, gi.bypass_eos_token = True, False        # EOS ends the request once the grammar is complete
    gi.grammar, gi.grammar_retain_state = grammar, retain
    return gi


def _gen(K, h, gi, front=True):
    """(status, stop reason, text, token ids, grammar counters) of one generate()"""
    L = K.raw()
    L.kcpp_expose_set_sample_front(int(front))
    L.kcpp_expose_mirostat_mu(1, 2.0 * gi.mirostat_tau)
    gs = (ctypes.c_int64 * 6)()
    L.kcpp_expose_grammar_stats(gs)
    try:
        out = h.generate(gi)
        status, stop, text = out.status, out.stopreason, bytes(out.text)
    finally:
        L.kcpp_expose_set_sample_front(-1)
    L.kcpp_expose_grammar_stats(gs)
    ids = (ctypes.c_int * 128)()
    n = L.kcpp_expose_last_tokens(ids, 128)
    return status, stop, text, list(ids[:n]), list(gs)


def test_generate_follows_the_grammar_greedy_and_sampled(env, engine):
    """fails without the feature: the random model's text does not match the pattern"""
    _, K = env
    h, X, _ = engine
    pat = re.compile(rb"^(yes|no) [0-9]{3}$")
    status, stop, text, toks, gs = _gen(K, h, _req(X, YESNO, top_k=1))
    print("greedy", text, toks, gs)
    assert status == 1 and stop == 1 and pat.match(text), text
    assert gs[0] == len(toks) and gs[1] + gs[2] + gs[3] + gs[4] + gs[5] == len(toks) and gs[2] >= 1 and gs[4] == 0
    _gen(K, h, _req(X, YESNO), False)                # the prompt into the cache (see _on_equals_off)
    on = _gen(K, h, _req(X, YESNO), True)
    off = _gen(K, h, _req(X, YESNO), False)
    print("sampled", on, off)
    for status, stop, text, toks, gs in (on, off):
        assert status == 1 and stop == 1 and pat.match(text), text
    assert on[3] == off[3]
    assert on[4][0] == len(on[3]) and on[4][3] + on[4][5] == len(on[3]) and on[4][3] >= 1 and on[4][4] == 0
    assert off[4][4] == len(off[3]) and off[4][3] == 0


# a vocabulary with no unused token: every id past the control tokens has a piece.  (With WORDS alone 7900 of the 8192
# ids are unused tokens with an empty piece, which every grammar rejects, and the random model's own choice is almost
# always one of them: no request would ever take the path where the device argmax stands.)
WORDS_FULL = WORDS + ["w%04d" % i for i in range(8192 - 259 - len(WORDS))]


def _accepted_then_masked(K, h, X, toks_text):
    """One greedy request that takes both greedy paths, on a model with the WORDS_FULL vocabulary.  The grammar is the
    text of the first three tokens the model picks unconstrained, then three digits: for those three tokens the device
    argmax stands and the host only tests it (counter 1, the in-graph greedy step goes on), after them the random
    model's choice is no digit and the masked argmax runs (counter 2).  Returns that request's (status, stop reason,
    text, token ids, counters)."""
    from test_gpu_expose import piece
    _, _, ttypes = GW.spm_vocab(8192, WORDS_FULL)
    _gen(K, h, _req(X, b"", top_k=1, max_length=6))              # the prompt into the cache (see _on_equals_off)
    free = _gen(K, h, _req(X, b"", top_k=1, max_length=6))
    assert free[0] == 1 and len(free[3]) == 6 and 2 not in free[3][:3] and free[4] == [0] * 6
    lead = b"".join(piece(toks_text, ttypes, t) for t in free[3][:3])
    literal = "".join("\\U%08X" % ord(c) for c in lead.decode("utf-8"))
    got = _gen(K, h, _req(X, ('root ::= "%s" [0-9]{3}' % literal).encode(), top_k=1, max_length=16))
    print("free", free, "lead", lead, "constrained", got)
    status, stop, text, ids, gs = got
    assert status == 1 and stop == 1 and ids[:3] == free[3][:3]
    tail = b"".join(piece(toks_text, ttypes, t) for t in ids[3:-1])
    assert ids[-1] == 2 and re.match(rb"^[0-9]{3}$", tail), (ids, tail)
    assert gs[0] == len(ids) and gs[1] >= 3 and gs[2] >= 1 and gs[1] + gs[2] == len(ids) and gs[3:] == [0, 0, 0]
    return got


def _replay(K, toks_text, grammar, ids):
    """feed the generated ids back through the grammar hooks: every prefix must leave a stack"""
    from test_gpu_expose import piece
    L = K.raw()
    _, _, ttypes = GW.spm_vocab(8192, WORDS)
    g = L.kcpp_grammar_create(grammar)
    assert g
    try:
        for t in ids:
            p = b"" if t == 2 else piece(toks_text, ttypes, t)
            assert L.kcpp_grammar_accept_piece(g, p, len(p), int(t == 2)) == 0, (t, p)
            assert L.kcpp_grammar_n_stacks(g) > 0
    finally:
        L.kcpp_grammar_free(g)


@pytest.mark.parametrize("greedy", [True, False])
def test_generate_json_grammar_every_prefix_is_accepted(env, engine, greedy):
    _, K = env
    h, X, toks_text = engine
    over = dict(top_k=1) if greedy else {}
    status, stop, text, ids, gs = _gen(K, h, _req(X, JSON, max_length=48, **over))
    print(text, ids, gs)
    assert status == 1 and 1 <= len(ids) <= 48 and gs[0] == len(ids)
    _replay(K, toks_text, JSON, ids)


def test_grammar_retain_state(env, engine):
    _, K = env
    h, X, toks_text = engine
    two = b'root ::= "ab" "ab"'                       # the text is forced; one token of it is "a" or "ab"
    first = _gen(K, h, _req(X, two, retain=True, top_k=1, max_length=1))
    again = _gen(K, h, _req(X, two, retain=True, top_k=1, max_length=8))
    assert first[2] in (b"a", b"ab") and first[2] + again[2] == b"abab" and again[1] == 1     # continued, then EOS
    first = _gen(K, h, _req(X, two, retain=False, top_k=1, max_length=1))
    again = _gen(K, h, _req(X, two, retain=False, top_k=1, max_length=8))
    assert first[2] in (b"a", b"ab") and again[2] == b"abab" and again[1] == 1                # restarted
    _gen(K, h, _req(X, two, retain=True, top_k=1, max_length=1))
    other = _gen(K, h, _req(X, b'root ::= "ab" "ab" ', retain=True, top_k=1, max_length=8))
    assert other[2] == b"abab"                                                # a changed string restarts it


def test_bad_grammar_generates_unconstrained(env, engine):
    _, K = env
    h, X, _ = engine
    bad = _gen(K, h, _req(X, b'root ::= root "a" | "b"', top_k=1, max_length=12))
    none = _gen(K, h, _req(X, b"", top_k=1, max_length=12))
    assert bad[0] == 1 and bad[3] == none[3] and bad[4] == [0] * 6


def test_greedy_request_takes_the_unmasked_and_the_masked_path(env, engine, tmp_path):
    """Runs after the tests on the module's model: it replaces the loaded model (see WORDS_FULL)."""
    from test_gpu_sample_front import _load
    _, K = env
    h, X, _ = engine
    path = str(tmp_path / "full.gguf")
    toks_text = GW.llama_gguf(path, dict(R.TINY, n_vocab=8192), R.q4_k_m_types(R.TINY["n_layer"]), 1234, WORDS_FULL)
    _load(h, X, path)
    _accepted_then_masked(K, h, X, toks_text)


def test_generate_layer_split_same_tokens_as_one_stage(env, engine, tmp_path, monkeypatch):
    """two stages (KCPP_VIRTUAL_DEVICES puts both on the one GPU): the mask goes to the last stage's front end and to its
    masked argmax, the token from the host to the first stage.  The same requests on a fresh one-stage load and on a
    fresh two-stage load of one file must give the same tokens by the same paths.  Runs last in the module: it replaces
    the loaded model."""
    from test_gpu_sample_front import _load
    _, K = env
    h, X, _ = engine
    hp = dict(R.TINY, n_vocab=8192, n_layer=4)
    path = str(tmp_path / "split.gguf")
    toks_text = GW.llama_gguf(path, hp, R.q4_k_m_types(hp["n_layer"]), 1234, WORDS_FULL)

    def requests():
        out = [_gen(K, h, _req(X, YESNO, top_k=1))]
        _gen(K, h, _req(X, YESNO), False)                # the prompt into the cache (see _on_equals_off)
        out.append(_gen(K, h, _req(X, YESNO), True))
        out.append(_gen(K, h, _req(X, JSON, max_length=24), True))
        out.append(_accepted_then_masked(K, h, X, toks_text))    # asserts both greedy paths in one request
        return out

    _load(h, X, path)
    one = requests()
    monkeypatch.setenv("KCPP_VIRTUAL_DEVICES", "2")
    _load(h, X, path, split=(1.0, 1.0))
    two = requests()
    print(one, two)
    pat = re.compile(rb"^(yes|no) [0-9]{3}$")
    assert pat.match(two[0][2]) and pat.match(two[1][2]) and two[0][1] == two[1][1] == 1
    assert two[0][4][2] >= 1 and two[1][4][3] >= 1 and two[1][4][4] == 0     # the masked argmax and the rebuild ran split
    assert one == two
