"""The sampling front end on the GPU (koboldcpp_amd/csrc/cand.hip): the sparse logit edits, the bucket cut of
SampleLogits' top_k(5000) and the survivors' compaction on the device.

* kcpp_logit_candidates against the CPU model kcpp_cand_front_ref on the same inputs: header, the 128 bucket counts,
  survivor ids and logit bits, ascending;
* kcpp_model_candidates on a model's own logits, which it must leave as they are;
* generate() through load_model with the front end on and off: the same token ids, and the counters say which path ran."""
import ctypes

import numpy as np
import pytest

import gguf_writer as GW
import refharness as R

pytestmark = pytest.mark.gpu

CAP = 16384
TF = None                   # tests/test_sample_front.py (its inputs), imported by env


@pytest.fixture(scope="module")
def env():
    """torch, then the library, then the modules that load the library at import: the library names the HIP runtime by
    the soname torch's bundled copy carries, so after torch the process has that one runtime; the other way round it
    would have two"""
    global TF
    import torch
    assert torch.cuda.is_available()
    import koboldcpp_amd.lib as K
    import test_sample_front
    TF = test_sample_front
    return torch, K


def on_device(env, raw, k, set_ids=(), adds=(), subs=(), cap=CAP, guard=0):
    torch, K = env
    d = torch.from_numpy(np.ascontiguousarray(raw, dtype=np.float32)).cuda()
    torch.cuda.synchronize()
    out = K.candidates("dev", (d.data_ptr(), d.numel()), k, set_ids, adds, subs, cap, guard,
                       torch.cuda.current_stream().cuda_stream)
    assert (d.cpu().numpy().view(np.uint32) == np.asarray(raw, np.float32).view(np.uint32)).all()    # input untouched
    return out


def same_result(K, got, want, cap, have_low):
    (h, ids, vals), (rh, rids, rvals) = got, want
    assert (h.ib, h.nhave, h.n_bad) == (rh.ib, rh.nhave, rh.n_bad)
    assert list(h.hist) == list(rh.hist)
    if have_low:                                  # without a set-low list no min pass runs: low is not specified
        assert np.float32(h.low).view(np.uint32) == np.float32(rh.low).view(np.uint32)
    have = min(h.nhave, cap)
    assert (ids[:have] == rids[:have]).all() and (np.diff(ids[:have]) > 0).all()
    assert (vals[:have].view(np.uint32) == rvals[:have].view(np.uint32)).all()
    assert (ids[have:] == K.CAND_GUARD_ID).all() and (vals[have:].view(np.uint32) == K.CAND_GUARD_BITS).all()


def sizes(K):
    """(n, k): one past the engage threshold; two slice seams and a ragged last wave (the cut inside the data: k 500);
    the Llama-3 and Qwen2 vocabularies"""
    return [(5001, 5000), (2 * K.cand_plan(5001)["slice"] + 37, 500), (128256, 5000), (151936, 5000)]


@pytest.mark.parametrize("pattern", ["gauss", "edges"])
@pytest.mark.parametrize("which", range(4))
def test_kernels_equal_cpu_model(env, which, pattern):
    _, K = env
    n, k = sizes(K)[which]
    assert K.cand_plan(n)["nblk"] == -(-n // K.cand_plan(n)["slice"])
    raw, set_ids, adds, subs = TF.make_input(n, pattern, 77 + which, k)
    want = K.candidates("ref", raw, k, set_ids, adds, subs)
    assert want[0].n_bad == 0 and k <= want[0].nhave <= CAP
    same_result(K, on_device(env, raw, k, set_ids, adds, subs), want, CAP, bool(set_ids))


def test_no_set_low_list(env):
    """biases and penalties alone: no min pass, the header's low is to be ignored"""
    _, K = env
    raw, _, adds, subs = TF.make_input(128256, "edges", 5)
    want = K.candidates("ref", raw, 5000, [], adds, subs)
    same_result(K, on_device(env, raw, 5000, [], adds, subs), want, CAP, False)


def test_overflow_is_a_status_and_writes_stop_at_cap(env):
    _, K = env
    raw = np.full(20000, 1.25, np.float32)
    h, ids, vals = on_device(env, raw, 5000, guard=256)
    assert h.nhave == 20000 > CAP and h.n_bad == 0 and h.hist[h.ib] == 20000
    assert (ids[:CAP] == np.arange(CAP)).all() and (vals[:CAP] == np.float32(1.25)).all()
    assert (ids[CAP:] == K.CAND_GUARD_ID).all() and (vals[CAP:].view(np.uint32) == K.CAND_GUARD_BITS).all()
    same_result(K, (h, ids[:CAP], vals[:CAP]), K.candidates("ref", raw, 5000), CAP, False)
    # a smaller capacity: nothing past it either
    h, ids, vals = on_device(env, raw, 5000, cap=1000, guard=64)
    assert h.nhave == 20000 and (ids[:1000] == np.arange(1000)).all() and (ids[1000:] == K.CAND_GUARD_ID).all()


def test_non_finite_logits_are_counted(env):
    """an inf and a NaN are plain values in the buffer; the header reports them (generate() then reads every logit)"""
    _, K = env
    raw = TF.make_input(8229, "gauss", 3)[0]
    raw[100], raw[4000] = np.inf, np.nan
    h, ids, vals = on_device(env, raw, 5000)
    assert h.n_bad == 2
    same_result(K, (h, ids, vals), K.candidates("ref", raw, 5000), CAP, False)
    h2 = on_device(env, raw, 5000, set_ids=[5])[0]            # with a set-low list the raw values count as well
    assert h2.n_bad == 2


def test_bad_arguments_are_errors(env):
    _, K = env
    raw = TF.make_input(5001, "gauss", 3)[0]
    for kw in (dict(set_ids=[5001]), dict(adds=[(-1, 1.0)]), dict(cap=CAP + 1)):
        with pytest.raises(K.KcppError):
            on_device(env, raw, 5000, **kw)


def test_model_candidates_leave_the_logits_alone(env):
    _, K = env
    hp = dict(R.TINY, n_vocab=8192)
    m = K.Model(hp, R.q4_k_m_types(hp["n_layer"]))
    m.synth(1234)
    before = m.decode(list(range(1, 24)), 0)
    edits = ([2, 17], [(0, 1.5), (8191, -2.0), (17, 0.5)], [(40, 0.25)])
    for set_ids, adds, subs in (edits, ([], [], [])):
        got = K.candidates(m, None, 5000, set_ids, adds, subs)
        after = np.empty(8192, np.float32)
        K.call("kcpp_model_read_logits", m.m, after.ctypes.data_as(ctypes.c_void_p))
        assert (after.view(np.uint32) == before.view(np.uint32)).all()
        want = K.candidates("ref", before, 5000, set_ids, adds, subs)
        assert want[0].n_bad == 0 and 5000 <= want[0].nhave <= CAP
        same_result(K, got, want, CAP, bool(set_ids))
    m.close()


# ---- generate() end to end
def _load(h, X, path, split=None, ubatch=512):
    li = X.load_model_inputs()
    li.model_filename = path.encode()
    li.max_context_length = 248
    li.blasbatchsize = ubatch
    li.gpulayers = 999
    li.rope_freq_base = 10000.0
    li.rope_freq_scale = 0.0
    for i, v in enumerate(split or ()):
        li.tensor_split[i] = v
    assert h.load_model(li)


@pytest.fixture(scope="module")
def engine(env, tmp_path_factory):
    from koboldcpp_amd import expose as X
    hp = dict(R.TINY, n_vocab=8192)
    path = str(tmp_path_factory.mktemp("gguf") / "v8192.gguf")
    toks = GW.llama_gguf(path, hp, R.q4_k_m_types(hp["n_layer"]), 1234, GW.WORDS)
    h = X.init_library()
    _load(h, X, path)
    return h, X, toks


def _request(X, **over):
    """koboldcpp's default request (koboldcpp.py:876-897), 48 tokens, a fixed seed; EOS neither stops nor is banned"""
    gi = X.generation_inputs()
    gi.prompt, gi.memory = b" ".join([b"hello world the a b of to"] * 3), b""
    gi.max_context_length, gi.max_length, gi.seed = 248, 48, 1234
    gi.temperature, gi.top_k, gi.top_a, gi.top_p, gi.min_p, gi.typical_p, gi.tfs = 0.7, 100, 0.0, 0.92, 0.0, 1.0, 1.0
    gi.rep_pen, gi.rep_pen_range, gi.rep_pen_slope, gi.presence_penalty = 1.0, 320, 1.0, 0.0
    gi.mirostat, gi.mirostat_tau, gi.mirostat_eta = 0, 5.0, 0.1
    gi.dry_multiplier, gi.dry_base, gi.dry_allowed_length, gi.dry_penalty_last_n = 0.0, 1.75, 2, 320
    gi.xtc_threshold, gi.xtc_probability = 0.2, 0.0
    gi.dynatemp_range, gi.dynatemp_exponent, gi.smoothing_factor = 0.0, 1.0, 0.0
    order = over.pop("sampler_order", [6, 0, 1, 3, 4, 2, 5])
    for i, v in enumerate(order):
        gi.sampler_order[i] = v
    gi.sampler_len = len(order)
    gi.allow_eos_token, gi.bypass_eos_token = True, True
    for i, (t, b) in enumerate(over.pop("biases", [])):
        gi.logit_biases[i].token_id, gi.logit_biases[i].bias = t, b
    for i, s in enumerate(over.pop("banned", [])):
        gi.banned_tokens[i] = s
    for k, v in over.items():
        setattr(gi, k, v)
    return gi


def _run(K, h, gi, front):
    """(token ids, front-end counters) of one generate() with the front end on or off"""
    L = K.raw()
    L.kcpp_expose_set_sample_front(int(front))
    L.kcpp_expose_mirostat_mu(1, 2.0 * gi.mirostat_tau)      # the process-lifetime mu: the same start for both runs
    stats = (ctypes.c_int64 * 4)()
    L.kcpp_expose_sample_front_stats(stats)                  # reading resets
    try:
        assert h.generate(gi).status == 1
    finally:
        L.kcpp_expose_set_sample_front(-1)
    L.kcpp_expose_sample_front_stats(stats)
    out = (ctypes.c_int * 64)()
    n = L.kcpp_expose_last_tokens(out, 64)
    return list(out[:n]), list(stats)


def _on_equals_off(K, h, gi):
    # a first run puts the prompt into the KV cache: the two compared runs then both fast-forward over it and evaluate
    # its last token as a single-token step (after a batched prefill the first logits come from other kernels, equal
    # only within rounding, and a sampled token is entitled to differ on that)
    _run(K, h, gi, False)
    on, s_on = _run(K, h, gi, True)
    off, s_off = _run(K, h, gi, False)
    # 8192 < the capacity and the logits are finite: nothing can need a fallback, a non-zero count is a bug
    assert s_on == [48, 0, 0, 0] and s_off == [0, 0, 0, 0]
    assert len(on) == 48 and on == off
    assert len(set(on)) > 4                                  # sampled text, not one token over and over
    return on


REQUESTS = {
    "defaults": dict(),
    "edits": dict(rep_pen=1.1, dry_multiplier=0.8, biases=[(300, 4.0), (5000, -3.0)], banned=[b"a"],
                  allow_eos_token=False, bypass_eos_token=False),
    "mirostat2": dict(mirostat=2),
    "temp_first_top_k_0": dict(sampler_order=[5, 6, 0, 1, 3, 4, 2], top_k=0),
}


@pytest.mark.parametrize("name", list(REQUESTS))
def test_generate_same_tokens_with_and_without_front_end(env, engine, name):
    _, K = env
    h, X, toks = engine
    tokens = _on_equals_off(K, h, _request(X, **dict(REQUESTS[name])))
    if name == "edits":                                      # the ban and the EOS suppression did reach the device
        from test_gpu_expose import piece
        _, _, ttypes = GW.spm_vocab(8192, GW.WORDS)
        banned = {t for t in range(8192) if b"a" in piece(toks, ttypes, t).lower()}
        assert len(banned) >= 5 and toks[2] == "</s>"
        assert 2 not in tokens and not banned & set(tokens)


def test_environment_switch_is_read_per_call(env, engine, monkeypatch):
    _, K = env
    h, X, _ = engine
    L, gi = K.raw(), _request(X)
    stats = (ctypes.c_int64 * 4)()
    for value, want in (("0", 0), ("1", 48)):
        monkeypatch.setenv("KCPP_SAMPLE_DEV", value)
        L.kcpp_expose_sample_front_stats(stats)
        assert h.generate(gi).status == 1
        L.kcpp_expose_sample_front_stats(stats)
        assert list(stats) == [want, 0, 0, 0]


def test_generate_layer_split_same_tokens(env, engine, tmp_path, monkeypatch):
    """three stages (KCPP_VIRTUAL_DEVICES puts them on the one GPU): the candidates come from the last stage.  Runs
    last in the module: it replaces the loaded model."""
    _, K = env
    h, X, _ = engine
    hp = dict(R.TINY, n_vocab=8192, n_layer=5)
    path = str(tmp_path / "split.gguf")
    GW.llama_gguf(path, hp, R.q4_k_m_types(hp["n_layer"]), 1234, GW.WORDS)
    monkeypatch.setenv("KCPP_VIRTUAL_DEVICES", "3")
    _load(h, X, path, split=(1.0, 2.0, 1.0), ubatch=16)
    _on_equals_off(K, h, _request(X))
