"""What a sampled request decodes at, beside the greedy figure: the drop-in generate() on the Llama-3-8B Q4_K_M bench
model (bench.generate_path's setup: the sparse full-size GGUF through load_model, weights from
kcpp_expose_synth_weights), a 256-token prompt, then ONE generate() of 256 tokens per leg --

  greedy    koboldcpp --benchmark's request (the chain is an argmax: the device's own argmax is read back)
  off / on  koboldcpp's default request (koboldcpp.py:876-897: temperature 0.7, top_k 100, top_p 0.92, rep_pen 1,
            sampler_order 6,0,1,3,4,2,5) with the sampling front end off / on, alternating off, on, off, on

-- tok/s = 1000 / get_last_eval_time() of each, one JSON line per leg.  The same seed in every leg: "same_tokens" says
the on legs drew what the off legs drew.  A library without the front end's hooks (KCPP_LIB pointing at an older build)
runs the greedy and the off legs only: the baseline the off legs are held to.

--grammar FILE puts that GBNF text (tools/json_stream.gbnf: JSON values in an array that never closes, so no request
ends early) into every request, the warm-up ones included (they also pay the one-time decode of the vocabulary's
pieces); EOS is allowed in all of them, so a grammar that can finish ends its request.  Each line then also carries the
grammar counters (kcpp_expose_grammar_stats) and the host milliseconds per token spent on the reject masks.

  python tools/sample_probe.py [--label NAME] [--out FILE.jsonl] [--prompt 256] [--gen 256] [--grammar FILE]"""
import argparse
import ctypes
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402,F401  (first: the library then shares torch's HIP runtime instead of loading a second one)
import bench  # noqa: E402
import gguf_writer as GW  # noqa: E402
from koboldcpp_amd import expose as X  # noqa: E402


def request(prompt, max_ctx, n, greedy, grammar=b""):
    gi = X.generation_inputs()
    gi.prompt, gi.memory = prompt, b""
    gi.max_context_length, gi.max_length, gi.seed = max_ctx, n, 7
    gi.temperature, gi.top_k, gi.rep_pen = (0.1, 1, 1.0) if greedy else (0.7, 100, 1.0)
    gi.top_a, gi.top_p, gi.min_p, gi.typical_p, gi.tfs = 0.0, 0.92, 0.0, 1.0, 1.0
    gi.rep_pen_range, gi.rep_pen_slope, gi.presence_penalty = 320, 1.0, 0.0
    gi.mirostat, gi.mirostat_tau, gi.mirostat_eta = 0, 5.0, 0.1
    gi.dry_multiplier, gi.dry_base, gi.dry_allowed_length, gi.dry_penalty_last_n = 0.0, 1.75, 2, 320
    gi.xtc_threshold, gi.xtc_probability = 0.2, 0.0
    gi.dynatemp_range, gi.dynatemp_exponent, gi.smoothing_factor = 0.0, 1.0, 0.0
    for i, v in enumerate([6, 0, 1, 3, 4, 2, 5]):
        gi.sampler_order[i] = v
    gi.sampler_len = 7
    # the benchmark bans EOS; the default request allows it (ban_eos_token False)
    gi.allow_eos_token, gi.bypass_eos_token = (False, False) if greedy and not grammar else (True, False)
    gi.grammar, gi.grammar_retain_state = grammar, False
    return gi


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="tree")
    ap.add_argument("--out", default=None)
    ap.add_argument("--prompt", type=int, default=256)
    ap.add_argument("--gen", type=int, default=256)
    ap.add_argument("--ubatch", type=int, default=512)
    ap.add_argument("--grammar", default=None, help="a GBNF file: every request is constrained by it")
    a = ap.parse_args()
    grammar = open(a.grammar, "rb").read() if a.grammar else b""
    hp, types, max_ctx = dict(bench.LLAMA3_8B), bench.q4_k_m_types(32), a.prompt + a.gen
    lines = []
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "llama3-8b-q4_k_m-synthetic.gguf")
        GW.llama_gguf(path, dict(hp, n_ctx=8192), types, 1234, GW.WORDS, sparse=True)
        h = X.init_library()
        li = X.load_model_inputs()
        li.model_filename = path.encode()
        li.max_context_length, li.blasbatchsize, li.gpulayers, li.flash_attention = max_ctx, a.ubatch, 999, True
        li.rope_freq_base, li.rope_freq_scale = 10000.0, 0.0
        if not h.load_model(li):
            raise RuntimeError("load_model failed")
        h.kcpp_expose_synth_weights.argtypes = [ctypes.c_uint64]
        if h.kcpp_expose_synth_weights(1234) != 0:
            raise RuntimeError("kcpp_expose_synth_weights failed")
        has_front = hasattr(h, "kcpp_expose_set_sample_front")
        prompt = b" 1" * (a.prompt + 64)                 # koboldcpp.py:4300-4303, cut to --prompt tokens
        if grammar:
            h.kcpp_expose_grammar_mask_ms.restype = ctypes.c_double

        def leg(name, greedy, front):
            if has_front:
                h.kcpp_expose_set_sample_front(-1 if front is None else int(front))
            if grammar:
                h.kcpp_expose_grammar_stats((ctypes.c_int64 * 6)())
            if h.generate(request(prompt, max_ctx, a.gen, greedy, grammar)).status != 1:
                raise RuntimeError("generate failed")
            r = {"label": a.label, "leg": name, "decode_tok_s": round(1000.0 / h.get_last_eval_time(), 2),
                 "ms_per_token": round(h.get_last_eval_time(), 4), "gen_tokens": h.get_last_token_count(),
                 "n_prompt": a.prompt}
            if has_front:
                stats, toks = (ctypes.c_int64 * 4)(), (ctypes.c_int * a.gen)()
                h.kcpp_expose_sample_front_stats(stats)
                r["front_stats"] = list(stats)
                r["tokens"] = list(toks[:h.kcpp_expose_last_tokens(toks, a.gen)])
            if grammar:
                gs = (ctypes.c_int64 * 6)()
                h.kcpp_expose_grammar_stats(gs)
                r["grammar_stats"] = list(gs)
                r["mask_ms_per_token"] = round(h.kcpp_expose_grammar_mask_ms() / max(1, r["gen_tokens"]), 4)
            return r

        for g in (True, False):                          # warm-up: first touch, graph capture, both kinds of request
            h.generate(request(b"hello world", max_ctx, 8, g, grammar))
        if has_front:
            h.kcpp_expose_sample_front_stats((ctypes.c_int64 * 4)())
        lines.append(leg("greedy", True, None))
        for i in range(4 if has_front else 2):
            on = has_front and i % 2 == 1
            lines.append(leg("on" if on else "off", False, on if has_front else None))
    if has_front:
        ref = next(r["tokens"] for r in lines if r["leg"] == "off")
        for r in lines:
            if r["leg"] != "greedy":
                r["same_tokens"] = r["tokens"] == ref
    for r in lines:
        r.pop("tokens", None)
        print(json.dumps(r))
    if a.out:
        with open(a.out, "a") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
