"""Qwen2 speed (tools only, not bench.py): a Qwen2.5-7B-shaped synthetic Q4_K_M model (28 layers, n_embd 3584,
n_ff 18944, 28 / 4 heads, vocab 152064) with q / k / v biases and NeoX rope pairs -- prefill tok/s over the
prompt (3328 tokens by default), then single-token decode over the following keys (3336-3848 by default), the fused
decode chain against set_fused_decode(0), alternated in one process (two models, the same weights) so that both see
the same machine state.

Times are host clocks around work that ends in a device synchronise; every timed shape is warmed first.
Each timed decode window is --steps tokens (256: about half a second); the context wraps nowhere: the prompt, the
warm-up and rounds x steps tokens per model must fit n_ctx.
usage: python tools/qwen2_bench.py [--steps 256] [--rounds 2] [--prompt 3328]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import koboldcpp_amd.lib as K  # noqa: E402
import refharness as R  # noqa: E402

HP = dict(n_vocab=152064, n_embd=3584, n_head=28, n_head_kv=4, n_layer=28, n_ff=18944, n_ctx=4096, eps=1e-6,
          rope_base=1000000.0)


def model(fused):
    m = K.Model(HP, R.q4_k_m_types(HP["n_layer"]), max_ubatch=512)
    m.synth(1234)
    m.set_rope_mode(2)
    ekv = HP["n_head_kv"] * (HP["n_embd"] // HP["n_head"])
    for il in range(HP["n_layer"]):
        rng = np.random.default_rng(il)
        m.set_qkv_bias(il, *[rng.standard_normal(n).astype(np.float32) for n in (HP["n_embd"], ekv, ekv)])
    m.set_fused_decode(fused)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--prompt", type=int, default=3328)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    assert a.prompt + 8 + a.rounds * a.steps <= HP["n_ctx"], "prompt + warm-up + timed tokens exceed n_ctx"
    prompt = [16 + (i * 7919) % 1000 for i in range(a.prompt)]
    ms = {"fused": model(True), "unfused": model(False)}
    pre = {}
    for name, m in ms.items():
        m.decode(prompt[:512], 0, want_logits=False)          # warm-up: every prefill kernel of a full ubatch
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m.decode(prompt, 0, want_logits=False)
        torch.cuda.synchronize()
        pre[name] = a.prompt / (time.perf_counter() - t0)
        m.argmax()
    n = {name: a.prompt for name in ms}
    for name, m in ms.items():                                 # warm-up: graph capture and first replays
        for _ in range(8):
            m.decode_greedy(n[name])
            n[name] += 1
    torch.cuda.synchronize()
    per = {name: [] for name in ms}
    for _ in range(a.rounds):
        for name, m in ms.items():
            t0 = time.perf_counter()
            for _ in range(a.steps):
                m.decode_greedy(n[name])
                n[name] += 1
            m.sync()
            per[name].append((time.perf_counter() - t0) / a.steps * 1e3)
    for m in ms.values():
        m.close()
    out = {"model": "qwen2.5-7b-shaped synthetic Q4_K_M", "prompt": a.prompt, "keys_at_end": n["fused"],
           "prefill_tok_s": {k: round(v, 1) for k, v in pre.items()},
           "decode_ms_per_token": {k: [round(x, 3) for x in v] for k, v in per.items()},
           "decode_tok_s_best": {k: round(1e3 / min(v), 1) for k, v in per.items()}}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
