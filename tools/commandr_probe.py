#!/usr/bin/env python3
"""Single-token decode ms of an Aya-23-8B-shaped Command-R model on synthetic weights: n_embd 4096,
32 / 8 heads, n_ff 14336, 32 layers, vocabulary 256000, Q4_K_M types with a Q6_K tied embedding, at ~3.8k context.

Two models of the same shape and weights per repeat: "command-r" (set_norm_mode(1) + set_parallel_block(1) +
set_logit_scale: the LayerNorm prologue instances of q|k|v, gate|up and the head) and "llama" (the switches off: the RMS
prologue instances, the serial block), so the difference is what LayerNorm's second workgroup reduction, the shared
normalised row and the scale launch cost together in the token graph.  Per model: the prompt prefilled in ubatches,
--warmup greedy steps, then --steps greedy steps (token kept on the device) timed between two synchronisations.
No pass bar.  Appends one JSON line to --out.

    python tools/commandr_probe.py --out profiles/commandr_decode.jsonl
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32, Q4_K, Q6_K = 0, 12, 14
AYA_8B = dict(n_vocab=256000, n_embd=4096, n_head=32, n_head_kv=8, n_layer=32, n_ff=14336, n_ctx=4096, eps=1e-5,
              rope_base=10000.0)


def q4_k_m_types(n):
    ty = [Q6_K, F32, Q6_K]
    for i in range(n):
        more = i < n // 8 or i >= 7 * n // 8 or (i - n // 8) % 3 == 2
        v = Q6_K if more else Q4_K
        ty += [F32, Q4_K, Q4_K, v, Q4_K, F32, Q4_K, Q4_K, v]
    return ty


def decode_ms(K, cmdr, args):
    m = K.Model(AYA_8B, q4_k_m_types(AYA_8B["n_layer"]), max_ubatch=args.ubatch)
    m.synth(1234)
    if cmdr:
        m.set_norm_mode(1)
        m.set_parallel_block(1)
        m.set_logit_scale(0.0625)
    prompt = [1 + (7 * i) % 1000 for i in range(args.prompt)]
    m.decode(prompt, 0, want_logits=False)
    m.argmax()
    n = args.prompt
    for _ in range(args.warmup):
        m.decode_greedy(n)
        n += 1
    m.sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        m.decode_greedy_lagged(n)
        n += 1
    m.greedy_drain()
    m.sync()
    dt = time.perf_counter() - t0
    m.close()
    return 1e3 * dt / args.steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompt", type=int, default=3840)
    ap.add_argument("--ubatch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "commandr_decode.jsonl"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("commandr_probe needs a GPU: nothing is measured without one")
    import koboldcpp_amd.lib as K
    ms = {"command-r": [], "llama": []}
    for _ in range(args.repeat):                      # alternating, so drift lands on both
        for name in ms:
            ms[name].append(round(decode_ms(K, name == "command-r", args), 4))
    rec = {"model": "aya-23-8b shape, synthetic Q4_K_M, tied Q6_K embedding", "path": "Model.decode_greedy_lagged",
           "prompt": args.prompt, "steps": args.steps, "keys_at_end": args.prompt + args.warmup + args.steps,
           "decode_ms_per_token": ms, "decode_tok_s_best": {k: round(1e3 / min(v), 1) for k, v in ms.items()}}
    line = json.dumps(rec)
    print(line, flush=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
