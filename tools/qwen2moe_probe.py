#!/usr/bin/env python3
"""Decode and prefill tok/s of Qwen2-MoE shapes on synthetic weights: Qwen1.5-MoE-A2.7B (24 layers,
60 experts top-4, expert width 1408 with Q5_0 / Q8_0 down experts, shared expert 5632) and Qwen2-57B-A14B (28 layers,
64 experts top-8, expert width 2560, shared expert 20480), Q4_K_M-like types, through the drop-in engine's bench path
(kcpp_engine_bench_ex: load_model's stages and forward(), one stage here).

Per shape and repeat: a fresh engine, a 64-token warm-up prefill, the timed prefill of --prompt tokens in ubatches of
--ubatch (to the stage's drain), then --warmup + --steps greedy single-token steps with the token kept on the device,
timed over the --steps ones between two device synchronisations.  No pass bar: the figures are the baseline for
batching the top-k slots into one gate|up and one down launch.  Appends one JSON line per shape to --out.

    python tools/qwen2moe_probe.py --out profiles/qwen2moe_decode.jsonl
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32, F16, Q4_K, Q6_K, Q5_0, Q8_0 = 0, 1, 12, 14, 6, 8

SHAPES = {
    "qwen1.5-moe-a2.7b": dict(n_vocab=151936, n_embd=2048, n_head=16, n_head_kv=16, n_layer=24, n_ff=1408, n_ctx=4096,
                              eps=1e-6, rope_base=1000000.0, n_expert=60, n_expert_used=4, n_ff_shexp=5632, moe_norm_w=0),
    "qwen2-57b-a14b": dict(n_vocab=151936, n_embd=3584, n_head=28, n_head_kv=4, n_layer=28, n_ff=2560, n_ctx=4096,
                           eps=1e-6, rope_base=1000000.0, n_expert=64, n_expert_used=8, n_ff_shexp=20480, moe_norm_w=0),
}


def q4_k_m_types(hp):
    """Q4_K_M's choices: Q6_K attn_v / down projections on the 'more bits' layers, Q6_K output; rows of 1408 cannot be
    K-quants, so such ffn_down_exps are Q5_0 (Q8_0 on the 'more bits' layers), llama.cpp's fallbacks"""
    n = hp["n_layer"]
    ty = [Q4_K, F32, Q6_K]
    for i in range(n):
        more = i < n // 8 or i >= 7 * n // 8 or (i - n // 8) % 3 == 2
        v = Q6_K if more else Q4_K
        down = v if hp["n_ff"] % 256 == 0 else (Q8_0 if more else Q5_0)
        ty += [F32, Q4_K, Q4_K, v, Q4_K, F32, Q4_K, Q4_K, down, F32, F32, Q4_K, Q4_K, v]
    return ty


def probe(K, name, args):
    hp = SHAPES[name]
    types = q4_k_m_types(hp)
    runs = [K.engine_bench(hp, types, 1, args.prompt, args.ubatch, args.warmup, args.steps) for _ in range(args.repeat)]
    dec_ms = [1e3 * r["decode_s"] / args.steps for r in runs]
    return {"model": name + " synthetic Q4_K_M-like", "path": "kcpp_engine_bench_ex, 1 stage", "prompt": args.prompt,
            "ubatch": args.ubatch, "steps": args.steps, "keys_at_end": runs[-1]["n_past"],
            "prefill_tok_s": [round(args.prompt / r["prefill_s"], 1) for r in runs],
            "decode_ms_per_token": [round(x, 3) for x in dec_ms], "decode_tok_s_best": round(1e3 / min(dec_ms), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=",".join(SHAPES))
    ap.add_argument("--prompt", type=int, default=512)
    ap.add_argument("--ubatch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qwen2moe_decode.jsonl"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("qwen2moe_probe needs a GPU: nothing is measured without one")
    import koboldcpp_amd.lib as K
    for name in args.shapes.split(","):
        rec = probe(K, name, args)
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
