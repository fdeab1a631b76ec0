"""Prefill flash-attention A/B (tools only), HIP-event timed, 512 queries at D 128 (Llama-3-8B's 32 / 8 heads by
default; --heads / --kv-heads for another GQA ratio).  Two modes, the candidates alternated in one process, --rounds
times each, every round printed (the spread is the rounds'):
  variants (default)  kcpp_flash_attn_prefill_mfma under kcpp_fa_prefill_set_variant numbers (default 2 vs 3; G = 4)
  --paths             kcpp_flash_attn force_path 2 (k_fa_prefill<128>, FMA tiles) vs 3 (k_fa_prefill_mfma3)
usage: python tools/fa_ab.py [--heads H --kv-heads HKV] [--paths] [--rounds N] [--out FILE.jsonl] [variants...]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import koboldcpp_amd.lib as K  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--heads", type=int, default=32)
    ap.add_argument("--kv-heads", type=int, default=8)
    ap.add_argument("--paths", action="store_true", help="alternate kcpp_flash_attn force_path 2 and 3")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--out", help="append the JSON lines to this file too")
    ap.add_argument("variants", nargs="*", type=int)
    a = ap.parse_args()
    s = torch.cuda.current_stream()
    H, HKV, D, T = a.heads, a.kv_heads, 128, 512
    n_ctx = 4096
    q = torch.randn(T, H, D, device="cuda").half()
    kc = (torch.randn(n_ctx, HKV, D, device="cuda") * 0.5).half()
    vc = torch.randn(n_ctx, HKV, D, device="cuda").half()
    out = torch.empty(T, H, D, device="cuda")
    ws = torch.zeros(K.fa_workspace_bytes(16, H, n_ctx), dtype=torch.uint8, device="cuda")
    cands = [2, 3] if a.paths else (a.variants or [2, 3])
    for n_past in [int(x) for x in os.environ.get("FA_NPAST", "0,1536,3328").split(",")]:
        for rnd in range(a.rounds):
            for v in cands:
                if a.paths:
                    run = lambda: K.call("kcpp_flash_attn", q.data_ptr(), kc.data_ptr(), vc.data_ptr(), out.data_ptr(), None,
                                         ws.data_ptr(), T, H, HKV, D, n_past, None, n_ctx, 1.0 / D ** 0.5, v, s.cuda_stream)
                else:
                    K.raw().kcpp_fa_prefill_set_variant(v)
                    run = lambda: K.call("kcpp_flash_attn_prefill_mfma", q.data_ptr(), kc.data_ptr(), vc.data_ptr(),
                                         out.data_ptr(), T, H, HKV, D, n_past, 1.0 / D ** 0.5, s.cuda_stream)
                for _ in range(3):
                    run()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record(s)
                for _ in range(10):
                    run()
                e1.record(s)
                torch.cuda.synchronize()
                us = e0.elapsed_time(e1) / 10 * 1e3
                fl = 4.0 * H * D * sum(n_past + t + 1 for t in range(T))       # causal QK^T + PV
                line = json.dumps({"heads": H, "kv_heads": HKV, "n_past": n_past, "T": T,
                                   "force_path" if a.paths else "variant": v, "round": rnd, "us": round(us, 1),
                                   "TFLOPs": round(fl / us / 1e6, 1)})
                print(line, flush=True)
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(line + "\n")
    K.raw().kcpp_fa_prefill_set_variant(0)


if __name__ == "__main__":
    main()
