"""Head-dim-256 graph-form attention (csrc/attn_d256.hip) beside the D = 128 production paths (tools only).

decode : kcpp_flash_attn_ext_dec_sc at the Gemma-2-9B shape (H 16, HKV 8, D 256) and, in the same run, at equal K/V
         bytes on the D = 128 pair (H 32, HKV 16, D 128: k_fa_dec5<GRAPH> + k_fa_comb4), n_kv 4096 and 8192.  32
         layers' caches are rotated so the Infinity Cache cannot serve them; the 32 calls are captured in one graph
         (as a decode step issues them) and the graph is timed with HIP events: warm-up replays, then the median of
         REPS replays.  Reported: us per layer, K/V bytes over time as a fraction of the HBM peak, the ratio.
prefill: kcpp_flash_attn_ext_sc, T 512 at n_kv 4096 under a causal mask, D = 256 (the MFMA tile kernel) beside D = 128
         at equal FLOPs (H 32, HKV 16: the masked k_fa_prefill<128>), 8 caches rotated; time and fraction of the f16
         MFMA peak over the live (query, key) pairs.
usage: python tools/fa_d256_bench.py [--out FILE]      (one JSON line per measurement, also appended to FILE)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import koboldcpp_amd.lib as K  # noqa: E402

HBM_PEAK_GBS = 8000.0            # spec (bench.py's constants)
MFMA_F16_PEAK_TFLOPS = 2500.0
WARMUP, REPS = 5, 30


def timed(fn, n_inner):
    """fn() issues n_inner calls on the current stream; captured once, replayed: us per call (min, median, max)"""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    for _ in range(WARMUP):
        g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / n_inner)
    ts = np.sort(np.array(ts))
    return float(ts[0]), float(np.median(ts)), float(ts[-1])


def decode(H, HKV, D, n_kv, NL=32):
    torch.manual_seed(0)
    kc = (torch.randn(NL, n_kv * HKV * D, device="cuda") * 0.5).half()
    vc = torch.randn(NL, n_kv * HKV * D, device="cuda").half()
    q = torch.randn(NL, H * D, device="cuda")
    mask = torch.zeros(n_kv, dtype=torch.float16, device="cuda")
    out = torch.zeros(NL, H * D, device="cuda")
    ws = torch.zeros(K.fa_ext_workspace_bytes(1, H, n_kv, D), dtype=torch.uint8, device="cuda")

    def step():
        sp = torch.cuda.current_stream().cuda_stream
        for l in range(NL):
            K.call("kcpp_flash_attn_ext_dec_sc", q[l].data_ptr(), D * 4, kc[l].data_ptr(), vc[l].data_ptr(), HKV * D, D,
                   mask.data_ptr(), out[l].data_ptr(), ws.data_ptr(), H, HKV, D, n_kv, 1.0 / D ** 0.5, sp, 0.0)
    lo, med, hi = timed(step, NL)
    kvb = 2 * n_kv * HKV * D * 2
    return {"what": "decode", "H": H, "HKV": HKV, "D": D, "n_kv": n_kv, "kv_bytes": kvb, "us_min": round(lo, 2),
            "us_median": round(med, 2), "us_max": round(hi, 2), "GBps": round(kvb / med / 1e3, 1),
            "hbm_frac": round(kvb / med / 1e3 / HBM_PEAK_GBS, 4)}


def prefill(H, HKV, D, T, n_kv, NL=8):
    torch.manual_seed(1)
    n_past = n_kv - T
    kc = (torch.randn(NL, n_kv * HKV * D, device="cuda") * 0.5).half()
    vc = torch.randn(NL, n_kv * HKV * D, device="cuda").half()
    q = torch.randn(NL, T * H * D, device="cuda")
    m = np.full((T, n_kv), -np.inf, np.float16)
    for t in range(T):
        m[t, :n_past + t + 1] = 0
    mask = torch.from_numpy(m.view(np.int16)).cuda()
    out = torch.zeros(NL, T * H * D, device="cuda")
    ws = torch.zeros(K.fa_ext_workspace_bytes(T, H, n_kv, D), dtype=torch.uint8, device="cuda")

    def step():
        sp = torch.cuda.current_stream().cuda_stream
        for l in range(NL):
            K.call("kcpp_flash_attn_ext_sc", q[l].data_ptr(), H * D * 4, D * 4, kc[l].data_ptr(), vc[l].data_ptr(),
                   mask.data_ptr(), n_kv, out[l].data_ptr(), ws.data_ptr(), T, H, HKV, D, n_kv, 1.0 / D ** 0.5, sp, 0.0)
    lo, med, hi = timed(step, NL)
    pairs = sum(n_past + t + 1 for t in range(T))
    flops = 4.0 * D * H * pairs
    return {"what": "prefill", "H": H, "HKV": HKV, "D": D, "T": T, "n_kv": n_kv, "mask": "causal", "flops": flops,
            "us_min": round(lo, 1), "us_median": round(med, 1), "us_max": round(hi, 1),
            "TFLOPS": round(flops / med / 1e6, 2), "f16_peak_frac": round(flops / med / 1e6 / MFMA_F16_PEAK_TFLOPS, 5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gemma2_fa_d256.jsonl"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    rows = []
    for n_kv in (4096, 8192):
        r256 = decode(16, 8, 256, n_kv)
        r128 = decode(32, 16, 128, n_kv)
        rows += [r256, r128, {"what": "decode_ratio", "n_kv": n_kv, "d256_over_d128_time": round(r256["us_median"] / r128["us_median"], 3),
                              "d128_spread": round((r128["us_max"] - r128["us_min"]) / r128["us_median"], 3)}]
    p256 = prefill(16, 8, 256, 512, 4096)
    p128 = prefill(32, 16, 128, 512, 4096)
    rows += [p256, p128, {"what": "prefill_ratio", "d256_over_d128_time": round(p256["us_median"] / p128["us_median"], 3)}]
    with open(a.out, "a") as f:
        for r in rows:
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
