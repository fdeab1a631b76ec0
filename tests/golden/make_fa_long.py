"""Generate tests/golden/fa_long.npz: the REFERENCE build's ggml_flash_attn_ext (oracle/_ref/ref_llama op fattn,
the AVX2 / F16C / FMA build of `make -C oracle ref`) on the strict-order attention cases of refharness.FA_CASES --
past the strict kernel's 512-key chunk, head dim 64, GQA ratios 1 / 4 / 8, a peaked softmax, masked prefixes and a
fully masked chunk, finite mask values.  Run in the build container only.

The inputs are not stored: refharness.fa_case() regenerates them from integer hashes, and the file keeps each
case's parameters, the CRC32 of the generated input bytes and the reference output y.  The reference harness takes
a contiguous [T][n_kv] mask; the layout variants of tests/test_gpu_fa_exact.py share these outputs."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import refharness as R  # noqa: E402


def main():
    out = {"cases": np.array(R.FA_FIXTURE_CASES)}
    for name in R.FA_FIXTURE_CASES:
        c = R.fa_case(name)
        T, H, HKV, D, n_kv = (c[n] for n in ("T", "H", "HKV", "D", "n_kv"))
        y = R.run_ref_op("fattn", c["q"].tobytes() + c["k"].tobytes() + c["v"].tobytes() + c["mask"].tobytes(),
                         T * H * D, [D, T, H, HKV, n_kv])
        assert np.all(np.isfinite(y))
        out[name + "_meta"] = np.array([T, H, HKV, D, n_kv, c["n_past"]], np.int64)
        out[name + "_crc"] = np.array(c["crc"], np.uint32)
        out[name + "_y"] = y.reshape(T, H, D)
    path = os.path.join(HERE, "fa_long.npz")
    np.savez_compressed(path, **out)
    print("wrote fa_long.npz: %d cases, %d bytes" % (len(R.FA_FIXTURE_CASES), os.path.getsize(path)))


if __name__ == "__main__":
    main()
