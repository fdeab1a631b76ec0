"""orc_flash_attn_ext_strict (oracle/ggml_oracle.c, R.flash_attn_strict) pinned to the reference build's
ggml_flash_attn_ext bit for bit: the condition that lets it stand in for the reference as the expected value of the
strict-parity kernel at shapes that have no fixture (tests/test_gpu_fa_exact.py).

tests/golden/fa_long.npz (make_fa_long.py) holds the reference outputs of refharness.FA_CASES -- past 512 keys, head
dim 64, GQA ratios 1 / 4 / 8, a peaked softmax, masked ranges, finite mask values -- and the CRC32 of each case's
generated inputs; ops.npz holds fa_1_256 / fa_5_300 with their inputs."""
import os

import numpy as np
import pytest

import refharness as R


@pytest.fixture(scope="module")
def fa_long():
    return np.load(os.path.join(R.ROOT, "tests", "golden", "fa_long.npz"))


def test_fixture_lists_the_cases(fa_long):
    assert [str(n) for n in fa_long["cases"]] == R.FA_FIXTURE_CASES


@pytest.mark.parametrize("name", R.FA_FIXTURE_CASES)
def test_generator_matches_fixture_crc(fa_long, name):
    """generator drift (another numpy, an edited hash) fails here, not as a parity miss"""
    c = R.fa_case(name)
    assert [c[n] for n in ("T", "H", "HKV", "D", "n_kv", "n_past")] == [int(x) for x in fa_long[name + "_meta"]]
    assert c["crc"] == int(fa_long[name + "_crc"])


def _bits_equal(got, ref, tag):
    n_diff = int((got.view(np.uint32) != ref.view(np.uint32)).sum())
    print("%s: %d of %d outputs differ in any bit" % (tag, n_diff, got.size))
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("name", R.FA_FIXTURE_CASES)
def test_strict_oracle_is_bit_equal_to_reference(fa_long, name):
    c = R.fa_case(name)
    ref = fa_long[name + "_y"]
    _bits_equal(R.flash_attn_strict(c["q"], c["k"], c["v"], c["mask"]), ref, name)
    # the layouts the GPU test passes, here on the oracle itself: q as the permuted view of [H][T][D], the mask rows
    # 64 elements apart and padded to 32 rows (the padding NaN: never read)
    T, H, D, n_kv = c["T"], c["H"], c["D"], c["n_kv"]
    qp = np.ascontiguousarray(c["q"].transpose(1, 0, 2)).transpose(1, 0, 2)
    mp = np.full((32, n_kv + 64), np.nan, np.float16)
    mp[:T, :n_kv] = c["mask"]
    _bits_equal(R.flash_attn_strict(qp, c["k"], c["v"], mp, q_strides=(D * 4, T * D * 4), mask_ld=n_kv + 64), ref,
                name + " permuted q, padded mask")


@pytest.mark.parametrize("key", ["fa_1_256", "fa_5_300"])
def test_strict_oracle_is_bit_equal_on_ops_fixtures(golden_ops, key):
    q, k, v, mask = (golden_ops[key + s] for s in ("_q", "_k", "_v", "_mask"))
    _bits_equal(R.flash_attn_strict(q, k, v, mask), golden_ops[key + "_y"], key)


def test_nonstrict_oracle_differs():
    """the double-dot orc_flash_attn_ext is NOT this function: were the two equal on a long case, the strict dot
    order would be going untested"""
    c = R.fa_case("live701_768")
    a = R.flash_attn_strict(c["q"], c["k"], c["v"], c["mask"])
    b = R.flash_attn(c["q"], c["k"], c["v"], c["mask"])
    assert not np.array_equal(a, b)
