"""The prefill attention's launch plan at D = 128 (csrc/fa_plan.h through kcpp_fa_prefill_plan), host only.

k_fa_prefill_mfma3's workgroup has four slots of (one head, 16 queries).  For G = H / HKV the plan gives gh heads and
qb = 4 / gh consecutive 16-query blocks per workgroup; the kernel decodes its 1-D block index as (attn_mfma.hip):

    sp, b = divmod(bid, nb0)                                  the key split, outermost
    HKV % 8 == 0:  hk = b % 8 + 8 (b // 8 % (HKV // 8)), wq = b // 8 // (HKV // 8)       else:  wq, hk = divmod(b, HKV)
    qbg, gsub = divmod(wq, G // gh)
    slot s: head hk G + gsub gh + s % gh, query block qbg qb + s // gh

and walks the 64-key tiles [sp ch, min((sp + 1) ch, ntile_wg)) of the keys its LAST query block sees; a workgroup whose
sp ch >= ntile_wg leaves at once.  k_fa_split_merge has one workgroup per slot and reads, for a query block, the splits
below ceil(ntile_block / ch).  This file re-derives all of that from the plan's fields and checks that every (query,
head) has one owner, every key tile of every query block one split, every split the merge reads a workgroup that ran,
the partials fit the workspace, and that H = 4 HKV plans exactly what the code planned before there was a plan."""
import os
import subprocess
import sys

import numpy as np
import pytest

GS_ = range(1, 9)
HKVS = (1, 2, 4, 8)
TS = (1, 15, 16, 17, 33, 64, 65, 70, 512)
PASTS = (0, 63, 64, 130, 4090, 32760)
HEADER, PS_BYTES, SPLITS, SPLIT_T = 2048, 16 * 132 * 4, 32, 64


@pytest.fixture(scope="module")
def K():
    import koboldcpp_amd.lib as K
    return K


def cdiv(a, b):
    return -(-a // b)


def decode(b, HKV, G, gh, qb):
    """block index within a split -> (kv head, gsub, first query block)"""
    if HKV % 8 == 0:
        j = b // 8
        hk, wq = b % 8 + 8 * (j % (HKV // 8)), j // (HKV // 8)
    else:
        wq, hk = divmod(b, HKV)
    qbg, gsub = divmod(wq, G // gh)
    return hk, gsub, qbg * qb


@pytest.mark.parametrize("G", GS_)
@pytest.mark.parametrize("HKV", HKVS)
def test_every_query_and_head_has_one_owner(K, G, HKV):
    H = G * HKV
    for T in TS:
        p = K.fa_prefill_plan(T, H, HKV)
        gh, qb = p["gh"], p["qb"]
        assert gh == (4 if G % 4 == 0 else 2 if G % 2 == 0 else 1) and gh * qb == 4
        nqb = cdiv(T, 16)
        assert p["nb0"] == cdiv(nqb, qb) * HKV * (G // gh) == cdiv(cdiv(nqb, qb) * qb * H, 4)
        owners = np.zeros((cdiv(nqb, qb) * qb, H), np.int32)
        for b in range(p["nb0"]):
            hk, gsub, qb0 = decode(b, HKV, G, gh, qb)
            for s in range(4):
                owners[qb0 + s // gh, hk * G + gsub * gh + s % gh] += 1
        assert (owners == 1).all(), (T, H, HKV)        # (blocks at and past nqb hold no query: their slots store nothing)
        if HKV % 8 == 0 or 8 % HKV == 0:               # blocks b and b + 8 share an XCD: a kv head's blocks sit on the XCDs
            for b in range(p["nb0"]):                  # congruent to it mod min(8, HKV), so no XCD serves two kv heads
                assert decode(b, HKV, G, gh, qb)[0] % min(8, HKV) == b % min(8, HKV)


@pytest.mark.parametrize("G", GS_)
@pytest.mark.parametrize("HKV", HKVS)
@pytest.mark.parametrize("have_ws", [False, True])
def test_every_key_tile_in_one_split_and_partials_fit(K, G, HKV, have_ws):
    H = G * HKV
    ws_split = K.raw().kcpp_fa_split_ws_bytes(H)
    for T in TS:
        for n_past in PASTS:
            p = K.fa_prefill_plan(T, H, HKV, 128, n_past, have_ws)
            qb, nsp, ch, nb0 = p["qb"], p["nsp"], p["ch"], p["nb0"]
            nqb = cdiv(T, 16)
            ntile_all = cdiv(n_past + T, 64)
            split = have_ws and T <= SPLIT_T and nsp > 1
            assert p["kernel"] in ("fma", "mfma_split" if split else "mfma")
            assert 1 <= nsp <= SPLITS and nsp * ch >= ntile_all and (nsp - 1) * ch < ntile_all
            if not (have_ws and T <= SPLIT_T):
                assert nsp == 1
            if nsp == 1:
                assert (p["merge_grid"], p["part_bytes"]) == (0, 0)
            else:
                assert p["merge_grid"] == 4 * nb0                       # one merge workgroup per slot
                assert p["part_bytes"] == nb0 * nsp * 4 * PS_BYTES      # [workgroup][split][slot]
            assert HEADER + p["part_bytes"] <= ws_split <= K.fa_workspace_bytes(16, H, n_past + T)
            for blk in range(nqb):
                ntile_blk = cdiv(n_past + min(16 * (blk + 1), T), 64)
                ntile_wg = cdiv(n_past + min(16 * (blk // qb * qb + qb), T), 64)
                assert ntile_blk <= ntile_wg <= ntile_all
                seen = np.zeros(ntile_wg, np.int32)
                for sp in range(nsp):
                    if sp * ch < ntile_wg:                              # (else the workgroup returns at once)
                        seen[sp * ch:min(sp * ch + ch, ntile_wg)] += 1
                assert (seen == 1).all()
                nsp_blk = cdiv(ntile_blk, ch)                           # what the merge reads of this block
                assert 1 <= nsp_blk <= nsp and nsp_blk * ch >= ntile_blk
                assert (nsp_blk - 1) * ch < ntile_blk <= ntile_wg       # each of them ran and held a key of the block


@pytest.mark.parametrize("HKV", HKVS + (3, 16, 32))
def test_ratio_4_plans_what_it_always_did(K, HKV):
    """H = 4 HKV: the arithmetic of kcpp_flash_attn_prefill_mfma_ex before the plan existed, copied here"""
    H = 4 * HKV
    for T in TS:
        for n_past in PASTS:
            for have_ws in (False, True):
                nb0 = cdiv(T, 16) * HKV
                ntile = cdiv(n_past + T, 64)
                nsp, ch = 1, ntile
                if have_ws and T <= 64 and nb0 <= 512:
                    want = min(32, max(1, 512 // nb0))
                    ch = cdiv(ntile, want)
                    nsp = cdiv(ntile, ch)
                    if nsp == 1:
                        ch = ntile
                p = K.fa_prefill_plan(T, H, HKV, 128, n_past, have_ws)
                assert p == dict(kernel="mfma_split" if nsp > 1 else "mfma", gh=4, qb=1, nb0=nb0, nsp=nsp, ch=ch,
                                 merge_grid=4 * nb0 if nsp > 1 else 0,
                                 part_bytes=nb0 * nsp * 4 * PS_BYTES if nsp > 1 else 0), (T, HKV, n_past, have_ws)


def test_split_workspace_bytes(K):
    for H in range(4, 129, 4):       # what the library returned before: (64 / 16) (H / 4) 32 splits x 4 heads x partial
        assert K.raw().kcpp_fa_split_ws_bytes(H) == HEADER + 4 * (H // 4) * 32 * 4 * PS_BYTES
    for H in (1, 2, 3, 5, 6, 7, 10, 14):     # H / 4 used to truncate: 64 tokens x H heads x 32 splits must fit
        assert K.raw().kcpp_fa_split_ws_bytes(H) >= HEADER + 4 * H * 32 * PS_BYTES


def test_plan_rejects_what_the_kernel_does_not_cover(K):
    assert K.fa_prefill_plan(70, 8, 2, 64) is None             # D != 128
    assert K.fa_prefill_plan(70, 7, 2) is None                 # H % HKV
    assert K.fa_prefill_plan(70, 18, 2) is None                # G = 9
    assert K.fa_prefill_plan(70, 16, 2) is not None


def test_env_sends_other_ratios_to_the_fma_tiles():
    """KCPP_FA_PREFILL_MFMA=0 (read once, so in a child process): every ratio but 4 plans the FMA kernel in the auto
    path; the MFMA geometry in the other fields stays (the direct entries still run it)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import koboldcpp_amd.lib as K\n"
            "print([K.fa_prefill_plan(70, 2 * G, 2)['kernel'] for G in range(1, 9)])\n"
            "print(K.fa_prefill_plan(70, 14, 2)['nb0'])\n")
    env = dict(os.environ, KCPP_FA_PREFILL_MFMA="0", PYTHONPATH=root)
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout
    kern, nb0 = out.strip().splitlines()[-2:]
    assert eval(kern) == ["fma"] * 3 + ["mfma"] + ["fma"] * 4
    assert int(nb0) == 2 * 2 * 7                                # ceil(5 / 4) query groups x 2 kv heads x 7 heads
