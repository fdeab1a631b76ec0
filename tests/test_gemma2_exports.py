"""CPU-side check of the Gemma-2 additions to the C ABI: the built library exports the soft-cap forms of the graph
attention entry points and the GELU table setup, and koboldcpp_amd/lib.py declares them (no compute calls)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "koboldcpp_amd", "koboldcpp_hipblas.so")
NEW = ["kcpp_flash_attn_ext_sc", "kcpp_flash_attn_ext_dec_sc", "kcpp_flash_attn_ext_exact_sc", "kcpp_ggml_gelu_table_init"]


def test_library_exports_the_softcap_entry_points():
    assert os.path.exists(LIB), "run __graft_entry__.build() first"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    missing = [n for n in NEW if n not in exported]
    assert not missing, missing
    # the old names stay (thin wrappers passing cap 0)
    for n in ("kcpp_flash_attn_ext", "kcpp_flash_attn_ext_dec", "kcpp_flash_attn_ext_exact"):
        assert n in exported, n


def test_python_binding_declares_them():
    import ctypes
    import koboldcpp_amd.lib as K
    L = K.raw()
    for n in NEW:
        assert getattr(L, n).argtypes is not None, n
    # the trailing argument is the float logit_softcap, after the arguments of the old form
    for n in ("kcpp_flash_attn_ext", "kcpp_flash_attn_ext_exact"):
        old, new = getattr(L, n).argtypes, getattr(L, n + "_sc").argtypes
        assert list(new[:-1]) == list(old) and new[-1] is ctypes.c_float, n
    assert L.kcpp_flash_attn_ext_dec_sc.argtypes[-1] is ctypes.c_float
    # the D = 256 workspace goes through the existing size function; its D <= 128 results are the old formula's
    assert K.fa_ext_workspace_bytes(1, 16, 4096, 256) >= 2048 + 16 * 64 * (256 * 4 + 8)
    assert K.fa_ext_workspace_bytes(16, 16, 4096, 256) >= 2048 + 16 * 16 * 64 * (256 * 4 + 8)
    for T, H, n_kv in ((1, 8, 701), (5, 32, 4096), (40, 8, 300)):
        want = ((L.kcpp_fa_workspace_bytes(T, H, n_kv) + 255) & ~255) + T * H * 128 * 2 + 256
        assert K.fa_ext_workspace_bytes(T, H, n_kv, 128) == want
        assert K.fa_ext_workspace_bytes(T, H, n_kv, 64) == ((L.kcpp_fa_workspace_bytes(T, H, n_kv) + 255) & ~255) + T * H * 64 * 2 + 256
