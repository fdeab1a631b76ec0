"""The entries of the fused single-token mat-vec return what the launch plan says (csrc/gemv_plan.h): for the smallest
call that reaches each (kernel, instance parameters) the plan can return -- and each refusal code, which comes back
before any launch -- the real entry is called once on real buffers and its return code is the plan's.  A plan that named
an instance the kernel file does not build would come back as GEMV_ERR_NO_INSTANCE (-30).  No numerical result is
asserted here: tests/test_gpu_rs.py, test_gpu_gemv_dec.py, test_gpu_qkv_mixed.py, test_gpu_qwen2_kernels.py and the
test_gpu_moe*.py files do that."""
import pytest

import gemv_cells as C

pytestmark = pytest.mark.gpu


def test_entries_return_the_plans_code():
    import torch
    assert torch.cuda.is_available()
    import koboldcpp_amd.lib as K
    cells = C.enumerate_cells(K)
    kernels, codes = set(), set()
    for c in cells:
        p = C.plan_of(K, c)
        rc, _ = C.run_cell(torch, K, c)
        assert rc == c["rc"], (rc, c)
        if rc == 0:
            kernels.add(p.get("kernel", c["entry"]))
        codes.add(rc)
    assert kernels == {"rs", "rs_aux", "q4k", "stream", "unit", "mixed", "dual"}
    assert codes == {0, -3, -5, -6, -7, -8}
