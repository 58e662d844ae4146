"""Register / spill budget of the position-averaging kernels, read from the compiler's own metadata as
tests/test_kernel_resources.py does (hipcc -S cross-compiles for gfx950 without a GPU)."""
import os
import re

import pytest

from test_kernel_resources import HIPCC, _find, _resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_merge_kernels_use_no_scratch_and_no_spills(tmp_path):
    res = _resources("bz_merge.hip", tmp_path)
    zero = _find(res, "k_merge_zero")
    assert zero["vspill"] == 0 and zero["sspill"] == 0 and zero["scratch"] == 0 and zero["vgpr"] <= 32, zero
    for na in ("ILi9E", "ILi65E"):
        for name in ("k_merge_reduce", "k_merge_finish"):
            k = _find(res, name, na)
            assert k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0 and k["vgpr"] <= 64, (name, na, k)
    # the reduce kernel's staging area fits the 64 KiB a workgroup may declare, with room for several workgroups per CU
    for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)", _resources.asm):
        assert int(m.group(1)) <= 40 * 1024, m.group(0)
