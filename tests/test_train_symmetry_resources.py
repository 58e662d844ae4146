"""The staging kernel of the per-row training symmetry in the compiler's own metadata (tests/kernel_meta.py: each
source once per process): one kernel, no VGPR spills, no SGPR spills, no scratch; its only shared memory is the four waves' error
counts, and it contains no atomic -- a workgroup adds to its own error word."""
import os
import re

import pytest

import kernel_meta
from kernel_meta import compile_asm

needs_hipcc = pytest.mark.skipif(not os.path.exists(kernel_meta.HIPCC), reason="needs hipcc")


@needs_hipcc
def test_no_spills_no_scratch_no_atomics():
    asm = compile_asm("bz_train_sym.hip")
    assert len(asm.kernels) == 1, list(asm.kernels)
    sym = asm.find("k_train_sym_batch")
    k = asm.kernels[sym]
    assert (k["vspill"], k["sspill"], k["scratch"]) == (0, 0, 0), k
    assert k["max_wg"] == 256 and k["lds_static"] == 4 * 4 and k["agpr"] == 0, k
    assert k["vgpr"] <= 64, k   # 16 policy entries in flight per lane and their addresses
    assert not re.search(r"atomic", asm.body(sym))
