"""Register / spill budget of the extended optimiser's kernels, read from the compiler's own metadata as
tests/test_kernel_resources.py does (hipcc -S cross-compiles for gfx950 without a GPU).  The two new kernels stream their
operands once and must not touch scratch; the kernels they stand next to -- k_train_finish, and k_train_adam, whose arithmetic
the new update repeats -- must compile to what they were before the feature existed: the values pinned below were read from
the commit before it.  (The update kernel is k_train_optim and not k_train_adamw: the other resource tests look kernels up
by substring and expect exactly one hit for "k_train_adam".)"""
import os

import pytest

from test_kernel_resources import HIPCC, _find, _resources

# VGPRs at the commit before the feature
BEFORE = {"k_train_finish": 54, "k_train_adam": 30}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_optimiser_kernels_use_no_scratch_and_leave_their_neighbours_alone(tmp_path):
    res = _resources("bz_train_ends.hip", tmp_path)
    for name, cap in (("k_train_gnorm", 32), ("k_train_optim", 48)):   # (a streaming pass: more than k_train_adam's 30 + the EMA's operands would be a sign of trouble)
        k = _find(res, name)
        assert k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0 and k["vgpr"] <= cap, (name, k)
    for name, vgpr in BEFORE.items():
        k = _find(res, name)                      # exactly one hit each: the new names do not shadow the old ones
        assert k["vgpr"] == vgpr and k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0, (name, k, vgpr)
