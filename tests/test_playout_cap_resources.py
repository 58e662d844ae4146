"""Register / spill budget of the playout-cap kernels, read from the compiler's own metadata as
tests/test_kernel_resources.py does (hipcc -S cross-compiles for gfx950 without a GPU).  k_cap_step is k_tree_step's body with
one more load and one more comparison: it must keep that kernel's occupancy class; the one-lane-per-game kernels must not
fall back to scratch memory (k_cap_play chooses a fast search's move without a pi row to write to)."""
import os

import pytest

from test_kernel_resources import HIPCC, _find, _resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_cap_kernels_stay_within_their_register_budget(tmp_path):
    res = _resources("bz_mcts.hip", tmp_path)
    step = _find(res, "k_cap_step", "ReversiTILi8")
    assert step["vgpr"] <= 128 and step["vspill"] == 0 and step["sspill"] == 0 and step["scratch"] == 0, step
    for name, parts in (("k_cap_play", ("ReversiTILi8",)), ("k_cap_play", ("TicTacToe",)), ("k_cap_budget", ()), ("k_cap_noise", ())):
        k = _find(res, name, *parts)
        assert k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0, (name, parts, k)
    # the names the other resource tests search by substring still match one kernel each
    for name in ("k_tree_step", "k_play", "k_leaf_step", "k_root_policy"):
        _find(res, name, "ReversiTILi8")
