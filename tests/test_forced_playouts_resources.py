"""Register / spill budget of the forced-playout kernels, read from the compiler's own metadata as
tests/test_kernel_resources.py does (hipcc -S cross-compiles for gfx950 without a GPU).  k_forced_step / k_forced_cap_step are
k_tree_step's / k_cap_step's bodies with three multiplications, a square root and a comparison per root edge: they must keep
that kernel's occupancy class; the one-lane-per-game kernels (the pruning loop runs in them) must not fall back to scratch
memory.  (The play kernels hold EngineDev, the pruning's scalars and the play tail's at once and park a few SGPRs in VGPR
lanes -- 2 to 32, which is not memory: what is pinned for them is no VGPR spill and no scratch.)"""
import os

import pytest

from test_kernel_resources import HIPCC, _find, _resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_forced_kernels_stay_within_their_register_budget(tmp_path):
    res = _resources("bz_mcts.hip", tmp_path)
    for name in ("k_forced_step", "k_forced_cap_step"):
        step = _find(res, name, "ReversiTILi8")
        assert step["vgpr"] <= 128 and step["vspill"] == 0 and step["sspill"] == 0 and step["scratch"] == 0, (name, step)
    for name in ("k_forced_play", "k_forced_cap_play", "k_forced_root_policy"):
        for game in ("ReversiTILi8", "ReversiTILi6", "ReversiTILi4", "TicTacToe"):
            k = _find(res, name, game)
            assert k["vspill"] == 0 and k["scratch"] == 0, (name, game, k)
            assert k["sspill"] == 0 or name != "k_forced_root_policy", (name, game, k)
    # the names the other resource tests search by substring still match one kernel each
    for name in ("k_tree_step", "k_cap_step", "k_play", "k_cap_play", "k_leaf_step", "k_gumbel_step", "k_root_policy"):
        _find(res, name, "ReversiTILi8")
