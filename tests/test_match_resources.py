"""Register / spill budget of the match driver's kernels, read from the compiler's own metadata like
tests/test_kernel_resources.py does for the tree kernels: k_match_ply and k_match_begin keep no VGPR or SGPR spill and no
scratch for every game.  The VGPR budgets are what the compiler reported when the kernel was first built (57 for the
Reversi boards, 38 for tic-tac-toe): one lane per game and about 60 bytes per game per ply, so occupancy is not the point --
the budget is there to notice a rule function that stops inlining or a per-lane array that lands in scratch."""
import os

import pytest

from test_kernel_resources import HIPCC, _find, _resources

BUDGET = {"TicTacToe": 38, "ReversiTILi8": 57, "ReversiTILi6": 57, "ReversiTILi4": 57}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_match_kernels_have_no_spills_and_no_scratch(tmp_path):
    res = _resources("bz_match.hip", tmp_path)
    for game, cap in BUDGET.items():
        ply = _find(res, "k_match_ply", game)
        assert ply["vspill"] == 0 and ply["sspill"] == 0 and ply["scratch"] == 0 and ply["vgpr"] <= cap, (game, ply)
        begin = _find(res, "k_match_begin", game)
        assert begin["vspill"] == 0 and begin["sspill"] == 0 and begin["scratch"] == 0, (game, begin)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_match_kernel_names_hit_none_of_the_tree_kernels_name_searches(tmp_path):
    """the other resource tests find their kernels by substring and need exactly one hit"""
    res = _resources("bz_match.hip", tmp_path)
    for name in res:
        for part in ("k_play", "k_tree_step", "k_leaf_step", "k_gumbel_", "k_root_policy"):
            assert part not in name, (name, part)
