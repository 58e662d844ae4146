"""Register / spill budget of the Gumbel interior tree step, read from the compiler's own metadata like
tests/test_kernel_resources.py does for the other tree kernels: k_gfull_step on Reversi 8x8 keeps no VGPR or SGPR spill and no
scratch and stays within the 128 VGPRs tests/test_gumbel_resources.py holds k_gumbel_step to -- although it keeps a node's three
edge chunks and their per-edge terms in registers; k_gumbel_step and k_tree_step still meet theirs; and the new kernel's name
does not collide with what the other resource tests look up by substring."""
import os

import pytest

from test_kernel_resources import HIPCC, _find, _resources


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    return _resources("bz_mcts.hip", tmp_path_factory.mktemp("gfull_res"))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_gfull_step_has_no_spills_no_scratch_and_at_most_128_vgprs_on_reversi8(res):
    k = _find(res, "k_gfull_step", "ReversiTILi8")
    assert k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0 and k["vgpr"] <= 128, k
    for game in ("ReversiTILi6", "ReversiTILi4", "TicTacToe"):  # (no local array in scratch on any game)
        k = _find(res, "k_gfull_step", game)
        assert k["vspill"] == 0 and k["scratch"] == 0, (game, k)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_gumbel_step_and_tree_step_still_meet_their_budgets(res):
    k = _find(res, "k_gumbel_step", "ReversiTILi8")
    assert k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0 and k["vgpr"] <= 128, k
    k = _find(res, "k_tree_step", "ReversiTILi8")
    assert k["vgpr"] <= 96 and k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0, k


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_the_names_the_other_resource_tests_search_for_still_match_one_kernel_each(res):
    for game in ("TicTacToe", "ReversiTILi8", "ReversiTILi6", "ReversiTILi4"):
        for name in ("k_tree_step", "k_leaf_step", "k_play", "k_cap_step", "k_forced_step", "k_forced_cap_step", "k_gumbel_step", "k_gfull_step",
                     "k_fpu_step", "k_fpu_cap_step", "k_fpu_forced_step", "k_fpu_forced_cap_step", "k_gumbel_play", "k_gumbel_root",
                     "k_root_policy"):
            _find(res, name, game)  # (asserts exactly one hit)
