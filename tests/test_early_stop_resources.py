"""Register / spill budget of the early-stop tree steps, read from the compiler's own metadata like
tests/test_solver_resources.py does for the solver's steps: k_stop_step and k_fpu_stop_step keep no VGPR or SGPR spill and no
scratch on Reversi 8x8 and tic-tac-toe and stay within 128 VGPRs, the budget of the other mode steps; the plain k_tree_step stays
within its 96.  And the new kernels' names do not collide with what the other resource tests look up by substring."""
import os

import pytest

from test_kernel_resources import HIPCC, _find, _resources

STOP_KERNELS = ("k_stop_step", "k_fpu_stop_step")
OTHERS = ("k_tree_step", "k_leaf_step", "k_play", "k_cap_step", "k_forced_step", "k_forced_cap_step", "k_gumbel_step", "k_fpu_step",
          "k_fpu_cap_step", "k_fpu_forced_step", "k_fpu_forced_cap_step", "k_cap_play", "k_root_policy", "k_gfull_step",
          "k_solve_step", "k_solve_cap_step", "k_solve_play", "k_solve_cap_play", "k_solve_read")


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    return _resources("bz_mcts.hip", tmp_path_factory.mktemp("early_stop_res"))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_stop_steps_have_no_spills_no_scratch_and_at_most_128_vgprs(res):
    for name in STOP_KERNELS:
        for game in ("ReversiTILi8", "TicTacToe"):
            k = _find(res, name, game)
            print(name, game, k)
            assert k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0 and k["vgpr"] <= 128, (name, game, k)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_the_plain_tree_step_stays_within_96_vgprs(res):
    k = _find(res, "k_tree_step", "ReversiTILi8")
    print(k)
    assert k["vgpr"] <= 96 and k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0, k


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_the_names_the_other_resource_tests_search_for_still_match_one_kernel_each(res):
    for game in ("TicTacToe", "ReversiTILi8", "ReversiTILi6", "ReversiTILi4"):
        for name in OTHERS + STOP_KERNELS:
            _find(res, name, game)  # (asserts exactly one hit)
    for gw in ("ILi2E", "ILi4E"):
        for uni in ("Lb1E", "Lb0E"):
            _find(res, "k_search_fused_ttt", gw + uni)
    assert len([k for k in res if "k_stop_begin" in k]) == 1
