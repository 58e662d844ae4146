"""Register / spill budget of the first-play urgency tree steps, read from the compiler's own metadata like
tests/test_kernel_resources.py does for the other tree kernels: k_fpu_step, k_fpu_cap_step, k_fpu_forced_step and
k_fpu_forced_cap_step keep no VGPR or SGPR spill and no scratch on Reversi 8x8 and tic-tac-toe and stay within the 128 VGPRs
tests/test_leaf_step_resources.py holds k_leaf_step to -- although they keep a node's three edge chunks in registers.  And
the new kernels' names do not collide with what the other resource tests look up by substring."""
import os

import pytest

from test_kernel_resources import HIPCC, _find, _resources

FPU_KERNELS = ("k_fpu_step", "k_fpu_cap_step", "k_fpu_forced_step", "k_fpu_forced_cap_step")


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    return _resources("bz_mcts.hip", tmp_path_factory.mktemp("fpu_res"))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_fpu_steps_have_no_spills_no_scratch_and_at_most_128_vgprs(res):
    for name in FPU_KERNELS:
        for game in ("ReversiTILi8", "TicTacToe"):
            k = _find(res, name, game)
            assert k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0 and k["vgpr"] <= 128, (name, game, k)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_the_names_the_other_resource_tests_search_for_still_match_one_kernel_each(res):
    for game in ("TicTacToe", "ReversiTILi8", "ReversiTILi6", "ReversiTILi4"):
        for name in ("k_tree_step", "k_leaf_step", "k_play", "k_cap_step", "k_forced_step", "k_forced_cap_step", "k_gumbel_step") + FPU_KERNELS:
            _find(res, name, game)  # (asserts exactly one hit)
    for gw in ("ILi2E", "ILi4E"):
        for uni in ("Lb1E", "Lb0E"):
            _find(res, "k_search_fused_ttt", gw + uni)
