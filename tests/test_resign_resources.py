"""Register / spill budget of the two resignation kernels, read from the compiler's own metadata like
tests/test_solver_resources.py does for the solver's steps: k_resign_note and k_resign_finish -- one lane per game around the play
kernel -- keep no VGPR or SGPR spill and no scratch and stay within 64 VGPRs on the four games.  And their names do not collide with
what the other resource tests look up by substring."""
import os

import pytest

from test_kernel_resources import HIPCC, _find, _resources
from test_solver_resources import OTHERS, SOLVER_KERNELS

RESIGN_KERNELS = ("k_resign_note", "k_resign_finish")
GAMES = ("TicTacToe", "ReversiTILi8", "ReversiTILi6", "ReversiTILi4")


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    return _resources("bz_mcts.hip", tmp_path_factory.mktemp("resign_res"))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_resign_kernels_have_no_spills_no_scratch_and_at_most_64_vgprs(res):
    for name in RESIGN_KERNELS:
        for game in GAMES:
            k = _find(res, name, game)
            print(name, game, k)
            assert k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0 and k["vgpr"] <= 64, (name, game, k)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_the_names_the_other_resource_tests_search_for_still_match_one_kernel_each(res):
    for game in GAMES:
        for name in OTHERS + SOLVER_KERNELS + ("k_solve_play", "k_solve_cap_play", "k_solve_read") + RESIGN_KERNELS:
            _find(res, name, game)  # (asserts exactly one hit)
    for gw in ("ILi2E", "ILi4E"):
        for uni in ("Lb1E", "Lb0E"):
            _find(res, "k_search_fused_ttt", gw + uni)
