"""Register / spill budget of the Gumbel kernels, read from the compiler's own metadata like
tests/test_kernel_resources.py does for the other tree kernels: k_gumbel_step (Reversi 8x8) keeps no VGPR or SGPR spill and
no scratch and stays within 128 VGPRs; k_gumbel_play and k_root_policy keep no spill and no scratch."""
import os

import pytest

from test_kernel_resources import HIPCC, _find, _resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_gumbel_kernels_have_no_spills_and_no_scratch(tmp_path):
    res = _resources("bz_mcts.hip", tmp_path)
    step = _find(res, "k_gumbel_step", "ReversiTILi8")
    assert step["vspill"] == 0 and step["sspill"] == 0 and step["scratch"] == 0 and step["vgpr"] <= 128, step
    for game in ("TicTacToe", "ReversiTILi8", "ReversiTILi6", "ReversiTILi4"):
        for name in ("k_gumbel_play", "k_root_policy", "k_gumbel_root"):
            k = _find(res, name, game)
            assert k["vspill"] == 0 and k["scratch"] == 0, (name, game, k)
    # the shared body leaves the PUCT tree step's budget where it was (tests/test_kernel_resources.py pins it too)
    assert _find(res, "k_tree_step", "ReversiTILi8")["vgpr"] <= 96
