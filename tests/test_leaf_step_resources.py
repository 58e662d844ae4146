"""Register / spill budget of the leaf-parallel tree step, read from the compiler's own metadata like
tests/test_kernel_resources.py does for the other tree kernels: k_leaf_step keeps no VGPR or SGPR spill and no scratch
for any game, and stays within 128 VGPRs (4 waves per SIMD)."""
import os

import pytest

from test_kernel_resources import HIPCC, _find, _resources


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_leaf_step_has_no_spills_and_no_scratch(tmp_path):
    res = _resources("bz_mcts.hip", tmp_path)
    for game in ("TicTacToe", "ReversiTILi8", "ReversiTILi6", "ReversiTILi4"):
        k = _find(res, "k_leaf_step", game)
        assert k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0 and k["vgpr"] <= 128, (game, k)
