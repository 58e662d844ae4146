"""Register / spill budget of the replay seed's kernels, read from the compiler's own metadata as
tests/test_early_stop_resources.py does: k_pace_step and k_replay_seed keep no VGPR or SGPR spill and no scratch; the paced step
stays within the plain step's 96 VGPRs on the Reversi boards; and the mode bit left every existing step kernel the registers it
had before it (the counts of the tree without the paced mode, on Reversi 8x8).  The new names collide with none the other
resource tests look up by substring."""
import os

import pytest

from test_kernel_resources import HIPCC, _find, _resources

# VGPRs on Reversi 8x8 before the paced mode existed
BEFORE = {"k_tree_step": 96, "k_leaf_step": 105, "k_gumbel_step": 110, "k_gfull_step": 126, "k_cap_step": 96, "k_forced_step": 96,
          "k_forced_cap_step": 96, "k_fpu_step": 96, "k_fpu_cap_step": 96, "k_fpu_forced_step": 96, "k_fpu_forced_cap_step": 96,
          "k_solve_step": 96, "k_solve_cap_step": 96, "k_stop_step": 96, "k_fpu_stop_step": 96}


@pytest.fixture(scope="module")
def res(tmp_path_factory):
    return _resources("bz_mcts.hip", tmp_path_factory.mktemp("replay_seed_res"))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_the_new_kernels_have_no_spills_and_no_scratch(res):
    for game in ("ReversiTILi8", "ReversiTILi6", "ReversiTILi4"):
        for name, cap in (("k_pace_step", 96), ("k_replay_seed", 64)):
            k = _find(res, name, game)
            print(name, game, k)
            assert k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0 and k["vgpr"] <= cap, (name, game, k)
    k = _find(res, "k_pace_step", "TicTacToe")  # (instantiated with the other steps; never launched: no net serves tic-tac-toe)
    assert k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0 and k["vgpr"] <= 128, k
    assert not [n for n in res if "k_replay_seed" in n and "TicTacToe" in n]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_the_existing_step_kernels_keep_their_registers(res):
    for name, vgpr in BEFORE.items():
        k = _find(res, name, "ReversiTILi8")
        print(name, k)
        assert k["vgpr"] == vgpr and k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0, (name, k)
