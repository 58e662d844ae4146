"""Register / spill budget of the policy surprise weighting kernels, read from the compiler's own metadata as
tests/test_kernel_resources.py does (hipcc -S cross-compiles for gfx950 without a GPU).  The feature observes: its kernels are
launched around the search and play kernels, whose code -- and so whose registers -- must be what it was before the feature
existed; the values pinned below were read from the commit before it.  The new kernels are small one-lane-per-game (or
per-row) kernels and must not touch scratch memory."""
import os

import pytest

from test_kernel_resources import HIPCC, _find, _resources

GAMES = ("ReversiTILi8", "ReversiTILi6", "ReversiTILi4", "TicTacToe")
# VGPRs of the kernels the feature is launched next to, at the commit before it (Reversi 8 / 6 / 4, tic-tac-toe).
# (Since fsqrt became the correctly rounded __builtin_sqrtf, DESIGN.md 3.4, the corrected sequence's residual takes one more
# register where a square root sits at the kernel's peak: k_tree_step of tic-tac-toe 104 -> 105, 4 waves per SIMD as before;
# k_forced_play 96 -> 97, 4 waves instead of 5 for a kernel that runs once per move.  The surprise kernels change neither.)
BEFORE = {
    "k_tree_step": (96, 96, 96, 105),
    "k_playI": (64, 64, 55, 52),
    "k_cap_play": (63, 63, 55, 52),
    "k_forced_playI": (97, 97, 97, 97),
    "k_gumbel_play": (65, 65, 61, 61),
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_surprise_kernels_use_no_scratch_and_leave_the_other_kernels_registers_alone(tmp_path):
    res = _resources("bz_mcts.hip", tmp_path)
    for name in ("k_surp_save", "k_surp_kl"):
        for game in GAMES:
            k = _find(res, name, game)
            assert k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0 and k["vgpr"] <= 32, (name, game, k)
    for name in ("k_surp_note", "k_pack_kl"):
        k = _find(res, name)
        assert k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0 and k["vgpr"] <= 32, (name, k)
    for name, want in BEFORE.items():
        for game, vgpr in zip(GAMES, want):
            k = _find(res, name, game)
            assert k["vgpr"] == vgpr and k["vspill"] == 0 and k["scratch"] == 0, (name, game, k, vgpr)
    noise = _find(res, "k_root_noise")
    assert noise["vgpr"] == 100 and noise["vspill"] == 0 and noise["sspill"] == 0 and noise["scratch"] == 0, noise
    # the names the other resource tests search by substring still match one kernel each
    for name in ("k_tree_step", "k_cap_step", "k_play", "k_cap_play", "k_leaf_step", "k_gumbel_step", "k_root_policy",
                 "k_forced_step", "k_forced_cap_step", "k_forced_play", "k_forced_cap_play", "k_forced_root_policy"):
        _find(res, name, "ReversiTILi8")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_resampler_kernels_use_no_scratch(tmp_path):
    res = _resources("bz_surprise.hip", tmp_path)
    for name in ("k_surp_sum", "k_surp_count", "k_surp_scan", "k_surp_emit"):
        k = _find(res, name)
        assert k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0 and k["vgpr"] <= 64, (name, k)
