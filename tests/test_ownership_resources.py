"""Register / spill budget of the ownership target kernels, read from the compiler's own metadata as
tests/test_kernel_resources.py does (hipcc -S cross-compiles for gfx950 without a GPU).  The feature observes the engine: the
kernels it is launched next to must compile to what they were before the feature existed (the values pinned in
tests/test_surprise_resources.py), and its own small one-lane-per-game (or per-row) kernels must not touch scratch memory."""
import os

import pytest

from test_kernel_resources import HIPCC, _find, _resources
from test_surprise_resources import BEFORE, GAMES

# VGPRs of the two kernels bz_engine_play now also launches in front of its play kernel, at the commit before the feature
# (Reversi 8 / 6 / 4, tic-tac-toe)
POLICY_BEFORE = {
    "k_root_policy": (33, 33, 33, 33),
    "k_forced_root_policy": (64, 64, 64, 64),
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_ownership_kernels_use_no_scratch_and_leave_the_other_kernels_registers_alone(tmp_path):
    res = _resources("bz_mcts.hip", tmp_path)
    for game in GAMES:
        k = _find(res, "k_own_final", game)
        assert k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0 and k["vgpr"] <= 64, (game, k)
    k = _find(res, "k_pack_own")
    assert k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0 and k["vgpr"] <= 32, k
    for name, want in list(BEFORE.items()) + list(POLICY_BEFORE.items()):
        for game, vgpr in zip(GAMES, want):
            k = _find(res, name, game)
            assert k["vgpr"] == vgpr and k["vspill"] == 0 and k["scratch"] == 0, (name, game, k, vgpr)
    # the names the other resource tests search by substring still match one kernel each
    for name in ("k_tree_step", "k_cap_step", "k_play", "k_cap_play", "k_leaf_step", "k_gumbel_step", "k_root_policy",
                 "k_forced_step", "k_forced_cap_step", "k_forced_play", "k_forced_cap_play", "k_forced_root_policy"):
        _find(res, name, "ReversiTILi8")
    for name in ("k_root_q", "k_pack_q", "k_surp_note", "k_pack_kl"):
        _find(res, name)


# VGPRs of k_train_heads<64> / <128> (and of their _vt forms) at the commit before the feature
HEADS_BEFORE = {"ILi64E": 148, "ILi128E": 234}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_the_head_kernels_keep_their_registers_and_the_own_kernels_need_no_scratch(tmp_path):
    """train_heads_body gained a template flag; k_train_heads / k_train_heads_vt must compile to what they were,
    and the new instances -- a fourth plane in flight at 234 VGPRs under __launch_bounds__(256) -- must neither spill nor touch
    scratch memory (256 threads a workgroup: a wave may hold up to 512 registers)"""
    res = _resources("bz_train_ends.hip", tmp_path)
    for c, vgpr in HEADS_BEFORE.items():
        z = _find(res, "k_train_heads" + c)       # (the lookup of tests/test_kernel_resources.py: exactly one hit)
        vt = _find(res, "k_train_heads_vt" + c)
        assert z["vgpr"] == vgpr and z["vspill"] == 0 and z["sspill"] == 0 and z["scratch"] == 0, (c, z)
        assert vt["vgpr"] <= vgpr and vt["vspill"] == 0 and vt["sspill"] == 0 and vt["scratch"] == 0, (c, vt)
        for name in ("k_train_heads_own", "k_train_heads_own_vt"):
            k = _find(res, name + c)
            assert k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0 and k["vgpr"] <= 256, (name, c, k)
    k = _find(res, "k_train_own_finish")
    assert k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0 and k["vgpr"] <= 64, k
    for parts in (("k_train_stemILi64E",), ("k_train_stemILi128E",), ("k_train_stem_wgradILi64E",), ("k_train_stem_wgradILi128E",),
                  ("k_train_heads_wgrad",), ("k_train_finish",), ("k_train_adam",), ("k_train_gnorm",), ("k_train_optim",)):
        k = _find(res, *parts)
        assert k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0, (parts, k)
