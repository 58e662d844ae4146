"""Register / spill budget of the search-value target kernels, read from the compiler's own metadata as
tests/test_kernel_resources.py does (hipcc -S cross-compiles for gfx950 without a GPU).  The feature observes the engine and
adds a second head kernel next to the first: the kernels it is launched next to, and k_train_heads itself -- whose body became
a template shared with k_train_heads_vt -- must compile to what they were before the feature existed; the values pinned below
were read from the commit before it."""
import os

import pytest

from test_kernel_resources import HIPCC, _find, _resources
from test_surprise_resources import BEFORE, GAMES

# VGPRs of k_train_heads<64> / <128> at the commit before the feature
HEADS_BEFORE = {"ILi64E": 148, "ILi128E": 234}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_engine_value_kernels_use_no_scratch_and_leave_the_other_kernels_registers_alone(tmp_path):
    res = _resources("bz_mcts.hip", tmp_path)
    for name in ("k_root_q", "k_pack_q", "k_surp_note", "k_pack_kl"):  # (k_surp_note shares the row rule with k_root_q)
        k = _find(res, name)
        assert k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0 and k["vgpr"] <= 32, (name, k)
    for name in ("k_surp_save", "k_surp_kl"):
        for game in GAMES:
            k = _find(res, name, game)
            assert k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0 and k["vgpr"] <= 32, (name, game, k)
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
    for gw in ("ILi2E", "ILi4E"):
        for uni in ("Lb1E", "Lb0E"):
            _find(res, "k_search_fused_ttt", gw + uni)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_value_target_kernels_use_no_scratch(tmp_path):
    res = _resources("bz_value.hip", tmp_path)
    for name in ("k_value_init", "k_value_tails"):
        k = _find(res, name)
        assert k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0 and k["vgpr"] <= 64, (name, k)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
def test_the_head_kernels_keep_their_registers_and_the_vt_kernel_needs_no_more(tmp_path):
    res = _resources("bz_train_ends.hip", tmp_path)
    for c, vgpr in HEADS_BEFORE.items():
        z = _find(res, "k_train_heads" + c)       # (the lookup of tests/test_kernel_resources.py: exactly one hit)
        vt = _find(res, "k_train_heads_vt" + c)
        assert z["vgpr"] == vgpr and z["vspill"] == 0 and z["sspill"] == 0 and z["scratch"] == 0, (c, z)
        assert vt["vgpr"] <= vgpr and vt["vspill"] == 0 and vt["sspill"] == 0 and vt["scratch"] == 0, (c, vt)
    for parts in (("k_train_stemILi64E",), ("k_train_stemILi128E",), ("k_train_stem_wgradILi64E",), ("k_train_stem_wgradILi128E",),
                  ("k_train_heads_wgrad",), ("k_train_finish",), ("k_train_adam",)):
        k = _find(res, *parts)
        assert k["vspill"] == 0 and k["sspill"] == 0 and k["scratch"] == 0, (parts, k)
