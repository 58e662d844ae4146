"""The checker behind tests/test_kernel_resources.py, on hand-written metadata (no compile): a table is only worth its rows if a
row that does not hold, or that names no kernel or two, is reported."""
import pytest

import kernel_meta
from kernel_meta import check, find, row, split_symbol

OK = {"vgpr": 96, "agpr": 0, "vspill": 0, "sspill": 0, "scratch": 0, "lds_static": 0, "max_wg": 1024}
R8 = "_ZN12_GLOBAL__N_111k_tree_stepIN2bz8ReversiTILi8EEEEEvNS_9EngineDevE"
R6 = "_ZN12_GLOBAL__N_111k_tree_stepIN2bz8ReversiTILi6EEEEEvNS_9EngineDevE"
KERNELS = {
    R8: dict(OK),
    R6: dict(OK, scratch=16),
    "_ZN12_GLOBAL__N_110k_cap_playIN2bz8ReversiTILi8EEEEEvNS_9EngineDevE": dict(OK, sspill=4),
    "_ZN12_GLOBAL__N_112k_root_noiseENS_9EngineDevE": dict(OK, vgpr=100),
    "_ZN12_GLOBAL__N_112k_tower_bf16IN8bz_tower2TwILi128ELi4ELb1ELi0EEEEEvNS_9TowerArgsE": dict(OK, vgpr=354, agpr=190),
}
Z3 = ("vspill", "sspill", "scratch")


def test_rows_that_hold_report_nothing():
    for r in (row("k_tree_step", "ReversiTILi8", vgpr=("==", 96), zero=Z3), row("k_tree_step", "ReversiTILi8", vgpr=("<=", 96), zero=Z3),
              row("k_root_noise", vgpr=("==", 100), zero=Z3), row("k_cap_play", "ReversiTILi8", zero=("vspill", "scratch")),
              row("k_tower_bf16", "Li128ELi4ELb1E", vgpr=("==", 354), agpr=("<=", 190), zero=Z3)):
        assert check(KERNELS, r) == [], r


def test_an_exact_row_off_by_one_register_is_reported():
    for n in (95, 97):
        bad = check(KERNELS, row("k_tree_step", "ReversiTILi8", vgpr=("==", n), zero=Z3))
        assert len(bad) == 1 and "vgpr is 96" in bad[0] and f"== {n}" in bad[0], bad
    bad = check(KERNELS, row("k_tower_bf16", "Li128ELi4ELb1E", vgpr=("==", 354), agpr=("==", 189)))
    assert len(bad) == 1 and "agpr is 190" in bad[0], bad


def test_a_bounded_row_one_over_its_bound_is_reported():
    bad = check(KERNELS, row("k_tree_step", "ReversiTILi8", vgpr=("<=", 95), zero=Z3))
    assert len(bad) == 1 and "vgpr is 96" in bad[0] and "<= 95" in bad[0], bad
    bad = check(KERNELS, row("k_tower_bf16", "Li128ELi4ELb1E", agpr=("<=", 189)))
    assert len(bad) == 1 and "agpr is 190" in bad[0], bad


def test_a_non_zero_field_is_reported_only_where_the_row_names_it():
    bad = check(KERNELS, row("k_tree_step", "ReversiTILi6", vgpr=("==", 96), zero=Z3))
    assert len(bad) == 1 and "scratch is 16" in bad[0], bad
    bad = check(KERNELS, row("k_cap_play", "ReversiTILi8", zero=Z3))
    assert len(bad) == 1 and "sspill is 4" in bad[0], bad


def test_a_row_without_a_kernel_is_reported():
    for r in (row("k_tree_step", "TicTacToe", zero=Z3), row("k_leaf_step", "ReversiTILi8", zero=Z3), row("k_tree", "ReversiTILi8")):
        bad = check(KERNELS, r)
        assert len(bad) == 1 and "0 kernels match" in bad[0], (r, bad)


def test_a_row_that_fits_two_kernels_is_reported():
    for r in (row("k_tree_step", vgpr=("<=", 96)), row("k_tree_step", "ReversiT", zero=Z3)):
        bad = check(KERNELS, r)
        assert len(bad) == 1 and "2 kernels match" in bad[0] and R8 in bad[0] and R6 in bad[0], (r, bad)
    with pytest.raises(AssertionError):
        find(KERNELS, "k_tree_step")


def test_find_is_by_exact_name_and_by_template_arguments_only():
    kernels = {"_ZN12_GLOBAL__N_110k_cap_playIN2bz9TicTacToeEEEvNS_9EngineDevE": OK}
    assert kernel_meta.matches(kernels, "k_play") == []
    with pytest.raises(AssertionError):
        find(kernels, "k_play")
    kernels["_ZN12_GLOBAL__N_16k_playIN2bz9TicTacToeEEEvNS_9EngineDevE"] = OK
    assert find(kernels, "k_play") == "_ZN12_GLOBAL__N_16k_playIN2bz9TicTacToeEEEvNS_9EngineDevE"
    adam = {"_ZN12_GLOBAL__N_112k_train_adamENS_8AdamArgsE": OK, "_ZN12_GLOBAL__N_113k_train_adamwENS_8AdamArgsE": OK}
    assert find(adam, "k_train_adam") == "_ZN12_GLOBAL__N_112k_train_adamENS_8AdamArgsE"
    assert kernel_meta.matches(KERNELS, "k_tree_step", "EngineDev") == []      # a parameter type is no template argument
    assert kernel_meta.matches(KERNELS, "k_root_noise", "EngineDev") == []


def test_split_symbol():
    assert split_symbol(R8) == ("k_tree_step", "IN2bz8ReversiTILi8EEEE")
    assert split_symbol("_ZN12_GLOBAL__N_12f811k_tower_fp8ENS_9TowerArgsE") == ("k_tower_fp8", "")
    assert split_symbol("_ZN12_GLOBAL__N_118k_search_fused_tttILi4ELb1EEEvNS_9EngineDevE") == ("k_search_fused_ttt", "ILi4ELb1EE")
    assert split_symbol("_ZN12_GLOBAL__N_113k_train_wgradILi128EEEvNS_9WgradArgsE") == ("k_train_wgrad", "ILi128EE")
    assert split_symbol("_ZN12_GLOBAL__N_111k_sym_headsIfEEvPKT_iPKjiiPKfS7_PfS8_PKmSA_N6bz_sym4ArgsE") == ("k_sym_heads", "IfE")
    assert split_symbol("_Z6k_playI9TicTacToeEvPfi") == ("k_play", "I9TicTacToeE")
    assert split_symbol("_Z6k_playPfi") == ("k_play", "")
    assert split_symbol("k_plain_c_name") == ("k_plain_c_name", "")
