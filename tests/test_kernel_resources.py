"""Register / spill budget of the kernels, read from the compiler's own metadata (tests/kernel_meta.py: hipcc -S cross-compiles
for gfx950 without a GPU, each source once).  A feature that inlines into a tree kernel can silently double its registers --
round 2's Dirichlet sampler took k_tree_step from 78 to 129 VGPRs with SGPR spills until it got a kernel of its own -- so the
budgets are pinned here: ONE table, grouped by source file, one row per (kernel, instantiation).  A row states what the kernel is
held to -- its VGPRs exactly ("==", where a feature had to leave the kernel as it was) or at most ("<="), its AGPRs, and which
of vspill / sspill / scratch must be 0 -- and, in its comment, why.  Kernels are looked up by their exact name, so a new kernel
cannot shadow a row, and a row that matches no kernel or more than one fails.  What is no row -- instruction counts, LDS, the
number of instantiations -- follows the table as named tests on the same compiles."""
import os

import pytest

import kernel_meta
from kernel_meta import compile_asm, row

needs_hipcc = pytest.mark.skipif(not os.path.exists(kernel_meta.HIPCC), reason="needs hipcc")

Z3 = ("vspill", "sspill", "scratch")
Z2 = ("vspill", "scratch")   # the play kernels park a few SGPRs in VGPR lanes, which is not memory: sspill is left alone
R8, R6, R4, TTT = "ReversiTILi8", "ReversiTILi6", "ReversiTILi4", "TicTacToe"
GAMES = (R8, R6, R4, TTT)
REVERSI = (R8, R6, R4)


def per_game(name, values, zero):
    """rows holding a kernel to an exact VGPR count per game (Reversi 8 / 6 / 4, tic-tac-toe)"""
    return [row(name, g, vgpr=("==", v), zero=zero) for g, v in zip(GAMES, values)]


TABLE = {
    "bz_mcts.hip": [
        # -- the PUCT tree step: 96 VGPRs on Reversi is cfg 3's 4+ waves per SIMD; every later feature (surprise
        #    3.17, value targets 3.18, ownership 3.22, the paced mode 3.11) had to leave it as before the feature existed
        row("k_tree_step", R8, vgpr=("==", 96), zero=Z3),
        row("k_tree_step", R6, vgpr=("==", 96), zero=Z2),
        row("k_tree_step", R4, vgpr=("==", 96), zero=Z2),
        row("k_tree_step", TTT, vgpr=("==", 105), zero=Z2),   # 104 + the correctly rounded sqrt's residual (3.4); 4 waves per SIMD as before
        # -- cfg 2's fused tic-tac-toe search: 2 and 4 lanes per game (4 is the default), uniform / hash evaluator
        row("k_search_fused_ttt", "Li2ELb1E", vgpr=("<=", 128), zero=Z3),
        row("k_search_fused_ttt", "Li2ELb0E", vgpr=("<=", 128), zero=Z3),
        row("k_search_fused_ttt", "Li4ELb1E", vgpr=("<=", 128), zero=Z3),
        row("k_search_fused_ttt", "Li4ELb0E", vgpr=("<=", 128), zero=Z3),
        # -- the mode steps on Reversi 8x8: each keeps the registers it had before the paced mode's bit existed (3.11), which is
        #    within the 128 (4 waves per SIMD) its own feature set for it
        row("k_leaf_step", R8, vgpr=("==", 105), zero=Z3),             # leaf-parallel step, 3.12
        row("k_gumbel_step", R8, vgpr=("==", 110), zero=Z3),           # Gumbel root, 3.13
        row("k_gfull_step", R8, vgpr=("==", 126), zero=Z3),            # Gumbel interior, 3.21: three edge chunks and their terms in registers
        row("k_cap_step", R8, vgpr=("==", 96), zero=Z3),               # playout cap, 3.15: k_tree_step + one load, one comparison
        row("k_forced_step", R8, vgpr=("==", 96), zero=Z3),            # forced playouts, 3.16: + 3 mul, a sqrt, a comparison per root edge
        row("k_forced_cap_step", R8, vgpr=("==", 96), zero=Z3),        # 3.16
        row("k_fpu_step", R8, vgpr=("==", 96), zero=Z3),               # first-play urgency, 3.20
        row("k_fpu_cap_step", R8, vgpr=("==", 96), zero=Z3),           # 3.20
        row("k_fpu_forced_step", R8, vgpr=("==", 96), zero=Z3),        # 3.20
        row("k_fpu_forced_cap_step", R8, vgpr=("==", 96), zero=Z3),    # 3.20
        row("k_solve_step", R8, vgpr=("==", 96), zero=Z3),             # solver, 3.23: the proof pass behind the backup included
        row("k_solve_cap_step", R8, vgpr=("==", 96), zero=Z3),         # 3.23
        row("k_stop_step", R8, vgpr=("==", 96), zero=Z3),              # early stop, 3.25
        row("k_fpu_stop_step", R8, vgpr=("==", 96), zero=Z3),          # 3.25
        row("k_pace_step", R8, vgpr=("<=", 96), zero=Z3),              # paced step, 3.11: within the plain step's 96 on the Reversi boards
        row("k_pace_step", R6, vgpr=("<=", 96), zero=Z3),
        row("k_pace_step", R4, vgpr=("<=", 96), zero=Z3),
        # -- the mode steps on the other games: 128 VGPRs is 4 waves per SIMD
        row("k_leaf_step", R6, vgpr=("<=", 128), zero=Z3),
        row("k_leaf_step", R4, vgpr=("<=", 128), zero=Z3),
        row("k_leaf_step", TTT, vgpr=("<=", 128), zero=Z3),
        row("k_gfull_step", R6, zero=Z2),                              # no local array in scratch on any game; tic-tac-toe parks 2 SGPRs (3.21)
        row("k_gfull_step", R4, zero=Z2),
        row("k_gfull_step", TTT, zero=Z2),
        row("k_fpu_step", TTT, vgpr=("<=", 128), zero=Z3),
        row("k_fpu_cap_step", TTT, vgpr=("<=", 128), zero=Z3),
        row("k_fpu_forced_step", TTT, vgpr=("<=", 128), zero=Z3),
        row("k_fpu_forced_cap_step", TTT, vgpr=("<=", 128), zero=Z3),
        row("k_solve_step", TTT, vgpr=("<=", 128), zero=Z3),
        row("k_solve_cap_step", TTT, vgpr=("<=", 128), zero=Z3),
        row("k_stop_step", TTT, vgpr=("<=", 128), zero=Z3),
        row("k_fpu_stop_step", TTT, vgpr=("<=", 128), zero=Z3),
        row("k_pace_step", TTT, vgpr=("<=", 128), zero=Z3),            # instantiated with the other steps, never launched: no net serves tic-tac-toe
        # -- the one-lane-per-game play and root kernels: as before the observing features existed (3.17, 3.18, 3.22); no VGPR
        #    spill and no scratch (they hold EngineDev and the play tail's scalars at once and may park SGPRs in VGPR lanes)
        *per_game("k_play", (64, 64, 55, 52), Z2),
        row("k_cap_play", R8, vgpr=("==", 63), zero=Z3),               # 3.15: chooses a fast search's move without a pi row to write to
        row("k_cap_play", R6, vgpr=("==", 63), zero=Z2),
        row("k_cap_play", R4, vgpr=("==", 55), zero=Z2),
        row("k_cap_play", TTT, vgpr=("==", 52), zero=Z3),
        *per_game("k_forced_play", (97, 97, 97, 97), Z2),              # 96 + the sqrt's residual (3.4): 4 waves, for a kernel that runs once per move
        *[row("k_forced_cap_play", g, zero=Z2) for g in GAMES],        # 3.16: the pruning loop runs in it and must not fall back to scratch
        *per_game("k_gumbel_play", (65, 65, 61, 61), Z2),
        *per_game("k_root_policy", (33, 33, 33, 33), Z2),              # as before ownership (3.22) launched it in front of the play kernel
        *per_game("k_forced_root_policy", (64, 64, 64, 64), Z3),       # 3.16 and 3.22
        *[row("k_gumbel_root", g, zero=Z2) for g in GAMES],            # 3.13
        row("k_root_noise", vgpr=("==", 100), zero=Z3),                # the Dirichlet sampler's own kernel; as before 3.17 / 3.18
        # -- small kernels around the search: one lane per game or per row, nothing in scratch
        row("k_cap_budget", zero=Z3),                                  # 3.15
        row("k_cap_noise", zero=Z3),
        *[row("k_replay_seed", g, vgpr=("<=", 64), zero=Z3) for g in REVERSI],      # 3.11
        *[row("k_resign_note", g, vgpr=("<=", 64), zero=Z3) for g in GAMES],        # 3.24: around the play kernel
        *[row("k_resign_finish", g, vgpr=("<=", 64), zero=Z3) for g in GAMES],
        *[row("k_own_final", g, vgpr=("<=", 64), zero=Z3) for g in GAMES],          # 3.22
        row("k_pack_own", vgpr=("<=", 32), zero=Z3),
        *[row("k_surp_save", g, vgpr=("<=", 32), zero=Z3) for g in GAMES],          # 3.17
        *[row("k_surp_kl", g, vgpr=("<=", 32), zero=Z3) for g in GAMES],
        row("k_surp_note", vgpr=("<=", 32), zero=Z3),                  # shares the row rule with k_root_q
        row("k_root_q", vgpr=("<=", 32), zero=Z3),                     # 3.18
        row("k_pack_f32", vgpr=("<=", 32), zero=Z3),                   # 3.17's kl and 3.18's q into the packed block's row order
    ],
    "bz_net.hip": [
        # -- the bf16 towers: one workgroup per CU (<= 512); each plain tower keeps the count it had before the
        #    symmetric kernels (3.19) were compiled from the same text; the throughput shape Tw<128,4,true> and the latency
        #    shape Tw<128,1,false> keep the AGPRs they had before the adaptive gate sat in front of their first barrier
        row("k_tower_bf16", "Li128ELi4ELb1E", vgpr=("==", 354), agpr=("<=", 190), zero=Z3),
        row("k_tower_bf16", "Li64ELi8E", vgpr=("==", 320), zero=Z3),
        row("k_tower_bf16", "Li256ELi2E", vgpr=("==", 388), zero=Z3),
        row("k_tower_bf16", "Li128ELi1ELb0E", vgpr=("==", 176), agpr=("<=", 32), zero=Z3),
        row("k_tower_bf16", "Li64ELi2E", vgpr=("==", 148), zero=Z3),
        row("k_tower_bf16", "Li256ELi1E", vgpr=("==", 324), zero=Z3),
        row("k_tower_fp8", vgpr=("==", 256), zero=Z2),                 # two workgroups per CU; as before 3.19
        # -- their symmetric forms (3.19): the plain kernels' occupancy
        row("k_sym_bf16", "Li128ELi4ELb1E", vgpr=("<=", 380), agpr=("<=", 216), zero=Z3),   # as before the adaptive gate (5)
        row("k_sym_bf16", "Li64ELi8E", vgpr=("<=", 512), zero=Z3),
        row("k_sym_bf16", "Li256ELi2E", vgpr=("<=", 512), zero=Z3),
        row("k_sym_bf16", "Li128ELi1ELb0E", vgpr=("<=", 176), agpr=("<=", 32), zero=Z3),    # as before the adaptive gate (5)
        row("k_sym_bf16", "Li64ELi2E", vgpr=("<=", 512), zero=Z3),
        row("k_sym_bf16", "Li256ELi1E", vgpr=("<=", 512), zero=Z3),
        row("k_sym_fp8", vgpr=("<=", 256), zero=Z3),
        row("k_sym_mean", zero=Z3),
        row("k_sym_stem", zero=Z3),
        row("k_sym_heads", zero=Z3),
        # -- the throughput tower on the edge-aware cell tiling (5, csrc/bz_tile_map.h): one workgroup per CU
        row("k_edge_bf16", vgpr=("<=", 512), zero=Z3),
    ],
    "bz_train.hip": [
        # -- forward / backward-data keep the inference tower's budget (one workgroup per CU); the weight-gradient kernel keeps
        #    its staging registers in registers (an array of HIP's uint4 STRUCT had put them into scratch: 272 bytes per lane)
        row("k_train_fwd", "Li64ELi8E", vgpr=("<=", 512), zero=Z3),
        row("k_train_fwd", "Li128ELi4ELb1E", vgpr=("<=", 512), zero=Z3),
        row("k_train_fwd", "Li64ELi4E", vgpr=("<=", 512), zero=Z3),
        row("k_train_bwd", "Li64ELi8E", vgpr=("<=", 512), zero=Z3),
        row("k_train_bwd", "Li128ELi4ELb1E", vgpr=("<=", 512), zero=Z3),
        row("k_train_bwd", "Li64ELi4E", vgpr=("<=", 512), zero=Z3),
        row("k_train_wgrad", "Li64E", vgpr=("<=", 512), zero=Z3),
        row("k_train_wgrad", "Li128E", vgpr=("<=", 512), zero=Z3),
        # -- fp8 quantisation-aware training (12.3)
        row("k_qat_scales", vgpr=("<=", 512), zero=Z3),
        row("k_qat_pack", vgpr=("<=", 512), zero=Z3),
        row("k_qat_fwd", vgpr=("<=", 512), zero=Z3),
    ],
    "bz_train_ends.hip": [
        # -- the stem keeps its 8 x 18 weights, its weight gradient its 2 x 19 and the FC weight-gradient kernel its 49
        #    accumulators in registers
        row("k_train_stem", "Li64E", vgpr=("<=", 512), zero=Z3),
        row("k_train_stem", "Li128E", vgpr=("<=", 512), zero=Z3),
        row("k_train_stem_wgrad", "Li64E", vgpr=("<=", 512), zero=Z3),
        row("k_train_stem_wgrad", "Li128E", vgpr=("<=", 512), zero=Z3),
        row("k_train_heads_wgrad", vgpr=("<=", 512), zero=Z3),
        # -- the heads kernel holds a whole position's x tile in flight (64 registers at 128 channels); its body became a template
        #    shared with the _vt (3.18) and _own (12.2) forms and compiles to what it was before either
        row("k_train_heads", "Li64E", vgpr=("==", 148), zero=Z3),
        row("k_train_heads", "Li128E", vgpr=("==", 234), zero=Z3),
        row("k_train_heads_vt", "Li64E", vgpr=("<=", 148), zero=Z3),   # needs no more than the plain form
        row("k_train_heads_vt", "Li128E", vgpr=("<=", 234), zero=Z3),
        row("k_train_heads_own", "Li64E", vgpr=("<=", 256), zero=Z3),  # a fourth plane in flight under __launch_bounds__(256)
        row("k_train_heads_own", "Li128E", vgpr=("<=", 256), zero=Z3),
        row("k_train_heads_own_vt", "Li64E", vgpr=("<=", 256), zero=Z3),
        row("k_train_heads_own_vt", "Li128E", vgpr=("<=", 256), zero=Z3),
        row("k_train_own_finish", vgpr=("<=", 64), zero=Z3),           # 12.2
        # -- the extended optimiser (12.1) left its neighbours as they were; its own kernels stream their operands once
        row("k_train_finish", vgpr=("==", 54), zero=Z3),
        row("k_train_adam", vgpr=("==", 30), zero=Z3),
        row("k_train_gnorm", vgpr=("<=", 32), zero=Z3),
        row("k_train_optim", vgpr=("<=", 48), zero=Z3),                # more than k_train_adam's 30 + the EMA's operands would be a sign of trouble
        row("k_qat_stem", vgpr=("<=", 512), zero=Z3),                  # 12.3
    ],
    "bz_match.hip": [
        # -- the match driver (3.14): one lane per game, so occupancy is not the point -- the bounds, what the compiler reported
        #    when the kernel was first built, notice a rule function that stops inlining or a per-lane array that lands in scratch
        row("k_match_ply", R8, vgpr=("<=", 57), zero=Z3),
        row("k_match_ply", R6, vgpr=("<=", 57), zero=Z3),
        row("k_match_ply", R4, vgpr=("<=", 57), zero=Z3),
        row("k_match_ply", TTT, vgpr=("<=", 38), zero=Z3),
        *[row("k_match_begin", g, zero=Z3) for g in GAMES],
    ],
    "bz_merge.hip": [
        # -- position averaging (3.26)
        row("k_merge_zero", vgpr=("<=", 32), zero=Z3),
        row("k_merge_reduce", "Li9E", vgpr=("<=", 64), zero=Z3),
        row("k_merge_reduce", "Li65E", vgpr=("<=", 64), zero=Z3),
        row("k_merge_finish", "Li9E", vgpr=("<=", 64), zero=Z3),
        row("k_merge_finish", "Li65E", vgpr=("<=", 64), zero=Z3),
    ],
    "bz_surprise.hip": [
        # -- the surprise resampler (3.17)
        row("k_surp_sum", vgpr=("<=", 64), zero=Z3),
        row("k_surp_count", vgpr=("<=", 64), zero=Z3),
        row("k_surp_scan", vgpr=("<=", 64), zero=Z3),
        row("k_surp_emit", vgpr=("<=", 64), zero=Z3),
    ],
    "bz_value.hip": [
        # -- TD(lambda) value targets (3.18)
        row("k_value_init", vgpr=("<=", 64), zero=Z3),
        row("k_value_tails", vgpr=("<=", 64), zero=Z3),
    ],
}

VARIANTS = [("bz_net.hip", ("-DBZ_EXPERIMENT", "-DBZ_EXP_STAMPS", "-DBZ_EXP_STAMPS_TAPS")),
            ("bz_train.hip", ("-DBZ_EXPERIMENT", "-DBZ_EXP_STAMPS", "-DBZ_EXP_STAMPS_TAPS")),
            ("bz_mcts.hip", ("-DBZ_EXPERIMENT", "-DBZ_EXP_TREE_STAMPS", "-DBZ_EXP_TT_WEAK_HASH"))]


def _holds(src, r):
    bad = kernel_meta.check(compile_asm(src).kernels, r)
    assert not bad, "\n".join(bad)


@needs_hipcc
@pytest.mark.parametrize("r", TABLE["bz_mcts.hip"], ids=str)
def test_bz_mcts(r):
    _holds("bz_mcts.hip", r)


@needs_hipcc
@pytest.mark.parametrize("r", TABLE["bz_net.hip"], ids=str)
def test_bz_net(r):
    _holds("bz_net.hip", r)


@needs_hipcc
@pytest.mark.parametrize("r", TABLE["bz_train.hip"], ids=str)
def test_bz_train(r):
    _holds("bz_train.hip", r)


@needs_hipcc
@pytest.mark.parametrize("r", TABLE["bz_train_ends.hip"], ids=str)
def test_bz_train_ends(r):
    _holds("bz_train_ends.hip", r)


@needs_hipcc
@pytest.mark.parametrize("r", TABLE["bz_match.hip"], ids=str)
def test_bz_match(r):
    _holds("bz_match.hip", r)


@needs_hipcc
@pytest.mark.parametrize("r", TABLE["bz_merge.hip"], ids=str)
def test_bz_merge(r):
    _holds("bz_merge.hip", r)


@needs_hipcc
@pytest.mark.parametrize("r", TABLE["bz_surprise.hip"], ids=str)
def test_bz_surprise(r):
    _holds("bz_surprise.hip", r)


@needs_hipcc
@pytest.mark.parametrize("r", TABLE["bz_value.hip"], ids=str)
def test_bz_value(r):
    _holds("bz_value.hip", r)


def test_no_row_is_stated_twice():
    for src, rows in TABLE.items():
        ids = [str(r) for r in rows]
        assert len(ids) == len(set(ids)), (src, sorted(i for i in ids if ids.count(i) > 1))


@needs_hipcc
def test_the_bf16_tower_family_has_twelve_members():
    """six geometries x (plain, symmetric): the adaptive gate added no kernel and no instantiation"""
    k = compile_asm("bz_net.hip").kernels
    family = kernel_meta.matches(k, "k_tower_bf16") + kernel_meta.matches(k, "k_sym_bf16")
    assert len(family) == 12, sorted(family)


@needs_hipcc
def test_the_edge_kernel_is_one_instantiation_of_four_waves_without_scratch():
    """k_edge_bf16<Tw<128, 4, true, 1>>: one kernel under a name of its own; 4 waves, one per SIMD: one workgroup per CU"""
    net = compile_asm("bz_net.hip")
    sym = net.find("k_edge_bf16")
    assert "Li128ELi4ELb1ELi1E" in sym, sym
    assert net.kernels[sym]["max_wg"] == 256, net.kernels[sym]
    assert "scratch_" not in net.body(sym)


@needs_hipcc
def test_replay_seed_has_no_tic_tac_toe_instantiation():
    assert not kernel_meta.matches(compile_asm("bz_mcts.hip").kernels, "k_replay_seed", TTT)


@needs_hipcc
def test_towers_skip_the_padding_row_mfmas():
    """Row-tile units: per conv layer a wave issues 9 taps x 8 k-steps x 8 units = 576 MFMAs minus the 6
    taps x 8 k-steps whose unit reads only padding rows = 528 (bf16; fp8: 144 - 12 = 132).  Two layer bodies per kernel
    + stem + heads: a regression to position-major units would show up here as 1184 / 292."""
    net = compile_asm("bz_net.hip")
    # round 4: the benchmark net's throughput shape runs on v_mfma_f32_16x16x32_bf16 (half the MACs each): 2 x 528 per
    # layer body, 2 x 16 for the stem (4 quarters x 8 units); the heads stay on 32x32x16 (16)
    thr = net.find("k_tower_bf16", "Li128ELi4ELb1E")
    assert net.count(thr, "v_mfma_f32_16x16x32_bf16") == 2 * (2 * 528) + 32
    assert net.count(thr, "v_mfma_f32_32x32x16_bf16") == 16
    assert net.count(net.find("k_tower_bf16", "Li64ELi8ELb0E"), "v_mfma_f32_32x32x16_bf16") == 2 * 264 + 8 + 16  # C = 64: 4 k-steps per tap
    assert net.count(net.find("k_tower_fp8"), "v_mfma_scale_f32_32x32x64_f8f6f4") == 2 * 132 + 4


@needs_hipcc
def test_symmetric_towers_do_the_plain_towers_matrix_work():
    net = compile_asm("bz_net.hip")
    for geo, mnemonics in (("Li128ELi4ELb1E", ("v_mfma_f32_16x16x32_bf16", "v_mfma_f32_32x32x16_bf16")),
                           ("Li64ELi8ELb0E", ("v_mfma_f32_32x32x16_bf16",))):
        for mn in mnemonics:
            assert net.count(net.find("k_sym_bf16", geo), mn) == net.count(net.find("k_tower_bf16", geo), mn), (geo, mn)
    mn = "v_mfma_scale_f32_32x32x64_f8f6f4"
    assert net.count(net.find("k_sym_fp8"), mn) == net.count(net.find("k_tower_fp8"), mn)


@needs_hipcc
def test_the_edge_kernel_skips_the_column_tiles():
    """per layer body 126 tile-taps x 4 k-steps x 2 channel halves = 1008 v_mfma_f32_16x16x32_bf16 (board-row tiles: 1056), plus
    32 for the stem; the heads stay on 16 v_mfma_f32_32x32x16_bf16"""
    net = compile_asm("bz_net.hip")
    edge = net.find("k_edge_bf16")
    assert net.count(edge, "v_mfma_f32_16x16x32_bf16") == 2 * 1008 + 32
    assert net.count(edge, "v_mfma_f32_32x32x16_bf16") == 16


@needs_hipcc
def test_the_weight_gradient_reads_both_operands_through_the_lds_transpose_read():
    train = compile_asm("bz_train.hip")
    assert train.count(train.find("k_train_wgrad", "Li128E"), "ds_read_b64_tr_b16") >= 14


@needs_hipcc
def test_merge_kernels_declare_at_most_40_kib_of_lds():
    """the reduce kernel's staging area fits the 64 KiB a workgroup may declare, with room for several workgroups per CU"""
    kernels = compile_asm("bz_merge.hip").kernels
    assert kernels
    for sym, k in kernels.items():
        assert k["lds_static"] <= 40 * 1024, (sym, k)


@needs_hipcc
@pytest.mark.parametrize("src, flags", VARIANTS)
def test_diagnostic_variants_compile(src, flags):
    """the variants build.build_variant makes (in-kernel clock stamps, the weak TT hash of a GPU test) in every source that
    reads their flags (bz_train.hip through bz_tower.h): the product build never compiles these paths, so nothing else
    notices when one stops compiling.  The stamps must really be there."""
    assert "s_memtime" in compile_asm(src, flags).asm


def test_build_variant_refuses_unknown_flags():
    """a flag that no source reads (e.g. a retired A/B option) would build the product library under a variant's name"""
    from betazero_amd import build
    for flag in ("-DBZ_EXP_NO_ROWT", "-DBZ_EXP_NOPS=2"):
        with pytest.raises(ValueError, match="BZ_EXP_STAMPS, BZ_EXP_STAMPS_TAPS, BZ_EXP_TREE_STAMPS, BZ_EXP_TT_WEAK_HASH"):
            build.build_variant("retired", ["-DBZ_EXP_STAMPS", flag])


@needs_hipcc
def test_each_source_was_compiled_once():
    """(last in the file) every (source, flags) pair the tests above read -- eight product sources, three variants -- stands once
    in the helper's command log: asking again, as here, compiles nothing"""
    want = [(src, ()) for src in TABLE] + VARIANTS
    for src, flags in want:
        compile_asm(src, flags)
    ran = [(os.path.basename(cmd[-1]), tuple(cmd[1 + len(kernel_meta.FLAGS):-3])) for cmd in kernel_meta.COMMANDS]
    assert len(ran) == len(set(ran)) and set(want) <= set(ran), ran
