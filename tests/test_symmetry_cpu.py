"""The evaluator's board symmetries on the host: bz_sym_index / bz_sym_board / bz_sym_action_map against
a numpy twin written here with np.flip / np.rot90 / .T, the tie to the Reversi rules on every board size, the spread of
the hash, and the option checks -- none of which needs a GPU.  tests/test_gpu_symmetry.py imports the twin."""
import ctypes as C

import numpy as np
import pytest

from betazero_amd import _lib
from betazero_amd.symmetry import (SYM_INVERSE, EvalSymmetry, check_eval_symmetry, check_forward_symmetry, sym_action_map,
                                   sym_board, sym_index)

SIZES = (8, 6, 4)
M64 = (1 << 64) - 1


# ---------------------------------------------------------------- the numpy twin
def grid_of(b, n):
    """bitboard -> the n x n corner as a 0/1 array (bit 8 r + c)"""
    return np.array([[(int(b) >> (8 * r + c)) & 1 for c in range(n)] for r in range(n)], dtype=np.int64)


def bits_of(g):
    n = g.shape[0]
    return sum(int(g[r, c]) << (8 * r + c) for r in range(n) for c in range(n))


def twin_grid(g, s):
    """the eight transforms on an n x n array: 0..6 in the order of the D4 augmentation (id, flip rows, flip columns,
    rot90 x1, x2, x3, transpose), 7 = the anti-transpose out[r][c] = x[n-1-c][n-1-r]"""
    return (g, np.flip(g, 0), np.flip(g, 1), np.rot90(g, 1), np.rot90(g, 2), np.rot90(g, 3), g.T, np.rot90(g, 2).T)[s]


def corner_mask(n):
    return sum(1 << (8 * r + c) for r in range(n) for c in range(n))


def twin_board(b, n, s):
    """T_s on the corner; bits outside it stay"""
    b = int(b)
    return bits_of(twin_grid(grid_of(b, n), s)) | (b & ~corner_mask(n) & M64)


def twin_tau(n, s):
    """tau_s [65]: where a stone on cell j goes"""
    tau = np.arange(65)
    for j in range(64):
        if j >> 3 < n and (j & 7) < n:
            tau[j] = int(twin_board(1 << j, n, s)).bit_length() - 1
    return tau


def twin_index(seed, own, opp):
    h = (seed ^ (own * 0x9E3779B97F4A7C15)) & M64
    h = ((h ^ (h >> 29)) * 0xBF58476D1CE4E5B9) & M64
    h ^= (opp * 0xC2B2AE3D27D4EB4F) & M64
    h = ((h ^ (h >> 32)) * 0x94D049BB133111EB) & M64
    return (h ^ (h >> 31)) >> 61


def random_positions(n, count, seed, distinct=False):
    """`count` seeded random (own, opp) pairs on the n x n corner: disjoint, any density"""
    rng = np.random.default_rng(seed)
    out, seen = [], set()
    while len(out) < count:
        cells = rng.integers(0, 3, size=(n, n))
        p = (bits_of(cells == 1), bits_of(cells == 2))
        if distinct and p in seen:
            continue
        seen.add(p)
        out.append(p)
    return out


def test_the_twin_matches_its_own_definition():
    """the anti-transpose entry really is (r, c) <- (n-1-c, n-1-r), and rot90 is numpy's (counter-clockwise)"""
    n = 6
    g = np.arange(n * n).reshape(n, n)
    a = twin_grid(g, 7)
    assert all(a[r, c] == g[n - 1 - c, n - 1 - r] for r in range(n) for c in range(n))
    r3 = twin_grid(g, 3)
    assert all(r3[r, c] == g[c, n - 1 - r] for r in range(n) for c in range(n))
    assert len({twin_grid(g, s).tobytes() for s in range(8)}) == 8  # eight different elements (the reference's list has seven)


# ---------------------------------------------------------------- tables
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("s", range(8))
def test_action_map_and_board_against_the_twin(n, s):
    tau = sym_action_map(n, s)
    assert np.array_equal(tau, twin_tau(n, s))
    assert sorted(tau.tolist()) == list(range(65))                      # a permutation ...
    assert tau[64] == 64                                                # ... that fixes the pass action ...
    off = [j for j in range(64) if j >> 3 >= n or (j & 7) >= n]
    assert all(tau[j] == j for j in off)                                # ... and every cell outside the corner
    for j in range(64):                                                 # single stones move to tau(j)
        assert sym_board(1 << j, n, s) == 1 << int(tau[j]), (n, s, j)
    inv = sym_action_map(n, SYM_INVERSE[s])
    assert np.array_equal(inv[tau], np.arange(65))
    for own, opp in random_positions(n, 24, 100 * n + s):
        for b in (own, opp, own | opp, own | (1 << 63 if n < 8 else 0)):
            t = sym_board(b, n, s)
            assert t == twin_board(b, n, s), (n, s, hex(b))
            assert sym_board(t, n, SYM_INVERSE[s]) == b                 # s then its inverse is the identity


@pytest.mark.parametrize("n", SIZES)
def test_the_tables_commute_with_the_rules(n):
    """legal(T_s own, T_s opp) == T_s legal(own, opp): ties the tables to the Reversi rules on the small boards"""
    L = _lib.lib()

    def legal(own, opp):
        out = C.c_uint64()
        _lib.check(L.bz_reversi_legal(own, opp, n, C.byref(out)))
        return out.value

    some = 0
    for own, opp in random_positions(n, 300, 7 + n):
        lg = legal(own, opp)
        some += lg != 0
        for s in range(8):
            assert legal(sym_board(own, n, s), sym_board(opp, n, s)) == sym_board(lg, n, s), (n, s, hex(own), hex(opp))
    assert some > 100  # the positions do have legal moves


# ---------------------------------------------------------------- the hash
@pytest.mark.parametrize("n", SIZES)
def test_sym_index_is_the_formula_and_spreads(n):
    pos = random_positions(n, 512, 11 * n, distinct=True)
    per_seed = {}
    for seed in (0, 1, 12345):
        idx = np.array([sym_index(seed, o, p) for o, p in pos])
        assert np.array_equal(idx, [twin_index(seed, o, p) for o, p in pos])
        counts = np.bincount(idx, minlength=8)
        assert counts.min() >= 32, (n, seed, counts)  # the formula alone gives 47..79
        per_seed[seed] = idx
    assert (per_seed[0] != per_seed[1]).any()
    big = (1 << 64) - 1
    assert sym_index(big, big, big) == twin_index(big, big, big)  # wrapping arithmetic


def test_bad_arguments_are_refused():
    L = _lib.lib()
    out = C.c_uint64()
    m = np.zeros(65, np.uint8)
    assert L.bz_sym_board(1, 9, 0, C.byref(out)) == _lib.BZ_EINVAL
    assert L.bz_sym_board(1, 8, 8, C.byref(out)) == _lib.BZ_EINVAL
    assert L.bz_sym_board(1, 8, 0, None) == _lib.BZ_EINVAL
    assert L.bz_sym_action_map(0, 0, m.ctypes.data) == _lib.BZ_EINVAL
    assert L.bz_sym_action_map(8, -1, m.ctypes.data) == _lib.BZ_EINVAL
    assert L.bz_net_sym_scratch_bytes(7) >= 8 * 7 * 66 * 4 and L.bz_net_sym_scratch_bytes(7) % 256 == 0
    assert L.bz_net_sym_scratch_bytes(-1) == -1
    assert L.bz_abi_version() == 7  # the ABI only grew


# ---------------------------------------------------------------- option checks (no device is touched)
def test_eval_symmetry_option_values():
    assert check_eval_symmetry(None) is None and check_eval_symmetry(False) is None
    assert check_eval_symmetry(True, seed=9) == EvalSymmetry(9)
    assert check_eval_symmetry(EvalSymmetry(seed=2**64 - 1)) == EvalSymmetry(2**64 - 1)
    assert check_eval_symmetry(EvalSymmetry(np.int64(5)), game="reversi6", evaluator="net_fp8") == EvalSymmetry(5)
    for bad in (1, 0, "hash", "on", 3.0, (1,), EvalSymmetry(-1), EvalSymmetry(2**64), EvalSymmetry(1.5), EvalSymmetry(True),
                EvalSymmetry(None)):
        with pytest.raises(ValueError, match="eval_symmetry"):
            check_eval_symmetry(bad)
    for game in ("ttt", "tic_tac_toe", _lib.GAME_TTT):
        with pytest.raises(ValueError, match="Reversi"):
            check_eval_symmetry(True, game=game, evaluator="net_bf16")
    for ev in ("uniform", "hash", "external", "mlp_f32", "mlp_bf16"):
        with pytest.raises(ValueError, match="net_f32 / net_bf16 / net_fp8"):
            check_eval_symmetry(True, game="reversi", evaluator=ev)
        assert check_eval_symmetry(None, game="reversi", evaluator=ev) is None  # off is always accepted


def test_every_surface_refuses_before_a_device_is_touched():
    """no GPU here: a bad value or a refused evaluator must raise ValueError, not the RuntimeError of a missing device"""
    from betazero_amd.arena import play_arena
    from betazero_amd.engine import PipelinedSelfPlay, SelfPlayEngine, self_play
    from betazero_amd.match import MatchPlayer, check_match
    from betazero_amd.players import MCTSPlayer
    for ev, game in (("uniform", "reversi"), ("hash", "reversi6"), ("external", "reversi"), ("net_bf16", "ttt"), ("mlp_f32", "ttt")):
        with pytest.raises(ValueError, match="eval_symmetry"):
            SelfPlayEngine(game, 4, 8, ev, eval_symmetry=True)
        with pytest.raises(ValueError, match="eval_symmetry"):
            PipelinedSelfPlay(game, 4, 8, ev, eval_symmetry=EvalSymmetry(3))
        with pytest.raises(ValueError, match="eval_symmetry"):
            self_play(game, 4, 8, evaluator=ev, eval_symmetry=True)
    with pytest.raises(ValueError, match="eval_symmetry"):
        SelfPlayEngine("reversi", 4, 8, "net_bf16", eval_symmetry="yes")
    with pytest.raises(ValueError, match="eval_symmetry"):
        self_play("reversi", 4, 8, evaluator="net_bf16", eval_symmetry=7)
    with pytest.raises(ValueError, match="eval_symmetry"):
        MCTSPlayer(1, sims=8, evaluator="uniform", eval_symmetry=True)
    with pytest.raises(ValueError, match="eval_symmetry"):
        MCTSPlayer(1, sims=8, evaluator=lambda own, opp, kind: None, eval_symmetry=True)  # the external evaluator
    with pytest.raises(ValueError, match="eval_symmetry"):
        MCTSPlayer(1, sims=8, evaluator="net_bf16", eval_symmetry="hash")
    with pytest.raises(ValueError, match="eval_symmetry"):
        check_match("reversi", 4, MatchPlayer(sims=8, evaluator="hash", eval_symmetry=True), MatchPlayer(sims=8), 8, 0)
    with pytest.raises(ValueError, match="eval_symmetry"):
        check_match("ttt", 4, MatchPlayer(sims=8, evaluator="uniform", eval_symmetry=EvalSymmetry(1)), MatchPlayer(sims=8), 8, 0)
    with pytest.raises(ValueError, match="eval_symmetry"):
        play_arena("reversi", 4, 8, evaluator="uniform", eval_symmetry=True)
    with pytest.raises(ValueError, match="eval_symmetry"):
        play_arena("ttt", 4, 8, evaluator="uniform", eval_symmetry=EvalSymmetry(0))
    assert MatchPlayer().eval_symmetry is None and MCTSPlayer(1, sims=8).eval_symmetry is None  # the default is off


def test_forward_symmetry_option_values():
    assert check_forward_symmetry(None) is None
    assert check_forward_symmetry(0) == (0, 0) and check_forward_symmetry(np.int32(7), size=4) == (0, 7)
    assert check_forward_symmetry("hash", seed=2**63) == (1, 2**63)
    assert check_forward_symmetry("mean", size=6) == (2, 0)
    for bad in (8, -1, True, 1.0, "Hash", "all", (0,)):
        with pytest.raises(ValueError, match="symmetry"):
            check_forward_symmetry(bad)
    with pytest.raises(ValueError, match="size"):
        check_forward_symmetry(0, size=5)
    with pytest.raises(ValueError, match="seed"):
        check_forward_symmetry("hash", seed=-1)
