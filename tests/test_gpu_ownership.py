"""Ownership targets on the GPU: k_own_final / k_pack_own against the twins of tests/test_ownership_cpu.py and
the engine's own rows, and the carrying of the targets through the pipelines and the augmentation.  "Equal" = bit for bit.  The
feature observes: with it on, every byte the engine wrote without it is the same byte.

The twins are Python: tic-tac-toe and Reversi 4x4 are pinned on 64 games per mode, Reversi 6x6 / 8x8 (sixty plies a game) on 8."""
import functools

import numpy as np
import pytest
import torch

from betazero_amd.engine import ForcedPlayouts, Fpu, GumbelConfig, PlayoutCap
from betazero_amd.symmetry import sym_board
from test_gpu_playout_cap import _run, _same_rows
from test_ownership_cpu import after_last_row, own_games, ownership_row, winner_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NOISE = dict(dirichlet_alpha=0.3, dirichlet_eps=0.25)
SIMS = 8
# the engine's options and the twin's (test_ownership_cpu.own_games) of every mode
MODES = {
    "plain": ({}, ("plain", {})),
    "noise": (dict(temp_moves=4, **NOISE), ("plain", dict(noise=True, temp_moves=4))),
    "cap0": (dict(playout_cap=PlayoutCap(4, 0.0), **NOISE), ("cap", dict(noise=True, cap=(4, 0)))),
    "cap16384": (dict(playout_cap=PlayoutCap(4, 0.25), **NOISE), ("cap", dict(noise=True, cap=(4, 16384)))),
    "cap65536": (dict(playout_cap=PlayoutCap(4, 1.0), **NOISE), ("cap", dict(noise=True, cap=(4, 65536)))),
    "forced_cap": (dict(forced_playouts=ForcedPlayouts(2.0), playout_cap=PlayoutCap(4, 0.5), **NOISE),
                   ("forced", dict(noise=True, cap=(4, 32768)))),
    "gumbel": (dict(gumbel=GumbelConfig(), temp_moves=3), ("gumbel", dict(temp_moves=3))),
    "gumbel_interior": (dict(gumbel=GumbelConfig(interior="gumbel"), temp_moves=3), ("gfull", dict(temp_moves=3))),
    "fpu": (dict(fpu=Fpu(0.2, 0.1), **NOISE), ("fpu", dict(noise=True))),
    "leaves8": (dict(leaves_per_step=8, **NOISE), ("k8", dict(noise=True))),
    "reuse": (dict(reuse_subtree=True, **NOISE), ("plain", dict(noise=True, reuse=True))),
}
CAPPED = ("cap0", "cap16384", "cap65536", "forced_cap")


def _engine(game, n, sims=SIMS, ev="hash", **kw):
    from betazero_amd.engine import SelfPlayEngine
    return SelfPlayEngine(game, n, sims, ev, **kw)


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _fin(eng):
    """(fin_x, fin_o) uint64 [rounds, B]"""
    fx, fo = eng.ownership_rows()
    return _u64(fx), _u64(fo)


@functools.lru_cache(maxsize=None)
def _twins(mode, game, n, seed, base, openings=0, stagger=0):
    kind, tkw = MODES[mode][1]
    return own_games(kind, game, n, SIMS, seed=seed, base=base, openings=openings, stagger=stagger, **tkw)


def _rows_targets(eng):
    """the rows' targets in (round, slot, ply) order, from the engine's own arrays: bz_ownership_row's restatement of every
    finished game's final board and its rows' movers"""
    t = eng.example_tensors()
    lens, mover = t["len"].cpu().numpy(), t["mover"].cpu().numpy()
    fx, fo = _fin(eng)
    a, b = [np.zeros(0, np.uint64)], [np.zeros(0, np.uint64)]
    for r in range(lens.shape[0]):
        for g in range(lens.shape[1]):
            n = max(0, lens[r, g])
            to, tp = ownership_row(np.full(n, fx[r, g]), np.full(n, fo[r, g]), mover[r, g, :n])
            a.append(to); b.append(tp)
    return np.concatenate(a), np.concatenate(b)


# ---------------------------------------------------------------- observes only
@pytest.mark.parametrize("game", ["ttt", "reversi4", "reversi6", "reversi"])
@pytest.mark.parametrize("mode", list(MODES))
def test_ownership_on_and_off_write_the_same_bytes(game, mode):
    kw = dict(openings=1, seed=11, game_id_base=5)
    kw.update(MODES[mode][0])
    off, on = _engine(game, 64, **kw), _engine(game, 64, ownership=True, **kw)
    _, (w0, l0), c0 = _run(off)
    ex, (w1, l1), c1 = _run(on)
    assert (l0 >= 0).all() and np.array_equal(w0, w1) and np.array_equal(l0, l1)
    assert torch.equal(off.example_block(), on.example_block())
    print(mode, game, "counters off / on:", c0, c1)
    assert c0 == c1, (c0, c1)
    assert ex.fown.shape == ex.fopp.shape == (int(l1.sum()),) and ex.fown.dtype == np.uint64 and ex.q is None and ex.kl is None
    assert off.examples().fown is None and off.examples().fopp is None
    fx, fo = _fin(on)
    assert not (fx & fo).any() and (fx | fo).all()  # every game finished: a board each, no cell owned twice
    d = np.array([[bin(int(a)).count("1") - bin(int(b)).count("1") for a, b in zip(ra, rb)] for ra, rb in zip(fx, fo)])
    if game != "ttt":
        assert np.array_equal(np.sign(d), w1)  # the winner the engine recorded is the one the final board gives
    with pytest.raises(RuntimeError, match="ownership=True"):
        off.ownership_rows()


# ---------------------------------------------------------------- pinned to the twins
def _pinned(mode, game, n, seed=3, base=2, openings=0):
    eng = _engine(game, n, ownership=True, seed=seed, game_id_base=base, openings=openings, **MODES[mode][0])
    ex, (winners, lens), _ = _run(eng)
    fx, fo = _fin(eng)
    for g, (rows, (tx, to), w) in enumerate(_twins(mode, game, n, seed, base, openings)):
        assert lens[0, g] == len(rows) and winners[0, g] == w, (mode, game, g, lens[0, g], len(rows))
        assert (int(fx[0, g]), int(fo[0, g])) == (tx, to), (mode, game, g, hex(fx[0, g]), hex(fo[0, g]), hex(tx), hex(to))
        m = ex.game == base + g
        want = ownership_row(np.full(len(rows), tx, np.uint64), np.full(len(rows), to, np.uint64), np.array([r[3] for r in rows]))
        assert np.array_equal(ex.fown[m], want[0]) and np.array_equal(ex.fopp[m], want[1]), (mode, game, g)
    return eng, ex, lens


@pytest.mark.parametrize("game", ["ttt", "reversi4"])
@pytest.mark.parametrize("mode", list(MODES))
def test_final_boards_equal_the_twins_on_every_game(game, mode):
    """Reversi 4x4 has forced passes and games that end before the board is full"""
    eng, ex, lens = _pinned(mode, game, 64)
    if mode == "cap0":  # no search was full: no row anywhere, and a final board for every game all the same
        assert len(ex) == 0 and ex.fown.shape == (0,) and (lens == 0).all()
    if mode in ("cap16384", "forced_cap"):
        assert (lens == 0).any() or (lens < lens.max()).any()
    if mode not in CAPPED:  # the last move is recorded: the final board follows from the last row
        for g in range(0, 64, 7):
            m = np.nonzero(ex.game == 2 + g)[0][-1]
            row = (int(ex.own[m]), int(ex.opp[m]), None, int(ex.mover[m]), int(ex.act[m]))
            fx, fo = _fin(eng)
            assert after_last_row(game, row) == (int(fx[0, g]), int(fo[0, g]))


@pytest.mark.parametrize("game,mode,openings", [("reversi6", "noise", 0), ("reversi", "cap16384", 1), ("reversi", "gumbel", 1)])
def test_final_boards_equal_the_twins_reversi6_and_reversi8(game, mode, openings):
    _pinned(mode, game, 8, seed=5, base=7, openings=openings)


def test_two_rounds_with_restart_and_stagger_unfinished_games_stay_zero():
    """tic-tac-toe, two rounds, a staggered pool, 11 moves with restart: the first round is over, the second partly.  A slot
    that restarts overwrites its position; the final board of its finished game stays"""
    B, base, seed = 64, 300, 5
    eng = _engine("ttt", B, rounds=2, stagger=3, seed=seed, game_id_base=base, ownership=True, **MODES["noise"][0])
    eng.reset_games()
    for _ in range(11):
        eng.search()
        eng.play(True)
    eng.status()
    winners, lens = eng.winners()
    fx, fo = _fin(eng)
    assert (lens[0] >= 0).all() and (lens[1] >= 0).any() and (lens[1] < 0).any(), lens.tolist()
    kind, tkw = MODES["noise"][1]
    for r in range(2):
        twins = own_games(kind, "ttt", B, SIMS, seed=seed, base=base + r * B, stagger=3 if r == 0 else 0, **tkw)
        for g, (rows, (tx, to), w) in enumerate(twins):
            if lens[r, g] < 0:
                assert fx[r, g] == 0 and fo[r, g] == 0, (r, g)
            else:
                assert (int(fx[r, g]), int(fo[r, g]), lens[r, g], winners[r, g]) == (tx, to, len(rows), w), (r, g)
    want = _rows_targets(eng)
    ex = eng.examples()
    assert len(ex) == int(lens[lens >= 0].sum()) and np.array_equal(ex.fown, want[0]) and np.array_equal(ex.fopp, want[1])
    eng.reset_games()  # a new iteration: no game is finished, every final board is 0 again
    fx, fo = _fin(eng)
    assert not fx.any() and not fo.any()


def test_with_the_bf16_net_the_final_board_follows_the_last_row_and_gives_the_winner():
    """the bf16 net in the loop, 64 channels x 2 blocks (the smallest width the MFMA tower is built for), no cap: every game's
    last move is recorded, so apply(last row) -- by the board classes -- is the final board"""
    from test_gpu_search_net import _dn, _net
    P, _ = _net("bf16", 64, 2)
    eng = _engine("reversi6", 64, 8, "net_bf16", net=_dn(P, 64), ownership=True, temp_moves=4, seed=2)
    ex, (winners, lens), _ = _run(eng)
    fx, fo = _fin(eng)
    assert (lens > 0).all()
    for g in range(64):
        m = np.nonzero(ex.game == g)[0][-1]
        row = (int(ex.own[m]), int(ex.opp[m]), None, int(ex.mover[m]), int(ex.act[m]))
        assert after_last_row("reversi6", row) == (int(fx[0, g]), int(fo[0, g])), g
        assert winner_of("reversi6", int(fx[0, g]), int(fo[0, g])) == (True, winners[0, g]), g
    want = _rows_targets(eng)
    assert np.array_equal(ex.fown, want[0]) and np.array_equal(ex.fopp, want[1])


def test_the_step_api_and_selfplay_run_record_the_same_final_boards():
    """the same games through search() / play(), through the step API and through bz_selfplay_run (PipelinedSelfPlay.step)"""
    from betazero_amd.engine import PipelinedSelfPlay
    kw = dict(seed=6, temp_moves=2, **NOISE)
    a = _engine("reversi4", 64, ownership=True, **kw)
    _run(a)
    b = _engine("reversi4", 64, ownership=True, **kw)
    b.reset_games()
    for _ in range(40):
        b.root_begin(); b.evaluate(); b.expand_backup(); b.root_noise()
        for s in range(SIMS):
            b.select(s); b.evaluate(); b.expand_backup()
        b.play(False)
        if b.status()[0] == 0:
            break
    sp = PipelinedSelfPlay("reversi4", 64, SIMS, "hash", pipelines=1, ownership=True, **kw)
    sp.run_iteration()
    sp.status()
    want = _fin(a)
    assert (want[0] | want[1]).all()  # (a side may be wiped out: one of the two boards can be 0)
    for got in (_fin(b), tuple(_u64(t) for t in sp.ownership_rows())):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


# ---------------------------------------------------------------- packing
CAP_KW = dict(temp_moves=4, seed=1, playout_cap=PlayoutCap(4, 0.15), **NOISE)  # (the cap: games of unequal row counts, some of none)


def test_device_examples_carry_the_targets_in_round_slot_ply_order():
    eng = _engine("reversi4", 64, ownership=True, search_value=True, **CAP_KW)
    _, (_, lens), _ = _run(eng)
    assert (lens == 0).any() and (lens > 0).any()  # rows of 0-row games: none, and the next game's rows follow at once
    want = _rows_targets(eng)
    dx = eng.device_examples()
    assert dx.fown.is_cuda and dx.fown.dtype == torch.int64 and len(dx) == len(want[0]) > 0
    assert np.array_equal(_u64(dx.fown), want[0]) and np.array_equal(_u64(dx.fopp), want[1])
    hx = eng.examples()
    assert np.array_equal(hx.fown, want[0]) and np.array_equal(hx.fopp, want[1]) and np.array_equal(dx.cpu().fown, want[0])
    assert dx.q is not None and dx.q.shape == dx.fown.shape and dx.vt is None
    # every row's target is its game's final board: the stones of both sides, whoever moves
    t = eng.example_tensors()
    assert (np.unique(hx.fown | hx.fopp) == np.unique((_fin(eng)[0] | _fin(eng)[1])[t["len"].cpu().numpy() > 0])).all()


def test_two_pipelines_append_at_the_right_offset_and_self_play_carries_the_targets():
    from betazero_amd.engine import PipelinedSelfPlay, self_play
    sp = PipelinedSelfPlay("reversi4", 64, SIMS, "hash", pipelines=2, ownership=True, **CAP_KW)
    sp.run_iteration()
    assert sp.status()[0] == 0
    parts = [_rows_targets(e) for e in sp.engines]
    want = tuple(np.concatenate([p[k] for p in parts]) for k in (0, 1))
    assert len(parts[0][0]) > 0 and len(parts[1][0]) > 0
    dx, hx = sp.device_examples(), sp.examples()
    assert len(dx) == len(want[0]) and np.array_equal(_u64(dx.fown), want[0]) and np.array_equal(_u64(dx.fopp), want[1])
    assert np.array_equal(hx.fown, want[0]) and np.array_equal(hx.fopp, want[1]) and hx.q is None
    blk, fown, fopp = sp.pack_examples_with_ownership()
    assert np.array_equal(_u64(fown[:len(dx)]), want[0]) and np.array_equal(_u64(fopp[:len(dx)]), want[1])
    assert not fown[len(dx):].any() and not fopp[len(dx):].any()
    one = _engine("reversi4", 64, ownership=True, **CAP_KW)  # the same games on one engine: the same rows, the same targets
    _run(one)
    ox = one.examples()
    assert np.array_equal(ox.game, hx.game) and np.array_equal(ox.fown, hx.fown) and np.array_equal(ox.fopp, hx.fopp)
    _, _, _, sx = self_play("reversi4", 64, SIMS, evaluator="hash", ownership=True, pipelines=2, **CAP_KW)
    assert np.array_equal(sx.fown, want[0]) and np.array_equal(sx.fopp, want[1])
    assert self_play("reversi4", 4, 8, evaluator="hash")[3].fown is None
    with pytest.raises(RuntimeError, match="ownership=True"):
        PipelinedSelfPlay("reversi4", 4, 8, "hash", pipelines=1).pack_examples_with_ownership()


def test_a_block_too_small_leaves_the_same_games_out_and_writes_nothing_behind_the_capacity():
    from betazero_amd.engine import _packed_views, packed_block_header
    eng = _engine("reversi4", 64, ownership=True, **CAP_KW)
    _run(eng)
    want = _rows_targets(eng)
    cap = len(want[0]) // 2
    blk = eng.pack_examples(cap_rows=cap)
    out = (torch.full((cap + 64,), -7, dtype=torch.int64, device=DEV), torch.full((cap + 64,), -7, dtype=torch.int64, device=DEV))
    eng.pack_ownership(out, cap)
    h = packed_block_header(blk, strict=False)
    n = h["n_rows"]
    assert 0 < n <= cap and h["dropped_rows"] == len(want[0]) - n
    for got, w in zip(out, want):
        got = got.cpu().numpy()
        assert np.array_equal(got[:n].view(np.uint64), w[:n]) and (got[n:] == -7).all()  # (the games that fit are a prefix)
    games = _packed_views(blk, h)["game"].cpu().numpy()
    assert np.array_equal(games, eng.examples().game[:n])


# ---------------------------------------------------------------- augmentation
@pytest.mark.parametrize("game,size", [("reversi", 8), ("ttt", 3)])
def test_augmentation_transforms_every_copys_target_by_the_symmetry_of_its_position(game, size):
    from betazero_amd.augment import augment_examples
    eng = _engine(game, 64, ownership=True, temp_moves=4, seed=3, openings=1)
    _run(eng)
    ex = eng.device_examples()
    n = len(ex)
    aug = augment_examples(ex, dedupe=False)
    assert len(aug) == 8 * n
    if size == 3:  # the engine's tic-tac-toe bit is 3 * row + col; bz_sym_board works on the corner of the 8-stride plane
        def wide(b):
            return sum(((int(b) >> (3 * r + c)) & 1) << (8 * r + c) for r in range(3) for c in range(3))

        def narrow(b):
            return sum(((int(b) >> (8 * r + c)) & 1) << (3 * r + c) for r in range(3) for c in range(3))
    else:
        wide = narrow = int
    sym = lambda b, s: narrow(sym_board(wide(b), size, s))  # noqa: E731
    src = {f: _u64(getattr(ex, f)) for f in ("own", "opp", "fown", "fopp")}
    got = {f: _u64(getattr(aug, f)) for f in ("own", "opp", "fown", "fopp")}
    pop = lambda a: np.array([bin(int(v)).count("1") for v in a])  # noqa: E731
    assert np.array_equal(pop(got["fown"]), np.repeat(pop(src["fown"]), 8)) and np.array_equal(pop(got["fopp"]), np.repeat(pop(src["fopp"]), 8))
    for i in range(0, n, max(1, n // 40)):
        for t in range(8):
            k = 8 * i + t
            fits = [s for s in range(8) if sym(src["own"][i], s) == got["own"][k] and sym(src["opp"][i], s) == got["opp"][k]]
            assert fits and (t > 6 or t in fits), (i, t, fits)  # (transforms 0..6 are bz_sym_board's 0..6)
            cand = [t] if t <= 6 else fits
            assert any((sym(src["fown"][i], s), sym(src["fopp"][i], s)) == (int(got["fown"][k]), int(got["fopp"][k])) for s in cand), (i, t)
    # the dedupe key does not see the target: the kept rows are the ones kept without it, each with its own copy's target
    bare = eng.device_examples()
    bare.fown = bare.fopp = None
    kept, kept_bare = augment_examples(ex), augment_examples(bare)
    assert kept_bare.fown is None and torch.equal(kept.own, kept_bare.own) and torch.equal(kept.pi, kept_bare.pi)
    assert np.array_equal(pop(_u64(kept.fown)) + pop(_u64(kept.fopp)), pop(_u64(kept.fown) | _u64(kept.fopp)))
    host = augment_examples(ex.cpu(), dedupe=False)
    assert host.fown.dtype == np.uint64 and np.array_equal(host.fown, got["fown"]) and np.array_equal(host.fopp, got["fopp"])
