"""Resignation in self-play on the GPU: k_resign_note / k_resign_finish around the play kernels against the
resignation twin of tests/test_resign_cpu.py and against the host functions the kernels run.  "Equal" = bit for bit, every
game: the rows (positions, pi bits, movers, actions, z), winners, ex_len and resign_rows()."""
import ctypes as C

import numpy as np
import pytest
import torch

from betazero_amd import _lib
from betazero_amd.engine import (ForcedPlayouts, Fpu, GumbelConfig, PipelinedSelfPlay, PlayoutCap, Resign, SelfPlayEngine,
                                 packed_block_header, unpack_packed_block)
from test_forced_playouts_cpu import ForcedTwin
from test_gumbel_cpu import GumbelTwin
from test_leaf_parallel_cpu import KTwin, boards
from test_playout_cap_cpu import CapTwin
from test_resign_cpu import FAST_DECIDES, f32, resign_twin
from test_solver_cpu import SolverTwin

pytestmark = pytest.mark.gpu
NOISE = dict(dirichlet_alpha=0.3, dirichlet_eps=0.25)
THR, CONS = -0.2, 2
# the four sizes, with temperature, openings, stagger and noise: at seed 1 the twin resigns 11 of 12, 5 of 16, 3 of 6 and 5 of 8
# games at (-0.2, 2), with 2, 1, 1 and 1 false positives among them (found on the twin alone)
CASES = {"reversi": dict(n=12, sims=24, temp_moves=8, openings=1, seed=1, base=7, stagger=5, noise=True),
         "ttt": dict(n=16, sims=40, temp_moves=4, openings=0, seed=1, base=0, stagger=3, noise=True),
         "reversi6": dict(n=6, sims=30, temp_moves=2, openings=0, seed=1, base=0, stagger=4, noise=False),
         "reversi4": dict(n=8, sims=16, temp_moves=3, openings=0, seed=1, base=0, stagger=0, noise=True)}


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)


def _rs(playout_q, threshold=THR, consecutive=CONS):
    rs = Resign(threshold, consecutive, playout_q / 65536)
    assert rs.playout_q == playout_q
    return rs


_GAMES = {}


def _twin(base_cls, game, gid, sims, temp_moves, openings, seed, slot=0, stagger=0, noise=False, args=(), **kw):
    """the resignation twin of one game with its base game played (once per process); apply() then costs nothing"""
    key = (base_cls, game, gid, sims, temp_moves, openings, seed, slot if stagger else 0, stagger, noise, args, tuple(sorted(kw.items())))
    if key not in _GAMES:
        tw = resign_twin(base_cls)(game, "hash", *args, boards=boards(), resign=(THR, CONS, 0),
                                   **(dict(dir_alpha=NOISE["dirichlet_alpha"], dir_eps=NOISE["dirichlet_eps"]) if noise else {}), **kw)
        tw.selfplay(gid, sims, temp_moves, openings, seed, slot=slot, stagger=stagger)
        _GAMES[key] = tw
    return _GAMES[key]


def _applied(tw, gid, seed, playout_q, threshold=THR, consecutive=CONS):
    """(rows, winner) of the twin's game under the rule; the twin then carries record / played_out / resigned / n_searches"""
    tw.threshold, tw.consecutive, tw.playout_q = f32(threshold), consecutive, playout_q
    rows, w, _ = tw.apply(gid, seed)
    return rows, w


def _same_rows(ex, gid, rows, w):
    msk = ex.game == gid
    assert int(msk.sum()) == len(rows), (gid, int(msk.sum()), len(rows))
    na = ex.pi.shape[1]
    assert np.array_equal(ex.own[msk], np.array([r[0] for r in rows], np.uint64))
    assert np.array_equal(ex.opp[msk], np.array([r[1] for r in rows], np.uint64))
    assert np.array_equal(_bits(ex.pi[msk]).reshape(-1, na), _bits([r[2] for r in rows]).reshape(len(rows), na))
    assert np.array_equal(ex.mover[msk], np.array([r[3] for r in rows], np.int8))
    assert np.array_equal(ex.act[msk], np.array([r[4] for r in rows], np.uint8))
    assert np.array_equal(ex.z[msk], (w * np.array([r[3] for r in rows], np.int64)).astype(np.int8))
    assert np.array_equal(ex.ply[msk], np.arange(len(rows)))


def _same_record(rec, r, g, tw):
    """resign_rows() at [r, g] against the twin's record"""
    side, move, q, out = rec
    assert bool(out[r, g]) == tw.played_out, (r, g)
    if tw.record is None:
        assert side[r, g] == 0, (r, g, side[r, g])
    else:
        assert (side[r, g], move[r, g]) == tw.record[:2] and _bits(q[r, g]) == _bits(tw.record[2]), (r, g, side[r, g], move[r, g], q[r, g], tw.record)


def _play_to_the_end(eng, twins, restart=False):
    """search + play until no slot is active; without restart the active slots after every play are those whose twin has a
    search left"""
    eng.reset_counters()
    eng.reset_games()
    step = 0
    while True:
        eng.search()
        eng.play(restart)
        step += 1
        active = eng.status()[0]
        if not restart:
            assert active == sum(tw.n_searches > step for tw in twins), (step, active)
        if active == 0:
            return step
        assert step < 400


def _check_games(eng, twins, gids, want, rnd=0, ex=None, rec=None, wl=None):
    ex = eng.examples() if ex is None else ex
    rec = eng.resign_rows() if rec is None else rec
    winners, lens = eng.winners() if wl is None else wl
    for g, (tw, gid, (rows, w)) in enumerate(zip(twins, gids, want)):
        assert lens[rnd, g] == len(rows) and winners[rnd, g] == w, (rnd, g, lens[rnd, g], len(rows), winners[rnd, g], w)
        _same_rows(ex, gid, rows, w)
        _same_record(rec, rnd, g, tw)
    return ex, rec


def _case(game, playout_q, base_cls=KTwin, args=(), twin_kw=None, engine_kw=None, threshold=THR, some_stay=None, **over):
    """one of CASES (or an override of it) to the end against the twins.  Returns (engine, twins, want)"""
    c = dict(CASES[game], **over)
    n, sims, seed, base = c["n"], c["sims"], c["seed"], c["base"]
    eng = SelfPlayEngine(game, n, sims, "hash", temp_moves=c["temp_moves"], openings=c["openings"], seed=seed, game_id_base=base,
                         stagger=c["stagger"], resign=_rs(playout_q, threshold), **(NOISE if c["noise"] else {}), **(engine_kw or {}))
    twins = [_twin(base_cls, game, base + g, sims, c["temp_moves"], c["openings"], seed, slot=g, stagger=c["stagger"], noise=c["noise"],
                   args=args, **(twin_kw or {})) for g in range(n)]
    # the case is not vacuous, on the twin's side alone: with nobody played out at least one game resigns, and one does not
    resigned = []
    for g, tw in enumerate(twins):
        _applied(tw, base + g, seed, 0, threshold)
        resigned.append(tw.resigned)
    assert any(resigned), "no game of the case resigns"
    if some_stay if some_stay is not None else game != "reversi6":
        assert not all(resigned), "every game of the case resigns"
    want = [_applied(tw, base + g, seed, playout_q, threshold) for g, tw in enumerate(twins)]
    _play_to_the_end(eng, twins)
    _check_games(eng, twins, [base + g for g in range(n)], want)
    assert len(eng.examples()) == sum(len(r) for r, _ in want)
    assert eng.counters()["n_sims"] == sum(tw.n_sims for tw in twins)  # the twin's searches x their budgets
    if 0 < playout_q < 65536:
        assert {tw.played_out for tw in twins} == {True, False}
    return eng, twins, want


# ---------------------------------------------------------------- 1. self-play against the twin
@pytest.mark.parametrize("playout_q", [0, 16384, 65536])
@pytest.mark.parametrize("game", list(CASES))
def test_selfplay_equals_the_twin_with_temperature_openings_stagger_and_noise(game, playout_q):
    eng, twins, _ = _case(game, playout_q)
    st = eng.resign_stats()
    assert st["n_finished"] == len(twins) and st["n_resigned"] == sum(tw.resigned for tw in twins)
    assert st["n_played_out"] == sum(tw.played_out for tw in twins)
    assert st["n_would_resign"] == sum(tw.played_out and tw.record is not None for tw in twins)


# ---------------------------------------------------------------- 2. every game played out = resignation off
def _raw(eng):
    torch.cuda.synchronize()
    return eng.example_block().cpu().numpy().copy()


@pytest.mark.parametrize("game", ["reversi", "ttt"])
def test_every_game_played_out_writes_the_block_of_the_engine_without_resignation(game):
    eng, twins, want = _case(game, 65536)
    c = CASES[game]
    ref = SelfPlayEngine(game, c["n"], c["sims"], "hash", temp_moves=c["temp_moves"], openings=c["openings"], seed=c["seed"],
                         game_id_base=c["base"], stagger=c["stagger"], **(NOISE if c["noise"] else {}))
    ref.reset_counters()
    ref.run_iteration()
    ref.status()
    assert np.array_equal(_raw(eng), _raw(ref))  # rows, z, ex_len, winners, the header: every byte
    assert eng.counters() == ref.counters()
    fp = sum(tw.record is not None and w != -tw.record[0] for tw, (_, w) in zip(twins, want))
    assert fp >= 1, "the case must hold a false positive"
    st = eng.resign_stats()
    assert st == {"n_finished": c["n"], "n_resigned": 0, "n_played_out": c["n"], "n_would_resign": sum(tw.record is not None for tw in twins),
                  "n_false_positive": fp, "false_positive_rate": fp / sum(tw.record is not None for tw in twins)}, st


# ---------------------------------------------------------------- 3. restart
def _streaks(eng):
    """the engine's streak array u8 [rounds, B, 2] (side +1, side -1): the first array of the resignation buffer"""
    torch.cuda.synchronize()
    n = eng.rounds * eng.B * 2
    return eng._buffers["resign"][:n].cpu().numpy().reshape(eng.rounds, eng.B, 2)


@pytest.mark.parametrize("reuse", [False, True])
def test_restart_plays_every_round_of_every_slot_as_its_own_twin(reuse):
    game, n, sims, seed, rounds, tm = "reversi4", 8, 16, 1, 3, 3
    eng = SelfPlayEngine(game, n, sims, "hash", temp_moves=tm, seed=seed, rounds=rounds, game_id_base=40, reuse_subtree=reuse,
                         resign=_rs(16384))
    twins = [[_twin(KTwin, game, 40 + r * n + g, sims, tm, 0, seed, reuse=reuse) for g in range(n)] for r in range(rounds)]
    want = [[_applied(tw, 40 + r * n + g, seed, 16384) for g, tw in enumerate(row)] for r, row in enumerate(twins)]
    flat = [tw for row in twins for tw in row]
    assert any(tw.resigned for tw in flat[:2 * n]) and not all(tw.resigned for tw in flat) and any(tw.played_out and tw.record for tw in flat)
    steps = _play_to_the_end(eng, flat, restart=True)
    assert eng.status() == (0, rounds * n)  # FLAG_FINISHED
    # every slot ran its three games back to back: a resigned slot started its next game in the same play
    assert steps == max(sum(twins[r][g].n_searches for r in range(rounds)) for g in range(n))
    ex, rec, wl = eng.examples(), eng.resign_rows(), eng.winners()
    for r in range(rounds):
        _check_games(eng, twins[r], [40 + r * n + g for g in range(n)], want[r], rnd=r, ex=ex, rec=rec, wl=wl)
    st = _streaks(eng)
    for r in range(rounds):  # every game's streaks started at zero: they end where the twin's end
        for g in range(n):
            assert (st[r, g, 0], st[r, g, 1]) == (twins[r][g].streaks[1], twins[r][g].streaks[-1]), (r, g)
    assert eng.counters()["n_sims"] == sum(tw.n_sims for tw in flat)


# ---------------------------------------------------------------- 4. q and the rule through the step API
def _step_search(eng):
    eng.root_begin(); eng.evaluate(); eng.expand_backup(); eng.root_noise()
    for s in range(0, eng.sims, eng.K):
        eng.select(s); eng.evaluate(); eng.expand_backup()


def _host_rule_case(eng, rs, step_api=True, max_plies=140):
    """the engine to the end; after every search root_stats() -> bz_root_value -> bz_resign_step on the host give the streaks,
    the records and the slots that resign, and the engine's play does exactly that"""
    L = _lib.lib()
    B, na = eng.B, eng.na
    streak = np.zeros((B, 2), np.int64)
    side, move, qrec = np.zeros(B, np.int8), np.zeros(B, np.int32), np.zeros(B, np.float32)
    resigned, made = np.zeros(B, bool), np.zeros(B, np.int64)
    out = np.array([L.bz_resign_playout(int(eng.cfg.seed), int(eng.cfg.game_id_base) + g, rs.playout_q) for g in range(B)], bool)
    eng.reset_games()
    for ply in range(max_plies):
        _, _, tm, st0 = eng.positions()
        if ply == 0:
            own0, opp0, _, _ = eng.positions()
            made[:] = [bin(int(a | b)).count("1") - (4 if eng.size > 3 else 0) for a, b in zip(own0, opp0)]
        (_step_search if step_api else type(eng).search)(eng)
        N, W, _ = eng.root_stats()
        budgets = eng.budgets() if eng.playout_cap is not None else np.full(B, eng.sims)
        quit_now = np.zeros(B, bool)
        for g in np.nonzero(st0 == 0)[0]:
            if budgets[g] < eng.sims:
                continue
            q = C.c_float()
            _lib.check(L.bz_root_value(np.ascontiguousarray(N[g]).ctypes.data, np.ascontiguousarray(W[g]).ctypes.data, na, C.byref(q)))
            s = C.c_int32()
            k = 0 if tm[g] == 1 else 1
            fire = L.bz_resign_step(q, C.c_float(rs.threshold), rs.consecutive, int(streak[g, k]), C.byref(s))
            streak[g, k] = s.value
            if fire and side[g] == 0:
                side[g], move[g], qrec[g] = tm[g], made[g], q.value
            quit_now[g] = bool(fire) and not out[g]
        eng.play(False)
        own1, opp1, _, st1 = eng.positions()
        winners, lens = eng.winners()
        for g in np.nonzero(st0 == 0)[0]:
            if quit_now[g]:  # the engine's play ended exactly these games, for the other side
                resigned[g] = True
                assert st1[g] == 1 and winners[0, g] == -tm[g] and lens[0, g] >= 0, (ply, g)
        made[:] = [bin(int(a | b)).count("1") - (4 if eng.size > 3 else 0) for a, b in zip(own1, opp1)]
        if eng.status()[0] == 0:
            break
    rs_, rm, rq, ro = eng.resign_rows()
    assert np.array_equal(ro[0], out) and np.array_equal(rs_[0], side), (rs_[0], side)
    has = side != 0
    assert np.array_equal(rm[0][has], move[has]) and np.array_equal(_bits(rq[0][has]), _bits(qrec[has]))
    assert not (resigned & out).any() and np.array_equal(resigned, has & ~out)
    assert np.array_equal(_streaks(eng)[0], streak.astype(np.uint8))
    return side, out, resigned


@pytest.mark.parametrize("mode", ["k8", "reuse", "gumbel", "gumbel_interior", "forced_cap", "fpu", "solver", "net_bf16"])
def test_the_record_is_the_host_rule_on_root_stats_taken_before_play(mode):
    kw = {"k8": dict(leaves_per_step=8), "reuse": dict(reuse_subtree=True, **NOISE), "gumbel": dict(gumbel=GumbelConfig(8)),
          "gumbel_interior": dict(gumbel=GumbelConfig(8, interior="gumbel")),
          "forced_cap": dict(forced_playouts=ForcedPlayouts(2.0), playout_cap=PlayoutCap(6, 0.5), **NOISE), "fpu": dict(fpu=Fpu(), **NOISE),
          "solver": dict(solver=True), "net_bf16": {}}[mode]
    if mode == "net_bf16":  # the 64 x 2 bf16 net in the loop (an untrained net's values are small: the threshold sits at 0)
        from test_gpu_search_net import _dn, _net
        P, _ = _net("bf16", 64, 2)
        kw, rs = dict(net=_dn(P, 8)), _rs(16384, threshold=0.0)
    else:
        rs = _rs(16384)
    n, sims = (8, 16) if mode == "net_bf16" else (12, 24)
    eng = SelfPlayEngine("reversi6", n, sims, "net_bf16" if mode == "net_bf16" else "hash", temp_moves=4, seed=1, resign=rs, **kw)
    side, out, resigned = _host_rule_case(eng, rs, step_api=mode in ("k8", "net_bf16"))
    assert (side != 0).any(), "no side fires in this case"
    if mode != "net_bf16":
        assert resigned.any()


# ---------------------------------------------------------------- 5. composition against the twins
def test_under_the_cap_only_full_searches_touch_the_streaks():
    game, gid, seed, sims, fast = FAST_DECIDES
    _case(game, 0, base_cls=CapTwin, args=(fast, 32768), engine_kw=dict(playout_cap=PlayoutCap(fast, 0.5)), n=8, sims=sims, seed=seed,
          base=0, temp_moves=2, stagger=0, noise=False, some_stay=True)  # (gids 0 .. 7: the game is among them)
    tw = _twin(CapTwin, game, gid, sims, 2, 0, seed, args=(fast, 32768))
    _applied(tw, gid, seed, 0)
    right = (tw.resigned, tw.record)
    tw.apply(gid, seed, fast_counts=True)
    assert right != (tw.resigned, tw.record)  # the game the engine has just agreed on is one the wrong rule ends differently


def test_forced_playouts_under_the_cap_equal_the_twin():
    _case("reversi6", 16384, base_cls=ForcedTwin, args=(2.0,), twin_kw=dict(cap=(6, 32768)),
          engine_kw=dict(forced_playouts=ForcedPlayouts(2.0), playout_cap=PlayoutCap(6, 0.5)), n=8, stagger=0, noise=True, some_stay=False)


def test_gumbel_root_search_equals_the_twin():
    _case("reversi6", 16384, base_cls=GumbelTwin, twin_kw=dict(m=8), engine_kw=dict(gumbel=GumbelConfig(8)), n=8, stagger=0, some_stay=False)


def test_eight_leaves_per_step_equal_the_twin():
    _case("reversi4", 16384, base_cls=KTwin, twin_kw=dict(leaves=8), engine_kw=dict(leaves_per_step=8), noise=False)


def test_the_solver_under_the_cap_equals_the_twin():
    _case("reversi4", 16384, base_cls=SolverTwin, twin_kw=dict(cap=(4, 32768)), engine_kw=dict(solver=True, playout_cap=PlayoutCap(4, 0.5)),
          sims=32, some_stay=False)


def test_surprise_and_search_value_of_the_rows_that_exist_are_those_without_resignation():
    c = CASES["reversi"]
    kw = dict(temp_moves=c["temp_moves"], openings=c["openings"], seed=c["seed"], game_id_base=c["base"], surprise=True, search_value=True, **NOISE)
    a = SelfPlayEngine("reversi", c["n"], c["sims"], "hash", resign=_rs(16384), **kw)
    b = SelfPlayEngine("reversi", c["n"], c["sims"], "hash", **kw)
    a.run_iteration(); b.run_iteration()
    a.status(); b.status()
    xa, xb = a.examples(), b.examples()
    (_, la), (_, lb) = a.winners(), b.winners()
    side, _, _, out = a.resign_rows()
    cut = (side[0] != 0) & ~out[0]
    assert cut.any() and (la[0][cut] < lb[0][cut]).all() and np.array_equal(la[0][~cut], lb[0][~cut])
    assert len(xa) == int(la.sum()) < len(xb) == int(lb.sum())  # no row beyond ex_len is packed
    for g in range(c["n"]):
        ma, mb = xa.game == c["base"] + g, xb.game == c["base"] + g
        k = int(ma.sum())
        assert k == la[0, g]
        for f in ("kl", "q", "pi"):
            assert np.array_equal(_bits(getattr(xa, f)[ma]), _bits(getattr(xb, f)[mb][:k])), (g, f)
        for f in ("own", "opp", "mover", "act"):
            assert np.array_equal(getattr(xa, f)[ma], getattr(xb, f)[mb][:k]), (g, f)


# ---------------------------------------------------------------- 6. two pipelines
def test_two_pipelines_report_in_global_order_and_pack_the_finished_games():
    c = CASES["reversi"]
    kw = dict(temp_moves=c["temp_moves"], openings=c["openings"], seed=c["seed"], game_id_base=c["base"], resign=_rs(16384), **NOISE)
    sp = PipelinedSelfPlay("reversi", c["n"], c["sims"], "hash", pipelines=2, **kw)
    one = SelfPlayEngine("reversi", c["n"], c["sims"], "hash", **kw)
    sp.run_iteration(); one.run_iteration()
    assert sp.status()[0] == 0 and one.status()[0] == 0
    ra, rb = sp.resign_rows(), one.resign_rows()
    has = rb[0] != 0
    assert has.any() and not has.all()
    for x, y in zip(ra, rb):
        assert x.shape == (1, c["n"]) and np.array_equal(np.where(has, x, 0), np.where(has, y, 0))
    assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[3], rb[3])
    parts = [e.resign_stats() for e in sp.engines]
    tot = sp.resign_stats()
    for k in ("n_finished", "n_resigned", "n_played_out", "n_would_resign", "n_false_positive"):
        assert tot[k] == sum(p[k] for p in parts) == one.resign_stats()[k], k
    assert tot["n_resigned"] > 0 and tot["n_finished"] == c["n"]
    (wa, la), (wb, lb) = sp.winners(), one.winners()
    assert np.array_equal(wa, wb) and np.array_equal(la, lb)
    blk = sp.pack_examples()
    h = packed_block_header(blk)
    assert h["n_games"] == c["n"] and h["n_rows"] == int(lb.sum()) and h["dropped_rows"] == 0, h  # resigned games included
    px, ox = unpack_packed_block(blk), one.examples()
    for f in ("own", "opp", "z", "mover", "act", "game", "ply"):
        assert np.array_equal(getattr(px, f), getattr(ox, f)), f
    assert np.array_equal(_bits(px.pi), _bits(ox.pi))


# ---------------------------------------------------------------- 7. the setter
def test_loosening_the_threshold_mid_game_keeps_the_records_already_written():
    kw = dict(temp_moves=3, seed=1)
    eng = SelfPlayEngine("reversi4", 8, 16, "hash", resign=_rs(65536), **kw)
    eng.reset_games()
    before = None
    for ply in range(40):
        eng.search(); eng.play(False)
        side, move, q, _ = eng.resign_rows()
        if before is None and (side != 0).sum() >= 2:
            before = (side.copy(), move.copy(), q.copy())
            eng.set_resign(_rs(65536, threshold=0.9, consecutive=1))  # from now on nearly every search fires
        if eng.status()[0] == 0:
            break
    assert before is not None
    side, move, q, _ = eng.resign_rows()
    had = before[0] != 0
    assert np.array_equal(side[had], before[0][had]) and np.array_equal(move[had], before[1][had]) and np.array_equal(_bits(q[had]), _bits(before[2][had]))
    assert (side != 0).sum() > had.sum() and (move[~had & (side != 0)] > before[1][had].min()).all()  # the later records came with the new rule


def test_switching_it_off_restores_the_engine_without_it_and_off_is_off():
    kw = dict(temp_moves=4, openings=1, seed=2)
    a = SelfPlayEngine("reversi", 8, 16, "hash", resign=_rs(0), **kw)
    a.set_resign(None)
    with pytest.raises(RuntimeError, match="resign"):
        a.resign_rows()
    b = SelfPlayEngine("reversi", 8, 16, "hash", resign=None, **kw)
    c = SelfPlayEngine("reversi", 8, 16, "hash", **kw)
    blocks = []
    for e in (a, b, c):
        e.reset_counters(); e.run_iteration(); e.status()
        blocks.append((_raw(e), e.counters()))
    assert np.array_equal(blocks[0][0], blocks[2][0]) and np.array_equal(blocks[1][0], blocks[2][0])
    assert blocks[0][1] == blocks[1][1] == blocks[2][1]
    assert "resign" not in b._buffers and "resign" not in c._buffers  # no buffer, no launch


def test_the_setter_refuses_a_small_buffer_and_ownership_in_either_order():
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros(1 << 14, dtype=torch.uint8, device="cuda:0")
    p = buf.data_ptr() + ((-buf.data_ptr()) & 255)
    eng = SelfPlayEngine("reversi", 4, 16, "hash")
    need = L.bz_engine_resign_bytes(C.byref(eng.cfg))
    assert L.bz_engine_set_resign(eng.h, C.c_float(-0.9), 2, 0, p, need - 1, st) == _lib.BZ_EINVAL
    assert b"bz_engine_set_resign" in L.bz_last_error() and b"too small" in L.bz_last_error()
    assert L.bz_engine_resign_rows(eng.h, p, p, p, p, st) == _lib.BZ_EINVAL and b"is off" in L.bz_last_error()
    assert L.bz_engine_set_resign(eng.h, C.c_float(-0.9), 2, 0, p, need, st) == _lib.BZ_OK
    obuf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda:0")
    op = obuf.data_ptr() + ((-obuf.data_ptr()) & 255)
    assert L.bz_engine_set_ownership(eng.h, op, 1 << 15, st) == _lib.BZ_EINVAL  # resignation is on
    assert b"bz_engine_set_ownership" in L.bz_last_error() and b"resign" in L.bz_last_error()
    assert L.bz_engine_set_resign(eng.h, C.c_float(0), 0, 0, None, 0, st) == _lib.BZ_OK  # off needs no buffer and no rule
    assert L.bz_engine_set_ownership(eng.h, op, 1 << 15, st) == _lib.BZ_OK
    assert L.bz_engine_set_resign(eng.h, C.c_float(-0.9), 2, 0, p, need, st) == _lib.BZ_EINVAL  # ownership is on
    assert b"bz_engine_set_resign" in L.bz_last_error() and b"ownership" in L.bz_last_error()
    torch.cuda.synchronize()
