"""Proven wins, losses and draws on the GPU: k_solve_step / k_solve_cap_step, the proof pass behind their backup,
k_solve_play / k_solve_cap_play, the solver branch of k_root_policy and the reader kernel against the solver twin of
tests/test_solver_cpu.py.  "Equal" = bit for bit: root N / W / P, the proof state of every root edge and of the root, the two
counts, the played move, and in self-play every row, winner and length.  Every proof the engine reports on the tic-tac-toe and
4x4 sets is also held to the negamax value directly."""
import ctypes as C

import numpy as np
import pytest
import torch

import betazero_amd as bz
from betazero_amd import _lib
from betazero_amd.engine import PlayoutCap, SelfPlayEngine
from betazero_amd.match import MatchPlayer, play_match
from oracle.py_twin import Twin
from test_gpu_playout_cap import _bits, _run, _same_rows
from test_solver_cpu import (S_COMPLETE, SolverTwin, boards, forced_win_fixtures, negamax, rev4_positions, rev4_roots, ttt5_roots,
                             ttt_positions)

pytestmark = pytest.mark.gpu
NOISE = dict(dirichlet_alpha=0.3, dirichlet_eps=0.25)


def _search_roots(game, positions, sims, ev, tw=None, **kw):
    """one search of every position (set_roots + search) -> (engine, N, W, P, action, (root, edges, counts))"""
    tw = tw or Twin(game, "uniform", boards=boards())
    eng = SelfPlayEngine(game, len(positions), sims, ev, solver=True, **kw)
    bits = [tw.bits(b, p) for b, p in positions]
    eng.set_roots([x[0] for x in bits], [x[1] for x in bits], [p for _, p in positions])
    eng.reset_counters()
    eng.search()
    N, W, P = eng.root_stats()
    _, act = eng.root_policy()
    pr = eng.proven()
    eng.status()
    return eng, N, W, P, act, pr


def _equal_twin(roots, tw, N, W, P, act, pr, sims):
    """the engine's searches equal the twin's searched roots in everything the engine reports"""
    proven, edges, counts = pr
    for g, root in enumerate(roots):
        e = root["edges"]
        a = [x["a"] for x in e]
        assert int(N[g].sum()) == sims, g
        assert np.array_equal(N[g, a], np.array([x["N"] for x in e], np.uint32)), (g, N[g, a], [x["N"] for x in e])
        assert np.array_equal(_bits(W[g, a]), _bits([x["W"] for x in e])) and np.array_equal(_bits(P[g, a]), _bits([x["P"] for x in e])), g
        assert [None if v == 2 else int(v) for v in edges[g, a]] == [x.get("c") for x in e], (g, edges[g, a], [x.get("c") for x in e])
        assert int((edges[g] != 2).sum()) == sum(x.get("c") is not None for x in e), g
        assert proven[g] == root["proven"], (g, proven[g], root["proven"])
        assert act[g] == tw.pick(root, False, 0)["a"], g
    assert counts["n_decided"] == sum(r["n_decided"] for r in roots) and counts["n_proven_stops"] == sum(r["n_stops"] for r in roots), counts


def _sound(game, positions, pr):
    """every proof the engine itself reports equals negamax: the root's record, and every decided root edge"""
    tw, memo, n = Twin(game, "uniform", boards=boards()), {}, 0
    proven, edges, _ = pr
    for g, (b, p) in enumerate(positions):
        if proven[g] is not None:
            assert proven[g] == negamax(tw, b, p, memo), g
            n += 1
        for a in np.nonzero(edges[g] != 2)[0]:
            assert int(edges[g, a]) == negamax(tw, tw.play(b, p, int(a)), -p, memo), (g, a)
            n += 1
    return n


# ---------------------------------------------------------------- single searches from given roots
@pytest.mark.parametrize("ev,sims", [("hash", 64), ("uniform", S_COMPLETE)])
def test_tictactoe_endgames_equal_the_twin_and_every_reported_proof_is_the_negamax_value(ev, sims):
    pos = ttt_positions(5)
    tw, roots = ttt5_roots(ev, sims)
    eng, N, W, P, act, pr = _search_roots("ttt", pos, sims, ev)
    _equal_twin(roots, tw, N, W, P, act, pr, sims)
    assert _sound("ttt", pos, pr) > len(pos)
    und = sum(v is None for v in pr[0])
    assert und == (0 if ev == "uniform" else 355), und  # (tests/test_solver_cpu.py: the hash evaluator leaves 355 of 3430 at 64)
    assert pr[2]["n_proven_stops"] > 0


@pytest.mark.parametrize("ev", ["uniform", "hash"])
def test_reversi4_positions_equal_the_twin_and_every_reported_proof_is_the_negamax_value(ev):
    pos = rev4_positions()
    tw, roots = rev4_roots(ev, 128)
    eng, N, W, P, act, pr = _search_roots("reversi4", pos, 128, ev)
    _equal_twin(roots, tw, N, W, P, act, pr, 128)
    assert _sound("reversi4", pos, pr) > 64 and tw.n_pass_proofs > 0


def test_tictactoe_from_three_stones_walks_deeper_than_the_lane_group_and_equals_the_twin():
    """walks of up to six plies on the four-lane group: path entries beyond the registers, proofs through them"""
    pos = [x for x in ttt_positions(3) if int((x[0].board != 0).sum()) == 3][::4]
    tw = SolverTwin("ttt", "hash", boards=boards())
    roots = [tw.search(b, p, 96) for b, p in pos]
    assert tw.max_depth > 4
    eng, N, W, P, act, pr = _search_roots("ttt", pos, 96, "hash")
    _equal_twin(roots, tw, N, W, P, act, pr, 96)
    assert _sound("ttt", pos, pr) > 0


# ---------------------------------------------------------------- self-play: noise, the cap, every row
def test_selfplay_reversi6_with_noise_and_the_cap_equals_the_twin_to_the_end_of_the_games():
    n, sims, cap, tm, seed, base = 32, 64, (16, 32768), 6, 4, 11
    eng = SelfPlayEngine("reversi6", n, sims, "hash", solver=True, playout_cap=PlayoutCap(cap[0], cap[1] / 65536), temp_moves=tm, seed=seed,
                         game_id_base=base, **NOISE)
    twins = []
    for g in range(n):
        tw = SolverTwin("reversi6", "hash", cap=cap, dir_alpha=0.3, dir_eps=0.25, boards=boards())
        rows, w, _ = tw.selfplay(base + g, sims, tm, 0, seed, slot=g)
        twins.append((tw, rows, w))
    eng.reset_counters()
    eng.reset_games()
    step = decided = avoided = 0
    while True:
        eng.search()
        want = [tw.budgets[step] if step < len(tw.budgets) else 0 for tw, _, _ in twins]
        assert np.array_equal(eng.budgets(), np.array(want, np.uint32)), step
        N, W, P = eng.root_stats()
        pi, act = eng.root_policy()
        proven, edges, counts = eng.proven()
        nd = ns = 0
        for g, (tw, _, _) in enumerate(twins):
            if step >= len(tw.log):
                assert act[g] == -1 and proven[g] is None and (edges[g] == 2).all(), (step, g)
                continue
            lg = tw.log[step]
            a = lg["a"]
            assert np.array_equal(N[g, a], np.array(lg["N"], np.uint32)) and int(N[g].sum()) == lg["budget"], (step, g)
            assert np.array_equal(_bits(W[g, a]), _bits(lg["W"])) and np.array_equal(_bits(P[g, a]), _bits(lg["P"])), (step, g)
            assert [None if v == 2 else int(v) for v in edges[g, a]] == lg["c"] and proven[g] == lg["proven"], (step, g)
            assert act[g] == lg["act"] and np.array_equal(_bits(pi[g]), _bits(lg["pi"])), (step, g)
            nd, ns = nd + lg["n_decided"], ns + lg["n_stops"]
            decided += lg["proven"] is not None
            avoided += lg["act"] != a[int(np.argmax(lg["N"]))]
        assert counts == {"n_decided": nd, "n_proven_stops": ns}, (step, counts, nd, ns)
        eng.play(False)
        step += 1
        if eng.status()[0] == 0:
            break
        assert step < 100
    ex = eng.examples()
    winners, lens = eng.winners()
    for g, (tw, rows, w) in enumerate(twins):
        assert lens[0, g] == len(rows) and winners[0, g] == w, g
        _same_rows(ex, base + g, rows, w)
    assert len(ex) == sum(len(r) for _, r, _ in twins) and decided > 0
    assert {b for tw, _, _ in twins for b in tw.budgets} == {sims, cap[0]}


# ---------------------------------------------------------------- the net in the loop and every evaluation-cache mode
def _late_roots(n=32, min_stones=52, seed=7):
    tw = Twin("reversi", "uniform", boards=boards())
    rng = np.random.default_rng(seed)
    out, seen = [], set()
    while len(out) < n:
        b, p = bz.ReversiBoard(size=8), 1
        while not tw.terminal(b)[0]:
            mv = tw.moves(b, p)
            if not mv:
                p = -p
                continue
            x, o = tw.bits(b, 1)
            k = (x, o, p)
            if bin(x | o).count("1") >= min_stones and k not in seen and len(out) < n and rng.random() < 0.4:
                seen.add(k)
                out.append((b, p))
            b, p = tw.play(b, p, mv[int(rng.integers(len(mv)))]), -p
    return out


def test_reversi8_late_positions_with_the_bf16_net_equal_the_twin_in_every_cache_mode():
    from test_gpu_search_net import _dn, _net
    from test_search_net_cpu import oracle_eval_fn
    Pn, on = _net("bf16", 64, 2)
    pos = _late_roots()
    assert len(pos) == 32 and min(bin(b.bits(1)[0] | b.bits(1)[1]).count("1") for b, _ in pos) >= 52
    tw = SolverTwin("reversi", "net", eval_fn=oracle_eval_fn(on, "bf16"), boards=boards())
    roots = [tw.search(b, p, 200) for b, p in pos]
    assert sum(r["proven"] is not None for r in roots) > 0
    evals = []
    for cache in (True, "search", False):
        eng, N, W, P, act, pr = _search_roots("reversi", pos, 200, "net_bf16", tw=tw, net=_dn(Pn, 32), eval_cache=cache)
        _equal_twin(roots, tw, N, W, P, act, pr, 200)
        cnt = eng.counters()
        evals.append(cnt["n_net_leaves"] + cnt["n_cache_hits"])
        assert (cnt["n_cache_hits"] > 0) == (cache is not False), (cache, cnt)
    assert evals[0] == evals[1] == evals[2] == tw.n_evals, (evals, tw.n_evals)


# ---------------------------------------------------------------- off is off
def test_switching_the_solver_on_and_off_again_gives_the_arrays_of_an_engine_that_never_had_it():
    kw = dict(temp_moves=4, seed=2, **NOISE)
    eng = SelfPlayEngine("reversi4", 16, 48, "hash", solver=True, **kw)
    on1, (w1, _), _ = _run(eng)
    eng.set_solver(False)
    a, (wa, la), ca = _run(eng)
    b, (wb, lb), cb = _run(SelfPlayEngine("reversi4", 16, 48, "hash", **kw))
    assert np.array_equal(wa, wb) and np.array_equal(la, lb) and ca == cb
    for f in ("own", "opp", "z", "mover", "act", "game", "ply"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert np.array_equal(_bits(a.pi), _bits(b.pi))
    with pytest.raises(RuntimeError, match="solver is off"):
        eng.proven()
    eng.set_solver(True)  # ... and on again: the first run's games, which are not the plain engine's
    c, (wc, _), _ = _run(eng)
    assert np.array_equal(wc, w1) and np.array_equal(c.act, on1.act) and np.array_equal(_bits(c.pi), _bits(on1.pi))
    assert c.pi.shape != a.pi.shape or not np.array_equal(_bits(c.pi), _bits(a.pi))
    # without noise or the cap the plain engine runs the fused search; the solver's option leaves that path alone too
    e2 = SelfPlayEngine("ttt", 8, 32, "hash", solver=True)
    e2.set_solver(False)
    x, (wx, _), cx = _run(e2)
    y, (wy, _), cy = _run(SelfPlayEngine("ttt", 8, 32, "hash"))
    assert np.array_equal(wx, wy) and np.array_equal(x.act, y.act) and np.array_equal(_bits(x.pi), _bits(y.pi)) and cx == cy


def test_set_solver_refuses_the_refused_combinations_and_bad_arguments():
    from betazero_amd.engine import ForcedPlayouts, Fpu
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda:0")
    p = buf.data_ptr() + ((-buf.data_ptr()) & 255)
    on = lambda e, ptr=p, nb=4096: L.bz_engine_set_solver(e.h, 1, ptr, nb, st)  # noqa: E731
    for kw, word in (({"leaves_per_step": 2}, b"leaves_per_step"), ({"reuse_subtree": True}, b"subtree reuse"), ({"gumbel": True}, b"Gumbel"),
                     ({"forced_playouts": ForcedPlayouts(2.0)}, b"forced playouts"), ({"fpu": Fpu()}, b"first-play urgency")):
        eng = SelfPlayEngine("reversi", 4, 16, "hash", **kw)
        assert on(eng) == _lib.BZ_EINVAL
        assert word in L.bz_last_error() and b"solver" in L.bz_last_error(), L.bz_last_error()
        assert L.bz_engine_set_solver(eng.h, 0, None, 0, st) == _lib.BZ_OK  # "off" is always accepted
    eng = SelfPlayEngine("reversi", 4, 16, "hash", playout_cap=PlayoutCap(4, 0.25), **NOISE)  # all allowed
    assert on(eng, ptr=None) == _lib.BZ_EINVAL and on(eng, ptr=p + 4) == _lib.BZ_EINVAL and b"aligned" in L.bz_last_error()
    assert on(eng, nb=8) == _lib.BZ_ENOMEM and b"too small" in L.bz_last_error()
    assert on(eng) == _lib.BZ_OK
    # with the solver on the other setters refuse
    gbuf = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda:0")
    eng = SelfPlayEngine("reversi", 4, 16, "hash", solver=True)  # (Gumbel root search refuses the noise first)
    assert L.bz_engine_set_gumbel(eng.h, 16, 1.0, 50.0, 0.1, gbuf.data_ptr(), gbuf.numel(), st) == _lib.BZ_EINVAL and b"solver" in L.bz_last_error()
    assert L.bz_engine_set_forced_playouts(eng.h, 2.0, 1, st) == _lib.BZ_EINVAL and b"solver" in L.bz_last_error()
    assert L.bz_engine_set_fpu(eng.h, 1, C.c_float(0.2), C.c_float(0.1), p, 4096, st) == _lib.BZ_EINVAL and b"solver" in L.bz_last_error()
    torch.cuda.synchronize()


# ---------------------------------------------------------------- matches and players
def test_the_same_solver_player_on_both_sides_scores_exactly_half():
    p = MatchPlayer(sims=48, evaluator="hash", solver=True)
    res = play_match("reversi", 16, p, p, size=4, opening_plies=2, seed=5)
    assert res.summary()["score"] == 0.5 and not res.pair_score.any()
    plain = play_match("reversi", 16, MatchPlayer(sims=48, evaluator="hash"), MatchPlayer(sims=48, evaluator="hash"), size=4,
                       opening_plies=2, seed=5)
    assert not np.array_equal(plain.actions, res.actions)  # the solver's moves are in it


def test_mcts_player_with_the_solver_plays_the_lowest_forced_win_that_plain_argmax_n_does_not_play():
    fx = forced_win_fixtures()
    assert len(fx) >= 1
    for b, p, win in fx:
        sv = bz.MCTSPlayer(p, sims=32, evaluator="hash", solver=True)
        pl = bz.MCTSPlayer(p, sims=32, evaluator="hash")
        assert sv.get_move(b) == (win // 3, win % 3) and sv.last_proven == 1, (b.board, p, win)
        assert pl.get_move(b) != (win // 3, win % 3), (b.board, p, win)
        assert int(sv.last_visits.sum()) == 32


def test_arena_with_the_solver_plays_its_games_to_the_end():
    from betazero_amd.arena import play_arena
    s = play_arena("ttt", 16, 64, evaluator="uniform", solver=True, opening_plies=1, seed=1).summary()
    assert s["games"] == 16 and s["wins"] + s["draws"] + s["losses"] == 16, s
