"""Proven wins, losses and draws on the GPU: k_solve_step / k_solve_cap_step, the proof pass behind their backup,
k_solve_play / k_solve_cap_play, the solver branch of k_root_policy and the reader kernel against the solver twin of
tests/test_solver_cpu.py.  "Equal" = bit for bit: root N / W / P, the proof state of every root edge and of the root, the two
counts, the played move, and in self-play every row, winner and length.  Every proof the engine reports on the tic-tac-toe and
4x4 sets is also held to the negamax value directly.  The second half runs self-play with a net in the loop -- every evaluation
cache mode, so that a slot's previous arena and the root store's trees hold proven edges --, the step API, two pipelines and
the observing options against the same twin."""
import ctypes as C

import numpy as np
import pytest
import torch

import betazero_amd as bz
from betazero_amd import _lib
from betazero_amd.engine import PlayoutCap, SelfPlayEngine
from betazero_amd.match import MatchPlayer, play_match
from oracle import py_twin
from oracle.py_twin import Twin
from test_gpu_playout_cap import _bits, _run, _same_rows
from test_solver_cpu import (NET_CAP, NET_CAP_BASE, NET_CASE, OBSERVER_CASE, S_COMPLETE, SolverTwin, boards, exact_bf16_net, forced_win_fixtures, negamax,
                             net_case_store, net_case_twins, observer_case_twins, rev4_positions, rev4_roots, solver_twins, ttt5_roots, ttt_positions,
                             twin_figures)

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


# ---------------------------------------------------------------- self-play with the net in the loop, the step API, observers
def _case(game, n, sims, ev, twins, cap=None, external=None, base=0, noise=False, **kw):
    """n games to the end against their twins, search by search as in the noise-and-cap test above: N, W, P, the proof of every
    root edge and of the root, pi, the action, both counts, under the cap the budgets; then rows, winners, lengths and
    n_sims.  The previous search of a slot is a solver search: what the carry-over cache (and the root store) copy from holds
    proven edges.  Returns (engine, counters, searches with a decided root, decided root edges)."""
    eng = SelfPlayEngine(game, n, sims, "external" if external else ev, solver=True, game_id_base=base,
                         playout_cap=PlayoutCap(cap[0], cap[1] / 65536) if cap else None, **(NOISE if noise else {}), **kw)
    eng.reset_counters()
    eng.reset_games()
    step = roots = edges_dec = 0
    while True:
        if external:
            eng.search_external(external)
        else:
            eng.search()
        if cap:
            want = [tw.budgets[step] if step < len(tw.budgets) else 0 for tw, _, _ in twins]
            assert np.array_equal(eng.budgets(), np.array(want, np.uint32)), step
        N, W, P = eng.root_stats()
        pi, act = eng.root_policy()
        proven, edges, counts = eng.proven()
        nd = ns = 0
        for g, (tw, _, _) in enumerate(twins):
            if step >= len(tw.log):
                assert act[g] == -1 and proven[g] is None and (edges[g] == 2).all() and not pi[g].any(), (step, g)
                continue
            lg = tw.log[step]
            a = lg["a"]
            assert np.array_equal(N[g, a], np.array(lg["N"], np.uint32)) and int(N[g].sum()) == lg["budget"], (step, g, N[g, a], lg["N"])
            assert np.array_equal(_bits(W[g, a]), _bits(lg["W"])) and np.array_equal(_bits(P[g, a]), _bits(lg["P"])), (step, g)
            assert [None if v == 2 else int(v) for v in edges[g, a]] == lg["c"] and proven[g] == lg["proven"], (step, g, edges[g, a], lg["c"])
            assert int((edges[g] != 2).sum()) == sum(c is not None for c in lg["c"]), (step, g)
            assert act[g] == lg["act"] and np.array_equal(_bits(pi[g]), _bits(lg["pi"])), (step, g)
            nd, ns = nd + lg["n_decided"], ns + lg["n_stops"]
            roots += lg["proven"] is not None
            edges_dec += sum(c is not None for c in lg["c"])
        assert counts == {"n_decided": nd, "n_proven_stops": ns}, (step, counts, nd, ns)
        eng.play(False)
        step += 1
        if eng.status()[0] == 0:
            break
        assert step < 200
    ex = eng.examples()
    winners, lens = eng.winners()
    cnt = eng.counters()
    for g, (tw, rows, w) in enumerate(twins):
        assert lens[0, g] == len(rows) and winners[0, g] == w, (g, lens[0, g], len(rows), winners[0, g], w)
        _same_rows(ex, base + g, rows, w)
    assert len(ex) == sum(len(r) for _, r, _ in twins)
    assert cnt["n_sims"] == sum(b for tw, _, _ in twins for b in tw.budgets)
    assert roots > 0 and edges_dec > 0  # the run holds decided roots and decided edges
    return eng, cnt, roots, edges_dec


def _net_case(cache, capped):
    from test_gpu_search_net import _dn
    Pn, _ = exact_bf16_net()
    twins = net_case_twins(capped)
    kw = dict(NET_CASE)
    eng, cnt, _, _ = _case(kw.pop("game"), kw.pop("n"), kw.pop("sims"), "net_bf16", twins, cap=NET_CAP if capped else None, noise=capped,
                           base=NET_CAP_BASE if capped else 0, net=_dn(Pn, NET_CASE["n"]), eval_cache=cache, **kw)
    assert cnt["n_net_leaves"] + cnt["n_cache_hits"] == sum(tw.n_evals for tw, _, _ in twins), cnt
    assert (cnt["n_cache_hits"] > 0) == (cache is not False), cnt
    assert (cnt["n_cache_hits_prev"] > 0) == (cache is True), cnt
    r = eng.root_store_counters()
    print("cache", cache, "capped", capped, cnt, r)
    if cache is True:  # the default engine: the carry-over and the root store copy from trees that hold proven edges
        assert eng.root_store == (256, 3) and r["n_seeded_searches"] > 0 and r["n_seeded_evals"] > 0 and r["n_root_saves"] > 0, r
        assert (r["n_root_saves"], r["n_seeded_searches"]) == net_case_store(capped), r  # ... exactly where the games say it does
    else:
        assert eng.root_store is None and r == {"n_seeded_evals": 0, "n_seeded_searches": 0, "n_root_saves": 0}, r
    return twins


@pytest.mark.parametrize("cache", [False, "search", True])
def test_selfplay_with_the_exact_bf16_net_equals_the_twin_in_every_cache_mode(cache):
    """the search-grade exact bf16 net (tests/test_search_net_cpu.py), the twin's evaluator the oracle's bf16 forward.  From the
    second move on a slot's previous arena is a solver tree: the carry-over re-creates its nodes from edges that carry proofs,
    and the staggered pool brings roots back that the store holds -- n_net_leaves + n_cache_hits stays the twin's evaluation
    count in every mode"""
    twins = _net_case(cache, False)
    assert {b for tw, _, _ in twins for b in tw.budgets} == {NET_CASE["sims"]}


def test_selfplay_with_the_exact_bf16_net_under_the_cap_with_noise_equals_the_twin():
    twins = _net_case(True, True)
    assert {b for tw, _, _ in twins for b in tw.budgets} == {NET_CASE["sims"], NET_CAP[0]}


def test_net_f32_selfplay_equals_the_twin_with_the_per_position_forward():
    from test_gpu_leaf_parallel import _net32, _net_fn
    dn = _net32()
    kw = dict(temp_moves=8, openings=1, seed=3)
    twins = solver_twins("reversi", "net", 4, 16, eval_fn=_net_fn(dn), **kw)
    _case("reversi", 4, 16, "net_f32", twins, net=dn, **kw)


@pytest.mark.parametrize("cap", [None, (8, 32768)], ids=["plain", "cap"])
def test_external_evaluator_through_the_step_api_equals_the_twin(cap):
    """select / expand_backup as separate launches: every proof pass runs in an expand-only step, behind a backup whose walk
    an earlier launch selected"""
    na = 65

    def external(own, opp, kind):
        o = own.cpu().numpy().view(np.uint64)
        q = opp.cpu().numpy().view(np.uint64)
        k = kind.cpu().numpy()
        lg = np.zeros((len(o), na), np.float32)
        v = np.zeros(len(o), np.float32)
        for i in np.nonzero(k == 1)[0]:
            lg[i], v[i] = py_twin.eval_hash(int(o[i]), int(q[i]), na)
        return torch.from_numpy(lg).cuda(), torch.from_numpy(v).cuda()
    kw = dict(temp_moves=3, seed=8)
    twins = solver_twins("reversi4", "hash", 6, 32, cap=cap, noise=True, **kw)
    _case("reversi4", 6, 32, "hash", twins, cap=cap, external=external, noise=True, **kw)
    assert {b for tw, _, _ in twins for b in tw.budgets} == ({32, 8} if cap else {32})
    assert sum(lg["n_stops"] for tw, _, _ in twins for lg in tw.log) > 0


def test_two_pipelines_equal_the_twin():
    from betazero_amd.engine import PipelinedSelfPlay
    n, sims = 12, 32
    kw = dict(temp_moves=4, seed=9)
    sp = PipelinedSelfPlay("reversi4", n, sims, "hash", pipelines=2, solver=True, game_id_base=100, **kw, **NOISE)
    sp.reset_counters()
    sp.run_iteration()
    assert sp.status()[0] == 0
    ex, (winners, lens), cnt = sp.examples(), sp.winners(), sp.counters()
    # the two engines hold slots 0..5 of games 100..105 and 106..111: every draw is keyed by the global game id
    twins = solver_twins("reversi4", "hash", 6, sims, base=100, noise=True, **kw) + \
        solver_twins("reversi4", "hash", 6, sims, base=100, noise=True, slot0=6, **kw)
    for g, (tw, rows, w) in enumerate(twins):
        assert lens[0, g] == len(rows) and winners[0, g] == w, g
        _same_rows(ex, 100 + g, rows, w)
    assert cnt["n_sims"] == sum(b for tw, _, _ in twins for b in tw.budgets) and len(ex) == sum(len(r) for _, r, _ in twins)
    f = twin_figures(twins)
    assert f["decided_roots"] > 0 and f["n_stops"] > 0, f


def test_surprise_search_value_and_ownership_columns_equal_the_twins():
    """q is the value of the RAW visits of its root -- sum W / sum N -- also where the root is decided: a proven win still reads
    what the walks backed up, not +1 (tests/test_solver_cpu.py holds that this case has such rows)"""
    from test_ownership_cpu import ownership_row
    twins = observer_case_twins()
    kw = dict(OBSERVER_CASE)
    eng, _, _, _ = _case(kw.pop("game"), kw.pop("n"), kw.pop("sims"), "hash", twins, noise=True, surprise=True, search_value=True,
                         ownership=True, **kw)
    ex = eng.examples()
    for g, (tw, rows, w) in enumerate(twins):
        msk = ex.game == g
        assert np.array_equal(_bits(ex.kl[msk]), _bits(tw.kl_rows(rows))), g
        assert np.array_equal(_bits(ex.q[msk]), _bits(tw.q_rows(rows))), g
        fx, fo = tw.final_bits()
        want = ownership_row(np.full(len(rows), fx, np.uint64), np.full(len(rows), fo, np.uint64), np.array([r[3] for r in rows]))
        assert np.array_equal(ex.fown[msk], want[0]) and np.array_equal(ex.fopp[msk], want[1]), g
    assert (ex.kl > 0).any() and (ex.q != 0).any() and len(np.unique(ex.fown)) > 1


def test_eval_symmetry_with_the_solver_plays_the_games_of_a_second_identical_engine_and_every_proof_is_the_negamax_value():
    """(the symmetry changes the evaluator, not the rule: pinned product against product, as tests/test_gpu_symmetry.py does;
    a proof does not depend on the evaluator at all, so every reported one is still held to negamax)"""
    from betazero_amd.engine import EvalSymmetry
    from test_gpu_leaf_parallel import _net32
    dn = _net32()
    kw = dict(net=dn, temp_moves=4, seed=6, solver=True)

    def run(**more):
        eng = SelfPlayEngine("reversi4", 8, 32, "net_f32", **kw, **more)
        eng.reset_counters(); eng.reset_games()
        pos, roots, edges, acts = [], [], [], []
        for step in range(64):
            eng.search()
            own, opp, tm, st = eng.positions()
            pr = eng.proven()
            _, act = eng.root_policy()
            for g in np.nonzero(st == 0)[0]:
                x, o = (own[g], opp[g]) if tm[g] == 1 else (opp[g], own[g])
                pos.append((bz.ReversiBoard.from_bits(int(x), int(o), 4), int(tm[g])))
                roots.append(pr[0][g]); edges.append(pr[1][g])
            acts.append(act.copy())
            eng.play(False)
            if eng.status()[0] == 0:
                break
        else:
            raise AssertionError("the games did not end")
        return eng.examples(), eng.winners(), np.array(acts), (pos, roots, np.array(edges))
    a, (wa, la), aa, (pos, roots, edges) = run(eval_symmetry=EvalSymmetry(11))
    b, (wb, lb), ab, _ = run(eval_symmetry=EvalSymmetry(11))
    assert len(a) == len(b) > 0 and np.array_equal(wa, wb) and np.array_equal(la, lb) and np.array_equal(aa, ab)
    assert np.array_equal(a.act, b.act) and np.array_equal(_bits(a.pi), _bits(b.pi)) and np.array_equal(a.own, b.own)
    c, _, ac, _ = run()
    assert c.pi.shape != a.pi.shape or not np.array_equal(_bits(c.pi), _bits(a.pi))  # not the games without the symmetry
    n = _sound("reversi4", pos, (roots, edges, None))
    assert n > 0 and sum(r is not None for r in roots) > 0, n
