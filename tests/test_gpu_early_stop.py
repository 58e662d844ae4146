"""Exact early stop on the GPU: k_stop_step / k_fpu_stop_step against the stop twin of
tests/test_early_stop_cpu.py, bit for bit (stopped(), root N / W / P, pi, the move); the engine against a plain engine driven
simulation by simulation through the step API with a bf16 net in the loop; edge shapes of the root; matches and arenas that are
the same matches with fewer simulations; host exit and run-ahead that change nothing; switching and the live refusals."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import betazero_amd as bz
from betazero_amd import _lib
from betazero_amd.engine import EarlyStop, Fpu, PlayoutCap, SelfPlayEngine
from betazero_amd.match import MatchPlayer, play_match
from oracle.py_twin import f32, rng_draw
from test_early_stop_cpu import Enough, StopTwin, boards, c_decided, decided, stop_twin
from test_fpu_cpu import FpuTwin

pytestmark = pytest.mark.gpu
GW = {"ttt": 4, "reversi": 16}  # lanes per game in the tree kernels (csrc/bz_rules.h)
FPU = (float(np.float32(0.2)), float(np.float32(0.1)))


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _engine(game, n, sims, ev, early_stop=True, **kw):
    return SelfPlayEngine(game, n, sims, ev, early_stop=early_stop, **kw)


# ---------------------------------------------------------------- the twin's games, computed once per process
def _twin_games(game, ev, sims, n, temp_moves=0, openings=0, seed=7, fpu=False, whole=None, plies=6):
    """StopTwins after selfplay(gid) for gid in range(n): whole games for gid < whole (None: all), else the first `plies` searches"""
    return _twin_games_cached(game, ev, sims, n, temp_moves, openings, seed, bool(fpu), n if whole is None else whole, plies)


@functools.lru_cache(maxsize=None)
def _twin_games_cached(game, ev, sims, n, temp_moves, openings, seed, fpu, whole, plies):
    out = []
    for gid in range(n):
        tw = stop_twin(FpuTwin)(game, ev, FPU, boards=boards()) if fpu else StopTwin(game, ev, boards=boards())
        if gid >= whole:
            tw.max_searches = plies
        try:
            tw.selfplay(gid, sims, temp_moves, openings, seed)
        except Enough:
            pass
        out.append(tw)
    return out


def _twin_move(rec, seed, gid, temp_moves):
    """the edge index DESIGN.md 3.7 plays from the record's visits"""
    N = rec["N"]
    if rec["made"] < temp_moves:
        r, cum = rng_draw(seed, gid, rec["made"]) % sum(N), 0
        for i, n in enumerate(N):
            cum += n
            if cum > r:
                return i
    return N.index(max(N))


def _assert_slot(g, rec, stopped, N, W, P, pi, act, move_idx, what):
    a, s = rec["a"], rec["stop_at"]
    assert stopped[g] == s, (what, g, int(stopped[g]), s)
    assert np.array_equal(N[g, a], np.array(rec["N"], np.uint32)) and int(N[g].sum()) == s, (what, g, N[g, a], rec["N"])
    assert np.array_equal(_bits(W[g, a]), _bits(rec["W"])) and np.array_equal(_bits(P[g, a]), _bits(rec["P"])), (what, g)
    want = np.zeros(pi.shape[1], np.float32)
    want[a] = [f32(n) / f32(s) for n in rec["N"]]  # pi = N / stop_at
    assert np.array_equal(_bits(pi[g]), _bits(want)), (what, g)
    assert act[g] == a[move_idx], (what, g, int(act[g]), a[move_idx])


def _results(eng):
    N, W, P = eng.root_stats()
    pi, act = eng.root_policy()
    eng.status()
    return eng.stopped(), N, W, P, pi, act


# ---------------------------------------------------------------- engine = twin
ROOT_CASES = [("ttt", "hash", 64, 64, 16), ("ttt", "uniform", 64, 64, 16), ("reversi", "hash", 48, 16, 1)]


@pytest.mark.parametrize("game,ev,sims,B,whole", ROOT_CASES, ids=[f"{c[0]}-{c[1]}" for c in ROOT_CASES])
def test_one_search_from_positions_along_the_twins_games_equals_the_twin(game, ev, sims, B, whole):
    twins = _twin_games(game, ev, sims, 16 if game == "ttt" else 8, openings=int(game == "reversi"), whole=whole)
    recs = [r for tw in twins[:whole] for r in tw.stops]
    recs = recs[::max(1, len(recs) // B)][:B]
    assert len(recs) == B
    tw0 = twins[0]
    pos = [tw0.bits(r["b"], r["p"]) + (r["p"],) for r in recs]
    eng = _engine(game, B, sims, ev)
    eng.set_roots([p[0] for p in pos], [p[1] for p in pos], [p[2] for p in pos])
    eng.search()
    stopped, N, W, P, pi, act = _results(eng)
    for g, rec in enumerate(recs):
        _assert_slot(g, rec, stopped, N, W, P, pi, act, _twin_move(rec, 0, 0, 0), (game, ev))
    assert 2 * int((stopped < sims).sum()) >= B or ev == "uniform"   # not vacuous: the twin's share (ISSUE: 100 % / 86 % with hash)
    assert (stopped < sims).any() and len({len(r["a"]) for r in recs}) > 2


def _six_plies(game, ev, sims, B, temp_moves=0, openings=0, fpu=False, whole=None, **kw):
    twins = _twin_games(game, ev, sims, B, temp_moves, openings, 7, fpu, whole)
    eng = _engine(game, B, sims, ev, fpu=Fpu(*FPU) if fpu else None, temp_moves=temp_moves, openings=openings, seed=7, **kw)
    eng.reset_counters()
    eng.reset_games()
    n_early = n_sims = 0
    for step in range(6):
        eng.search()
        stopped, N, W, P, pi, act = _results(eng)
        for g, tw in enumerate(twins):
            if step >= len(tw.stops):  # the game is over: the slot sits the search out
                assert stopped[g] == 0 and act[g] == -1 and not pi[g].any(), (step, g)
                continue
            rec = tw.stops[step]
            _assert_slot(g, rec, stopped, N, W, P, pi, act, _twin_move(rec, 7, g, temp_moves), (game, ev, step))
            if rec["made"] < temp_moves:
                assert stopped[g] == sims
            n_early += rec["stop_at"] < sims
            n_sims += rec["stop_at"]
        eng.play(False)
    assert n_early > 0 and eng.counters()["n_sims"] == n_sims  # every walk the twin made, and no other
    return eng, twins


def test_six_plies_of_selfplay_equal_the_twin_tictactoe():
    _six_plies("ttt", "hash", 64, 16)


def test_six_plies_of_selfplay_equal_the_twin_reversi8_with_openings():
    _six_plies("reversi", "hash", 48, 8, openings=1, whole=1)


def test_six_plies_with_fpu_equal_the_stop_twin_over_the_fpu_twin():
    """(k_fpu_stop_step)"""
    _six_plies("ttt", "hash", 64, 16, fpu=True)


def test_six_plies_with_temp_moves_2_run_the_sampled_searches_whole():
    _, twins = _six_plies("ttt", "hash", 64, 16, temp_moves=2)
    assert all(tw.stops[0]["stop_at"] == 64 and tw.stops[1]["stop_at"] == 64 for tw in twins)


# ---------------------------------------------------------------- positions by seeded random play on the host boards
@functools.lru_cache(maxsize=None)
def _random_positions(seed=3, games=24):
    """Reversi 8x8 roots -> [(own, opp, to_move, n_legal)] for the side to move, every position of `games` random games that has a move"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(games):
        b, p = bz.ReversiBoard(size=8), 1
        while not b.is_game_over():
            mv = b.generate_possible_moves(p)
            if not mv:
                p = -p
                continue
            own, opp = b.bits(p)
            out.append((own, opp, p, len(mv)))
            r, c = mv[int(rng.integers(len(mv)))]
            b = b.make_move(r, c, p)
            p = -p
    return out


def _twin_search(own, opp, tm, sims, ev="hash"):
    x, o = (own, opp) if tm == 1 else (opp, own)
    tw = StopTwin("reversi", ev, boards=boards())
    tw.search(bz.ReversiBoard.from_bits(x, o, 8), tm, sims)
    return tw.stops[0]


def test_edge_shapes_one_move_gw_edges_more_than_gw_edges_and_an_idle_slot():
    pos = _random_positions()
    gw = GW["reversi"]
    one = next(p for p in pos if p[3] == 1)
    at_gw = max((p for p in pos if p[3] <= gw and p[3] > 1), key=lambda p: p[3])
    wide = max((p for p in pos if p[3] > gw), key=lambda p: p[3])
    two_chunks_min = next(p for p in pos if p[3] == gw + 1) if any(p[3] == gw + 1 for p in pos) else wide
    assert one[3] == 1 and 1 < at_gw[3] <= gw and wide[3] > gw
    print("edges:", one[3], at_gw[3], two_chunks_min[3], wide[3])
    roots = [one, at_gw, wide, (0, 0, 0, 0), two_chunks_min, one, wide, at_gw]
    sims = 64
    eng = _engine("reversi", len(roots), sims, "hash")
    eng.set_roots([r[0] for r in roots], [r[1] for r in roots], [r[2] for r in roots])
    eng.search()
    stopped, N, W, P, pi, act = _results(eng)
    for g, (own, opp, tm, nl) in enumerate(roots):
        if tm == 0:  # idle
            assert stopped[g] == 0 and act[g] == -1 and not N[g].any() and not pi[g].any()
            continue
        rec = _twin_search(own, opp, tm, sims)
        assert len(rec["a"]) == nl
        _assert_slot(g, rec, stopped, N, W, P, pi, act, rec["N"].index(max(rec["N"])), ("shape", nl))
        if nl == 1:
            assert stopped[g] == 1 and pi[g, rec["a"][0]] == 1.0 and int(N[g].sum()) == 1
    assert (stopped[[1, 2, 4]] < sims).any()


# ---------------------------------------------------------------- engine against itself, a bf16 net in the loop
@functools.lru_cache(maxsize=None)
def _bf16_net(max_batch=32):
    from betazero_amd.net import DeviceNet, PolicyValueNet
    torch.manual_seed(25)
    return DeviceNet.from_module(PolicyValueNet(64, 2, 64).round_to_bf16_(), max_batch)


def _net_roots(B):
    pos = _random_positions()
    picks = pos[3::max(1, len(pos) // B)][:B - 1] + [next(p for p in pos if p[3] == 1)]
    assert len(picks) == B
    return [p[0] for p in picks], [p[1] for p in picks], [p[2] for p in picks]


@pytest.mark.parametrize("cache,sym", [(True, False), ("search", False), (False, False), (True, True)],
                         ids=["carry", "search", "nocache", "carry-symmetry"])
def test_net_search_stops_exactly_where_the_plain_engines_snapshots_say(cache, sym):
    B, sims = 16, 48
    dn = _bf16_net()
    kw = dict(net=dn, eval_cache=cache, eval_symmetry=True if sym else None, seed=5)
    roots = _net_roots(B)
    plain = _engine("reversi", B, sims, "net_bf16", None, root_store=False, **kw)
    plain.set_roots(*roots)
    plain.root_begin(); plain.evaluate(); plain.expand_backup()
    snaps = [plain.root_stats()[0].copy()]
    for s in range(sims):
        plain.select(s); plain.evaluate(); plain.expand_backup()
        snaps.append(plain.root_stats()[0].copy())  # N after s + 1 simulations
    _, act_plain = plain.root_policy()
    plain.status()
    eng = _engine("reversi", B, sims, "net_bf16", True, **kw)
    eng.reset_counters()
    eng.set_roots(*roots)
    eng.search()
    stopped, N, W, P, pi, act = _results(eng)
    for g in range(B):
        s = int(stopped[g])
        assert 1 <= s <= sims and np.array_equal(N[g], snaps[s][g]), (g, s)
        edges = lambda k: [int(x) for x in snaps[k][g][P[g] > 0]]  # noqa: E731  (the root's edges in ascending action order)
        assert c_decided(edges(s), sims - s) == 1 and decided(edges(s), sims - s)
        for t in range(1, s):
            assert c_decided(edges(t), sims - t) == 0, (g, t)
        assert act[g] == act_plain[g], g
    print("stop_at:", stopped.tolist())
    assert stopped[B - 1] == 1  # (the one-move root: the case holds at least this early stop, whatever the net's priors)
    assert eng.counters()["n_sims"] == int(stopped.sum())


# ---------------------------------------------------------------- a match is the same match
class _Recorder:
    """wraps SelfPlayEngine where a function looks it up, keeping every engine built"""

    def __init__(self):
        self.engines = []

    def __call__(self, *a, **k):
        e = SelfPlayEngine(*a, **k)
        self.engines.append(e)
        return e


def _match(monkeypatch, player, n=32, **kw):
    import betazero_amd.engine as engine_mod
    rec = _Recorder()
    monkeypatch.setattr(engine_mod, "SelfPlayEngine", rec)
    plies = []
    res = play_match("reversi", n, player, player, size=8, opening_plies=4, seed=11, on_ply=lambda engs, go: plies.append((engs, list(go))), **kw)
    monkeypatch.setattr(engine_mod, "SelfPlayEngine", SelfPlayEngine)
    # the measuring hook: once per ply with the match's two engines and the indices of those that searched (none in an opening ply)
    assert len(plies) >= int(res.plies.max()) and all(e == rec.engines and set(g) <= {0, 1} for e, g in plies)
    assert sum(bool(g) for _, g in plies) >= int(res.plies.max()) - 4
    cnt = [e.counters() for e in rec.engines]
    return res, cnt


def _same_match(a, b):
    return (np.array_equal(a.actions, b.actions) and np.array_equal(a.movers, b.movers) and np.array_equal(a.winner, b.winner) and
            np.array_equal(a.plies, b.plies))


@pytest.mark.parametrize("ev", ["hash", "net_bf16"])
def test_a_match_with_early_stop_is_the_same_match_with_fewer_simulations(ev, monkeypatch):
    net = _bf16_net() if ev == "net_bf16" else None
    sims = 64
    off, c_off = _match(monkeypatch, MatchPlayer(sims=sims, evaluator=ev, net=net))
    on, c_on = _match(monkeypatch, MatchPlayer(sims=sims, evaluator=ev, net=net, early_stop=True))
    assert _same_match(on, off) and int(off.plies.sum()) > 0
    for a, b in zip(c_on, c_off):
        assert a["n_sims"] < b["n_sims"], (a, b)
        if net is not None:
            assert a["n_net_leaves"] < b["n_net_leaves"], (a, b)
    print(ev, "simulations on / off:", [(a["n_sims"], b["n_sims"]) for a, b in zip(c_on, c_off)])


def test_host_exit_and_the_run_ahead_change_nothing_in_a_match(monkeypatch):
    runs = [_match(monkeypatch, MatchPlayer(sims=64, evaluator="hash", early_stop=es), **kw)
            for kw, es in ((dict(run_ahead=16), True), (dict(run_ahead=2), True), (dict(run_ahead=16), EarlyStop(host_exit=False)))]
    for other, c in runs[1:]:
        assert _same_match(other, runs[0][0])
        assert [x["n_sims"] for x in c] == [x["n_sims"] for x in runs[0][1]]


def test_an_arena_with_early_stop_is_the_same_arena_with_fewer_simulations(monkeypatch):
    import betazero_amd.arena as arena_mod
    out = {}
    for es in (None, True):
        rec = _Recorder()
        monkeypatch.setattr(arena_mod, "SelfPlayEngine", rec)
        res = arena_mod.play_arena("ttt", 32, 64, evaluator="hash", seed=3, opening_plies=2, early_stop=es)
        monkeypatch.setattr(arena_mod, "SelfPlayEngine", SelfPlayEngine)
        out[es] = (res, rec.engines[0].counters())
    (a, ca), (b, cb) = out[None], out[True]
    assert np.array_equal(a.winner, b.winner) and np.array_equal(a.plies, b.plies) and len(a.moves) == len(b.moves)
    for (xa, xm), (ya, ym) in zip(a.moves, b.moves):
        assert np.array_equal(xa, ya) and np.array_equal(xm, ym)
    assert cb["n_sims"] < ca["n_sims"], (ca, cb)


# ---------------------------------------------------------------- host exit changes nothing
def test_host_exit_on_and_off_give_identical_searches():
    pos = _random_positions()[5::7][:32]
    roots = ([p[0] for p in pos], [p[1] for p in pos], [p[2] for p in pos])
    got = []
    for es in (EarlyStop(host_exit=False), EarlyStop(host_exit=True)):
        eng = _engine("reversi", 32, 64, "hash", es)
        eng.reset_counters()
        eng.set_roots(*roots)
        eng.search()
        got.append(_results(eng) + (eng.counters()["n_sims"],))
        eng.set_roots(*roots)  # ... and a second search on the same engine
        eng.search()
        again = _results(eng)
        assert all(np.array_equal(x, y) for x, y in zip(again, got[-1][:6]))
    for x, y in zip(*got):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    assert (got[0][0] < 64).any()


def test_host_exit_issues_fewer_tree_steps_once_every_slot_has_stopped():
    """a one-move root stops at s = 1: with run_ahead 16 the marks follow steps 7, 15, 23, ..., the third one finds the first
    complete and its count (1) says step 7 was empty -- 24 select launches instead of 64; without host exit all 64"""
    one = next(q for q in _random_positions() if q[3] == 1)
    L = _lib.lib()
    launches = {}
    for he in (False, True):
        eng = _engine("reversi", 1, 64, "hash", EarlyStop(host_exit=he))
        eng.set_roots([one[0]], [one[1]], [one[2]])
        torch.cuda.synchronize()
        L.bz_profile_reset(); L.bz_profile_enable(1)
        try:
            eng.search()
            torch.cuda.synchronize()
            launches[he] = _lib.profile_read()["select"][0]
        finally:
            L.bz_profile_enable(0); L.bz_profile_reset()
        assert eng.stopped()[0] == 1 and int(eng.root_stats()[0].sum()) == 1
    assert launches == {False: 64, True: 24}, launches


def test_mcts_player_stops_at_a_one_move_root_and_plays_the_plain_players_game():
    players = {s: (bz.MCTSPlayer(s, sims=64, evaluator="hash", early_stop=True), bz.MCTSPlayer(s, sims=64, evaluator="hash"))
               for s in (1, -1)}
    b, p, sims_run = bz.TicTacToeBoard(), 1, []
    while not b.is_game_over()[0]:
        on, off = players[p]
        mv = on.get_move(b)
        assert mv == off.get_move(b)
        assert 1 <= on.last_sims <= 64 and int(on.last_visits.sum()) == on.last_sims and off.last_sims is None
        if len(b.generate_possible_moves()) == 1:
            assert on.last_sims == 1 < 64
        sims_run.append(on.last_sims)
        b = b.make_move(mv[0], mv[1], p)
        p = -p
    assert min(sims_run) < 64
    one = next(q for q in _random_positions() if q[3] == 1)  # a Reversi root with one legal move
    x, o = (one[0], one[1]) if one[2] == 1 else (one[1], one[0])
    pl = bz.MCTSPlayer(one[2], sims=48, evaluator="hash", early_stop=True)
    mv = pl.get_move(bz.ReversiBoard.from_bits(x, o, 8))
    assert pl.last_sims == 1 and mv == bz.MCTSPlayer(one[2], sims=48, evaluator="hash").get_move(bz.ReversiBoard.from_bits(x, o, 8))


# ---------------------------------------------------------------- switching and the live refusals
def test_switching_off_restores_the_plain_search_of_the_same_roots_bit_for_bit():
    pos = _random_positions()[2::9][:16]
    roots = ([p[0] for p in pos], [p[1] for p in pos], [p[2] for p in pos])

    def run(eng):
        eng.set_roots(*roots)
        eng.search()
        N, W, P = eng.root_stats()
        pi, act = eng.root_policy()
        eng.status()
        return N, W, P, pi, act
    eng = _engine("reversi", 16, 64, "hash", True)
    on1 = run(eng)
    assert (eng.stopped() < 64).any()
    eng.set_early_stop(None)
    with pytest.raises(RuntimeError, match="early stop is off"):
        eng.stopped()
    off = run(eng)
    plain = run(_engine("reversi", 16, 64, "hash", None))
    for x, y in zip(off, plain):
        assert np.array_equal(_bits(x) if x.dtype == np.float32 else x, _bits(y) if y.dtype == np.float32 else y)
    assert (off[0].sum(1) == 64).all() and not np.array_equal(off[0], on1[0])
    eng.set_early_stop(True)  # ... and on again: the first search's results
    on2 = run(eng)
    for x, y in zip(on1, on2):
        assert np.array_equal(x, y)
    assert np.array_equal(on1[4], plain[4])  # the moves never differ


def test_the_setters_refuse_each_other_on_a_live_engine_in_both_orders():
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros(1 << 22, dtype=torch.uint8, device="cuda:0")
    p, nb = buf.data_ptr() + ((-buf.data_ptr()) & 255), (1 << 22) - 256
    dn = _bf16_net()
    setters = {
        "gumbel": (lambda h: L.bz_engine_set_gumbel(h, 16, 1.0, 50.0, 0.1, p, nb, st), dict(gumbel=True), b"Gumbel"),
        "playout_cap": (lambda h: L.bz_engine_set_playout_cap(h, 4, 16384, p, nb, st), dict(playout_cap=PlayoutCap(4, 0.25)), b"playout cap"),
        "forced_playouts": (lambda h: L.bz_engine_set_forced_playouts(h, 2.0, 1, st), dict(forced_playouts=True), b"forced playouts"),
        "solver": (lambda h: L.bz_engine_set_solver(h, 1, p, nb, st), dict(solver=True), b"solver"),
        "surprise": (lambda h: L.bz_engine_set_surprise(h, p, nb, st), dict(surprise=True), b"surprise"),
        "search_value": (lambda h: L.bz_engine_set_search_value(h, p, nb, st), dict(search_value=True), b"search-value"),
        "ownership": (lambda h: L.bz_engine_set_ownership(h, p, nb, st), dict(ownership=True), b"ownership"),
        "resign": (lambda h: L.bz_engine_set_resign(h, -0.9, 2, 6554, p, nb, st), dict(resign=True), b"resignation"),
        "root_store": (lambda h: L.bz_engine_set_root_store(h, p, nb, 16, 2, st), dict(root_store=(16, 2)), b"root store"),
    }
    ebuf = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    ep = ebuf.data_ptr() + ((-ebuf.data_ptr()) & 255)
    stop_on = lambda h, ptr=ep, n=1024: L.bz_engine_set_early_stop(h, 1, 1, ptr, n, st)  # noqa: E731
    live = _engine("reversi", 4, 16, "net_bf16", True, net=dn)  # early stop on: every refused setter is refused
    for name, (setter, kw, word) in setters.items():
        assert setter(live.h) == _lib.BZ_EINVAL, name
        assert b"early stop" in L.bz_last_error() and word in L.bz_last_error(), (name, L.bz_last_error())
        other = _engine("reversi", 4, 16, "net_bf16", None, net=dn, **{"root_store": False, **kw})  # ... and the other order
        assert stop_on(other.h) == _lib.BZ_EINVAL, name
        assert b"bz_engine_set_early_stop" in L.bz_last_error() and word in L.bz_last_error(), (name, L.bz_last_error())
    for kw, word in ((dict(reuse_subtree=True), b"subtree reuse"), (dict(leaves_per_step=2), b"leaves_per_step")):
        assert stop_on(_engine("reversi", 4, 16, "hash", None, **kw).h) == _lib.BZ_EINVAL and word in L.bz_last_error()
    ok = _engine("reversi", 4, 16, "hash", None, fpu=True, temp_moves=2, dirichlet_alpha=0.3, dirichlet_eps=0.25)  # all accepted
    assert stop_on(ok.h, None) == _lib.BZ_EINVAL and stop_on(ok.h, ep + 4) == _lib.BZ_EINVAL and b"aligned" in L.bz_last_error()
    assert stop_on(ok.h, n=256) == _lib.BZ_ENOMEM and b"too small" in L.bz_last_error()
    assert stop_on(ok.h) == _lib.BZ_OK and L.bz_engine_set_early_stop(ok.h, 0, 0, None, 0, st) == _lib.BZ_OK
    out = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    assert L.bz_engine_stopped(ok.h, out.data_ptr(), st) == _lib.BZ_EINVAL and b"early stop is off" in L.bz_last_error()
    # Python: ValueError naming the other option, both orders
    with pytest.raises(ValueError, match="early stop"):
        live.set_solver(True)
    with pytest.raises(ValueError, match="early stop"):
        live.set_resign(True)
    with pytest.raises(ValueError, match="solver"):
        _engine("reversi", 4, 16, "hash", None, solver=True).set_early_stop(True)
    with pytest.raises(ValueError, match="root_store"):
        _engine("reversi", 4, 16, "net_bf16", None, net=dn).set_early_stop(True)  # (the default engine keeps a root store)
    torch.cuda.synchronize()
