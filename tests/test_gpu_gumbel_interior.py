"""Gumbel interior selection on the GPU: k_gfull_step against GumbelFullTwin of
tests/test_gumbel_interior_cpu.py.  "Bit-exact" = root N / W / P, root_policy()'s pi' and move, the work counters, and in
self-play every row, winner and length equal to the twin's.  Shapes: at most 12 games; 8 simulations (fewer than the root has
edges) and 40 (interior nodes reach several visits); Reversi 8x8 (16 lanes per game, passes), Reversi 4x4 (forced-pass one-edge
nodes, early endings), tic-tac-toe (4 lanes: an 8-edge interior node is two chunks).  The cases must hold interior selections
in which the rule took another edge than PUCT would have from the same statistics (GumbelFullTwin.n_changed) -- all but the
uniform evaluator's single Reversi searches: there every value is 0 until a walk meets the end of a game, sigma is 0, p is the
uniform prior, and both rules take the first least-visited edge (counted on the CPU: 0 of them differ)."""
import ctypes as C

import numpy as np
import pytest
import torch

import betazero_amd as bz
from betazero_amd import _lib
from betazero_amd.engine import GumbelConfig
from betazero_amd.match import MatchPlayer, play_match
from oracle import py_twin
from test_gpu_leaf_parallel import _net32, _net_fn, _root_arrays, _same_root
from test_gpu_playout_cap import _bits, _run, _same_rows
from test_gumbel_cpu import GumbelTwin, boards, game_roots
from test_gumbel_interior_cpu import COUNTERS, GfullSide, GumbelFullTwin
from test_match_cpu import MatchTwin, Side, assert_same_match

pytestmark = pytest.mark.gpu


def _cfg(m=16, scale=1.0, interior="gumbel"):
    return GumbelConfig(m, scale, interior=interior)


def _engine(game, n, sims, ev, gumbel, **kw):
    from betazero_amd.engine import SelfPlayEngine
    return SelfPlayEngine(game, n, sims, ev, gumbel=gumbel, **kw)


def _twin(game, ev, m, scale=1.0, eval_fn=None, interior="gumbel"):
    return GumbelFullTwin(game, ev, interior=interior, m=m, scale=scale, eval_fn=eval_fn, boards=boards())


def _search_case(game, ev, m, scale, sims, roots, eval_fn=None, net=None, external=None, seed=5, engine_ev=None, counters=True):
    """one search from every root (temp_moves 1: the noise is on when scale > 0), engine vs twin; returns the twins"""
    B = len(roots)
    eng = _engine(game, B, sims, "external" if external else (engine_ev or ev), _cfg(m, scale), net=net, temp_moves=1, seed=seed)
    eng.set_roots([r[2] for r in roots], [r[3] for r in roots], [r[1] for r in roots])
    eng.reset_counters()
    if external:
        eng.search_external(external)
    else:
        eng.search()
    NWP = eng.root_stats()
    pi, act = eng.root_policy()
    eng.status()
    cnt = eng.counters()
    twins = []
    for g, (b, p, _, _) in enumerate(roots):
        tw = _twin(game, ev, m, scale, eval_fn)
        root = tw.search(b, p, sims, scale > 0, (seed, g, 0))
        _same_root(NWP, g, tw, root)
        tpi, ta = tw.policy(root)
        assert np.array_equal(_bits(pi[g]), _bits(tpi)), (g, pi[g], tpi)
        assert act[g] == ta, (g, act[g], ta)
        twins.append(tw)
    if counters:
        for k in COUNTERS:
            assert cnt[k] == sum(tw.cnt[k] for tw in twins), (k, cnt, [tw.cnt for tw in twins])
    return twins


@pytest.mark.parametrize("game", ["ttt", "reversi", "reversi6", "reversi4"])
@pytest.mark.parametrize("ev", ["hash", "uniform"])
def test_single_searches_bitexact_vs_twin(game, ev):
    roots = game_roots(game, 4, seed=7)
    changed = 0
    for m in (1, 4, 16):
        for sims in (8, 40):
            changed += sum(tw.n_changed for tw in _search_case(game, ev, m, 1.0 if m != 4 else 0.0, sims, roots))
    assert changed > 0 or (ev == "uniform" and game != "ttt")


def test_wide_fixture_roots_score_interior_nodes_of_two_chunks():
    """Reversi 8x8 roots with 18 and 23 legal moves: their children hold more than 16 edges, two chunks on the 16-lane group
    (the fixtures hold no position with more than 32 moves; tic-tac-toe's 8-edge nodes are the other two-chunk case)"""
    from test_gpu_fpu import _fixture_roots
    r = _fixture_roots()
    roots = []
    for own, opp, tm, nl in (r["widest"], r["two"], r["one"], r["widest"]):
        x, o = (own, opp) if tm == 1 else (opp, own)
        roots.append((bz.ReversiBoard.from_bits(x, o, 8), tm, own, opp))
    twins = _search_case("reversi", "hash", 16, 1.0, 40, roots)
    assert max(tw.max_n for tw in twins) > 16 and sum(tw.n_changed for tw in twins) > 0


def _selfplay_case(game, n, sims, ev, m=16, scale=1.0, temp_moves=0, openings=0, seed=0, base=0, stagger=0, eval_fn=None, net=None,
                   engine_ev=None, interior="gumbel", **kw):
    eng = _engine(game, n, sims, engine_ev or ev, _cfg(m, scale, interior), net=net, temp_moves=temp_moves, openings=openings, seed=seed,
                  game_id_base=base, stagger=stagger, **kw)
    ex, (winners, lens), cnt = _run(eng)
    twins = []
    for g in range(n):
        tw = _twin(game, ev, m, scale, eval_fn, interior)
        rows, w, _ = tw.selfplay(base + g, sims, temp_moves, openings, seed, slot=g, stagger=stagger)
        assert lens[0, g] == len(rows) and winners[0, g] == w, (g, lens[0, g], len(rows), winners[0, g], w)
        _same_rows(ex, base + g, rows, w)
        twins.append((tw, rows, w))
    assert len(ex) == sum(len(r) for _, r, _ in twins)
    assert cnt["n_sims"] == len(ex) * sims, cnt
    if interior == "gumbel":
        assert sum(tw.n_changed for tw, _, _ in twins) > 0
    return eng, twins, cnt


def test_selfplay_bitexact_with_temperature_openings_and_a_staggered_pool():
    _, twins, cnt = _selfplay_case("reversi", 12, 24, "hash", m=8, temp_moves=8, openings=1, seed=3, base=7, stagger=5)
    for k in COUNTERS:
        assert cnt[k] == sum(tw.cnt[k] for tw, _, _ in twins), (k, cnt)


@pytest.mark.parametrize("game,n,sims,ev,m", [("ttt", 12, 40, "hash", 4), ("reversi4", 12, 16, "uniform", 2), ("reversi6", 6, 30, "hash", 16)])
def test_selfplay_small_boards_bitexact(game, n, sims, ev, m):
    _selfplay_case(game, n, sims, ev, m=m, temp_moves=3, seed=4, stagger=3)


def test_net_f32_search_and_selfplay_vs_twin_with_the_per_position_forward():
    dn = _net32()
    fn = _net_fn(dn)
    roots = game_roots("reversi", 3, seed=11)
    tw = _search_case("reversi", "net", 16, 1.0, 40, roots, eval_fn=fn, net=dn, engine_ev="net_f32")
    assert sum(t.n_changed for t in tw) > 0
    _selfplay_case("reversi", 4, 12, "net", m=8, temp_moves=8, openings=1, eval_fn=fn, net=dn, engine_ev="net_f32")


def test_mlp_f32_search_vs_twin_with_the_per_position_forward():
    from betazero_amd.mlp import DeviceMLP, TicTacToeNet
    torch.manual_seed(2)
    mlp = DeviceMLP.from_module(TicTacToeNet(9, 64, 9), max_batch=64)

    def fn(own, opp):
        return mlp.forward(np.array([own], np.uint64), np.array([opp], np.uint64))[0].cpu().numpy(), np.float32(0.0)
    roots = game_roots("ttt", 3, seed=5)
    changed = 0
    for m, scale, sims in ((4, 1.0, 40), (16, 0.0, 8)):
        changed += sum(t.n_changed for t in _search_case("ttt", "mlp", m, scale, sims, roots, eval_fn=fn, net=mlp, engine_ev="mlp_f32"))
    assert changed > 0


def test_external_evaluator_through_the_step_api_vs_twin():
    """select / expand_backup as separate launches: the expand-only step stores v_X, the select-only step reads it"""
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
    roots = game_roots("reversi", 3, seed=2)
    tw = _search_case("reversi", "hash", 16, 1.0, 40, roots, external=external)
    assert sum(t.n_changed for t in tw) > 0
    _search_case("reversi4", "hash", 2, 0.0, 8, game_roots("reversi4", 3, seed=2), external=external)


@pytest.mark.parametrize("cache", [False, "search", True])
def test_exact_bf16_net_and_every_cache_mode_equal_the_twin(cache):
    """the search-grade exact bf16 net (tests/test_search_net_cpu.py).  A COPY leaf takes its v_X from the node it copies, in
    this search's arena or in the previous one's: a wrong v_X changes the interior choices of every later walk through it.
    n_net_leaves + n_cache_hits is the twin's evaluation count in every mode."""
    from test_gpu_search_net import _dn, _net
    from test_search_net_cpu import oracle_eval_fn
    P, on = _net("bf16", 64, 1)
    _, twins, cnt = _selfplay_case("reversi6", 8, 32, "net", engine_ev="net_bf16", eval_fn=oracle_eval_fn(on, "bf16"), net=_dn(P, 8),
                                   temp_moves=4, seed=2, stagger=3, eval_cache=cache)
    assert cnt["n_net_leaves"] + cnt["n_cache_hits"] == sum(tw.n_evals for tw, _, _ in twins), cnt
    assert (cnt["n_cache_hits"] > 0) == (cache is not False), cnt
    assert (cnt["n_cache_hits_prev"] > 0) == (cache is True), cnt


def test_two_pipelines_give_the_rows_of_one_engine_and_of_the_twin():
    from betazero_amd.engine import PipelinedSelfPlay
    kw = dict(temp_moves=6, openings=1, seed=9)
    sp = PipelinedSelfPlay("reversi", 12, 24, "hash", pipelines=2, gumbel=_cfg(8), **kw)
    sp.run_iteration()
    a = sp.examples()
    eng, twins, _ = _selfplay_case("reversi", 12, 24, "hash", m=8, **kw)
    b = eng.examples()
    ia, ib = np.lexsort((a.ply, a.game)), np.lexsort((b.ply, b.game))
    assert len(a) == len(b) > 0
    for f in ("own", "opp", "z", "mover", "act", "game", "ply"):
        assert np.array_equal(getattr(a, f)[ia], getattr(b, f)[ib]), f
    assert np.array_equal(_bits(a.pi[ia]), _bits(b.pi[ib]))


def test_mcts_player_plays_the_twins_move():
    from betazero_amd.players import MCTSPlayer
    b = bz.ReversiBoard(size=8)
    for sims, m in ((8, 16), (40, 4)):
        pl = MCTSPlayer(1, sims, evaluator="hash", gumbel=_cfg(m))
        r, c = pl.get_move(b)
        tw = _twin("reversi", "hash", m)
        root = tw.search(b, 1, sims)
        tpi, ta = tw.policy(root)
        n, _, _ = _root_arrays(tw, root)
        assert np.array_equal(pl.last_visits, n) and 8 * r + c == ta
        assert np.array_equal(_bits(pl.last_policy), _bits(tpi))


def test_match_between_the_two_interiors_equals_the_match_twin():
    a, b = MatchPlayer(sims=32, evaluator="hash", gumbel=_cfg(8)), MatchPlayer(sims=32, evaluator="hash", gumbel=_cfg(8, interior="puct"))
    ga, gb = a.checked("reversi", 12, "a")[1], b.checked("reversi", 12, "b")[1]
    sa = GfullSide(32, "hash", gumbel=ga)
    ref, _ = MatchTwin("reversi4", sa, Side(32, "hash", gumbel=gb), 2, 3).play(12)
    res = play_match("reversi", 12, a, b, size=4, opening_plies=2, seed=3)
    assert_same_match(res, ref, "interior gumbel vs puct")
    assert sa.twin("reversi4").n_changed > 0
    ref, _ = MatchTwin("reversi4", Side(32, "hash", gumbel=gb), GfullSide(32, "hash", gumbel=ga), 2, 3).play(12)
    assert_same_match(play_match("reversi", 12, b, a, size=4, opening_plies=2, seed=3), ref, "interior puct vs gumbel")
    both = play_match("reversi", 12, b, b, size=4, opening_plies=2, seed=3)
    assert not np.array_equal(both.actions, res.actions)  # (and it is not the match of two root-only players)


def test_switching_the_rule_off_restores_the_root_only_engine_and_on_again_the_first_games():
    kw = dict(temp_moves=4, openings=1, seed=2)
    eng = _engine("reversi", 8, 16, "hash", _cfg(8), **kw)
    on1, (w1, _), _ = _run(eng)
    eng.set_gumbel_interior("puct")
    a, (wa, la), ca = _run(eng)
    b, (wb, lb), cb = _run(_engine("reversi", 8, 16, "hash", _cfg(8, interior="puct"), **kw))
    assert np.array_equal(wa, wb) and np.array_equal(la, lb) and np.array_equal(a.act, b.act) and np.array_equal(_bits(a.pi), _bits(b.pi))
    assert ca == cb
    tw = GumbelTwin("reversi", "hash", m=8, boards=boards())  # ... which is k_gumbel_step's: the Gumbel twin's game 0
    rows, w, _ = tw.selfplay(0, 16, 4, 1, 2, slot=0)
    _same_rows(a, 0, rows, w)
    eng.set_gumbel_interior("gumbel")
    c, (wc, _), _ = _run(eng)
    assert np.array_equal(wc, w1) and np.array_equal(c.act, on1.act) and np.array_equal(_bits(c.pi), _bits(on1.pi))
    assert c.pi.shape != a.pi.shape or not np.array_equal(_bits(c.pi), _bits(a.pi))


def test_set_gumbel_interior_refusals_through_the_raw_abi():
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda:0")
    p = buf.data_ptr() + ((-buf.data_ptr()) & 255)
    plain = _engine("reversi", 4, 16, "hash", None)
    need = L.bz_engine_gumbel_interior_bytes(C.byref(plain.cfg))
    assert need == 4 * 18 * 4 + (-4 * 18 * 4) % 256
    assert L.bz_engine_set_gumbel_interior(plain.h, 1, p, need, st) == _lib.BZ_EINVAL and b"Gumbel root search" in L.bz_last_error()
    assert L.bz_engine_set_gumbel_interior(plain.h, 0, None, 0, st) == _lib.BZ_OK  # "off" is always accepted
    eng = _engine("reversi", 4, 16, "hash", _cfg(8, interior="puct"))
    assert L.bz_engine_set_gumbel_interior(eng.h, 1, None, need, st) == _lib.BZ_EINVAL and b"aligned" in L.bz_last_error()
    assert L.bz_engine_set_gumbel_interior(eng.h, 1, p + 4, need, st) == _lib.BZ_EINVAL and b"aligned" in L.bz_last_error()
    assert L.bz_engine_set_gumbel_interior(eng.h, 1, p, need - 1, st) == _lib.BZ_EINVAL and b"too small" in L.bz_last_error()
    assert L.bz_engine_set_gumbel_interior(eng.h, 1, p, need, st) == _lib.BZ_OK
    # switching Gumbel root search off switches the rule off: a PUCT search again, the plain engine's statistics
    assert L.bz_engine_set_gumbel(eng.h, 0, 0.0, 0.0, 0.0, None, 0, st) == _lib.BZ_OK
    roots = game_roots("reversi", 4, seed=1)
    for e in (eng, plain):
        e.set_roots([r[2] for r in roots], [r[3] for r in roots], [r[1] for r in roots])
        e.search()
    for x, y in zip(eng.root_stats(), plain.root_stats()):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    eng.status()
    plain.status()
    torch.cuda.synchronize()


def test_engines_step_refuses_mixed_interiors():
    from betazero_amd.engine import PipelinedSelfPlay
    sp = PipelinedSelfPlay("reversi", 8, 8, "hash", pipelines=2, gumbel=_cfg(8))
    sp.engines[1].set_gumbel_interior("puct")
    sp.reset_games()
    with pytest.raises(RuntimeError, match="interior"):
        sp.step()
