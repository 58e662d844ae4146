"""Playout cap randomisation on the GPU: k_cap_budget / k_cap_step / k_cap_noise / k_cap_play against the cap
twin of tests/test_playout_cap_cpu.py.  "Equal" = bit for bit, every game: the rows (positions, pi bits, movers, actions, z),
winners, ex_len, the budgets after every search and n_sims = the sum of the budgets."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from betazero_amd import _lib
from betazero_amd.engine import PlayoutCap
from oracle import py_twin
from test_gpu_leaf_parallel import _net32, _net_fn
from test_playout_cap_cpu import CapTwin, boards, cap_budget

pytestmark = pytest.mark.gpu
NOISE = dict(dirichlet_alpha=0.3, dirichlet_eps=0.25)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _cap(fast, full_q):
    cap = PlayoutCap(fast, full_q / 65536)
    assert cap.full_q == full_q
    return cap


def _engine(game, n, sims, ev, cap, **kw):
    from betazero_amd.engine import SelfPlayEngine
    return SelfPlayEngine(game, n, sims, ev, playout_cap=cap, **kw)


def _twins(game, ev, n, sims, fast, full_q, temp_moves, openings, seed, base, stagger, eval_fn, noise, slot0=0):
    """every game's cap twin, played to the end: [(twin, rows, winner)]"""
    out = []
    for g in range(n):
        tw = CapTwin(game, ev, fast, full_q, eval_fn=eval_fn, boards=boards(),
                     **(dict(dir_alpha=NOISE["dirichlet_alpha"], dir_eps=NOISE["dirichlet_eps"]) if noise else {}))
        rows, w, _ = tw.selfplay(base + slot0 + g, sims, temp_moves, openings, seed, slot=g, stagger=stagger)
        out.append((tw, rows, w))
    return out


def _same_rows(ex, gid, rows, w):
    msk = ex.game == gid
    assert int(msk.sum()) == len(rows), (gid, int(msk.sum()), len(rows))
    assert np.array_equal(ex.own[msk], np.array([r[0] for r in rows], np.uint64))
    assert np.array_equal(ex.opp[msk], np.array([r[1] for r in rows], np.uint64))
    na = ex.pi.shape[1]
    assert np.array_equal(_bits(ex.pi[msk]), _bits([r[2] for r in rows]).reshape(len(rows), na))
    assert np.array_equal(ex.mover[msk], np.array([r[3] for r in rows], np.int8))
    assert np.array_equal(ex.act[msk], np.array([r[4] for r in rows], np.uint8))
    assert np.array_equal(ex.z[msk], (w * np.array([r[3] for r in rows], np.int64)).astype(np.int8))
    assert np.array_equal(ex.ply[msk], np.arange(len(rows)))  # the row index inside its game


def _selfplay_case(game, n, sims, fast, full_q, ev, temp_moves=0, openings=0, seed=0, base=0, stagger=0, eval_fn=None, net=None,
                   engine_ev=None, noise=False, external=None, mixed=None, **kw):
    """n games to the end, search by search, against the twins.  mixed (default: 0 < full_q < 65536): the games must hold
    both kinds of search.  Returns (engine, twins, counters)."""
    eng = _engine(game, n, sims, "external" if external else (engine_ev or ev), _cap(fast, full_q), net=net, temp_moves=temp_moves,
                  openings=openings, seed=seed, game_id_base=base, stagger=stagger, **(NOISE if noise else {}), **kw)
    twins = _twins(game, ev, n, sims, fast, full_q, temp_moves, openings, seed, base, stagger, eval_fn, noise)
    eng.reset_counters()
    eng.reset_games()
    assert not eng.budgets().any()  # no search yet
    step = 0
    while True:
        if external:
            eng.search_external(external)
        else:
            eng.search()
        want = [tw.budgets[step] if step < len(tw.budgets) else 0 for tw, _, _ in twins]
        got = eng.budgets()
        assert np.array_equal(got, np.array(want, np.uint32)), (step, got, want)
        N, _, _ = eng.root_stats()
        assert np.array_equal(N.sum(1), got), (step, N.sum(1), got)  # root visit sum = the budget (finished slots: 0)
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
    all_b = [b for tw, _, _ in twins for b in tw.budgets]
    assert cnt["n_sims"] == sum(all_b), (cnt, sum(all_b))
    if mixed if mixed is not None else 0 < full_q < 65536:
        assert set(all_b) == {sims, fast}, set(all_b)  # the draw is not stuck
    return eng, twins, cnt


# ---------------------------------------------------------------- self-play against the twin
@pytest.mark.parametrize("full_q", [0, 16384, 49152, 65536])
@pytest.mark.parametrize("ev", ["hash", "uniform"])
def test_selfplay_equals_the_twin_with_temperature_openings_stagger_and_noise(ev, full_q):
    _selfplay_case("reversi", 12, 24, 6, full_q, ev, temp_moves=8, openings=1, seed=3, base=7, stagger=5, noise=True)
    _selfplay_case("ttt", 16, 40, 4, full_q, ev, temp_moves=4, seed=1, stagger=3, noise=True)
    _selfplay_case("reversi6", 6, 30, 5, full_q, ev, temp_moves=2, seed=2, stagger=4)
    _selfplay_case("reversi4", 8, 16, 1, full_q, ev, temp_moves=3, seed=4, noise=(ev == "hash"))


def test_the_quoted_draw_counts_hold_for_the_games_played():
    """seed 3, gids 7..18: 175 full of 720 draws over moves 0..59, 11 to 19 per game; seed 1, gids 0..15: 232 of 960, and six
    games without a full search in their first five moves -- then the games actually played"""
    per = [sum(cap_budget(3, g, m, 24, 6, 16384) == 24 for m in range(60)) for g in range(7, 19)]
    assert sum(per) == 175 and min(per) == 11 and max(per) == 19
    assert sum(cap_budget(1, g, m, 40, 4, 16384) == 40 for g in range(16) for m in range(60)) == 232
    assert sum(all(cap_budget(1, g, m, 40, 4, 16384) == 4 for m in range(5)) for g in range(16)) == 6
    _, twins, _ = _selfplay_case("reversi", 12, 24, 6, 16384, "hash", temp_moves=8, openings=1, seed=3, base=7)
    for tw, rows, _ in twins:  # every single game holds both kinds
        assert set(tw.budgets) == {24, 6} and 0 < len(rows) < len(tw.budgets)


def test_games_that_finish_without_a_row():
    """tic-tac-toe, seed 1, gids 0..15, full_q 16384: games whose every search was fast finish with ex_len = 0 (not -1), keep
    their winner, and the packed block counts them as games without rows"""
    from betazero_amd.engine import packed_block_header, unpack_packed_block
    eng, twins, _ = _selfplay_case("ttt", 16, 40, 4, 16384, "hash", temp_moves=9, seed=1, noise=True)
    zero = [g for g, (_, rows, _) in enumerate(twins) if not rows]
    assert zero, "the case must hold a game without a full search"
    winners, lens = eng.winners()
    for g in zero:
        assert lens[0, g] == 0 and winners[0, g] == twins[g][2]
    assert (lens >= 0).all()  # every game finished
    n_rows = sum(len(r) for _, r, _ in twins)
    blk = eng.pack_examples()
    h = packed_block_header(blk)
    assert h["n_games"] == 16 and h["n_rows"] == n_rows and h["dropped_rows"] == 0, h
    px = unpack_packed_block(blk)
    for g, (_, rows, w) in enumerate(twins):
        _same_rows(px, g, rows, w)
    # a block with exactly the capacity the rows need still carries the zero-row games behind the last row
    h2 = packed_block_header(eng.pack_examples(cap_rows=n_rows))
    assert h2["n_games"] == 16 and h2["n_rows"] == n_rows and h2["dropped_rows"] == 0, h2


# ---------------------------------------------------------------- product against product
def _run(eng):
    eng.reset_counters()
    eng.run_iteration()
    eng.status()
    return eng.examples(), eng.winners(), eng.counters()


@pytest.mark.parametrize("game,ev", [("reversi", "hash"), ("ttt", "hash"), ("reversi", "net_f32")])
def test_every_search_full_equals_the_engine_without_the_cap(game, ev):
    net = _net32() if ev == "net_f32" else None
    kw = dict(temp_moves=6, openings=1, seed=9, net=net, **NOISE)  # (noise: both engines run the step kernels)
    n, sims = (6, 12) if net else (12, 24)
    a, (wa, la), ca = _run(_engine(game, n, sims, ev, _cap(3, 65536), **kw))
    b, (wb, lb), cb = _run(_engine(game, n, sims, ev, None, **kw))
    assert len(a) == len(b) > 0 and np.array_equal(wa, wb) and np.array_equal(la, lb) and ca == cb, (ca, cb)
    for f in ("own", "opp", "z", "mover", "act", "game", "ply"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert np.array_equal(_bits(a.pi), _bits(b.pi))


@pytest.mark.parametrize("game", ["reversi", "ttt", "reversi4"])
def test_every_search_fast_plays_the_moves_of_an_engine_with_the_small_budget(game):
    kw = dict(temp_moves=4, openings=1, seed=5)
    n, sims, fast = 12, 32, 7
    a = _engine(game, n, sims, "hash", _cap(fast, 0), **kw, **NOISE)  # (a fast search draws no noise)
    b = _engine(game, n, fast, "hash", None, **kw)
    a.reset_counters(); b.reset_counters()
    a.reset_games(); b.reset_games()
    for step in range(200):
        a.search(); b.search()
        a.play(False); b.play(False)
        pa, pb = a.positions(), b.positions()
        for x, y in zip(pa, pb):
            assert np.array_equal(x, y), step
        if a.status()[0] == 0:
            break
    assert b.status()[0] == 0
    (wa, la), (wb, lb) = a.winners(), b.winners()
    assert np.array_equal(wa, wb) and not la.any() and (lb > 0).all() and len(a.examples()) == 0
    assert a.counters()["n_sims"] == b.counters()["n_sims"] == fast * int(lb.sum())


# ---------------------------------------------------------------- evaluators and the evaluation cache
def test_net_f32_selfplay_equals_the_twin_with_the_per_position_forward():
    dn = _net32()
    _selfplay_case("reversi", 4, 12, 3, 16384, "net", engine_ev="net_f32", eval_fn=_net_fn(dn), net=dn, temp_moves=8, openings=1,
                   seed=3, noise=True)


def test_mlp_f32_selfplay_equals_the_twin_with_the_per_position_forward():
    from betazero_amd.mlp import DeviceMLP, TicTacToeNet
    torch.manual_seed(2)
    mlp = DeviceMLP.from_module(TicTacToeNet(9, 64, 9), max_batch=64)

    def fn(own, opp):
        return mlp.forward(np.array([own], np.uint64), np.array([opp], np.uint64))[0].cpu().numpy(), np.float32(0.0)
    _selfplay_case("ttt", 12, 30, 5, 32768, "mlp", engine_ev="mlp_f32", eval_fn=fn, net=mlp, temp_moves=3, seed=6, stagger=2)


@pytest.mark.parametrize("cache", [False, "search", True])
def test_exact_bf16_net_and_every_cache_mode_equal_the_twin(cache):
    """the search-grade exact bf16 net (tests/test_search_net_cpu.py): the device forward equals the oracle's, so the cap
    engine equals the twin whose evaluator is the oracle's forward -- with every cache mode, which only moves evaluations
    from the net (n_net_leaves) to the cache (n_cache_hits)"""
    from test_gpu_search_net import _dn, _net
    from test_search_net_cpu import oracle_eval_fn
    P, on = _net("bf16", 64, 1)
    _, twins, cnt = _selfplay_case("reversi6", 8, 32, 8, 16384, "net", engine_ev="net_bf16", eval_fn=oracle_eval_fn(on, "bf16"),
                                   net=_dn(P, 8), temp_moves=4, seed=2, stagger=3, eval_cache=cache)
    assert cnt["n_net_leaves"] + cnt["n_cache_hits"] == sum(tw.n_evals for tw, _, _ in twins), cnt
    assert (cnt["n_cache_hits"] > 0) == (cache is not False), cnt
    assert (cnt["n_cache_hits_prev"] > 0) == (cache is True), cnt


def test_external_evaluator_through_the_step_api_equals_the_twin():
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
    _selfplay_case("reversi4", 6, 16, 4, 32768, "hash", external=external, temp_moves=3, seed=8, noise=True)


# ---------------------------------------------------------------- pipelines and the loop
def test_two_pipelines_equal_the_twin():
    from betazero_amd.engine import PipelinedSelfPlay
    n, sims, fast, q = 16, 24, 6, 16384
    sp = PipelinedSelfPlay("reversi", n, sims, "hash", pipelines=2, playout_cap=_cap(fast, q), temp_moves=6, openings=1, seed=9,
                           game_id_base=100, **NOISE)
    sp.reset_counters()
    sp.run_iteration()
    assert sp.status()[0] == 0
    ex, (winners, lens), cnt = sp.examples(), sp.winners(), sp.counters()
    # the two engines hold slots 0..7 of games 100..107 and 108..115: every draw is keyed by the global game id
    twins = _twins("reversi", "hash", 8, sims, fast, q, 6, 1, 9, 100, 0, None, True) + \
        _twins("reversi", "hash", 8, sims, fast, q, 6, 1, 9, 100, 0, None, True, slot0=8)
    for g, (tw, rows, w) in enumerate(twins):
        assert lens[0, g] == len(rows) and winners[0, g] == w, g
        _same_rows(ex, 100 + g, rows, w)
    all_b = [b for tw, _, _ in twins for b in tw.budgets]
    assert cnt["n_sims"] == sum(all_b) and set(all_b) == {sims, fast} and len(ex) == sum(len(r) for _, r, _ in twins)
    last = sp.budgets()  # the last search: only the games that were still running drew a budget
    assert last.shape == (n,) and set(last.tolist()) <= {0, sims, fast} and last.any()


def test_az_loop_runs_two_iterations_with_the_cap():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "az_loop.py"), "--iters", "2", "--games", "64", "--sims", "16",
                          "--fast-sims", "4", "--full-prob", "0.5", "--channels", "64", "--blocks", "1",
                          "--arena-games", "16", "--arena-sims", "8", "--depth", "1", "--final-depths", ""],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    its = [d for d in (json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")) if d.get("what") == "iteration"]
    assert [d["iter"] for d in its] == [1, 2]
    for d in its:
        assert 0 < d["rows_per_game"] < d["plies"] and d["games_per_s"] > 0 and d["examples"] == round(d["rows_per_game"] * 64), d


# ---------------------------------------------------------------- the setter
def test_set_playout_cap_refuses_the_refused_combinations_and_bad_arguments():
    L = _lib.lib()
    buf = torch.zeros(1 << 12, dtype=torch.uint8, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    for kw, word in (({"leaves_per_step": 2}, b"leaves_per_step"), ({"reuse_subtree": True}, b"subtree reuse"), ({"gumbel": True}, b"Gumbel")):
        eng = _engine("reversi", 4, 16, "hash", None, **kw)
        assert L.bz_engine_set_playout_cap(eng.h, 4, 16384, buf.data_ptr(), buf.numel(), st) == _lib.BZ_EINVAL
        assert word in L.bz_last_error() and b"playout cap" in L.bz_last_error(), L.bz_last_error()
    eng = _engine("reversi", 4, 16, "hash", None)
    for fast, q in ((16, 1), (17, 1), (-1, 1), (4, 65537)):
        assert L.bz_engine_set_playout_cap(eng.h, fast, q, buf.data_ptr(), buf.numel(), st) == _lib.BZ_EINVAL
    assert L.bz_engine_set_playout_cap(eng.h, 4, 16384, buf.data_ptr(), 8, st) == _lib.BZ_ENOMEM
    assert L.bz_engine_set_playout_cap(eng.h, 4, 16384, buf.data_ptr() + 4, buf.numel() - 4, st) == _lib.BZ_EINVAL
    assert L.bz_engine_set_playout_cap(eng.h, 4, 16384, buf.data_ptr(), buf.numel(), st) == _lib.BZ_OK
    gbuf = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda:0")
    assert L.bz_engine_set_gumbel(eng.h, 16, 1.0, 50.0, 0.1, gbuf.data_ptr(), gbuf.numel(), st) == _lib.BZ_EINVAL  # cap is on
    assert b"playout cap" in L.bz_last_error()
    assert L.bz_engine_set_playout_cap(eng.h, 0, 0, None, 0, st) == _lib.BZ_OK  # off needs no buffer
    assert L.bz_engine_set_gumbel(eng.h, 16, 1.0, 50.0, 0.1, gbuf.data_ptr(), gbuf.numel(), st) == _lib.BZ_OK


def test_switching_the_cap_off_restores_the_plain_engine():
    kw = dict(temp_moves=4, openings=1, seed=2)
    eng = _engine("reversi", 8, 16, "hash", _cap(4, 16384), **kw)
    _lib.check(_lib.lib().bz_engine_set_playout_cap(eng.h, 0, 0, None, 0, torch.cuda.current_stream().cuda_stream))
    a, (wa, la), _ = _run(eng)
    b, (wb, lb), _ = _run(_engine("reversi", 8, 16, "hash", None, **kw))
    assert np.array_equal(wa, wb) and np.array_equal(la, lb) and np.array_equal(a.act, b.act) and np.array_equal(_bits(a.pi), _bits(b.pi))
