"""Forced playouts and policy target pruning on the GPU: k_forced_step / k_forced_cap_step / k_forced_play /
k_forced_cap_play / k_forced_root_policy against the forced twin of tests/test_forced_playouts_cpu.py.  "Equal" = bit for bit,
every game and every search: root N / W / P, root_policy()'s pi and action, the budgets under the cap, then the rows
(positions, pi bits, movers, actions, z), winners and ex_len."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from betazero_amd import _lib
from betazero_amd.engine import ForcedPlayouts, PlayoutCap
from oracle import py_twin
from test_forced_playouts_cpu import TINY_K, ForcedTwin, boards
from test_gpu_leaf_parallel import _net32, _net_fn
from test_gpu_playout_cap import _bits, _run, _same_rows

pytestmark = pytest.mark.gpu
NOISE = dict(dirichlet_alpha=0.3, dirichlet_eps=0.25)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _engine(game, n, sims, ev, fp, cap=None, **kw):
    from betazero_amd.engine import SelfPlayEngine
    return SelfPlayEngine(game, n, sims, ev, forced_playouts=fp, playout_cap=PlayoutCap(cap[0], cap[1] / 65536) if cap else None, **kw)


def _twins(game, ev, n, sims, k, prune, cap, temp_moves, openings, seed, base, stagger, eval_fn, noise, slot0=0):
    out = []
    for g in range(n):
        tw = ForcedTwin(game, ev, k, prune=prune, cap=cap, eval_fn=eval_fn, boards=boards(),
                        **(dict(dir_alpha=NOISE["dirichlet_alpha"], dir_eps=NOISE["dirichlet_eps"]) if noise else {}))
        rows, w, _ = tw.selfplay(base + slot0 + g, sims, temp_moves, openings, seed, slot=g, stagger=stagger)
        out.append((tw, rows, w))
    return out


def _case(game, n, sims, ev, k=2.0, prune=True, cap=None, temp_moves=0, openings=0, seed=0, base=0, stagger=0, eval_fn=None,
          net=None, engine_ev=None, noise=True, external=None, vacuous_ok=False, **kw):
    """n games to the end, search by search, against the twins.  Unless vacuous_ok the case must hold walks in which the
    forced rule overrode PUCT and (prune) rows whose pi was pruned.  Returns (engine, twins, counters)."""
    eng = _engine(game, n, sims, "external" if external else (engine_ev or ev), ForcedPlayouts(k, prune), cap, net=net,
                  temp_moves=temp_moves, openings=openings, seed=seed, game_id_base=base, stagger=stagger, **(NOISE if noise else {}), **kw)
    twins = _twins(game, ev, n, sims, k, prune, cap, temp_moves, openings, seed, base, stagger, eval_fn, noise)
    eng.reset_counters()
    eng.reset_games()
    step = 0
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
        for g, (tw, _, _) in enumerate(twins):
            if step >= len(tw.log):
                assert act[g] == -1 and not pi[g].any(), (step, g)
                continue
            lg = tw.log[step]
            a = lg["a"]
            assert np.array_equal(N[g, a], np.array(lg["N"], np.uint32)), (step, g, N[g, a], lg["N"])  # the RAW visits
            assert int(N[g].sum()) == lg["budget"]
            assert np.array_equal(_bits(W[g, a]), _bits(lg["W"])) and np.array_equal(_bits(P[g, a]), _bits(lg["P"])), (step, g)
            assert act[g] == lg["act"] and np.array_equal(_bits(pi[g]), _bits(lg["pi"])), (step, g, pi[g], lg["pi"])
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
    if not vacuous_ok:
        assert sum(tw.n_overrides for tw, _, _ in twins) > 0
        if prune:
            assert any(lg["Np"] != lg["N"] for tw, _, _ in twins for lg in tw.log)
    return eng, twins, cnt


# ---------------------------------------------------------------- self-play against the twin
@pytest.mark.parametrize("prune", [True, False])
@pytest.mark.parametrize("ev", ["hash", "uniform"])
def test_selfplay_equals_the_twin_with_temperature_openings_stagger_and_noise(ev, prune):
    _case("reversi", 10, 24, ev, prune=prune, temp_moves=8, openings=1, seed=3, base=7, stagger=5)
    _case("ttt", 12, 40, ev, prune=prune, temp_moves=4, seed=1, stagger=3)
    _case("reversi6", 5, 30, ev, prune=prune, temp_moves=2, seed=2, stagger=4, noise=False)
    _case("reversi4", 8, 32, ev, k=0.5, prune=prune, temp_moves=3, seed=4, noise=(ev == "hash"))


def test_the_cases_hold_children_pruned_to_zero_and_a_large_k():
    _, twins, _ = _case("reversi", 8, 24, "hash", temp_moves=8, openings=1, seed=3, base=7)
    assert any(n0 > 0 and n1 == 0 for tw, _, _ in twins for lg in tw.log for n0, n1 in zip(lg["N"], lg["Np"]))
    _case("reversi4", 6, 32, "hash", k=50.0, temp_moves=2, seed=6)  # nf beyond most N: nearly every visited child is forced


@pytest.mark.parametrize("full_q", [0, 16384, 49152, 65536])
def test_selfplay_under_the_cap_equals_the_twin(full_q):
    """a fast search is plain PUCT without noise and reports its raw pi; only the full ones force, prune and record"""
    eng, twins, _ = _case("reversi", 10, 24, "hash", cap=(6, full_q), temp_moves=8, openings=1, seed=3, base=7, stagger=5,
                          vacuous_ok=full_q == 0)
    all_b = {b for tw, _, _ in twins for b in tw.budgets}
    assert all_b == ({24, 6} if 0 < full_q < 65536 else {24} if full_q else {6})
    if full_q == 0:
        assert sum(tw.n_overrides for tw, _, _ in twins) == 0 and len(eng.examples()) == 0
    _case("ttt", 12, 40, "uniform", prune=(full_q != 16384), cap=(4, full_q), temp_moves=4, seed=1, stagger=3, vacuous_ok=full_q == 0)


# ---------------------------------------------------------------- product against product
@pytest.mark.parametrize("game,ev", [("reversi", "hash"), ("ttt", "uniform"), ("reversi", "net_f32")])
def test_a_tiny_k_equals_the_plain_engine(game, ev):
    """nf < 1 always: nothing is forced.  prune off: every row of the plain engine bit for bit; prune on: m = ceil(nf) = 1
    visit of every other child is still offered to the pruning, so the games and moves are the plain engine's and pi may
    differ"""
    net = _net32() if ev == "net_f32" else None
    kw = dict(temp_moves=6, openings=1, seed=9, net=net, **NOISE)  # (noise: both engines run the step kernels)
    n, sims = (6, 12) if net else (12, 24)
    b, (wb, lb), cb = _run(_engine(game, n, sims, ev, None, **kw))
    a, (wa, la), ca = _run(_engine(game, n, sims, ev, ForcedPlayouts(TINY_K, False), **kw))
    assert len(a) == len(b) > 0 and np.array_equal(wa, wb) and np.array_equal(la, lb) and ca == cb, (ca, cb)
    for f in ("own", "opp", "z", "mover", "act", "game", "ply"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    assert np.array_equal(_bits(a.pi), _bits(b.pi))
    p, (wp, lp), cp = _run(_engine(game, n, sims, ev, ForcedPlayouts(TINY_K, True), **kw))
    assert np.array_equal(wp, wb) and np.array_equal(lp, lb) and cp == cb
    for f in ("own", "opp", "z", "mover", "act", "game", "ply"):
        assert np.array_equal(getattr(p, f), getattr(b, f)), f
    assert np.array_equal(p.pi > 0, (b.pi > 0) & (p.pi > 0)) and np.allclose(p.pi.sum(1), 1.0, atol=1e-5)


def test_switching_off_restores_the_plain_engine_and_the_fused_search():
    kw = dict(temp_moves=4, openings=1, seed=2)
    eng = _engine("reversi", 8, 16, "hash", ForcedPlayouts(2.0), **kw)
    _lib.check(_lib.lib().bz_engine_set_forced_playouts(eng.h, 0.0, 0, torch.cuda.current_stream().cuda_stream))
    a, (wa, la), ca = _run(eng)
    b, (wb, lb), cb = _run(_engine("reversi", 8, 16, "hash", None, **kw))
    assert np.array_equal(wa, wb) and np.array_equal(la, lb) and np.array_equal(a.act, b.act) and np.array_equal(_bits(a.pi), _bits(b.pi))
    assert ca == cb
    # ... and on again: the forced engine's games
    _lib.check(_lib.lib().bz_engine_set_forced_playouts(eng.h, 2.0, 1, torch.cuda.current_stream().cuda_stream))
    c, (wc, lc), _ = _run(eng)
    d, (wd, ld), _ = _run(_engine("reversi", 8, 16, "hash", ForcedPlayouts(2.0), **kw))
    assert np.array_equal(wc, wd) and np.array_equal(c.act, d.act) and np.array_equal(_bits(c.pi), _bits(d.pi))
    assert c.pi.shape != a.pi.shape or not np.array_equal(_bits(c.pi), _bits(a.pi))  # (and they are not the plain engine's)


# ---------------------------------------------------------------- evaluators and the evaluation cache
def test_net_f32_selfplay_equals_the_twin_with_the_per_position_forward():
    dn = _net32()
    _case("reversi", 4, 16, "net", engine_ev="net_f32", eval_fn=_net_fn(dn), net=dn, temp_moves=8, openings=1, seed=3)
    _case("reversi", 4, 16, "net", engine_ev="net_f32", eval_fn=_net_fn(dn), net=dn, cap=(4, 32768), temp_moves=8, openings=1, seed=3)


@pytest.mark.parametrize("cache", [False, "search", True])
def test_exact_bf16_net_and_every_cache_mode_equal_the_twin(cache):
    """the search-grade exact bf16 net (tests/test_search_net_cpu.py).  The cache is keyed by position and confirmed against it:
    the different search order changes which evaluations it serves, not what they are -- n_net_leaves + n_cache_hits is the
    twin's evaluation count in every mode"""
    from test_gpu_search_net import _dn, _net
    from test_search_net_cpu import oracle_eval_fn
    P, on = _net("bf16", 64, 1)
    _, twins, cnt = _case("reversi6", 8, 32, "net", engine_ev="net_bf16", eval_fn=oracle_eval_fn(on, "bf16"), net=_dn(P, 8),
                          temp_moves=4, seed=2, stagger=3, eval_cache=cache)
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
    _case("reversi4", 6, 32, "hash", external=external, temp_moves=3, seed=8)
    _case("reversi4", 6, 32, "hash", external=external, cap=(8, 32768), temp_moves=3, seed=8)


# ---------------------------------------------------------------- pipelines and the loop
@pytest.mark.parametrize("cap", [None, (6, 16384)])
def test_two_pipelines_equal_the_twin(cap):
    from betazero_amd.engine import PipelinedSelfPlay
    n, sims = 16, 24
    sp = PipelinedSelfPlay("reversi", n, sims, "hash", pipelines=2, forced_playouts=True, temp_moves=6, openings=1, seed=9,
                           playout_cap=PlayoutCap(cap[0], cap[1] / 65536) if cap else None, game_id_base=100, **NOISE)
    sp.reset_counters()
    sp.run_iteration()
    assert sp.status()[0] == 0
    ex, (winners, lens), cnt = sp.examples(), sp.winners(), sp.counters()
    twins = _twins("reversi", "hash", 8, sims, 2.0, True, cap, 6, 1, 9, 100, 0, None, True) + \
        _twins("reversi", "hash", 8, sims, 2.0, True, cap, 6, 1, 9, 100, 0, None, True, slot0=8)
    for g, (tw, rows, w) in enumerate(twins):
        assert lens[0, g] == len(rows) and winners[0, g] == w, g
        _same_rows(ex, 100 + g, rows, w)
    assert cnt["n_sims"] == sum(b for tw, _, _ in twins for b in tw.budgets) and len(ex) == sum(len(r) for _, r, _ in twins)
    assert sum(tw.n_overrides for tw, _, _ in twins) > 0 and any(lg["Np"] != lg["N"] for tw, _, _ in twins for lg in tw.log)


def test_self_play_takes_forced_playouts():
    from betazero_amd.engine import self_play
    s, pi, z, ex = self_play("reversi", 8, 24, seed=3, evaluator="hash", temp_moves=8, openings=1, forced_playouts=ForcedPlayouts(2.0),
                             **NOISE)
    twins = _twins("reversi", "hash", 8, 24, 2.0, True, None, 8, 1, 3, 0, 0, None, True)
    for g, (tw, rows, w) in enumerate(twins):
        _same_rows(ex, g, rows, w)


def test_az_loop_runs_two_iterations_with_forced_playouts_under_the_cap():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "az_loop.py"), "--iters", "2", "--games", "64", "--sims", "16",
                          "--forced-k", "2", "--fast-sims", "4", "--full-prob", "0.5", "--channels", "64", "--blocks", "1",
                          "--arena-games", "16", "--arena-sims", "8", "--depth", "1", "--final-depths", ""],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    its = [d for d in (json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")) if d.get("what") == "iteration"]
    assert [d["iter"] for d in its] == [1, 2]
    for d in its:
        assert 0 < d["rows_per_game"] < d["plies"] and d["games_per_s"] > 0 and d["forced_k"] == 2.0 and d["prune"] is True, d


# ---------------------------------------------------------------- the setter
def test_set_forced_playouts_refuses_the_refused_combinations_and_bad_arguments():
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    for kw, word in (({"leaves_per_step": 2}, b"leaves_per_step"), ({"reuse_subtree": True}, b"subtree reuse"), ({"gumbel": True}, b"Gumbel")):
        eng = _engine("reversi", 4, 16, "hash", None, **kw)
        assert L.bz_engine_set_forced_playouts(eng.h, 2.0, 1, st) == _lib.BZ_EINVAL
        assert word in L.bz_last_error() and b"forced playouts" in L.bz_last_error(), L.bz_last_error()
        assert L.bz_engine_set_forced_playouts(eng.h, 0.0, 0, st) == _lib.BZ_OK  # "off" is always accepted
    eng = _engine("reversi", 4, 16, "hash", None, cap=(4, 16384), **NOISE)  # the cap and the noise are allowed
    for k in (-1.0, float("inf"), float("nan")):
        assert L.bz_engine_set_forced_playouts(eng.h, k, 1, st) == _lib.BZ_EINVAL
        assert b"finite" in L.bz_last_error()
    assert L.bz_engine_set_forced_playouts(eng.h, 2.0, 1, st) == _lib.BZ_OK
    gbuf = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda:0")
    eng2 = _engine("reversi", 4, 16, "hash", ForcedPlayouts(2.0))
    assert L.bz_engine_set_gumbel(eng2.h, 16, 1.0, 50.0, 0.1, gbuf.data_ptr(), gbuf.numel(), st) == _lib.BZ_EINVAL  # forced is on
    assert b"forced playouts" in L.bz_last_error()
    assert L.bz_engine_set_forced_playouts(eng2.h, 0.0, 0, st) == _lib.BZ_OK
    assert L.bz_engine_set_gumbel(eng2.h, 16, 1.0, 50.0, 0.1, gbuf.data_ptr(), gbuf.numel(), st) == _lib.BZ_OK
