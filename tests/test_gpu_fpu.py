"""First-play urgency reduction on the GPU: k_fpu_step / k_fpu_cap_step / k_fpu_forced_step /
k_fpu_forced_cap_step against the FPU twin of tests/test_fpu_cpu.py.  "Equal" = bit for bit, every game and every search: root
N / W / P, root_policy()'s pi and action, the budgets under the cap, then the rows (positions, pi bits, movers, actions, z),
winners and ex_len.  Every case must hold walks in which the rule chose another edge than plain PUCT would have from the same
statistics (FpuTwin.n_changed): the uniform evaluator is therefore paired with tic-tac-toe and Reversi 4x4, Reversi 8x8 with
the hash evaluator (tests/test_fpu_cpu.py says why)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import betazero_amd as bz
from betazero_amd import _lib
from betazero_amd.engine import ForcedPlayouts, Fpu, PlayoutCap
from betazero_amd.match import MatchPlayer, play_match
from oracle import py_twin
from test_fpu_cpu import FpuSide, FpuTwin, boards
from test_gpu_leaf_parallel import _net32, _net_fn
from test_gpu_playout_cap import _bits, _run, _same_rows
from test_match_cpu import MatchTwin, Side, assert_same_match
from test_surprise_cpu import _Surprise
from test_value_targets_cpu import _Value

pytestmark = pytest.mark.gpu
NOISE = dict(dirichlet_alpha=0.3, dirichlet_eps=0.25)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def _engine(game, n, sims, ev, fpu=True, cap=None, forced=None, **kw):
    from betazero_amd.engine import SelfPlayEngine
    return SelfPlayEngine(game, n, sims, ev, fpu=fpu, forced_playouts=forced,
                          playout_cap=PlayoutCap(cap[0], cap[1] / 65536) if cap else None, **kw)


def _twins(game, ev, n, sims, fpu, k, prune, cap, temp_moves, openings, seed, base, stagger, eval_fn, noise, slot0=0, cls=FpuTwin):
    out = []
    for g in range(n):
        tw = cls(game, ev, fpu, k=k, prune=prune, cap=cap, eval_fn=eval_fn, boards=boards(),
                 **(dict(dir_alpha=NOISE["dirichlet_alpha"], dir_eps=NOISE["dirichlet_eps"]) if noise else {}))
        rows, w, _ = tw.selfplay(base + slot0 + g, sims, temp_moves, openings, seed, slot=g, stagger=stagger)
        out.append((tw, rows, w))
    return out


def _case(game, n, sims, ev, fpu=(0.2, 0.1), k=None, prune=True, cap=None, temp_moves=0, openings=0, seed=0, base=0, stagger=0,
          eval_fn=None, net=None, engine_ev=None, noise=True, external=None, vacuous_ok=False, cls=FpuTwin, **kw):
    """n games to the end, search by search, against the twins.  Unless vacuous_ok the case must hold walks in which the rule
    chose another edge than plain PUCT would have.  Returns (engine, twins, counters)."""
    eng = _engine(game, n, sims, "external" if external else (engine_ev or ev), Fpu(*fpu), cap,
                  ForcedPlayouts(k, prune) if k is not None else None, net=net, temp_moves=temp_moves, openings=openings, seed=seed,
                  game_id_base=base, stagger=stagger, **(NOISE if noise else {}), **kw)
    twins = _twins(game, ev, n, sims, fpu, k, prune, cap, temp_moves, openings, seed, base, stagger, eval_fn, noise, cls=cls)
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
            assert np.array_equal(N[g, a], np.array(lg["N"], np.uint32)), (step, g, N[g, a], lg["N"])
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
        assert sum(tw.n_changed for tw, _, _ in twins) > 0
    return eng, twins, cnt


# ---------------------------------------------------------------- self-play against the twin
def test_selfplay_reversi8_equals_the_twin_with_temperature_openings_stagger_and_noise():
    _case("reversi", 8, 32, "hash", temp_moves=8, openings=1, seed=3, base=7, stagger=5)


@pytest.mark.parametrize("ev", ["hash", "uniform"])
def test_selfplay_tictactoe_equals_the_twin_nine_root_edges_on_four_lanes(ev):
    """tic-tac-toe: the empty board's 9 edges on a 4-lane group are three chunks of the mass reduction"""
    _case("ttt", 16, 40, ev, temp_moves=4, seed=1, stagger=3)
    _case("ttt", 8, 64, ev, fpu=(1.0, 0.5), seed=2, noise=False)


@pytest.mark.parametrize("game,n,sims,ev,fpu", [("reversi6", 8, 48, "hash", (0.2, 0.1)), ("reversi4", 12, 32, "uniform", (0.2, 0.1)),
                                                ("reversi4", 64, 32, "hash", (0.0, 0.0)), ("reversi6", 8, 32, "hash", (3.0, 0.0))])
def test_selfplay_small_boards_equal_the_twin(game, n, sims, ev, fpu):
    """(reductions of 0: an unvisited child is worth exactly its parent -- still the rule; 3.0: f far below -1, no clamp)"""
    _case(game, n, sims, ev, fpu=fpu, temp_moves=3, seed=4, stagger=4 if game == "reversi6" else 0, noise=(ev == "hash"))


def _fixture_roots():
    """Reversi 8x8 roots from tests/golden/reversi_random_games.npz by the number of legal moves: one with <= 16 (one chunk of the
    mass reduction on the 16-lane group), one with 17 .. 32 (two chunks) and the widest the fixtures hold -- 23 legal moves,
    still two chunks: the fixtures have no root above 32, the three-chunk case is tic-tac-toe's"""
    rows = np.load(os.path.join(G, "reversi_random_games.npz"))["rows"]
    r8 = rows[(rows[:, 1] == 8) & (rows[:, 7] != 255)]
    cur = r8[:, 3].astype(np.int64) - 1
    own, opp = np.where(cur == 1, r8[:, 4], r8[:, 5]), np.where(cur == 1, r8[:, 5], r8[:, 4])
    out, lg = {}, C.c_uint64()
    for i in range(len(r8)):
        _lib.check(_lib.lib().bz_reversi_legal(int(own[i]), int(opp[i]), 8, C.byref(lg)))
        n = bin(lg.value).count("1")
        for key, ok in (("one", n == 12), ("two", n == 18), ("widest", n == 23)):
            if ok and key not in out:
                out[key] = (int(own[i]), int(opp[i]), int(cur[i]), n)
    assert set(out) == {"one", "two", "widest"}
    return out


def _root_case(roots, sims, ev="hash", fpu=(0.2, 0.1)):
    """one search from given roots (set_roots) against FpuTwin.search"""
    n = len(roots)
    eng = _engine("reversi", n, sims, ev, Fpu(*fpu))
    eng.set_roots([r[0] for r in roots], [r[1] for r in roots], [r[2] for r in roots])
    eng.search()
    N, W, P = eng.root_stats()
    eng.status()
    changed = 0
    for g, (own, opp, tm, nl) in enumerate(roots):
        x, o = (own, opp) if tm == 1 else (opp, own)
        tw = FpuTwin("reversi", ev, fpu, boards=boards())
        root = tw.search(bz.ReversiBoard.from_bits(x, o, 8), tm, sims)
        a = [e["a"] for e in root["edges"]]
        assert len(a) == nl and int(N[g].sum()) == sims
        assert np.array_equal(N[g, a], np.array([e["N"] for e in root["edges"]], np.uint32)), (g, nl)
        assert np.array_equal(_bits(W[g, a]), _bits([e["W"] for e in root["edges"]])), (g, nl)
        assert np.array_equal(_bits(P[g, a]), _bits([e["P"] for e in root["edges"]])), (g, nl)
        changed += tw.n_changed
    assert changed > 0


def test_fixture_roots_of_every_chunk_class_equal_the_twin_at_200_simulations():
    r = _fixture_roots()
    _root_case([r["one"], r["two"], r["widest"], r["two"], r["one"], r["widest"], r["one"], r["two"]], 200)


def test_one_search_at_800_simulations_equals_the_twin():
    _root_case([_fixture_roots()["widest"]], 800)


# ---------------------------------------------------------------- the cap and forced playouts
@pytest.mark.parametrize("full_q", [0, 16384, 65536])
def test_selfplay_under_the_cap_equals_the_twin(full_q):
    """fast searches use the rule too (without noise); only the full ones record"""
    eng, twins, _ = _case("reversi", 8, 32, "hash", cap=(8, full_q), temp_moves=8, openings=1, seed=3, base=7, stagger=5)
    all_b = {b for tw, _, _ in twins for b in tw.budgets}
    assert all_b == ({32, 8} if 0 < full_q < 65536 else {32} if full_q else {8})
    if full_q == 0:
        assert len(eng.examples()) == 0
    _case("ttt", 12, 40, "uniform", cap=(8, full_q), temp_moves=4, seed=1, stagger=3)


def test_forced_playouts_under_the_cap_with_pruning_equal_the_twin():
    _, twins, _ = _case("reversi", 8, 32, "hash", k=2.0, prune=True, cap=(8, 32768), temp_moves=8, openings=1, seed=3, base=7, stagger=5)
    assert sum(tw.n_overrides for tw, _, _ in twins) > 0 and any(lg["Np"] != lg["N"] for tw, _, _ in twins for lg in tw.log)
    _, twins, _ = _case("ttt", 12, 40, "hash", k=2.0, prune=True, temp_moves=4, seed=1, stagger=3)  # (k_fpu_forced_step)
    assert sum(tw.n_overrides for tw, _, _ in twins) > 0 and any(lg["Np"] != lg["N"] for tw, _, _ in twins for lg in tw.log)


# ---------------------------------------------------------------- evaluators and the evaluation cache
def test_net_f32_selfplay_equals_the_twin_with_the_per_position_forward():
    dn = _net32()
    _case("reversi", 4, 16, "net", engine_ev="net_f32", eval_fn=_net_fn(dn), net=dn, temp_moves=8, openings=1, seed=3)


@pytest.mark.parametrize("cache", [False, "search", True])
def test_exact_bf16_net_and_every_cache_mode_equal_the_twin(cache):
    """the search-grade exact bf16 net (tests/test_search_net_cpu.py); the cache is keyed by position and confirmed against it:
    n_net_leaves + n_cache_hits is the twin's evaluation count in every mode"""
    from test_gpu_search_net import _dn, _net
    from test_search_net_cpu import oracle_eval_fn
    P, on = _net("bf16", 64, 1)
    _, twins, cnt = _case("reversi6", 8, 32, "net", engine_ev="net_bf16", eval_fn=oracle_eval_fn(on, "bf16"), net=_dn(P, 8),
                          temp_moves=4, seed=2, stagger=3, eval_cache=cache)
    assert cnt["n_net_leaves"] + cnt["n_cache_hits"] == sum(tw.n_evals for tw, _, _ in twins), cnt
    assert (cnt["n_cache_hits"] > 0) == (cache is not False), cnt
    assert (cnt["n_cache_hits_prev"] > 0) == (cache is True), cnt


def test_external_evaluator_through_the_step_api_equals_the_twin():
    """select / expand_backup as separate launches: the expand-only step advances Wr, the select-only step reads it"""
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


# ---------------------------------------------------------------- the observing options
def test_surprise_and_search_value_columns_equal_the_twins():
    class cls(FpuTwin):  # both observers on one twin (each mixin keeps its own view of every searched root)
        kl_rows, row_kl, q_rows, row_q = _Surprise.kl_rows, _Surprise.row_kl, _Value.q_rows, _Value.row_q

        def root_noise(self, root):
            _Surprise._keep(self, root)
            _Value._keep(self, root)
            super().root_noise(root)
    eng, twins, _ = _case("reversi4", 8, 32, "hash", temp_moves=3, seed=5, cls=cls, surprise=True, search_value=True)
    ex = eng.examples()
    for g, (tw, rows, w) in enumerate(twins):
        msk = ex.game == g
        assert np.array_equal(_bits(ex.kl[msk]), _bits(tw.kl_rows(rows))), g
        assert np.array_equal(_bits(ex.q[msk]), _bits(tw.q_rows(rows))), g
    assert (ex.kl > 0).any() and (ex.q != 0).any()


def test_eval_symmetry_with_the_rule_plays_the_games_of_a_second_identical_engine_and_not_the_plain_ones():
    """(the symmetry changes the evaluator, not the rule: pinned product against product, as tests/test_gpu_symmetry.py does)"""
    from betazero_amd.engine import EvalSymmetry
    dn = _net32()
    kw = dict(net=dn, temp_moves=4, openings=1, seed=6, eval_symmetry=EvalSymmetry(11))
    a, (wa, la), ca = _run(_engine("reversi", 6, 16, "net_f32", True, **kw))
    b, (wb, lb), cb = _run(_engine("reversi", 6, 16, "net_f32", True, **kw))
    assert len(a) == len(b) > 0 and np.array_equal(wa, wb) and np.array_equal(a.act, b.act) and np.array_equal(_bits(a.pi), _bits(b.pi))
    c, _, _ = _run(_engine("reversi", 6, 16, "net_f32", None, **kw))
    assert c.pi.shape != a.pi.shape or not np.array_equal(_bits(c.pi), _bits(a.pi))


# ---------------------------------------------------------------- pipelines, matches, players
def test_two_pipelines_equal_the_twin():
    from betazero_amd.engine import PipelinedSelfPlay
    n, sims = 12, 32
    sp = PipelinedSelfPlay("reversi", n, sims, "hash", pipelines=2, fpu=True, temp_moves=6, openings=1, seed=9, game_id_base=100, **NOISE)
    sp.reset_counters()
    sp.run_iteration()
    assert sp.status()[0] == 0
    ex, (winners, lens), cnt = sp.examples(), sp.winners(), sp.counters()
    r = (float(np.float32(0.2)), float(np.float32(0.1)))
    twins = _twins("reversi", "hash", 6, sims, r, None, True, None, 6, 1, 9, 100, 0, None, True) + \
        _twins("reversi", "hash", 6, sims, r, None, True, None, 6, 1, 9, 100, 0, None, True, slot0=6)
    for g, (tw, rows, w) in enumerate(twins):
        assert lens[0, g] == len(rows) and winners[0, g] == w, g
        _same_rows(ex, 100 + g, rows, w)
    assert cnt["n_sims"] == sum(b for tw, _, _ in twins for b in tw.budgets) and len(ex) == sum(len(r) for _, r, _ in twins)
    assert sum(tw.n_changed for tw, _, _ in twins) > 0


def test_self_play_takes_fpu():
    from betazero_amd.engine import self_play
    s, pi, z, ex = self_play("reversi4", 8, 32, seed=3, evaluator="hash", temp_moves=4, fpu=Fpu(0.3, 0.2), **NOISE)
    twins = _twins("reversi4", "hash", 8, 32, (0.3, 0.2), None, True, None, 4, 0, 3, 0, 0, None, True)
    for g, (tw, rows, w) in enumerate(twins):
        _same_rows(ex, g, rows, w)


def test_match_with_fpu_on_side_a_only_equals_the_match_twin():
    a, b = MatchPlayer(sims=32, evaluator="hash", fpu=True), MatchPlayer(sims=32, evaluator="hash")
    sa = FpuSide(32, "hash")
    ref, _ = MatchTwin("reversi4", sa, Side(32, "hash"), 2, 3).play(16)
    res = play_match("reversi", 16, a, b, size=4, opening_plies=2, seed=3)
    assert_same_match(res, ref, "fpu vs plain")
    assert sa.twin("reversi4").n_changed > 0
    ref, _ = MatchTwin("reversi4", Side(32, "hash"), FpuSide(32, "hash"), 2, 3).play(16)
    assert_same_match(play_match("reversi", 16, b, a, size=4, opening_plies=2, seed=3), ref, "plain vs fpu")
    plain = play_match("reversi", 16, b, b, size=4, opening_plies=2, seed=3)
    assert not np.array_equal(plain.actions, res.actions)  # neither is the match without the option


def test_the_same_fpu_player_on_both_sides_scores_exactly_half():
    p = MatchPlayer(sims=32, evaluator="hash", fpu=Fpu(0.2, 0.1))
    res = play_match("reversi", 16, p, p, size=6, opening_plies=2, seed=5)
    assert res.summary()["score"] == 0.5 and not res.pair_score.any()


def test_mcts_player_get_move_equals_the_twin():
    board = bz.ReversiBoard(size=8)
    pl = bz.MCTSPlayer(1, sims=64, evaluator="hash", fpu=True)
    mv = pl.get_move(board)
    tw = FpuTwin("reversi", "hash", (float(np.float32(0.2)), float(np.float32(0.1))), boards=boards())
    root = tw.search(board, 1, 64)
    N = [e["N"] for e in root["edges"]]
    a = root["edges"][int(np.argmax(N))]["a"]
    assert mv == (a // 8, a % 8) and [int(pl.last_visits[e["a"]]) for e in root["edges"]] == N and tw.n_changed > 0


# ---------------------------------------------------------------- on and off
def test_switching_off_restores_the_plain_engine_and_the_fused_search():
    kw = dict(temp_moves=4, openings=1, seed=2)
    eng = _engine("reversi", 8, 16, "hash", True, **kw)
    on1, (w1, _), _ = _run(eng)
    eng.set_fpu(None)
    a, (wa, la), ca = _run(eng)
    b, (wb, lb), cb = _run(_engine("reversi", 8, 16, "hash", None, **kw))
    assert np.array_equal(wa, wb) and np.array_equal(la, lb) and np.array_equal(a.act, b.act) and np.array_equal(_bits(a.pi), _bits(b.pi))
    assert ca == cb
    eng.set_fpu(True)  # ... and on again: the first run's games
    c, (wc, _), _ = _run(eng)
    assert np.array_equal(wc, w1) and np.array_equal(c.act, on1.act) and np.array_equal(_bits(c.pi), _bits(on1.pi))
    assert c.pi.shape != a.pi.shape or not np.array_equal(_bits(c.pi), _bits(a.pi))  # (and they are not the plain engine's)


def test_set_fpu_refuses_the_refused_combinations_and_bad_arguments():
    L = _lib.lib()
    st = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda:0")
    p = buf.data_ptr() + ((-buf.data_ptr()) & 255)
    on = lambda e, r=0.2, r0=0.1, ptr=p, nb=4096: L.bz_engine_set_fpu(e.h, 1, C.c_float(r), C.c_float(r0), ptr, nb, st)  # noqa: E731
    for kw, word in (({"leaves_per_step": 2}, b"leaves_per_step"), ({"reuse_subtree": True}, b"subtree reuse"), ({"gumbel": True}, b"Gumbel")):
        eng = _engine("reversi", 4, 16, "hash", None, **kw)
        assert on(eng) == _lib.BZ_EINVAL
        assert word in L.bz_last_error() and b"first-play urgency" in L.bz_last_error(), L.bz_last_error()
        assert L.bz_engine_set_fpu(eng.h, 0, C.c_float(0.0), C.c_float(0.0), None, 0, st) == _lib.BZ_OK  # "off" is always accepted
    eng = _engine("reversi", 4, 16, "hash", None, cap=(4, 16384), forced=ForcedPlayouts(2.0), **NOISE)  # all allowed
    for r, r0 in ((-1.0, 0.1), (0.2, -0.1), (float("inf"), 0.1), (0.2, float("nan"))):
        assert on(eng, r, r0) == _lib.BZ_EINVAL and b"finite" in L.bz_last_error()
    assert on(eng, ptr=None) == _lib.BZ_EINVAL and on(eng, ptr=p + 4) == _lib.BZ_EINVAL and b"aligned" in L.bz_last_error()
    assert on(eng, nb=8) == _lib.BZ_ENOMEM and b"too small" in L.bz_last_error()
    assert on(eng) == _lib.BZ_OK and on(eng, 0.0, 0.0) == _lib.BZ_OK
    gbuf = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda:0")
    eng2 = _engine("reversi", 4, 16, "hash", True)
    assert L.bz_engine_set_gumbel(eng2.h, 16, 1.0, 50.0, 0.1, gbuf.data_ptr(), gbuf.numel(), st) == _lib.BZ_EINVAL  # the rule is on
    assert b"first-play urgency" in L.bz_last_error()
    eng2.set_fpu(None)
    assert L.bz_engine_set_gumbel(eng2.h, 16, 1.0, 50.0, 0.1, gbuf.data_ptr(), gbuf.numel(), st) == _lib.BZ_OK
    torch.cuda.synchronize()


# ---------------------------------------------------------------- the loop
def test_az_loop_runs_two_iterations_with_fpu_under_the_cap():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "az_loop.py"), "--iters", "2", "--games", "64", "--sims", "16",
                          "--fpu-reduction", "0.2", "--fast-sims", "4", "--full-prob", "0.5", "--channels", "64", "--blocks", "1",
                          "--arena-games", "16", "--arena-sims", "8", "--depth", "1", "--final-depths", "", "--gate-games", "8"],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    its = [d for d in (json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")) if d.get("what") == "iteration"]
    assert [d["iter"] for d in its] == [1, 2]
    for d in its:
        assert 0 < d["rows_per_game"] < d["plies"] and d["games_per_s"] > 0 and d["gate"]["games"] == 8, d
        assert np.allclose(d["fpu"], [0.2, 0.1])
