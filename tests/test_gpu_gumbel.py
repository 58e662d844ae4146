"""Gumbel root search on the GPU: k_gumbel_step / k_gumbel_root / k_gumbel_play against the Gumbel twin of
tests/test_gumbel_cpu.py.  "Bit-exact" = root N / W / P, pi', moves, z and every example row equal to the twin's."""

import numpy as np
import pytest
import torch

from betazero_amd import _lib
from betazero_amd.engine import GumbelConfig
from oracle import py_twin
from test_gpu_leaf_parallel import _net32, _net_fn, _root_arrays, _same_root
from test_gumbel_cpu import ARENA_SIMS, GumbelTwin, boards, game_roots

pytestmark = pytest.mark.gpu


def _engine(game, n, sims, ev, gumbel=True, **kw):
    from betazero_amd.engine import SelfPlayEngine
    return SelfPlayEngine(game, n, sims, ev, gumbel=gumbel, **kw)


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _search_case(game, ev, m, scale, sims, roots, eval_fn=None, net=None, external=None, seed=5, engine_ev=None):
    """one search from every root (temp_moves 1: the noise is on when scale > 0), engine vs twin (ev: the twin's evaluator;
    engine_ev: the engine's, when it is not the same name)"""
    B = len(roots)
    eng = _engine(game, B, sims, "external" if external else (engine_ev or ev), GumbelConfig(m, scale), net=net, temp_moves=1,
                  seed=seed)
    eng.set_roots([r[2] for r in roots], [r[3] for r in roots], [r[1] for r in roots])
    if external:
        eng.search_external(external)
    else:
        eng.search()
    NWP = eng.root_stats()
    pi, act = eng.root_policy()
    eng.status()
    for g, (b, p, _, _) in enumerate(roots):
        tw = GumbelTwin(game, ev, m=m, scale=scale, eval_fn=eval_fn, boards=boards())
        root = tw.search(b, p, sims, scale > 0, (seed, g, 0))
        _same_root(NWP, g, tw, root)
        tpi, ta = tw.policy(root)
        assert np.array_equal(_bits(pi[g]), _bits(tpi)), (g, pi[g], tpi)
        assert act[g] == ta, (g, act[g], ta)


@pytest.mark.parametrize("game", ["ttt", "reversi", "reversi6", "reversi4"])
@pytest.mark.parametrize("ev", ["hash", "uniform"])
def test_single_searches_bitexact_vs_twin(game, ev):
    roots = game_roots(game, 2, seed=7)
    for m in (1, 2, 4, 16):
        for scale in (0.0, 1.0):
            for sims in (1, 7, 32, 200) + ((800,) if m == 16 else ()):
                _search_case(game, ev, m, scale, sims, roots)


def _selfplay_case(game, n, sims, ev, m=16, scale=1.0, temp_moves=0, openings=0, seed=0, base=0, stagger=0, eval_fn=None,
                   net=None, **kw):
    eng = _engine(game, n, sims, ev, GumbelConfig(m, scale), net=net, temp_moves=temp_moves, openings=openings, seed=seed,
                  game_id_base=base, stagger=stagger, **kw)
    eng.reset_counters()
    eng.run_iteration()
    eng.status()
    ex = eng.examples()
    winners, lens = eng.winners()
    cnt = eng.counters()
    n_search = 0
    for g in range(n):
        tw = GumbelTwin(game, ev, m=m, scale=scale, eval_fn=eval_fn, boards=boards())
        rows, w, _ = tw.selfplay(base + g, sims, temp_moves, openings, seed, slot=g, stagger=stagger)
        msk = ex.game == base + g
        assert lens[0, g] == len(rows) and winners[0, g] == w, (g, lens[0, g], len(rows))
        assert np.array_equal(ex.own[msk], np.array([r[0] for r in rows], np.uint64))
        assert np.array_equal(ex.opp[msk], np.array([r[1] for r in rows], np.uint64))
        assert np.array_equal(_bits(ex.pi[msk]), _bits([r[2] for r in rows]))
        assert np.array_equal(ex.mover[msk], np.array([r[3] for r in rows], np.int8))
        assert np.array_equal(ex.act[msk], np.array([r[4] for r in rows], np.uint8))
        assert np.array_equal(ex.z[msk], (w * np.array([r[3] for r in rows])).astype(np.int8))
        n_search += len(rows)
    assert cnt["n_sims"] == n_search * sims, cnt
    return eng


def test_selfplay_bitexact_with_temperature_openings_and_a_staggered_pool():
    _selfplay_case("reversi", 12, 24, "hash", m=8, temp_moves=8, openings=1, seed=3, base=7, stagger=5)
    _selfplay_case("ttt", 16, 40, "hash", m=4, temp_moves=4, seed=1, stagger=3)
    _selfplay_case("reversi6", 6, 30, "uniform", m=16, temp_moves=2, seed=2, stagger=4)
    _selfplay_case("reversi4", 8, 16, "hash", m=2, scale=0.5, temp_moves=3, seed=4)


def test_net_f32_search_and_selfplay_vs_twin_with_the_per_position_forward():
    dn = _net32()
    fn = _net_fn(dn)
    roots = game_roots("reversi", 3, seed=11)
    _search_case("reversi", "net", 16, 1.0, 50, roots, eval_fn=fn, net=dn, engine_ev="net_f32")
    _search_case("reversi", "net", 4, 0.0, 32, roots, eval_fn=fn, net=dn, engine_ev="net_f32")
    eng = _engine("reversi", 4, 12, "net_f32", GumbelConfig(8), net=dn, temp_moves=8, openings=1)
    eng.run_iteration()
    eng.status()
    ex = eng.examples()
    for g in range(4):
        tw = GumbelTwin("reversi", "net", m=8, eval_fn=fn, boards=boards())
        rows, w, _ = tw.selfplay(g, 12, 8, 1, 0)
        msk = ex.game == g
        assert np.array_equal(ex.act[msk], np.array([r[4] for r in rows], np.uint8))
        assert np.array_equal(_bits(ex.pi[msk]), _bits([r[2] for r in rows]))
        assert eng.winners()[0][0, g] == w


def test_mlp_f32_search_vs_twin_with_the_per_position_forward():
    from betazero_amd.mlp import DeviceMLP, TicTacToeNet
    torch.manual_seed(2)
    mlp = DeviceMLP.from_module(TicTacToeNet(9, 64, 9), max_batch=64)

    def fn(own, opp):
        return mlp.forward(np.array([own], np.uint64), np.array([opp], np.uint64))[0].cpu().numpy(), np.float32(0.0)
    roots = game_roots("ttt", 3, seed=5)
    for m, scale, sims in ((4, 1.0, 50), (16, 0.0, 101)):
        _search_case("ttt", "mlp", m, scale, sims, roots, eval_fn=fn, net=mlp, engine_ev="mlp_f32")


def test_search_external_vs_twin():
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
    _search_case("reversi", "hash", 16, 1.0, 101, roots, external=external)
    _search_case("reversi", "hash", 2, 0.0, 32, roots, external=external)


def test_eval_cache_changes_no_result_under_gumbel():
    from betazero_amd.net import DeviceNet, PolicyValueNet
    torch.manual_seed(0)
    dn = DeviceNet.from_module(PolicyValueNet(64, 2, 64).round_to_bf16_(), 64)
    out = []
    for cache in (False, "search", True):
        eng = _engine("reversi", 8, 40, "net_bf16", True, net=dn, temp_moves=8, openings=1, eval_cache=cache)
        eng.reset_counters()
        eng.run_iteration(max_plies=8)
        eng.status()
        c = eng.counters()
        assert (c["n_cache_hits"] > 0) == (cache is not False), (cache, c)
        if cache is True:
            assert c["n_cache_hits_prev"] > 0, c
        t = eng.example_tensors()
        out.append((t["pi"].cpu().numpy().copy(), t["act"].cpu().numpy().copy(), eng.positions()[0].copy()))
    for x in out[1:]:
        assert np.array_equal(out[0][0].view(np.uint32), x[0].view(np.uint32))
        assert np.array_equal(out[0][1], x[1]) and np.array_equal(out[0][2], x[2])


def test_two_pipelines_give_the_rows_of_one_engine():
    from betazero_amd.engine import PipelinedSelfPlay
    kw = dict(temp_moves=6, openings=1, seed=9)
    sp = PipelinedSelfPlay("reversi", 16, 24, "hash", pipelines=2, gumbel=GumbelConfig(8), **kw)
    sp.run_iteration()
    a = sp.examples()
    eng = _engine("reversi", 16, 24, "hash", GumbelConfig(8), **kw)
    eng.run_iteration()
    eng.status()
    b = eng.examples()
    ia, ib = np.lexsort((a.ply, a.game)), np.lexsort((b.ply, b.game))
    assert len(a) == len(b) > 0
    for f in ("own", "opp", "z", "mover", "act", "game", "ply"):
        assert np.array_equal(getattr(a, f)[ia], getattr(b, f)[ib]), f
    assert np.array_equal(_bits(a.pi[ia]), _bits(b.pi[ib]))


@pytest.mark.parametrize("game,temp", [("reversi", 0), ("reversi", 64), ("ttt", 9), ("reversi4", 0)])
def test_root_policy_in_puct_mode_is_what_play_writes(game, temp):
    eng = _engine(game, 12, 40, "hash", None, temp_moves=temp, openings=1, seed=4)
    eng.reset_games()
    for ply in range(3):
        eng.search()
        pi, act = eng.root_policy()
        state = eng.positions()[3].copy()
        eng.play(False)
        eng.status()
        t = eng.example_tensors()
        for g in range(12):
            if state[g] != 0:
                assert act[g] == -1 and not pi[g].any()
                continue
            assert np.array_equal(_bits(t["pi"][0, g, ply].cpu().numpy()), _bits(pi[g])), (g, ply)
            assert int(t["act"][0, g, ply]) == act[g], (g, ply)


def test_root_policy_marks_idle_slots():
    tw = GumbelTwin("reversi", "hash", boards=boards())
    b, p, own, opp = game_roots("reversi", 1, seed=0)[0]
    eng = _engine("reversi", 3, 16, "hash", True)
    eng.set_roots([own, own, own], [opp, opp, opp], [p, 0, p])
    eng.search()
    pi, act = eng.root_policy()
    eng.status()
    assert act[1] == -1 and not pi[1].any()
    tpi, ta = tw.policy(tw.search(b, p, 16))
    for g in (0, 2):
        assert act[g] == ta and np.array_equal(_bits(pi[g]), _bits(tpi))


def test_mcts_player_plays_the_twins_move():
    import betazero_amd as bz
    from betazero_amd.players import MCTSPlayer
    b = bz.ReversiBoard(size=8)
    for sims, m in ((16, 16), (101, 4)):
        pl = MCTSPlayer(1, sims, evaluator="hash", gumbel=GumbelConfig(m))
        r, c = pl.get_move(b)
        tw = GumbelTwin("reversi", "hash", m=m, boards=boards())
        root = tw.search(b, 1, sims)
        tpi, ta = tw.policy(root)
        n, _, _ = _root_arrays(tw, root)
        assert np.array_equal(pl.last_visits, n) and 8 * r + c == ta
        assert np.array_equal(_bits(pl.last_policy), _bits(tpi))


def test_arena_in_gumbel_mode_never_loses_at_tictactoe():
    from betazero_amd.arena import play_arena
    res = play_arena("ttt", 64, ARENA_SIMS, evaluator="uniform", seed=1, gumbel=True)
    s = res.summary()
    print(f"ttt arena, Gumbel, {ARENA_SIMS} sims:", s)
    assert s["losses"] == 0 and s["games"] == 64


def test_set_gumbel_refuses_the_refused_combinations():
    L = _lib.lib()
    buf = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    for kw, word in (({"leaves_per_step": 2}, b"leaves_per_step"), ({"reuse_subtree": True}, b"subtree reuse"),
                     ({"dirichlet_alpha": 0.3, "dirichlet_eps": 0.25}, b"Dirichlet")):
        eng = _engine("reversi", 4, 16, "hash", None, **kw)
        assert L.bz_engine_set_gumbel(eng.h, 16, 1.0, 50.0, 0.1, buf.data_ptr(), buf.numel(), st) == _lib.BZ_EINVAL
        assert word in L.bz_last_error()
    eng = _engine("reversi", 4, 16, "hash", None)
    assert L.bz_engine_set_gumbel(eng.h, 16, -1.0, 50.0, 0.1, buf.data_ptr(), buf.numel(), st) == _lib.BZ_EINVAL
    assert L.bz_engine_set_gumbel(eng.h, 65, 1.0, 50.0, 0.1, buf.data_ptr(), buf.numel(), st) == _lib.BZ_EINVAL
    assert L.bz_engine_set_gumbel(eng.h, 16, 1.0, 50.0, 0.1, buf.data_ptr(), 64, st) == _lib.BZ_ENOMEM
    assert L.bz_engine_set_gumbel(eng.h, 0, 0.0, 0.0, 0.0, None, 0, st) == _lib.BZ_OK  # off needs no buffer


def test_engines_step_refuses_mixed_modes():
    from betazero_amd.engine import PipelinedSelfPlay
    sp = PipelinedSelfPlay("reversi", 8, 8, "hash", pipelines=2, gumbel=True)
    L = _lib.lib()
    assert L.bz_engine_set_gumbel(sp.engines[1].h, 0, 0.0, 0.0, 0.0, None, 0, torch.cuda.current_stream().cuda_stream) == 0
    sp.reset_games()
    with pytest.raises(RuntimeError, match="Gumbel"):
        sp.step()
