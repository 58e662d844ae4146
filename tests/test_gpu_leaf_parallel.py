"""Leaf-parallel MCTS on the GPU: k_leaf_step against the K-walk twin of tests/test_leaf_parallel_cpu.py.
"Bit-exact" = root N / W / P, pi, moves, z and every example row equal to the twin's."""

import numpy as np
import pytest
import torch

from betazero_amd import _lib
from oracle import py_twin
from test_leaf_parallel_cpu import KTwin, boards, hand_checked_collision_w, one_move_position

pytestmark = pytest.mark.gpu


def _engine(game, n, sims, ev, K, **kw):
    from betazero_amd.engine import SelfPlayEngine
    return SelfPlayEngine(game, n, sims, ev, leaves_per_step=K, **kw)


def _roots(game, n_roots, seed):
    """a few positions along a pseudo-random game: (board object, mover, own, opp)"""
    tw = KTwin(game, "uniform", boards=boards())
    rng = np.random.default_rng(seed)
    b = tw.TicTacToeBoard() if tw.game == "ttt" else tw.ReversiBoard(size=tw.size)
    p, out = 1, []
    while len(out) < n_roots:
        if tw.terminal(b)[0]:
            break
        mv = tw.moves(b, p)
        if not mv:
            p = -p
            continue
        own, opp = tw.bits(b, p)
        out.append((b, p, own, opp))
        b, p = tw.play(b, p, mv[int(rng.integers(len(mv)))]), -p
        if game == "ttt" and len(out) >= 3:
            break
    return out


def _root_arrays(tw, root):
    N = np.zeros(tw.na, np.uint32)
    W = np.zeros(tw.na, np.float32)
    P = np.zeros(tw.na, np.float32)
    for e in root["edges"]:
        N[e["a"]], W[e["a"]], P[e["a"]] = e["N"], e["W"], e["P"]
    return N, W, P


def _same_root(eng_NWP, g, tw, root):
    N, W, P = eng_NWP
    n, w, p = _root_arrays(tw, root)
    assert np.array_equal(N[g], n), (N[g], n)
    assert np.array_equal(W[g].view(np.uint32), w.view(np.uint32))
    assert np.array_equal(P[g].view(np.uint32), p.view(np.uint32))


def _search_case(game, ev, K, sims, eval_fn=None, net=None, external=None, **kw):
    roots = _roots(game, 3, seed=K * 1000 + sims)
    B = len(roots)
    eng = _engine(game, B, sims, external and "external" or ev, K, net=net, **kw)
    eng.set_roots([r[2] for r in roots], [r[3] for r in roots], [r[1] for r in roots])
    eng.reset_counters()
    if external:
        eng.search_external(external)
    else:
        eng.search()
    NWP = eng.root_stats()
    eng.status()
    cnt = eng.counters()
    n_coll = 0
    for g, (b, p, _, _) in enumerate(roots):
        tw = KTwin(game, ev, leaves=K, eval_fn=eval_fn, boards=boards())
        root = tw.search(b, p, sims)
        _same_root(NWP, g, tw, root)
        n_coll += tw.n_collisions
    assert cnt["n_sims"] == B * sims and cnt["n_collisions"] == n_coll, (cnt, n_coll)
    assert cnt["n_cache_hits"] == 0
    return n_coll


@pytest.mark.parametrize("game", ["ttt", "reversi", "reversi6", "reversi4"])
@pytest.mark.parametrize("ev", ["hash", "uniform"])
def test_single_searches_bitexact_vs_twin(game, ev):
    colls = 0
    for K in (2, 3, 8, 32):
        for sims in (50, 101) if game != "reversi4" or K != 32 else (50, 101, 800):
            colls += _search_case(game, ev, K, sims)
    if game != "ttt" or ev == "uniform":
        assert colls > 0  # the engine met the collision rule where the twin predicts it


def test_collision_backs_up_the_pending_nodes_value():
    """one K = 2 step over a root with a single legal move: walk 1 collides at the node walk 0 created; the root edge's W
    is the hand-computed (((0 - 1) - 1 + 1) - v + 1) - v of DESIGN.md 3.12, N = 2, one collision, one evaluator row"""
    b, p, ch, q = one_move_position()
    tw = KTwin("reversi", "hash", boards=boards())
    own, opp = tw.bits(b, p)
    cown, copp = tw.bits(ch, q)
    v = py_twin.eval_hash(cown, copp, 65)[1]
    eng = _engine("reversi", 1, 2, "hash", 2)
    eng.set_roots([own], [opp], [p])
    eng.reset_counters()
    eng.search()
    N, W, _ = eng.root_stats()
    eng.status()
    a = int(np.nonzero(N[0])[0][0])
    assert N[0][a] == 2 and N[0].sum() == 2
    assert float(W[0][a]).hex() == float(hand_checked_collision_w(v)).hex()
    c = eng.counters()
    assert c["n_collisions"] == 1 and c["n_sims"] == 2 and c["n_expanded"] == 2


def test_800_sim_search_bitexact_vs_twin():
    assert _search_case("reversi", "hash", 8, 800) > 0


def _selfplay_case(game, n, sims, ev, K, temp_moves=0, openings=0, seed=0, base=0, stagger=0, eval_fn=None, net=None,
                   dir_alpha=0.0, dir_eps=0.0, reuse=False, **kw):
    eng = _engine(game, n, sims, ev, K, net=net, temp_moves=temp_moves, openings=openings, seed=seed, game_id_base=base,
                  stagger=stagger, dirichlet_alpha=dir_alpha, dirichlet_eps=dir_eps, reuse_subtree=reuse, **kw)
    eng.reset_counters()
    eng.run_iteration()
    eng.status()
    ex = eng.examples()
    winners, lens = eng.winners()
    cnt = eng.counters()
    n_coll, n_search = 0, 0
    for g in range(n):
        tw = KTwin(game, ev, leaves=K, eval_fn=eval_fn, boards=boards(), dir_alpha=dir_alpha, dir_eps=dir_eps, reuse=reuse)
        rows, w, _ = tw.selfplay(base + g, sims, temp_moves, openings, seed, slot=g, stagger=stagger)
        m = ex.game == base + g
        assert lens[0, g] == len(rows) and winners[0, g] == w, (g, lens[0, g], len(rows))
        assert np.array_equal(ex.own[m], np.array([r[0] for r in rows], np.uint64))
        assert np.array_equal(ex.opp[m], np.array([r[1] for r in rows], np.uint64))
        assert np.array_equal(ex.pi[m].view(np.uint32), np.array([r[2] for r in rows], np.float32).view(np.uint32))
        assert np.array_equal(ex.mover[m], np.array([r[3] for r in rows], np.int8))
        assert np.array_equal(ex.act[m], np.array([r[4] for r in rows], np.uint8))
        assert np.array_equal(ex.z[m], (w * np.array([r[3] for r in rows])).astype(np.int8))
        n_coll += tw.n_collisions
        n_search += len(rows)
    assert cnt["n_sims"] == n_search * sims and cnt["n_collisions"] == n_coll, (cnt, n_coll)
    return n_coll


def test_selfplay_bitexact_with_temperature_openings_and_a_staggered_pool():
    assert _selfplay_case("reversi", 12, 24, "hash", 8, temp_moves=8, openings=1, seed=3, base=7, stagger=5) > 0
    _selfplay_case("ttt", 16, 40, "hash", 4, temp_moves=4, seed=1, stagger=3)
    _selfplay_case("reversi6", 6, 30, "uniform", 3, temp_moves=2, seed=2, stagger=4)


def test_selfplay_bitexact_with_dirichlet_noise():
    _selfplay_case("reversi", 8, 24, "hash", 8, temp_moves=4, openings=1, seed=5, dir_alpha=0.3, dir_eps=0.25)
    _selfplay_case("ttt", 8, 30, "uniform", 4, seed=6, dir_alpha=1.0, dir_eps=0.5)


def test_selfplay_bitexact_with_subtree_reuse():
    _selfplay_case("reversi", 8, 24, "hash", 8, temp_moves=4, openings=1, seed=8, reuse=True)
    _selfplay_case("reversi4", 8, 40, "hash", 3, temp_moves=2, seed=9, reuse=True, dir_alpha=0.5, dir_eps=0.25)


def _net32():
    from betazero_amd.net import DeviceNet, PolicyValueNet
    torch.manual_seed(4)
    m = PolicyValueNet(32, 2, 64)
    return DeviceNet.from_module(m, 64)


def _net_fn(dn):
    def fn(own, opp):
        t = lambda x: torch.tensor([np.uint64(x).view(np.int64)], device="cuda:0")  # noqa: E731
        lg, v = dn.forward(t(own), t(opp), bf16=False)
        return lg[0].cpu().numpy(), np.float32(v[0].item())
    return fn


def test_net_f32_search_and_selfplay_vs_twin_with_the_per_position_forward():
    dn = _net32()
    fn = _net_fn(dn)
    roots = _roots("reversi", 3, seed=11)
    eng = _engine("reversi", 3, 50, "net_f32", 8, net=dn)
    eng.set_roots([r[2] for r in roots], [r[3] for r in roots], [r[1] for r in roots])
    eng.search()
    NWP = eng.root_stats()
    eng.status()
    for g, (b, p, _, _) in enumerate(roots):
        tw = KTwin("reversi", "net", leaves=8, eval_fn=fn, boards=boards())
        _same_root(NWP, g, tw, tw.search(b, p, 50))
    eng = _engine("reversi", 4, 12, "net_f32", 4, net=dn, temp_moves=8, openings=1)
    eng.run_iteration()
    eng.status()
    ex = eng.examples()
    for g in range(4):
        tw = KTwin("reversi", "net", leaves=4, eval_fn=fn, boards=boards())
        rows, w, _ = tw.selfplay(g, 12, 8, 1, 0)
        m = ex.game == g
        assert np.array_equal(ex.act[m], np.array([r[4] for r in rows], np.uint8))
        assert np.array_equal(ex.pi[m].view(np.uint32), np.array([r[2] for r in rows], np.float32).view(np.uint32))
        assert eng.winners()[0][0, g] == w


def test_mlp_f32_search_vs_twin_with_the_per_position_forward():
    from betazero_amd.mlp import DeviceMLP, TicTacToeNet
    torch.manual_seed(2)
    mlp = DeviceMLP.from_module(TicTacToeNet(9, 64, 9), max_batch=64)

    def fn(own, opp):
        return mlp.forward(np.array([own], np.uint64), np.array([opp], np.uint64))[0].cpu().numpy(), np.float32(0.0)
    roots = _roots("ttt", 3, seed=5)
    for K, sims in ((3, 50), (8, 101)):
        eng = _engine("ttt", len(roots), sims, "mlp_f32", K, net=mlp)
        eng.set_roots([r[2] for r in roots], [r[3] for r in roots], [r[1] for r in roots])
        eng.search()
        NWP = eng.root_stats()
        eng.status()
        for g, (b, p, _, _) in enumerate(roots):
            tw = KTwin("ttt", "mlp", leaves=K, eval_fn=fn, boards=boards())
            _same_root(NWP, g, tw, tw.search(b, p, sims))


def test_search_external_with_k_gt_1_vs_twin():
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
    _search_case("reversi", "hash", 8, 101, external=external)
    _search_case("reversi", "hash", 3, 50, external=external)


def test_eval_cache_is_ignored_with_k_gt_1():
    from betazero_amd.net import DeviceNet, PolicyValueNet
    torch.manual_seed(0)
    dn = DeviceNet.from_module(PolicyValueNet(64, 2, 64).round_to_bf16_(), 64)
    out = []
    for cache in (True, False):
        eng = _engine("reversi", 8, 40, "net_bf16", 8, net=dn, temp_moves=8, openings=1, eval_cache=cache)
        eng.reset_counters()
        eng.run_iteration(max_plies=6)
        eng.status()
        c = eng.counters()
        assert c["n_cache_hits"] == 0 and c["n_cache_hits_prev"] == 0
        out.append((eng.example_tensors()["pi"].cpu().numpy().copy(), eng.positions()[0].copy(), c["n_net_leaves"]))
    assert np.array_equal(out[0][0].view(np.uint32), out[1][0].view(np.uint32))
    assert np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]


def test_set_net_and_set_mlp_refuse_max_batch_below_k_times_b():
    from betazero_amd.mlp import DeviceMLP, TicTacToeNet
    from betazero_amd.net import DeviceNet, PolicyValueNet
    dn = DeviceNet.from_module(PolicyValueNet(32, 2, 64), 15)
    with pytest.raises(RuntimeError, match="max_batch"):
        _engine("reversi", 4, 16, "net_f32", 4, net=dn)
    _engine("reversi", 4, 16, "net_f32", 3, net=dn)  # 12 rows fit
    mlp = DeviceMLP.from_module(TicTacToeNet(9, 32, 9), max_batch=15)
    with pytest.raises(ValueError, match="max_batch"):
        _engine("ttt", 4, 16, "mlp_f32", 4, net=mlp)
    eng = _engine("ttt", 4, 16, "mlp_f32", 4)
    L = _lib.lib()
    assert L.bz_engine_set_mlp(eng.h, mlp.h) == _lib.BZ_EINVAL and b"max_batch" in L.bz_last_error()
    assert L.bz_engine_set_net(_engine("reversi", 4, 16, "net_f32", 4).h, dn.h) == _lib.BZ_EINVAL


def test_arena_with_k8_never_loses_at_tictactoe():
    from betazero_amd.arena import play_arena
    res = play_arena("ttt", 64, 5000, evaluator="uniform", seed=1, leaves_per_step=8)
    s = res.summary()
    print("ttt arena, K = 8:", s)
    assert s["losses"] == 0 and s["games"] == 64


def test_mcts_player_with_k_gt_1_plays_the_twins_move():
    import betazero_amd as bz
    from betazero_amd.players import MCTSPlayer
    b = bz.ReversiBoard(size=8)
    pl = MCTSPlayer(1, 101, evaluator="hash", leaves_per_step=8)
    r, c = pl.get_move(b)
    tw = KTwin("reversi", "hash", leaves=8, boards=boards())
    n, _, _ = _root_arrays(tw, tw.search(b, 1, 101))
    assert np.array_equal(pl.last_visits, n) and 8 * r + c == int(np.argmax(n))


def test_bf16_net_selfplay_with_k8_terminates_legally():
    from betazero_amd.net import DeviceNet, PolicyValueNet
    from oracle import oracle as orc
    torch.manual_seed(0)
    dn = DeviceNet.from_module(PolicyValueNet(128, 6, 64).round_to_bf16_(), 16 * 8)
    eng = _engine("reversi", 16, 32, "net_bf16", 8, net=dn, temp_moves=8, openings=1)
    eng.reset_counters()
    eng.run_iteration()
    eng.status()  # raises on any error flag
    ex = eng.examples()
    winners, lens = eng.winners()
    assert (lens[0] > 40).all()
    for g in range(16):
        m_ = ex.game == g
        own, opp, act = ex.own[m_], ex.opp[m_], ex.act[m_]
        for k in range(len(own)):
            assert orc.reversi_legal(int(own[k]), int(opp[k])) >> int(act[k]) & 1
    c = eng.counters()
    assert c["n_sims"] == 32 * len(ex) and c["n_net_leaves"] + c["n_collisions"] <= c["n_sims"] + 16 * 64
