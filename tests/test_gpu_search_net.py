"""Searches with the bf16 and fp8 nets in the loop against the oracle, bit for bit, on the search-grade exact nets of
tests/test_search_net_cpu.py.

The engine reaches the net kernels through bz_engine_evaluate: max_n = B K picks the tower geometry (latency shape up to 256
rows, throughput shape above), the row count is a device-side, double-buffered count written by select, the rows are what
select packed after the evaluation cache removed repeats (none at all in some steps), and with pipelines two engines on two
streams share one DeviceNet.  On exact nets the device forward equals the oracle's (tests/test_gpu_net_numerics.py) and every
float after the net is specified to the bit, so the engine must equal the oracle's search with
EVAL_NET_BF16 / EVAL_NET_FP8 exactly: root N, W, P bits, every example row, winners, lengths and the work counters
(n_net_leaves + n_cache_hits = the oracle's n_net_leaves; the cache changes nothing else).  K > 1 and Gumbel are held to the
twins of tests/test_leaf_parallel_cpu.py / tests/test_gumbel_cpu.py whose evaluator is the oracle's forward.  Nothing here
has a tolerance."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc
from test_search_net_cpu import ENGINE_EVAL, ORC_EVAL, VH, flat_params, oracle_eval_fn, oracle_net, run_threads, search_net

pytestmark = pytest.mark.gpu
ORC_GAME = {"reversi": orc.GAME_REVERSI, "reversi6": orc.GAME_REVERSI6, "reversi4": orc.GAME_REVERSI4}
WORK = ("n_sims", "n_path_nodes", "n_child_scored", "n_edges_backed", "n_expanded", "n_child_written", "n_env_steps")
_NETS = {}


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _net(mode, C, NB, seed=1):
    """(P, oracle net) of search_net, built once per process"""
    key = (mode, C, NB, seed)
    if key not in _NETS:
        P = search_net(C, NB, VH, mode, seed)
        _NETS[key] = (P, oracle_net(P, mode))
    return _NETS[key]


def _dn(P, max_batch):
    from betazero_amd.net import DeviceNet
    C, L, vh = P["stem_w"].shape[0], P["tw"].shape[0], P["v1_w"].shape[0]
    return DeviceNet(C, L // 2, vh, flat_params(P), max_batch)


def _engine(game, B, sims, mode, dn, **kw):
    from betazero_amd.engine import SelfPlayEngine
    return SelfPlayEngine(game, B, sims, ENGINE_EVAL[mode], net=dn, **kw)


def _oracle_searches(game, mode, on, own, opp, tm, slots, sims):
    return run_threads(lambda i: orc.mcts_search(ORC_GAME[game], int(own[slots[i]]), int(opp[slots[i]]), int(tm[slots[i]]), sims,
                                                 ORC_EVAL[mode], net=on), len(slots))


def _search_equals_oracle(eng, game, mode, on, what, search=None):
    """one search (eng.search(), or search(eng)) from the engine's current positions against the oracle's searches of the
    active slots: root N / W / P bits and the work counters.  Returns (engine counters, oracle counter sums, number of roots)"""
    own, opp, tm, st = eng.positions()
    slots = np.nonzero(st == 0)[0]
    eng.reset_counters()
    (search or type(eng).search)(eng)
    N, W, P = eng.root_stats()
    eng.status()
    cnt = eng.counters()
    res = _oracle_searches(game, mode, on, own, opp, tm, slots, eng.sims)
    tot = {}
    for g, (n, w, p, oc) in zip(slots, res):
        assert np.array_equal(N[g], n), (what, "N", int(g), N[g][N[g] != n], n[N[g] != n])
        assert np.array_equal(_bits(W[g]), _bits(w)), (what, "W", int(g))
        assert np.array_equal(_bits(P[g]), _bits(p)), (what, "P", int(g))
        for k, v in oc.items():
            tot[k] = tot.get(k, 0) + v
    for k in WORK:
        assert cnt[k] == tot.get(k, 0), (what, k, cnt[k], tot.get(k, 0))
    assert cnt["n_net_leaves"] + cnt["n_cache_hits"] == tot.get("n_net_leaves", 0), (what, cnt, tot)
    return cnt, tot, len(slots)


def _moves(eng, game, mode, on, moves, what):
    """`moves` searches, each compared with the oracle, with a move (play) after each"""
    out = []
    for mv in range(moves):
        out.append(_search_equals_oracle(eng, game, mode, on, f"{what} move {mv}"))
        eng.play(False)
    return out


# ---------------------------------------------------------------- (a) every in-loop geometry
# (mode, C, NB, game, B, sims, cache, stagger, moves): B K = 256 is the latency shape, 257 the throughput shape
GEOMETRY = [
    ("bf16", 64, 1, "reversi", 256, 64, True, 30, 2), ("bf16", 64, 1, "reversi", 257, 16, "search", 30, 2),
    ("bf16", 128, 1, "reversi", 256, 16, False, 20, 2), ("bf16", 128, 1, "reversi", 257, 16, True, 20, 2),
    ("bf16", 256, 1, "reversi", 256, 2, "search", 40, 2), ("bf16", 256, 1, "reversi", 257, 2, True, 40, 2),
    ("bf16", 128, 1, "reversi", 1, 800, True, 0, 2), ("bf16", 64, 1, "reversi6", 7, 800, "search", 6, 2),
    ("bf16", 128, 1, "reversi", 384, 1, True, 50, 3), ("bf16", 64, 1, "reversi6", 384, 2, True, 16, 3),
    ("fp8", 128, 1, "reversi", 7, 800, True, 10, 2), ("fp8", 128, 1, "reversi", 257, 16, "search", 30, 2),
    ("fp8", 128, 1, "reversi6", 384, 2, False, 16, 2), ("fp8", 128, 1, "reversi", 384, 1, True, 50, 3),
]


@pytest.mark.parametrize("mode,C,NB,game,B,sims,cache,stagger,moves", GEOMETRY,
                         ids=[f"{m}-C{c}-{g}-B{b}-s{s}-cache_{k}" for m, c, _, g, b, s, k, _, _ in GEOMETRY])
def test_search_with_the_net_in_the_loop_equals_the_oracle(mode, C, NB, game, B, sims, cache, stagger, moves):
    P, on = _net(mode, C, NB)
    eng = _engine(game, B, sims, mode, _dn(P, B), eval_cache=cache, temp_moves=8, openings=1, seed=3, stagger=stagger)
    eng.reset_games()
    res = _moves(eng, game, mode, on, moves, f"{mode} C={C} {game} B={B} sims={sims} cache={cache}")
    hits = sum(c["n_cache_hits"] for c, _, _ in res)
    if cache is True and sims >= 16:
        assert hits > 0, res     # the cache really removed rows the net would otherwise have seen
    if cache is False:
        assert hits == 0


@pytest.mark.parametrize("mode,C", [("bf16", 64), ("fp8", 128)])
@pytest.mark.parametrize("cache", [True, "search", False])
def test_4x4_late_game_steps_with_nothing_left_to_evaluate(mode, C, cache):
    """a staggered 4x4 pool (all game phases, three moves): many simulations end in terminal leaves or cache hits, which
    take no evaluator row; every search still equals the oracle's.  (Steps where NO slot needs a row: the next test.)"""
    P, on = _net(mode, C, 1)
    B, sims = 48, 64
    eng = _engine("reversi4", B, sims, mode, _dn(P, B), eval_cache=cache, temp_moves=4, seed=5, stagger=7)
    eng.reset_games()
    res = _moves(eng, "reversi4", mode, on, 3, f"{mode} 4x4 cache={cache}")
    term = sum(t["n_sims"] + r - t["n_net_leaves"] for _, t, r in res)
    assert term > 0, res      # simulations that ended in a terminal leaf (no evaluation) occurred
    if cache is not False:
        assert sum(c["n_cache_hits"] for c, _, _ in res) > 0


def _late_4x4_roots():
    """8 roots one or two plies before the end of pseudo-random 4x4 games: (own, opp, mover); their whole game trees have a
    handful of nodes, so most of a 64-simulation search revisits terminal leaves"""
    from test_gpu_leaf_parallel import _roots
    out = []
    for seed in range(4):
        out += [(r[2], r[3], r[1]) for r in _roots("reversi4", 20, seed)[-2:]]
    return out


def _stepwise_search(zero_steps):
    """the step API's search (what bz_engine_search issues), counting the steps after whose select no slot's leaf needs an
    evaluator row: leaf kind 1 marks exactly the rows select packs, so such a step's device-side count is 0"""
    def run(eng):
        eng.root_begin(); eng.evaluate(); eng.expand_backup(); eng.root_noise()
        kind = eng.leaf_buffers()["kind"]
        for s_ in range(eng.sims):
            eng.select(s_)
            zero_steps[0] += int(not bool((kind == 1).any()))
            eng.evaluate(); eng.expand_backup()
    return run


@pytest.mark.parametrize("mode,C", [("bf16", 64), ("fp8", 128)])
@pytest.mark.parametrize("cache", [True, "search", False])
def test_steps_whose_device_count_is_zero_change_nothing(mode, C, cache):
    """late 4x4 roots (set_roots): once a slot's game tree is complete every walk ends in a terminal leaf, so whole tree
    steps leave no row for the net -- the count select writes is 0 and the net's launch must then change nothing.  The
    step-by-step search asserts that such steps happened; it and the fused search both equal the oracle's"""
    P, on = _net(mode, C, 1)
    roots = _late_4x4_roots()
    B, sims = len(roots), 64
    zero = [0]
    for search in (_stepwise_search(zero), None):
        eng = _engine("reversi4", B, sims, mode, _dn(P, B), eval_cache=cache)
        eng.set_roots([r[0] for r in roots], [r[1] for r in roots], [r[2] for r in roots])
        _search_equals_oracle(eng, "reversi4", mode, on, f"{mode} late 4x4 cache={cache}", search)
    assert zero[0] > 0, "no tree step without an evaluator row: the count-0 path was not reached"


# ---------------------------------------------------------------- (b) self-play
def _games_equal_oracle(eng, game, mode, on, gids, sims, slots=None, max_moves=0, **okw):
    """the engine's example rows, winners and lengths of games `gids` (slots `slots`) against orc.selfplay_game"""
    t = eng.example_tensors()
    ex = {k: v.cpu().numpy() for k, v in t.items()}
    slots = gids if slots is None else slots
    res = run_threads(lambda i: orc.selfplay_game(ORC_GAME[game], int(gids[i]), sims, ORC_EVAL[mode], net=on,
                                                  max_moves=max_moves, **okw), len(gids))
    for s, g, r in zip(slots, gids, res):
        n = len(r["act"])
        L = n if max_moves else int(ex["len"][0, s])
        assert L == n, (g, L, n)
        assert np.array_equal(ex["own"][0, s, :n].view(np.uint64), r["own"]) and np.array_equal(ex["opp"][0, s, :n].view(np.uint64), r["opp"]), g
        assert np.array_equal(ex["act"][0, s, :n], r["act"]) and np.array_equal(ex["mover"][0, s, :n], r["mover"]), g
        assert np.array_equal(_bits(ex["pi"][0, s, :n]), _bits(r["pi"])), g
        if not max_moves:
            assert np.array_equal(ex["z"][0, s, :n], r["z"]) and int(ex["winner"][0, s]) == r["winner"], g
    return res


@pytest.mark.parametrize("mode,C,game,kw", [
    ("bf16", 64, "reversi", dict(temp_moves=8, openings=1, seed=2)),
    ("bf16", 128, "reversi6", dict(temp_moves=4, seed=3, dirichlet_alpha=0.3, dirichlet_eps=0.25)),
    ("bf16", 64, "reversi", dict(temp_moves=4, openings=1, seed=4, reuse_subtree=True)),
    ("fp8", 128, "reversi", dict(temp_moves=8, openings=1, seed=5, dirichlet_alpha=0.5, dirichlet_eps=0.25)),
    ("fp8", 128, "reversi4", dict(temp_moves=2, seed=6, reuse_subtree=True))], ids=["bf16-temp-openings", "bf16-6x6-noise",
                                                                                   "bf16-reuse", "fp8-noise", "fp8-4x4-reuse"])
def test_selfplay_games_equal_the_oracle(mode, C, game, kw):
    P, on = _net(mode, C, 1)
    B, sims = 8, 16
    eng = _engine(game, B, sims, mode, _dn(P, B), **kw)
    eng.reset_counters()
    eng.run_iteration()
    eng.status()
    okw = dict(temp_moves=kw.get("temp_moves", 0), openings=kw.get("openings", 0), seed=kw["seed"],
               dir_alpha=kw.get("dirichlet_alpha", 0.0), dir_eps=kw.get("dirichlet_eps", 0.0), reuse=kw.get("reuse_subtree", False))
    res = _games_equal_oracle(eng, game, mode, on, list(range(B)), sims, **okw)
    cnt = eng.counters()
    for k in WORK:
        assert cnt[k] == sum(r["counters"][k] for r in res), k
    assert cnt["n_net_leaves"] + cnt["n_cache_hits"] == sum(r["counters"]["n_net_leaves"] for r in res)


# ---------------------------------------------------------------- (c) the headline's shape
def _pipelined_equals_oracle(mode, B, sims, moves, sampled, **kw):
    from betazero_amd.engine import PipelinedSelfPlay
    P, on = _net(mode, 128, 6)
    dn = _dn(P, B // 2)
    sp = PipelinedSelfPlay("reversi", B, sims, ENGINE_EVAL[mode], dn, pipelines=2, temp_moves=8, openings=1, seed=0, rounds=1, **kw)
    sp.reset_games(); sp.reset_counters()
    prev = []
    for _ in range(moves):
        sp.step(False)
        sp.status()                   # raises on any engine error flag
        prev.append(sp.counters()["n_cache_hits_prev"])
    cnt = sp.counters()
    h = B // 2
    for i, e in enumerate(sp.engines):
        slots = [s for s in sampled if s < h]
        _games_equal_oracle(e, "reversi", mode, on, [i * h + s for s in slots], sims, slots=slots, max_moves=moves,
                            temp_moves=8, openings=1, seed=0)
    return cnt, prev


def test_headline_shape_two_pipelines_4096_games_800_sims_bf16_equals_the_oracle():
    """cfg 3 as bench.py runs it -- PipelinedSelfPlay, 2 x 2048 games on two streams sharing one DeviceNet, 800 simulations,
    a bf16 128x6x64 net, openings + tau = 1, the evaluation cache with carry-over -- for two moves: 8 sampled games (both
    pipelines, first and last slots) equal the oracle's games row for row.  The cache must have fired, from the previous
    search too, or this would not be testing it."""
    cnt, prev = _pipelined_equals_oracle("bf16", 4096, 800, 2, [0, 1, 2046, 2047])
    print("headline shape, bf16: n_cache_hits", cnt["n_cache_hits"], "n_cache_hits_prev", cnt["n_cache_hits_prev"],
          "n_net_leaves", cnt["n_net_leaves"], "n_sims", cnt["n_sims"])
    assert cnt["n_sims"] == 2 * 4096 * 800 and cnt["n_net_leaves"] + cnt["n_cache_hits"] == cnt["n_expanded"]
    assert cnt["n_cache_hits"] > 0 and prev[0] == 0 and cnt["n_cache_hits_prev"] > 0, (cnt, prev)


def test_cfg5_shape_8192_games_fp8_equals_the_oracle():
    """the cfg-5 analogue: the fp8 net in the loop of 8192 games (two pipelines), 200 simulations, one move; 4 sampled games"""
    cnt, _ = _pipelined_equals_oracle("fp8", 8192, 200, 1, [0, 4095])
    print("cfg5 shape, fp8: n_cache_hits", cnt["n_cache_hits"], "n_net_leaves", cnt["n_net_leaves"])
    assert cnt["n_sims"] == 8192 * 200 and cnt["n_cache_hits"] > 0


# ---------------------------------------------------------------- (d) K > 1
def _twin_roots(n, seed):
    from test_gpu_leaf_parallel import _roots
    return _roots("reversi", n, seed)


def _k_case(mode, C, K, B, sims, seed):
    from test_gpu_leaf_parallel import _same_root
    from test_leaf_parallel_cpu import KTwin, boards
    P, on = _net(mode, C, 1)
    fn = oracle_eval_fn(on, mode)
    roots = _twin_roots(24, seed)
    pick = [i % len(roots) for i in range(B)]
    eng = _engine("reversi", B, sims, mode, _dn(P, B * K), leaves_per_step=K)
    eng.set_roots([roots[i][2] for i in pick], [roots[i][3] for i in pick], [roots[i][1] for i in pick])
    eng.reset_counters()
    eng.search()
    NWP = eng.root_stats()
    eng.status()
    cnt = eng.counters()
    twins = {}
    for i in sorted(set(pick)):
        tw = KTwin("reversi", "net", leaves=K, eval_fn=fn, boards=boards())
        twins[i] = (tw, tw.search(roots[i][0], roots[i][1], sims))
    for g, i in enumerate(pick):
        _same_root(NWP, g, *twins[i])
    assert cnt["n_sims"] == B * sims and cnt["n_cache_hits"] == 0
    assert cnt["n_collisions"] == sum(twins[i][0].n_collisions for i in pick), cnt
    return cnt


@pytest.mark.parametrize("mode,C", [("bf16", 64), ("fp8", 128)])
@pytest.mark.parametrize("K,B,sims", [(2, 129, 8), (8, 33, 32), (32, 9, 64), (8, 31, 24)])
def test_leaf_parallel_search_with_the_net_equals_the_twin(mode, C, K, B, sims):
    """leaves_per_step K: B K = 258, 264, 288 (throughput shape) and 248 (latency shape) rows per launch, against KTwin
    whose evaluator is the oracle's forward"""
    cnt = _k_case(mode, C, K, B, sims, seed=K + B)
    assert cnt["n_collisions"] > 0 or K == 2


@pytest.mark.parametrize("mode,C", [("bf16", 64), ("fp8", 128)])
def test_leaf_parallel_selfplay_with_the_net_equals_the_twin(mode, C):
    from test_leaf_parallel_cpu import KTwin, boards
    P, on = _net(mode, C, 1)
    fn = oracle_eval_fn(on, mode)
    B, K, sims = 4, 8, 24
    eng = _engine("reversi", B, sims, mode, _dn(P, B * K), leaves_per_step=K, temp_moves=8, openings=1, seed=7)
    eng.run_iteration()
    eng.status()
    ex = eng.examples()
    winners, lens = eng.winners()
    for g in range(B):
        rows, w, _ = KTwin("reversi", "net", leaves=K, eval_fn=fn, boards=boards()).selfplay(g, sims, 8, 1, 7)
        m = ex.game == g
        assert lens[0, g] == len(rows) and winners[0, g] == w, g
        assert np.array_equal(ex.own[m], np.array([r[0] for r in rows], np.uint64))
        assert np.array_equal(ex.act[m], np.array([r[4] for r in rows], np.uint8))
        assert np.array_equal(_bits(ex.pi[m]), _bits([r[2] for r in rows]))
        assert np.array_equal(ex.z[m], (w * np.array([r[3] for r in rows])).astype(np.int8))


# ---------------------------------------------------------------- (e) Gumbel
@pytest.mark.parametrize("mode,C", [("bf16", 64), ("fp8", 128)])
@pytest.mark.parametrize("cache", [True, "search", False])
def test_gumbel_selfplay_with_the_net_equals_the_twin(mode, C, cache):
    """Gumbel root search with the net in the loop and each cache mode, whole games against GumbelTwin whose evaluator is
    the oracle's forward.  v_root is the root's evaluation: k_root_begin always packs the root for the evaluator, so a root
    is never a cache copy (the copy branch's v_root store cannot run), while the nodes below it are copied from the
    current and, with carry-over, the previous search"""
    from betazero_amd.engine import GumbelConfig
    from test_gumbel_cpu import GumbelTwin, boards
    P, on = _net(mode, C, 1)
    fn = oracle_eval_fn(on, mode)
    B, sims, m = 4, 32, 8
    eng = _engine("reversi6", B, sims, mode, _dn(P, B), gumbel=GumbelConfig(m), eval_cache=cache, temp_moves=4, seed=8)
    eng.reset_counters()
    eng.run_iteration()
    eng.status()
    ex = eng.examples()
    winners, lens = eng.winners()
    for g in range(B):
        rows, w, _ = GumbelTwin("reversi6", "net", m=m, eval_fn=fn, boards=boards()).selfplay(g, sims, 4, 0, 8)
        msk = ex.game == g
        assert lens[0, g] == len(rows) and winners[0, g] == w, g
        assert np.array_equal(ex.own[msk], np.array([r[0] for r in rows], np.uint64))
        assert np.array_equal(ex.act[msk], np.array([r[4] for r in rows], np.uint8))
        assert np.array_equal(_bits(ex.pi[msk]), _bits([r[2] for r in rows]))
    c = eng.counters()
    if cache is not False:
        assert c["n_cache_hits"] > 0, c


# ---------------------------------------------------------------- (f) weight update
@pytest.mark.parametrize("mode", ["bf16", "fp8"])
def test_weight_update_on_a_live_engine_with_the_cache_carrying_over(mode):
    """search and play with net A, DeviceNet.update to net B, search again: every search equals the oracle's with the net
    that was current at that moment (the carried-over evaluations of net A must not be used)"""
    (PA, onA), (PB, onB) = _net(mode, 128, 1, 1), _net(mode, 128, 1, 2)
    B, sims = 32, 64
    dn = _dn(PA, B)
    eng = _engine("reversi", B, sims, mode, dn, temp_moves=8, openings=1, seed=9, stagger=12)
    eng.reset_games()
    prev = []
    for mv, on in enumerate((onA, onA, onB, onB)):
        if mv == 2:
            torch.cuda.synchronize()
            dn.update(flat_params(PB))
        c, _, _ = _search_equals_oracle(eng, "reversi", mode, on, f"{mode} update, move {mv}")
        prev.append(c["n_cache_hits_prev"])
        eng.play(False)
    assert prev[1] > 0 and prev[2] == 0 and prev[3] > 0, prev


# ---------------------------------------------------------------- (g) MCTSPlayer
def test_mcts_player_with_the_bf16_net_equals_the_oracle_every_move():
    """MCTSPlayer (B = 1, roots from set_roots, evaluations carried across its moves): last_visits equals the oracle's
    search for every move of a game"""
    import betazero_amd as bz
    P, on = _net("bf16", 64, 1)
    sims = 64
    dn = _dn(P, 1)
    players = {1: bz.MCTSPlayer(1, sims=sims, net=dn), -1: bz.MCTSPlayer(-1, sims=sims, net=dn)}
    b, side, moves = bz.ReversiBoard(), 1, 0
    while not b.is_game_over():
        if not b.generate_possible_moves(side):
            side = -side
            continue
        mv = players[side].get_move(b)
        own, opp = b.bits(side)
        n, _, _, _ = orc.mcts_search(orc.GAME_REVERSI, int(own), int(opp), side, sims, orc.EVAL_NET_BF16, net=on)
        assert np.array_equal(players[side].last_visits, n), moves
        b = b.make_move(mv[0], mv[1], side)
        side, moves = -side, moves + 1
    assert moves > 40
    assert sum(pl._engine("reversi").counters()["n_cache_hits_prev"] for pl in players.values()) > 0
