"""The net forward under a board symmetry on the GPU, bit for bit against the PLAIN forward -- which other
tests pin to the oracle -- never against the symmetric code itself: FIXED equals the plain forward on the transformed
boards with the logits gathered through tau_s, HASHED equals the FIXED rows its hash picks, MEAN equals the stated fp32
sum, an engine with eval_symmetry equals an external-evaluator engine fed by DeviceNet.forward(symmetry="hash"), the cache
stays exact, off is off, and a symmetric player against itself scores exactly one half.

Shapes: n = 7 reaches the latency geometries and the odd tail of the two-per-workgroup one; n = 261 is above the 256-row
threshold (throughput geometries) and no multiple of 8, 4 or 2.  Every comparison is on integer views of the floats."""
import numpy as np
import pytest
import torch

from betazero_amd import _lib
from betazero_amd.symmetry import EvalSymmetry, sym_action_map, sym_index
from test_symmetry_cpu import SIZES, random_positions, twin_board

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = (7, 261)
KINDS = [("f32", 32), ("f32", 64), ("bf16", 64), ("bf16", 128), ("bf16", 256), ("fp8", 128)]
KIND_IDS = [f"{k}-C{c}" for k, c in KINDS]
_NETS, _POS = {}, {}


def _net(C, NB=1, max_batch=261):
    """a random net (default init, bf16-representable weights), built once per process"""
    key = (C, NB, max_batch)
    if key not in _NETS:
        from betazero_amd.net import DeviceNet, PolicyValueNet
        torch.manual_seed(100 + C + NB)
        _NETS[key] = DeviceNet.from_module(PolicyValueNet(C, NB, 32).round_to_bf16_(), max_batch, DEV)
    return _NETS[key]


def _fwd(dn, kind, own, opp, **kw):
    return dn.forward(own, opp, bf16=kind != "f32", fp8=kind == "fp8", **kw)


def _dev(a):
    return torch.as_tensor(np.asarray(a, dtype=np.uint64).view(np.int64)).to(DEV)


def _twin_boards(b, n, s):
    """the numpy twin of T_s on an array of bitboards: the n x n corners as [N, n, n] arrays through np.flip / np.rot90 /
    transposition (the per-item form is test_symmetry_cpu.twin_board)"""
    b = np.asarray(b, dtype=np.uint64)
    sh = np.array([[8 * r + c for c in range(n)] for r in range(n)], dtype=np.uint64)
    g = (b[:, None, None] >> sh) & np.uint64(1)
    r180 = np.rot90(g, 2, axes=(1, 2))
    t = (g, np.flip(g, 1), np.flip(g, 2), np.rot90(g, 1, axes=(1, 2)), r180, np.rot90(g, 3, axes=(1, 2)), g.transpose(0, 2, 1),
         r180.transpose(0, 2, 1))[s]
    corner = np.uint64(sum(1 << int(v) for v in sh.reshape(-1)))
    return (t << sh).sum(axis=(1, 2), dtype=np.uint64) | (b & ~corner)


def _positions(size, n):
    """seeded random positions of a board size, and their eight transforms (twin), shared by all tests and never changed"""
    key = (size, n)
    if key not in _POS:
        pos = random_positions(size, n, 1000 * size + n)
        own = np.array([p[0] for p in pos], dtype=np.uint64)
        opp = np.array([p[1] for p in pos], dtype=np.uint64)
        tw = [(_twin_boards(own, size, s), _twin_boards(opp, size, s)) for s in range(8)]
        for s in range(8):  # the vectorised twin is the per-item twin
            for i in (0, n // 2, n - 1):
                assert int(tw[s][0][i]) == twin_board(own[i], size, s) and int(tw[s][1][i]) == twin_board(opp[i], size, s)
        _POS[key] = {"own": own, "opp": opp, "d_own": _dev(own), "d_opp": _dev(opp),
                     "tw": tw, "d_tw": [(_dev(a), _dev(b)) for a, b in tw]}
    return _POS[key]


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _expect_fixed(dn, kind, P, size, s):
    """what FIXED s must give, from the plain forward alone"""
    lt, vt = _fwd(dn, kind, *P["d_tw"][s])
    tau = torch.as_tensor(sym_action_map(size, s).astype(np.int64)).to(DEV)
    return lt[:, tau], vt


# ---------------------------------------------------------------- 1. FIXED
def test_the_shared_table_is_the_augmentation_table():
    """bz_augment_d4_batch's transforms 0..6 (it serves size 8 among the net's boards) give the twin's boards"""
    for n in NS:
        P = _positions(8, n)
        own8 = torch.empty(8 * n, dtype=torch.int64, device=DEV)
        opp8 = torch.empty_like(own8)
        pi = torch.zeros((n, 65), dtype=torch.float32, device=DEV)
        pi8 = torch.empty((8 * n, 65), dtype=torch.float32, device=DEV)
        _lib.check(_lib.lib().bz_augment_d4_batch(P["d_own"].data_ptr(), P["d_opp"].data_ptr(), pi.data_ptr(), n, 8, 65,
                                                  own8.data_ptr(), opp8.data_ptr(), pi8.data_ptr(), None,
                                                  torch.cuda.current_stream().cuda_stream))
        own8, opp8 = own8.view(n, 8).cpu().numpy().view(np.uint64), opp8.view(n, 8).cpu().numpy().view(np.uint64)
        for s in range(7):
            assert np.array_equal(own8[:, s], P["tw"][s][0]) and np.array_equal(opp8[:, s], P["tw"][s][1]), s


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind,C", KINDS, ids=KIND_IDS)
def test_fixed_equals_the_plain_forward_on_the_transformed_boards(kind, C, n):
    dn = _net(C)
    for size in SIZES:
        P = _positions(size, n)
        plain = _fwd(dn, kind, P["d_own"], P["d_opp"])
        for s in range(8):
            lg, v = _fwd(dn, kind, P["d_own"], P["d_opp"], symmetry=s, size=size)
            el, ev = _expect_fixed(dn, kind, P, size, s)
            assert _same(lg, el), (kind, C, n, size, s, int((lg.view(torch.int32) != el.view(torch.int32)).sum()))
            assert _same(v, ev), (kind, C, n, size, s)
            if s == 0:
                assert _same(lg, plain[0]) and _same(v, plain[1])
        # the symmetries are not all the same function on this net: the comparison above has teeth
        assert not _same(_fwd(dn, kind, P["d_own"], P["d_opp"], symmetry=3, size=size)[0], plain[0])


# ---------------------------------------------------------------- 2. HASHED
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind,C", KINDS, ids=KIND_IDS)
def test_hashed_rows_are_the_fixed_rows_the_hash_picks(kind, C, n):
    dn = _net(C)
    for size in SIZES:
        P = _positions(size, n)
        fixed = [_fwd(dn, kind, P["d_own"], P["d_opp"], symmetry=s, size=size) for s in range(8)]
        outs = {}
        for seed in (0, 1, 2**64 - 1):
            idx = np.array([sym_index(seed, int(o), int(p)) for o, p in zip(P["own"], P["opp"])])
            lg, v = _fwd(dn, kind, P["d_own"], P["d_opp"], symmetry="hash", size=size, seed=seed)
            rows = torch.arange(n, device=DEV)
            pick = torch.as_tensor(idx).to(DEV)
            el = torch.stack([f[0] for f in fixed])[pick, rows]
            ev = torch.stack([f[1] for f in fixed])[pick, rows]
            assert _same(lg, el) and _same(v, ev), (kind, C, n, size, seed)
            outs[seed] = lg
            if n > 100:
                assert len(set(idx.tolist())) == 8  # every symmetry occurs in the batch
        assert not _same(outs[0], outs[1])          # another seed, another assignment


# ---------------------------------------------------------------- 3. MEAN
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("kind,C", KINDS, ids=KIND_IDS)
def test_mean_is_the_sequential_fp32_sum_of_the_eight(kind, C, n):
    dn = _net(C)
    for size in (8, 6):
        P = _positions(size, n)
        fixed = [_fwd(dn, kind, P["d_own"], P["d_opp"], symmetry=s, size=size) for s in range(8)]
        lg, v = _fwd(dn, kind, P["d_own"], P["d_opp"], symmetry="mean", size=size)
        for got, parts in ((lg, [f[0] for f in fixed]), (v, [f[1] for f in fixed])):
            acc = parts[0] + parts[1]
            for s in range(2, 8):
                acc = acc + parts[s]
            assert _same(got, acc * 0.125), (kind, C, n, size)


def test_forward_sym_refuses_bad_arguments():
    dn = _net(64)
    P = _positions(8, 7)
    L = _lib.lib()
    lg = torch.empty((7, 65), dtype=torch.float32, device=DEV)
    v = torch.empty(7, dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    call = lambda kind, size, mode, arg, scr=None, sb=0: L.bz_net_forward_sym(  # noqa: E731
        dn.h, kind, P["d_own"].data_ptr(), P["d_opp"].data_ptr(), 7, size, mode, arg, scr, sb, lg.data_ptr(), v.data_ptr(), st)
    assert call(1, 8, 0, 8) == _lib.BZ_EINVAL      # FIXED takes 0..7
    assert call(1, 5, 0, 0) == _lib.BZ_EINVAL      # sizes 8, 6, 4
    assert call(1, 8, 3, 0) == _lib.BZ_EINVAL      # unknown mode
    assert call(3, 8, 0, 0) == _lib.BZ_EINVAL      # unknown kind
    assert call(2, 8, 0, 0) == _lib.BZ_EINVAL      # fp8 needs C == 128
    assert call(1, 8, 2, 0) == _lib.BZ_EINVAL      # MEAN without a scratch
    scr = torch.empty(1024, dtype=torch.uint8, device=DEV)
    assert call(1, 8, 2, 0, (scr.data_ptr() + 255) & ~255, 256) == _lib.BZ_ENOMEM
    for bad in (8, "all", True):
        with pytest.raises(ValueError, match="symmetry"):
            dn.forward(P["d_own"], P["d_opp"], symmetry=bad)


# ---------------------------------------------------------------- 4. in the search
SEED = 77


def _search_net():
    return _net(64, NB=2, max_batch=512)


def _run(eng, moves, external=None):
    """`moves` searches with a move after each -> [(N, W, P)] per search"""
    eng.reset_games()
    out = []
    for _ in range(moves):
        if external is not None:
            eng.search_external(external)
        else:
            eng.search()
        out.append(eng.root_stats())
        eng.status()
        eng.play(False)
    return out


def _stats_equal(a, b, what):
    for mv, ((n1, w1, p1), (n2, w2, p2)) in enumerate(zip(a, b)):
        assert np.array_equal(n1, n2), (what, mv, "N")
        assert np.array_equal(w1.view(np.uint32), w2.view(np.uint32)), (what, mv, "W")
        assert np.array_equal(p1.view(np.uint32), p2.view(np.uint32)), (what, mv, "P")


# Reversi 6 and 8 with the one-walk PUCT search; leaves_per_step = 8 and Gumbel once each
@pytest.mark.parametrize("game,size,mode", [("reversi6", 6, "puct"), ("reversi", 8, "puct"), ("reversi6", 6, "K8"), ("reversi", 8, "gumbel")])
def test_engine_equals_an_external_engine_fed_by_the_hashed_forward(game, size, mode):
    from betazero_amd.engine import SelfPlayEngine
    dn = _search_net()
    kw = {"K8": {"leaves_per_step": 8}, "gumbel": {"gumbel": True}}.get(mode, {})
    common = dict(openings=4, seed=3, **kw)
    on = SelfPlayEngine(game, 64, 32, "net_bf16", net=dn, eval_symmetry=EvalSymmetry(SEED), **common)
    ext = SelfPlayEngine(game, 64, 32, "external", **common)
    got = _run(on, 2)
    want = _run(ext, 2, lambda own, opp, kind: dn.forward(own, opp, symmetry="hash", size=size, seed=SEED))
    _stats_equal(got, want, (game, mode))
    if mode == "puct":  # with the option on the run differs from the run with it off
        off = _run(SelfPlayEngine(game, 64, 32, "net_bf16", net=dn, **common), 2)
        assert any(not np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)) for a, b in zip(got, off))
        # True takes the engine's seed
        same = _run(SelfPlayEngine(game, 64, 32, "net_bf16", net=dn, eval_symmetry=True, **dict(common, seed=SEED)), 1)
        ref = _run(SelfPlayEngine(game, 64, 32, "net_bf16", net=dn, eval_symmetry=EvalSymmetry(SEED), **dict(common, seed=SEED)), 1)
        _stats_equal(same, ref, (game, "True"))


def test_refused_evaluators_are_refused_by_the_library_too():
    from betazero_amd.engine import SelfPlayEngine
    L = _lib.lib()
    for game, ev in (("reversi", "uniform"), ("reversi", "hash"), ("reversi", "external"), ("ttt", "uniform")):
        e = SelfPlayEngine(game, 4, 8, ev)
        assert L.bz_engine_set_eval_symmetry(e.h, 1, 5) == _lib.BZ_EINVAL
        assert L.bz_engine_set_eval_symmetry(e.h, 0, 0) == _lib.BZ_OK  # off is always accepted


# ---------------------------------------------------------------- 5. the cache stays exact
def _self_play(cache, plies=8, **kw):
    from betazero_amd.engine import SelfPlayEngine
    # 4x4, 64 simulations: small enough for transpositions INSIDE one search, which is all the "search" mode can hit
    eng = SelfPlayEngine("reversi4", 32, 64, "net_bf16", net=_search_net(), eval_cache=cache, temp_moves=4, openings=1, seed=5,
                         eval_symmetry=EvalSymmetry(SEED), **kw)
    eng.reset_games()
    for _ in range(plies):
        eng.search()
        eng.play(False)
    eng.status()
    w, ln = eng.winners()
    return eng.example_block().clone(), w, ln, eng.counters()


def test_the_evaluation_cache_stays_exact_under_the_symmetry():
    ref = _self_play(False)
    assert ref[3]["n_cache_hits"] == 0
    for cache in ("search", "carry"):
        got = _self_play(cache)
        assert torch.equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]), cache
        assert got[3]["n_cache_hits"] > 0, cache
    assert _self_play("carry")[3]["n_cache_hits_prev"] > 0


def test_a_change_of_seed_carries_nothing_over():
    from betazero_amd.engine import SelfPlayEngine
    dn = _search_net()
    mk = lambda seed: SelfPlayEngine("reversi6", 32, 32, "net_bf16", net=dn, eval_cache="carry", openings=2, seed=5,  # noqa: E731
                                     eval_symmetry=EvalSymmetry(seed))
    live, ctl = mk(1), mk(1)
    for e in (live, ctl):
        e.reset_games()
        e.search()
        e.play(False)
        e.reset_counters()
    live.set_eval_symmetry(EvalSymmetry(2))
    live.search()
    ctl.search()
    assert ctl.counters()["n_cache_hits_prev"] > 0           # the same seed does carry evaluations over the move ...
    assert live.counters()["n_cache_hits_prev"] == 0         # ... a new seed carries none
    own, opp, tm, st = live.positions()
    fresh = mk(2)
    fresh.set_roots(own, opp, np.where(st == 0, tm, 0))
    fresh.search()
    _stats_equal([live.root_stats()], [fresh.root_stats()], "fresh engine with the new seed")
    assert not np.array_equal(live.root_stats()[2].view(np.uint32), ctl.root_stats()[2].view(np.uint32))
    # switching it off again gives the plain engine's search
    live.set_eval_symmetry(None)
    live.set_roots(own, opp, np.where(st == 0, tm, 0))
    live.search()
    plain = SelfPlayEngine("reversi6", 32, 32, "net_bf16", net=dn, eval_cache="carry", openings=2, seed=5)
    plain.set_roots(own, opp, np.where(st == 0, tm, 0))
    plain.search()
    _stats_equal([live.root_stats()], [plain.root_stats()], "off again")


# ---------------------------------------------------------------- 6. off is off
def test_off_is_off():
    from betazero_amd.engine import SelfPlayEngine
    dn = _search_net()
    runs = []
    for kw in ({}, {"eval_symmetry": None}, {"eval_symmetry": False}):
        eng = SelfPlayEngine("reversi6", 32, 32, "net_bf16", net=dn, temp_moves=4, openings=1, seed=5, **kw)
        stats = _run(eng, 3)
        runs.append((stats, eng.example_block().clone()))
    for stats, block in runs[1:]:
        _stats_equal(stats, runs[0][0], "off")
        assert torch.equal(block, runs[0][1])


# ---------------------------------------------------------------- 7. matches
def test_a_symmetric_player_against_itself_scores_one_half():
    from betazero_amd.match import MatchPlayer, play_match
    p = MatchPlayer(sims=32, net=_search_net(), eval_symmetry=EvalSymmetry(SEED))
    res = play_match("reversi", 16, p, p, size=6, opening_plies=2, seed=9)
    assert res.summary()["score"] == 0.5
    assert np.array_equal(res.pair_score, np.zeros(8, dtype=res.pair_score.dtype))
