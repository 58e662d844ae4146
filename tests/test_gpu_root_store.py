"""The root store: finished searches of early roots are kept per engine, and a slot whose next root is on file
gets that tree as its "previous search", so the carry-over cache shares its evaluations.  Nothing may change but the number of
rows the net computes: every test runs an engine with the store beside engines without it (eval_cache="search", and the
carry-over without the store) on the same games and compares bits.  Small shapes: net_f32 32 channels x 2 blocks, 8 - 16
games, 24 - 64 simulations; games restart inside the runs (4x4 and 6x6: a staggered pool; 8x8, whose games outlast any short
run: the pool is reset half way, which brings every slot back to an opening the store has seen)."""
import numpy as np
import pytest
import torch

from oracle import oracle as orc

pytestmark = pytest.mark.gpu
_CACHE = {}


def _module(seed=3):
    from betazero_amd.net import PolicyValueNet
    torch.manual_seed(seed)
    return PolicyValueNet(32, 2, 64)


def _dn(B, seed=3):
    from betazero_amd.net import DeviceNet
    return DeviceNet.from_module(_module(seed), B)


def _engine(game, B, sims, dn, **kw):
    from betazero_amd.engine import SelfPlayEngine
    return SelfPlayEngine(game, B, sims, "net_f32", net=dn, **kw)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _raw_rows(e):
    return {k: v.cpu().numpy().copy() for k, v in e.example_tensors().items()}


def _same_rows(a, b, what):
    for k in a:
        assert np.array_equal(_bits(a[k]), _bits(b[k])), (what, k)


def _same_examples(xa, xb, what):
    assert len(xa) == len(xb), what
    for k in ("own", "opp", "pi", "z", "act", "game", "ply"):
        assert np.array_equal(_bits(getattr(xa, k)), _bits(getattr(xb, k))), (what, k)


def _run(engines, steps, reset_at=None, stats_at=None):
    """`steps` moves (search, play with restart) on every engine in lockstep; the boards are compared after every move, the
    root N / W / P after the search of move `stats_at`; with reset_at the pools go back to their starts before that move"""
    for e in engines:
        e.reset_games(); e.reset_counters()
    for mv in range(steps):
        if mv == reset_at:
            for e in engines:
                e.reset_games()
        for e in engines:
            e.search()
        if mv == stats_at:
            ref = engines[0].root_stats()
            for e in engines[1:]:
                for x, y in zip(ref, e.root_stats()):
                    assert np.array_equal(_bits(x), _bits(y)), ("root stats", mv)
        for e in engines:
            e.play(True)
        ref = engines[0].positions()
        for e in engines[1:]:
            for x, y in zip(ref, e.positions()):
                assert np.array_equal(x, y), ("boards", mv)
    for e in engines:
        e.status()  # raises on any error flag


# (game, B, sims, stagger, steps, reset_at, temp_moves)
SHAPES = {"4x4": ("reversi4", 16, 32, 6, 10, None, 4), "6x6": ("reversi6", 12, 24, 0, 8, 4, 6),
          "8x8": ("reversi", 16, 64, 0, 6, 3, 8)}


def _trio(shape):
    """(store, carry-over without the store, in-search cache only) after the shape's run, built and run once per process"""
    if shape not in _CACHE:
        game, B, sims, stagger, steps, reset_at, temp = SHAPES[shape]
        dn = _dn(B)
        kw = dict(temp_moves=temp, openings=1, seed=5, rounds=6, stagger=stagger)
        engs = [_engine(game, B, sims, dn, eval_cache=True, **kw), _engine(game, B, sims, dn, eval_cache=True, root_store=False, **kw),
                _engine(game, B, sims, dn, eval_cache="search", **kw)]
        assert engs[0].root_store is not None and engs[1].root_store is None and engs[2].root_store is None
        _run(engs, steps, reset_at=reset_at, stats_at=steps - 2)
        _CACHE[shape] = (engs, dn)
    return _CACHE[shape][0]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_store_changes_no_result(shape):
    """rows, boards after every move (inside _run) and the root statistics of one search: bit for bit those of the engine
    whose cache works inside a search only; the evaluations add up to the same number"""
    st, carry, search = _trio(shape)
    ra = _raw_rows(st)
    _same_rows(ra, _raw_rows(search), shape)
    _same_rows(ra, _raw_rows(carry), shape)
    _same_examples(st.examples(), search.examples(), shape)
    cs, cc, c0 = st.counters(), carry.counters(), search.counters()
    assert cs["n_net_leaves"] + cs["n_cache_hits"] == c0["n_net_leaves"] + c0["n_cache_hits"] == cc["n_net_leaves"] + cc["n_cache_hits"]
    for k in cs:
        if k not in ("n_net_leaves", "n_cache_hits", "n_cache_hits_prev"):
            assert cs[k] == c0[k] == cc[k], k


@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_store_is_not_idle(shape):
    st, carry, search = _trio(shape)
    r, cs = st.root_store_counters(), st.counters()
    print(shape, r, "n_net_leaves", cs["n_net_leaves"], "without the store", carry.counters()["n_net_leaves"],
          "in-search only", search.counters()["n_net_leaves"])
    assert r["n_seeded_evals"] > 0 and r["n_seeded_searches"] > 0 and 0 < r["n_root_saves"] <= 256, r
    assert r["n_seeded_evals"] <= cs["n_cache_hits_prev"]
    assert cs["n_net_leaves"] < carry.counters()["n_net_leaves"] < search.counters()["n_net_leaves"]
    assert carry.root_store_counters() == {"n_seeded_evals": 0, "n_seeded_searches": 0, "n_root_saves": 0}


def test_a_repeated_root_costs_one_row():
    """4x4, no noise, no sampling: the 8 games are the same game, end on the same move and restart together at the root the
    store has held since the first search.  A search is a function of its root and the evaluator (the oracle's two searches
    below agree), so the restarted slots' first search finds every leaf in the seeded tree: one row per slot, the root's."""
    B, sims = 8, 32
    mod = _module()
    on = orc.Net(32, 2, 64, mod.flat_params())
    eng = _engine("reversi4", B, sims, _dn(B), rounds=4)
    eng.reset_games()
    own0, opp0, tm0, _ = (a.copy() for a in eng.positions())
    a, b = (orc.mcts_search(orc.GAME_REVERSI4, int(own0[0]), int(opp0[0]), int(tm0[0]), sims, orc.EVAL_NET_F32, net=on) for _ in range(2))
    assert np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1])) and a[3] == b[3]
    for mv in range(16):
        eng.search(); eng.play(True)
        own, opp, tm, st = eng.positions()
        if np.array_equal(own, own0) and np.array_equal(opp, opp0) and (st == 0).all():
            break
    else:
        raise AssertionError("the games did not restart")
    eng.reset_counters()
    eng.search()
    N, _, _ = eng.root_stats()
    c, r = eng.counters(), eng.root_store_counters()
    assert np.array_equal(N[0], a[0])
    assert c["n_net_leaves"] == B, c                                   # the roots, and not one leaf
    assert r["n_seeded_searches"] == B and r["n_root_saves"] == 0, r
    assert r["n_seeded_evals"] == c["n_cache_hits_prev"] > 0 and c["n_net_leaves"] + c["n_cache_hits"] == B * a[3]["n_net_leaves"], (c, r)


def test_nothing_stored_survives_a_weight_update():
    """a live engine with a warm store, DeviceNet.update, the pool reset: the next search takes nothing from the store (its
    counters stand still over that search) and it, and the moves after it, equal a fresh engine built with the new weights"""
    B, sims = 16, 32
    dn = _dn(B, seed=3)
    kw = dict(temp_moves=4, seed=7, rounds=8, stagger=6)
    live = _engine("reversi4", B, sims, dn, **kw)
    live.reset_games(); live.reset_counters()
    for _ in range(8):
        live.search(); live.play(True)
    warm = live.root_store_counters()
    assert warm["n_seeded_searches"] > 0 and warm["n_root_saves"] > 0, warm
    torch.cuda.synchronize()
    dn.update(_module(seed=11).flat_params())
    fresh = _engine("reversi4", B, sims, _dn(B, seed=11), eval_cache="search", **kw)
    live.reset_games(); fresh.reset_games()
    live.search(); fresh.search()
    after = live.root_store_counters()
    assert after["n_seeded_evals"] == warm["n_seeded_evals"] and after["n_seeded_searches"] == warm["n_seeded_searches"], (warm, after)
    assert after["n_root_saves"] > warm["n_root_saves"]                # ... and files the new evaluator's trees
    for x, y in zip(live.root_stats(), fresh.root_stats()):
        assert np.array_equal(_bits(x), _bits(y))
    for mv in range(8):
        live.play(True); fresh.play(True)
        for x, y in zip(live.positions(), fresh.positions()):
            assert np.array_equal(x, y), mv
        live.search(); fresh.search()
        for x, y in zip(live.root_stats(), fresh.root_stats()):
            assert np.array_equal(_bits(x), _bits(y)), mv
    assert live.root_store_counters()["n_seeded_searches"] > after["n_seeded_searches"]  # the store works again
    live.status(); fresh.status()


def test_a_tiny_store_fills_up_and_stays_exact():
    """2 entries, first searches only, against the 12 openings of 16 games: the store is full after the first search, files
    nothing more, seeds what it has after the reset -- and every result is what it is without it"""
    B, sims = 16, 24
    dn = _dn(B)
    kw = dict(temp_moves=8, openings=1, seed=2, rounds=2)
    tiny, off = _engine("reversi", B, sims, dn, root_store=(2, 1), **kw), _engine("reversi", B, sims, dn, eval_cache="search", **kw)
    assert tiny.root_store == (2, 1)
    _run([tiny, off], 4, reset_at=2, stats_at=2)
    _same_rows(_raw_rows(tiny), _raw_rows(off), "tiny")
    r = tiny.root_store_counters()
    assert r["n_root_saves"] == 2 and r["n_seeded_searches"] > 0, r
    ct, c0 = tiny.counters(), off.counters()
    assert ct["n_net_leaves"] + ct["n_cache_hits"] == c0["n_net_leaves"] + c0["n_cache_hits"]


def test_two_pipelines_with_the_store_equal_two_without():
    from betazero_amd.engine import PipelinedSelfPlay
    B, sims = 16, 32
    dn = _dn(B)
    kw = dict(pipelines=2, temp_moves=4, seed=9, rounds=8, stagger=6)
    on, off = PipelinedSelfPlay("reversi4", B, sims, "net_f32", dn, **kw), PipelinedSelfPlay("reversi4", B, sims, "net_f32", dn, root_store=False, **kw)
    for sp in (on, off):
        sp.reset_games(); sp.reset_counters()
    for mv in range(10):
        for sp in (on, off):
            sp.step(True)
        for sp in (on, off):
            sp.status()
        for ea, eb in zip(on.engines, off.engines):
            for x, y in zip(ea.positions(), eb.positions()):
                assert np.array_equal(x, y), mv
    for ea, eb in zip(on.engines, off.engines):
        _same_rows(_raw_rows(ea), _raw_rows(eb), "pipelines")
    _same_examples(on.examples(), off.examples(), "pipelines")
    r, ca, cb = on.root_store_counters(), on.counters(), off.counters()
    assert r["n_seeded_evals"] > 0 and off.root_store_counters()["n_seeded_searches"] == 0, r
    assert ca["n_net_leaves"] < cb["n_net_leaves"] and ca["n_net_leaves"] + ca["n_cache_hits"] == cb["n_net_leaves"] + cb["n_cache_hits"]


def test_with_root_noise_the_store_stays_exact_and_busy():
    """Dirichlet noise changes a root's priors, never what the net says about a position: the noisy searches of a root visit
    other leaves than the stored one did, take what they share with it, and end where they end without the store"""
    B, sims = 16, 32
    dn = _dn(B)
    kw = dict(temp_moves=4, seed=4, rounds=8, stagger=6, dirichlet_alpha=0.3, dirichlet_eps=0.25)
    on, off = _engine("reversi4", B, sims, dn, **kw), _engine("reversi4", B, sims, dn, root_store=False, **kw)
    _run([on, off], 10, stats_at=8)
    _same_rows(_raw_rows(on), _raw_rows(off), "noise")
    _same_examples(on.examples(), off.examples(), "noise")
    r, ca, cb = on.root_store_counters(), on.counters(), off.counters()
    assert r["n_seeded_evals"] > 0 and r["n_seeded_searches"] > 0, r
    assert ca["n_net_leaves"] + ca["n_cache_hits"] == cb["n_net_leaves"] + cb["n_cache_hits"]
