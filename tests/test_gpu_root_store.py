"""The root store: finished searches of early roots are kept per engine, and a slot whose next root is on file
gets that tree as its "previous search", so the carry-over cache shares its evaluations.  Nothing may change but the number of
rows the net computes: every test runs an engine with the store beside engines without it (eval_cache="search", and the
carry-over without the store) on the same games and compares bits.  Small shapes: net_f32 32 channels x 2 blocks, 8 - 16
games, 24 - 64 simulations; games restart inside the runs (4x4 and 6x6: a staggered pool; 8x8, whose games outlast any short
run: the pool is reset half way, which brings every slot back to an opening the store has seen).  The second half runs the
same trio under every search mode the default engine can have (the store is on whenever the carry-over cache is), compared
after every move, and across set_solver / set_fpu on a live store; each case also holds that the store filed and seeded and
that the mode acted, so that none passes idle."""
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


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _lockstep(engines, steps, reset_at=None, at=None):
    """_run, with everything a search reports compared after EVERY move: root N / W / P bits, root_policy()'s pi bits and
    action, under the cap budgets(), under the solver proven() -- root, edges and both counts -- then the boards after the
    play; resign_rows() at the end.  The LAST engine (the in-search cache) is the one the others are held to.  at: {move:
    fn(engines)}, called before that move's search.  Returns what the run saw: the budgets, the nodes the solver decided,
    the searches whose pi is not N / sum N."""
    seen = {"budgets": set(), "n_decided": 0, "n_pi_not_visits": 0}
    ref, rest = engines[-1], engines[:-1]
    for e in engines:
        e.reset_games(); e.reset_counters()
    for mv in range(steps):
        if mv == reset_at:
            for e in engines:
                e.reset_games()
        if at and mv in at:
            at[mv](engines)
        for e in engines:
            e.search()
        N, W, P = ref.root_stats()
        pi, act = ref.root_policy()
        for e in rest:
            for x, y, what in zip((N, W, P), e.root_stats(), "NWP"):
                assert np.array_equal(_bits(x), _bits(y)), ("root stats", what, mv)
            p2, a2 = e.root_policy()
            assert np.array_equal(_bits(pi), _bits(p2)) and np.array_equal(act, a2), ("root policy", mv)
        if ref.playout_cap is not None:
            b = ref.budgets()
            for e in rest:
                assert np.array_equal(b, e.budgets()), ("budgets", mv)
            seen["budgets"] |= set(int(x) for x in b)
        if ref.solver:
            root, edges, counts = ref.proven()
            for e in rest:
                r2, e2, c2 = e.proven()
                assert root == r2 and np.array_equal(edges, e2) and counts == c2, ("proven", mv, counts, c2)
            seen["n_decided"] += counts["n_decided"]
        tot = N.sum(1)
        live = tot > 0
        visits = N[live].astype(np.float32) / tot[live].astype(np.float32)[:, None]
        seen["n_pi_not_visits"] += int((_u32(pi[live]) != _u32(visits)).any(1).sum())
        for e in engines:
            e.play(True)
        pos = ref.positions()
        for e in rest:
            for x, y in zip(pos, e.positions()):
                assert np.array_equal(x, y), ("boards", mv)
    for e in engines:
        e.status()  # raises on any error flag
    if ref.resign is not None:
        rr = ref.resign_rows()
        for e in rest:
            for x, y in zip(rr, e.resign_rows()):
                assert np.array_equal(_bits(x), _bits(y)), "resign rows"
    return seen


EXTRA = ("kl", "q", "fown", "fopp")  # the observers' columns (None where the option is off)


def _same_everything(engines, what):
    """the end of a lockstep run: every example tensor (winners and lengths are two of them), the finished games' rows with
    the kl / q / fown / fopp columns the mode has, every work counter but the three the caches move evaluations between, and
    the sum of those"""
    ref = engines[-1]
    ra, xa, ca = _raw_rows(ref), ref.examples(), ref.counters()
    wa, la = ref.winners()
    for e in engines[:-1]:
        _same_rows(ra, _raw_rows(e), what)
        xb, cb = e.examples(), e.counters()
        _same_examples(xa, xb, what)
        assert np.array_equal(xa.mover, xb.mover), what
        for k in EXTRA:
            a, b = getattr(xa, k, None), getattr(xb, k, None)
            assert (a is None) == (b is None) and (a is None or np.array_equal(_bits(a), _bits(b))), (what, k)
        wb, lb = e.winners()
        assert np.array_equal(wa, wb) and np.array_equal(la, lb), what
        if ref.ownership:
            for a, b in zip(ref.ownership_rows(), e.ownership_rows()):
                assert torch.equal(a, b), what
        assert ca["n_net_leaves"] + ca["n_cache_hits"] == cb["n_net_leaves"] + cb["n_cache_hits"], (what, ca, cb)
        assert set(ca) == set(cb)
        for k in ca:
            if k not in ("n_net_leaves", "n_cache_hits", "n_cache_hits_prev"):
                assert ca[k] == cb[k], (what, k)


ZERO = {"n_seeded_evals": 0, "n_seeded_searches": 0, "n_root_saves": 0}


def _store_is_busy(st, carry, search, what):
    r, cs = st.root_store_counters(), st.counters()
    print(what, r, "n_net_leaves", cs["n_net_leaves"], "without the store", carry.counters()["n_net_leaves"],
          "in-search only", search.counters()["n_net_leaves"])
    assert r["n_seeded_evals"] > 0 and r["n_seeded_searches"] > 0 and 0 < r["n_root_saves"] <= 256, (what, r)
    assert r["n_seeded_evals"] <= cs["n_cache_hits_prev"], (what, r, cs)
    assert cs["n_net_leaves"] < carry.counters()["n_net_leaves"], what
    assert carry.root_store_counters() == ZERO and search.root_store_counters() == ZERO, what


def _three(shape, seed=5, **mode):
    """(store, carry-over without the store, in-search cache only) of the shape, every engine with the mode's options"""
    game, B, sims, stagger, steps, reset_at, temp = SHAPES[shape]
    dn = _dn(B)
    kw = dict(temp_moves=temp, openings=1, seed=seed, rounds=6, stagger=stagger, **mode)
    engs = [_engine(game, B, sims, dn, eval_cache=True, **kw), _engine(game, B, sims, dn, eval_cache=True, root_store=False, **kw),
            _engine(game, B, sims, dn, eval_cache="search", **kw)]
    assert engs[0].root_store == (256, 3) and engs[1].root_store is None and engs[2].root_store is None
    return engs, dn


def _trio(shape):
    """(store, carry-over without the store, in-search cache only) after the shape's run, built and run once per process"""
    if shape not in _CACHE:
        engs, dn = _three(shape)
        _lockstep(engs, SHAPES[shape][4], reset_at=SHAPES[shape][5])
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


# ---------------------------------------------------------------- every mode the store runs under
FAST = {"4x4": 8, "6x6": 6}  # the cap's fast budget per shape (sims 32 and 24)


def _modes():
    from betazero_amd.engine import EvalSymmetry, ForcedPlayouts, Fpu, GumbelConfig, PlayoutCap, Resign
    cap = lambda shape, p=0.5: PlayoutCap(FAST[shape], p)  # noqa: E731
    return {
        "noise": ("4x4", dict(dirichlet_alpha=0.3, dirichlet_eps=0.25)),
        "cap": ("4x4", dict(playout_cap=cap("4x4"))),
        "cap_all_fast": ("4x4", dict(playout_cap=cap("4x4", 0.0))),
        "forced": ("4x4", dict(forced_playouts=ForcedPlayouts(2.0, True))),
        "forced_cap": ("4x4", dict(forced_playouts=ForcedPlayouts(2.0, True), playout_cap=cap("4x4"))),
        "fpu": ("4x4", dict(fpu=Fpu(0.2, 0.1))),
        "fpu_forced_cap": ("4x4", dict(fpu=Fpu(0.2, 0.1), forced_playouts=ForcedPlayouts(2.0, True), playout_cap=cap("4x4"))),
        "solver": ("4x4", dict(solver=True)),
        "solver_cap": ("4x4", dict(solver=True, playout_cap=cap("4x4"))),
        # (6x6: roots wider than max_considered, so that the halving has candidates to drop.  Gumbel search refuses Dirichlet
        # noise; its own noise is drawn while moves made < temp_moves)
        "gumbel": ("6x6", dict(gumbel=GumbelConfig(8))),
        "gumbel_interior": ("6x6", dict(gumbel=GumbelConfig(8, interior="gumbel"))),
        "symmetry": ("4x4", dict(eval_symmetry=EvalSymmetry(11))),
        "resign": ("4x4", dict(resign=Resign(RESIGN[0], RESIGN[1], 0.5))),
        "observers": ("4x4", dict(surprise=True, search_value=True, ownership=True)),
    }


# (threshold, consecutive): this net's root values on 4x4 stay small until a search meets the end of the game, where a lost
# position's q falls towards -1 -- one search below -0.25 is a side that sees the loss coming
RESIGN = (-0.25, 1)
MODE_NAMES = ("noise", "cap", "cap_all_fast", "forced", "forced_cap", "fpu", "fpu_forced_cap", "solver", "solver_cap", "gumbel",
              "gumbel_interior", "symmetry", "resign", "observers")


def _mode_trio(mode):
    """the trio with the mode's options after its shape's run: (engines, what _lockstep saw), once per process"""
    key = ("mode", mode)
    if key not in _CACHE:
        shape, kw = _modes()[mode]
        engs, dn = _three(shape, **kw)
        seen = _lockstep(engs, SHAPES[shape][4], reset_at=SHAPES[shape][5])
        _CACHE[key] = (engs, seen, dn)
    return _CACHE[key][:2]


def test_the_mode_table_is_the_list_of_names():
    assert tuple(_modes()) == MODE_NAMES


@pytest.mark.parametrize("mode", MODE_NAMES)
def test_the_store_changes_no_result_in_any_mode(mode):
    """every search's N / W / P, pi, action, budgets and proofs and the boards after every move (inside _lockstep), then every
    example tensor, the rows with the mode's columns, winners, lengths and the counters: the store engine and the carry-over
    engine are bit for bit the engine whose cache works inside a search only"""
    engs, _ = _mode_trio(mode)
    _same_everything(engs, mode)


@pytest.mark.parametrize("mode", MODE_NAMES)
def test_the_store_is_not_idle_in_any_mode(mode):
    (st, carry, search), seen = _mode_trio(mode)
    if mode == "cap_all_fast":  # a fast search files nothing, so nothing is ever seeded: the store is there and stays empty
        assert st.root_store == (256, 3) and st.root_store_counters() == ZERO, st.root_store_counters()
        assert carry.root_store_counters() == ZERO and search.root_store_counters() == ZERO
        assert st.counters()["n_net_leaves"] == carry.counters()["n_net_leaves"]
        return
    _store_is_busy(st, carry, search, mode)


@pytest.mark.parametrize("mode", MODE_NAMES)
def test_the_mode_is_not_idle(mode):
    """the mode's rows are not the plain trio's at the same shape, and the mode's own machinery ran"""
    shape, kw = _modes()[mode]
    (st, carry, search), seen = _mode_trio(mode)
    plain = _trio(shape)[0]
    ra, rp = _raw_rows(st), _raw_rows(plain)
    differ = any(not np.array_equal(_bits(ra[k]), _bits(rp[k])) for k in ra)
    print(mode, seen, "rows", len(st.examples()), "plain rows", len(plain.examples()))
    if mode == "observers":  # the observers only observe: the plain rows, and three columns that are not constant beside them
        assert not differ
        ex = st.examples()
        assert len(ex) > 0 and (ex.kl > 0).any() and len(np.unique(ex.q)) > 2 and len(np.unique(ex.fown)) > 1 and ((ex.fown & ex.fopp) == 0).all()
    else:
        assert differ
    if "playout_cap" in kw:
        full = SHAPES[shape][2]
        assert seen["budgets"] - {0} == ({FAST[shape]} if mode == "cap_all_fast" else {FAST[shape], full}), seen
    if mode == "cap_all_fast":
        assert len(st.examples()) == 0 and (st.winners()[1] <= 0).all()
    if "solver" in kw:
        assert seen["n_decided"] > 0, seen
    if "forced_playouts" in kw:
        assert seen["n_pi_not_visits"] > 0, seen
    elif mode in ("noise", "fpu", "solver", "symmetry", "observers"):
        assert seen["n_pi_not_visits"] == 0, seen  # (a full PUCT search's pi is N / sum N: the count above is no artefact)
    if mode == "resign":
        s = st.resign_stats()
        print(s)
        assert s["n_resigned"] > 0 and s["n_played_out"] > 0, s
        assert 0 < kw["resign"].playout_frac < 1


@pytest.mark.parametrize("kw", [dict(reuse_subtree=True), dict(leaves_per_step=8)], ids=["reuse_subtree", "leaves_per_step_8"])
def test_an_engine_without_the_carry_over_has_no_store(kw):
    """subtree reuse and leaf-parallel search switch the carry-over cache off, and the store with it: root_store reads None
    although the default was asked for, and the counters stay zero over a run with restarts"""
    B, sims = 16, 32
    eng = _engine("reversi4", B, sims, _dn(B * kw.get("leaves_per_step", 1)), temp_moves=4, seed=5, rounds=6, stagger=6, **kw)
    assert eng.root_store is None
    eng.reset_games(); eng.reset_counters()
    for _ in range(10):
        eng.search(); eng.play(True)
    eng.status()
    assert eng.root_store_counters() == ZERO and eng.counters()["n_cache_hits_prev"] == 0


# ---------------------------------------------------------------- the rule changes over a live store
def _switched(first, then, steps=10, at=4):
    """the 4x4 trio built with `first`'s options; before move `at` every engine is switched by then(engine).  Returns the
    engines, what the run saw, and the store's counters at the switch."""
    engs, dn = _three("4x4", **first)
    mark = {}

    def switch(es):
        mark.update(es[0].root_store_counters())
        for e in es:
            then(e)
    seen = _lockstep(engs, steps, at={at: switch})
    return engs, seen, mark


@pytest.mark.parametrize("order", ["on_then_off", "off_then_on"])
def test_switching_the_solver_over_a_live_store_keeps_the_three_engines_equal(order):
    """trees filed by solver searches (proven bits and rewritten value bits in their edge words) seed plain searches, and
    the other way round: nothing of a stored edge but its prior and action may reach the new tree"""
    on = order == "on_then_off"
    engs, seen, mark = _switched(dict(solver=True) if on else {}, lambda e: e.set_solver(not on))
    assert all(e.solver == (not on) for e in engs)
    _same_everything(engs, order)
    _store_is_busy(*engs, order)
    after = engs[0].root_store_counters()
    print(order, "at the switch", mark, "at the end", after, seen)
    assert mark["n_root_saves"] > 0 and mark["n_seeded_searches"] > 0, mark         # the store was live at the switch ...
    assert after["n_seeded_searches"] > mark["n_seeded_searches"], (mark, after)     # ... and went on seeding behind it
    assert seen["n_decided"] > 0, seen                                               # the solver's moves decided nodes


@pytest.mark.parametrize("order", ["on_then_off", "off_then_on"])
def test_switching_fpu_over_a_live_store_keeps_the_three_engines_equal(order):
    from betazero_amd.engine import Fpu
    on = order == "on_then_off"
    engs, seen, mark = _switched(dict(fpu=Fpu(0.2, 0.1)) if on else {}, lambda e: e.set_fpu(None if on else Fpu(0.2, 0.1)))
    assert all((e.fpu is None) == on for e in engs)
    _same_everything(engs, order)
    _store_is_busy(*engs, order)
    after = engs[0].root_store_counters()
    print(order, "at the switch", mark, "at the end", after)
    assert mark["n_root_saves"] > 0 and mark["n_seeded_searches"] > 0, mark
    assert after["n_seeded_searches"] > mark["n_seeded_searches"], (mark, after)
    plain = _trio("4x4")[0]  # the run is neither the plain one nor (by the same token) the one with the rule throughout
    assert any(not np.array_equal(_bits(a), _bits(b)) for a, b in zip(_raw_rows(engs[0]).values(), _raw_rows(plain).values()))


def test_two_pipelines_under_the_solver_with_the_store_equal_two_without():
    from betazero_amd.engine import PipelinedSelfPlay
    B, sims = 16, 32
    dn = _dn(B)
    kw = dict(pipelines=2, solver=True, temp_moves=4, seed=9, rounds=8, stagger=6)
    on, off = PipelinedSelfPlay("reversi4", B, sims, "net_f32", dn, **kw), PipelinedSelfPlay("reversi4", B, sims, "net_f32", dn, root_store=False, **kw)
    assert all(e.root_store == (256, 3) and e.solver for e in on.engines) and all(e.root_store is None and e.solver for e in off.engines)
    for sp in (on, off):
        sp.reset_games(); sp.reset_counters()
    decided = 0
    for mv in range(10):
        for sp in (on, off):
            sp.step(True)
        for sp in (on, off):
            sp.status()
        for ea, eb, st in zip(on.engines, off.engines, on.streams):
            for x, y in zip(ea.positions(), eb.positions()):
                assert np.array_equal(x, y), mv
            with torch.cuda.stream(st):  # the proofs of the search behind this move
                (ra, xa, ca), (rb, xb, cb) = ea.proven(), eb.proven()
            assert ra == rb and np.array_equal(xa, xb) and ca == cb, (mv, ca, cb)
            decided += ca["n_decided"]
    for ea, eb in zip(on.engines, off.engines):
        _same_rows(_raw_rows(ea), _raw_rows(eb), "pipelines")
    _same_examples(on.examples(), off.examples(), "pipelines")
    r, ca, cb = on.root_store_counters(), on.counters(), off.counters()
    print(r, decided, ca["n_net_leaves"], cb["n_net_leaves"])
    assert decided > 0
    assert r["n_seeded_evals"] > 0 and r["n_seeded_searches"] > 0 and off.root_store_counters() == ZERO, r
    assert ca["n_net_leaves"] < cb["n_net_leaves"] and ca["n_net_leaves"] + ca["n_cache_hits"] == cb["n_net_leaves"] + cb["n_cache_hits"]
    for k in ca:
        if k not in ("n_net_leaves", "n_cache_hits", "n_cache_hits_prev"):
            assert ca[k] == cb[k], k
