"""Playout cap randomisation without a GPU: the budget draw against a restatement on py_twin.rng_draw, the
cap twin -- per-move budgets, rows after full searches only, noise on full searches only, built on oracle.py_twin.Twin -- and
its invariants, the buffer layout, and the ABI / Python validation.  tests/test_gpu_playout_cap.py pins the engine to this
twin."""
import ctypes as C

import numpy as np
import pytest

from betazero_amd import _lib
from oracle.py_twin import Twin, f32, rng_draw
from test_leaf_parallel_cpu import KTwin, boards

C_CAP = 0x706C61796F757443


def cap_budget(seed, gid, moves_made, sims, fast_sims, full_q):
    """DESIGN.md 3.15, restated: sims iff the low 16 bits of the draw are below full_q"""
    return sims if (rng_draw(seed ^ C_CAP, gid, moves_made) & 0xFFFF) < full_q else fast_sims


class CapTwin(Twin):
    """Twin with playout cap randomisation: selfplay() draws every move's budget, searches with it, appends a row only after
    a full search and draws Dirichlet noise only then.  eval_fn(own, opp) -> (logits [NA] f32, value f32) replaces the
    synthetic evaluators.  After selfplay(): budgets / root_sums (one entry per search) and n_evals (evaluator calls)."""

    def __init__(self, game, eval_kind, fast_sims, full_q, eval_fn=None, **kw):
        super().__init__(game, eval_kind, **kw)
        self.fast_sims, self.full_q, self.eval_fn = fast_sims, full_q, eval_fn
        self.noise_on, self.n_evals, self.budgets, self.root_sums = True, 0, [], []

    start = KTwin.start  # (openings, then the bench's stagger plies)

    def evaluate(self, b, p):
        self.n_evals += 1
        if self.eval_fn is None:
            return super().evaluate(b, p)
        return self.eval_fn(*self.bits(b, p))

    def root_noise(self, root):
        if self.noise_on:
            super().root_noise(root)

    def selfplay(self, gid, sims, temp_moves, openings, seed, slot=0, stagger=0):
        b, p, made = self.start(slot, gid, openings, seed, stagger)
        ex, passes = [], 0
        self.budgets, self.root_sums = [], []
        while True:
            budget = cap_budget(seed, gid, made, sims, self.fast_sims, self.full_q)
            full = budget == sims
            self.noise_key, self.noise_on = (seed, gid, made), full
            root = self.search(b, p, budget)
            sumN = sum(e["N"] for e in root["edges"])
            self.budgets.append(budget)
            self.root_sums.append(sumN)
            if made < temp_moves:
                r = rng_draw(seed, gid, made) % sumN
                cum = 0
                for e in root["edges"]:
                    cum += e["N"]
                    if cum > r:
                        pick = e
                        break
            else:
                pick, bn = root["edges"][0], 0
                for e in root["edges"]:
                    if e["N"] > bn:
                        pick, bn = e, e["N"]
            if full:
                pi = [f32(0.0)] * self.na
                for e in root["edges"]:
                    pi[e["a"]] = f32(e["N"]) / f32(sumN)
                own, opp = self.bits(b, p)
                ex.append((own, opp, pi, p, pick["a"]))
            b = self.play(b, p, pick["a"])
            p, made = -p, made + 1
            over, w = self.terminal(b)
            if over:
                return ex, w, passes
            if not self.moves(b, p):
                p, passes = -p, passes + 1


# ---------------------------------------------------------------- the budget draw
def test_budget_equals_the_restatement_on_the_twins_rng():
    L = _lib.lib()
    rng = np.random.default_rng(0)
    seeds = [0, 1, 3, 0xFFFFFFFFFFFFFFFF, C_CAP] + [int(x) for x in rng.integers(0, 1 << 63, 4)]
    gids = [0, 1, 7, 4095, (1 << 40) + 5] + [int(x) for x in rng.integers(0, 1 << 62, 3)]
    for seed in seeds:
        for gid in gids:
            for made in (0, 1, 2, 9, 59, 63, 200):
                for full_q in (0, 1, 16384, 49152, 65535, 65536):
                    got = L.bz_playout_cap_budget(seed, gid, made, 800, 100, full_q)
                    assert got == cap_budget(seed, gid, made, 800, 100, full_q), (seed, gid, made, full_q)
                    if full_q == 0:
                        assert got == 100
                    if full_q == 65536:
                        assert got == 800


def test_budget_full_count_is_the_pinned_one():
    L = _lib.lib()
    full = sum(L.bz_playout_cap_budget(0, gid, made, 800, 100, 16384) == 800 for gid in range(4096) for made in range(60))
    assert full == 61520  # of 245 760 draws: 0.2503


def test_budget_refuses_bad_arguments():
    L = _lib.lib()
    for sims, fast, q in ((800, 0, 1), (800, 800, 1), (800, 801, 1), (1, 1, 1), (800, -3, 1), (800, 100, 65537), (8190, 100, 1)):
        assert L.bz_playout_cap_budget(0, 0, 0, sims, fast, q) == -1
        assert b"fast_sims" in L.bz_last_error()


# ---------------------------------------------------------------- the twin
GAMES = ["ttt", "reversi", "reversi6", "reversi4"]
SIMS = {"ttt": (24, 6), "reversi": (12, 3), "reversi6": (16, 4), "reversi4": (20, 5)}


@pytest.mark.parametrize("game", GAMES)
@pytest.mark.parametrize("ev", ["hash", "uniform"])
def test_twin_root_visits_equal_the_budget_and_rows_follow_full_searches(game, ev):
    sims, fast = SIMS[game]
    both = set()
    for gid in (0, 5, 11) if game == "reversi" else (0, 1, 2, 3, 4, 5):
        tw = CapTwin(game, ev, fast, 16384, boards=boards(), dir_alpha=0.3, dir_eps=0.25)
        rows, w, _ = tw.selfplay(gid, sims, 4, 1, 3, slot=gid, stagger=3)
        assert w in (-1, 0, 1)
        assert tw.root_sums == tw.budgets and set(tw.budgets) <= {sims, fast}
        assert len(rows) == sum(b == sims for b in tw.budgets)
        both |= set(tw.budgets)
        for own, opp, pi, mover, a in rows:
            assert abs(sum(float(x) for x in pi) - 1.0) <= 1e-6 and pi[a] > 0
    assert both == {sims, fast}  # the games under test held both kinds of search


@pytest.mark.parametrize("game", GAMES)
@pytest.mark.parametrize("noise", [False, True])
def test_twin_every_search_full_gives_the_rows_of_the_plain_twin(game, noise):
    sims, fast = SIMS[game]
    kw = dict(dir_alpha=0.3, dir_eps=0.25) if noise else {}
    for gid in (2, 7):
        tw = CapTwin(game, "hash", fast, 65536, boards=boards(), **kw)
        rows, w, ps = tw.selfplay(gid, sims, 3, 1, 5)
        ref, rw, rps = Twin(game, "hash", boards=boards(), **kw).selfplay(gid, sims, 3, 1, 5)
        assert (w, ps) == (rw, rps) and len(rows) == len(ref) and set(tw.budgets) == {sims}
        for a, b in zip(rows, ref):
            assert a[0] == b[0] and a[1] == b[1] and a[3] == b[3] and a[4] == b[4]
            assert np.array_equal(np.asarray(a[2], np.float32).view(np.uint32), np.asarray(b[2], np.float32).view(np.uint32))


@pytest.mark.parametrize("game", GAMES)
def test_twin_every_search_fast_gives_no_rows_and_the_winner_of_the_small_budget(game):
    sims, fast = SIMS[game]
    for gid in (2, 7):
        # noise configured: a fast search draws none, so the games are those of the plain twin WITHOUT noise
        tw = CapTwin(game, "hash", fast, 0, boards=boards(), dir_alpha=0.3, dir_eps=0.25)
        rows, w, ps = tw.selfplay(gid, sims, 3, 1, 5)
        ref, rw, rps = Twin(game, "hash", boards=boards()).selfplay(gid, fast, 3, 1, 5)
        assert rows == [] and (w, ps) == (rw, rps) and set(tw.budgets) == {fast} and len(tw.budgets) == len(ref)


def test_twin_noise_is_drawn_on_full_searches_only_with_the_key_of_the_move(monkeypatch):
    drawn, orig = [], Twin.root_noise

    def spy(self, root):
        drawn.append(self.noise_key)
        orig(self, root)
    monkeypatch.setattr(Twin, "root_noise", spy)
    tw = CapTwin("reversi6", "hash", 4, 32768, boards=boards(), dir_alpha=0.3, dir_eps=0.25)
    tw.selfplay(1, 16, 0, 0, 9)
    assert set(tw.budgets) == {4, 16}
    assert drawn == [(9, 1, k) for k, b in enumerate(tw.budgets) if b == 16]  # (no openings on 6x6: move k has made = k)


# ---------------------------------------------------------------- buffer size and refusals
def _cfg(game=1, B=4, sims=8, flags=0, K=1):
    return _lib.EngineCfg(game, B, sims, 0, 1.5, 0, 0, 1, 64, 0, 0, 0, B, flags | ((K - 1) << _lib.ENGINE_LEAVES_SHIFT), 0.0, 0.0, 0)


def test_playout_cap_bytes_is_the_stated_layout():
    L = _lib.lib()
    for game in (0, 1, 2, 3):
        for B in (1, 4, 33, 64, 65, 4096, 16384):
            for sims in (2, 7, 800):
                assert L.bz_engine_playout_cap_bytes(C.byref(_cfg(game, B, sims))) == (4 * B + 255) // 256 * 256
    # the evaluation cache and Dirichlet noise are allowed
    assert L.bz_engine_playout_cap_bytes(C.byref(_cfg(1, 4, 8, flags=_lib.ENGINE_EVAL_CACHE | _lib.ENGINE_EVAL_CACHE_CARRY))) == 256
    noisy = _cfg()
    noisy.dirichlet_alpha, noisy.dirichlet_eps = 0.3, 0.25
    assert L.bz_engine_playout_cap_bytes(C.byref(noisy)) == 256


def test_playout_cap_bytes_refuses_the_refused_combinations_with_a_message():
    L = _lib.lib()
    for cfg, word in ((_cfg(flags=_lib.ENGINE_REUSE_SUBTREE), b"subtree reuse"), (_cfg(K=2), b"leaves_per_step"),
                      (_cfg(K=32), b"leaves_per_step")):
        assert L.bz_engine_playout_cap_bytes(C.byref(cfg)) == -1
        assert word in L.bz_last_error() and b"playout cap" in L.bz_last_error(), L.bz_last_error()
    assert L.bz_engine_playout_cap_bytes(None) == -1
    assert L.bz_engine_playout_cap_bytes(C.byref(_cfg(sims=0))) == -1


def test_set_playout_cap_refuses_a_null_engine_with_a_message():
    """(an engine needs a GPU: the setter's refusals of the combinations are in tests/test_gpu_playout_cap.py)"""
    L = _lib.lib()
    assert L.bz_engine_set_playout_cap(None, 4, 16384, None, 0, None) == _lib.BZ_EINVAL
    assert b"bz_engine_set_playout_cap" in L.bz_last_error()


# ---------------------------------------------------------------- Python validation (no GPU needed)
def _no_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("touched a device")
    monkeypatch.setattr(_lib, "require_gpu", no_device)
    monkeypatch.setattr(_lib, "lib", no_device)


@pytest.mark.parametrize("bad", [0, -1, 16, 17, 2.0, True, "4", None])
def test_python_refuses_bad_fast_sims_before_touching_a_device(bad, monkeypatch):
    from betazero_amd.engine import PipelinedSelfPlay, PlayoutCap, SelfPlayEngine, check_playout_cap, self_play
    _no_device(monkeypatch)
    cap = PlayoutCap(bad)
    with pytest.raises(ValueError, match="fast_sims"):
        check_playout_cap(cap, 16)
    with pytest.raises(ValueError, match="fast_sims"):
        SelfPlayEngine("reversi", 4, 16, "uniform", playout_cap=cap)
    with pytest.raises(ValueError, match="fast_sims"):
        PipelinedSelfPlay("reversi", 4, 16, "uniform", playout_cap=cap, streams=[None])
    with pytest.raises(ValueError, match="fast_sims"):
        self_play("ttt", 4, 16, playout_cap=cap)


def test_python_refuses_bad_full_prob_and_combinations_before_touching_a_device(monkeypatch):
    from betazero_amd.engine import PipelinedSelfPlay, PlayoutCap, SelfPlayEngine, check_playout_cap, self_play
    _no_device(monkeypatch)
    for bad in (-0.1, 1.5, float("nan"), float("inf"), True, "0.25", None):
        with pytest.raises(ValueError, match="full_prob"):
            check_playout_cap(PlayoutCap(4, bad), 16)
        with pytest.raises(ValueError, match="full_prob"):
            SelfPlayEngine("ttt", 4, 16, "uniform", playout_cap=PlayoutCap(4, bad))
    for bad in ("yes", 4, (4, 0.25), {"fast_sims": 4}, True):
        with pytest.raises(ValueError, match="playout_cap"):
            check_playout_cap(bad, 16)
    cap = PlayoutCap(4)
    for kw, word in (({"reuse_subtree": True}, "reuse"), ({"leaves_per_step": 2}, "leaves_per_step"), ({"gumbel": True}, "Gumbel")):
        with pytest.raises(ValueError, match=word):
            SelfPlayEngine("reversi", 4, 16, "uniform", playout_cap=cap, **kw)
        with pytest.raises(ValueError, match=word):
            PipelinedSelfPlay("reversi", 4, 16, "uniform", playout_cap=cap, streams=[None], **kw)
        with pytest.raises(ValueError, match=word):
            self_play("reversi", 4, 16, playout_cap=cap, **kw)


def test_python_accepts_off_and_a_cap_and_maps_full_prob_to_q():
    from betazero_amd.engine import PlayoutCap, check_playout_cap
    assert check_playout_cap(None, 16) is None and check_playout_cap(False, 16) is None
    assert check_playout_cap(PlayoutCap(np.int64(4), 1), 16) == PlayoutCap(4, 1.0)
    assert PlayoutCap(100).full_prob == 0.25
    assert [PlayoutCap(1, p).full_q for p in (0.0, 0.25, 0.75, 1.0, 1e-6, 0.99999)] == [0, 16384, 49152, 65536, 0, 65535]
