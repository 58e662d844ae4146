"""Resignation in self-play without a GPU: bz_resign_step / bz_resign_playout -- the functions the kernels run --
against restatements, the resignation twin (ResignTwin: a mixin in front of any of the twins: streaks, the full-search rule
under the cap, the record, resignation or play-out), its invariants, the buffer layout, the ABI / Python validation and the
arithmetic of resign_stats().  tests/test_gpu_resign.py pins the engine to this twin."""
import ctypes as C
import functools

import numpy as np
import pytest

from betazero_amd import _lib
from oracle.py_twin import Twin, f32, rng_draw
from test_forced_playouts_cpu import ForcedTwin
from test_gumbel_cpu import GumbelTwin
from test_leaf_parallel_cpu import KTwin, boards
from test_playout_cap_cpu import C_CAP, CapTwin, _cfg
from test_solver_cpu import SolverTwin

C_RESIGN = 0x72657369676E6564  # "resigned"


# ---------------------------------------------------------------- the rule, restated
def resign_step(q, threshold, consecutive, streak_in):
    """DESIGN.md 3.24, restated: (the streak behind a full search with root value q, whether the side fires)"""
    s = min(streak_in + 1, 255) if np.float32(q) < np.float32(threshold) else 0
    return s, s >= consecutive


def played_out(seed, gid, playout_q):
    return (rng_draw(seed ^ C_RESIGN, gid, 0) & 0xFFFF) < playout_q


def root_q(root):
    """DESIGN.md 3.18's q over a twin's root: W summed in edge order from 0, one division"""
    sW, sN = f32(0.0), 0
    for e in root["edges"]:
        sW = f32(sW + e["W"])
        sN += e["N"]
    return f32(sW / f32(sN)) if sN > 0 else f32(0.0)


class ResignTwin:
    """Mixin in front of a twin (class X(ResignTwin, CapTwin)): resign = (threshold, consecutive, playout_q).  selfplay() plays
    the base twin's game to the end, noting every search at the moment the move is played -- (moves made, mover, q, full
    search?, budget, rows recorded before it) in self.events -- and then applies the rule to that sequence: the searches of a
    game do not depend on the rule, so the resigned game is the base game cut at the firing search.  Afterwards: base = the
    base twin's (rows, winner, passes), record = (side, moves made, q) of the first fire or None, played_out, resigned,
    n_searches / n_sims = the searches / simulations the game ran, streaks = the two streaks at its end {+1: , -1: }."""

    def __init__(self, *a, resign=(-0.9, 2, 6554), **kw):
        super().__init__(*a, **kw)
        self.threshold, self.consecutive, self.playout_q = f32(resign[0]), int(resign[1]), int(resign[2])
        self._depth, self._root, self._made, self._sims, self.events = 0, None, 0, 0, []

    def _nested(self, fn, *a, **kw):
        self._depth += 1
        try:
            return fn(*a, **kw)
        finally:
            self._depth -= 1

    # every env transition inside these belongs to a search (or to the start position), not to the game's move
    def start(self, *a, **kw):
        r = self._nested(super().start, *a, **kw)
        self._made = r[2]
        return r

    def search(self, *a, **kw):
        root = self._nested(super().search, *a, **kw)
        if self._depth == 0:
            self._root = root
        return root

    def simulate(self, root):
        if self._depth == 0:  # (subtree reuse: Twin.selfplay goes on searching the kept root)
            self._root = root
        return self._nested(super().simulate, root)

    def run(self, root, *a, **kw):
        if self._depth == 0:  # (subtree reuse: KTwin.selfplay)
            self._root = root
        return self._nested(super().run, root, *a, **kw)

    def play(self, b, p, a):
        if self._depth == 0:  # the game's own move: after the search, before the move
            if self._root is not None:
                budgets = getattr(self, "budgets", None)
                budget = budgets[-1] if budgets else self._sims
                self.events.append({"made": self._made, "p": p, "q": root_q(self._root), "full": budget == self._sims, "budget": budget,
                                    "rows": sum(e["full"] for e in self.events)})
                self._root = None
            self._made += 1  # (without a root: one of Twin.selfplay's opening plies)
        return super().play(b, p, a)

    def selfplay(self, gid, sims, temp_moves, openings, seed, **kw):
        self._sims, self._made, self._root, self.events = sims, 0, None, []
        self.base = super().selfplay(gid, sims, temp_moves, openings, seed, **kw)
        return self.apply(gid, seed)

    def apply(self, gid, seed, fast_counts=False):
        """the rule over self.events.  fast_counts: the WRONG rule, under which a fast search goes through the streak too"""
        rows, w, passes = self.base
        self.streaks, self.record, self.resigned = {1: 0, -1: 0}, None, False
        self.played_out = played_out(seed, gid, self.playout_q)
        self.n_searches, self.n_sims = len(self.events), sum(e["budget"] for e in self.events)
        for k, ev in enumerate(self.events):
            if not (ev["full"] or fast_counts):
                continue
            self.streaks[ev["p"]], fire = resign_step(ev["q"], self.threshold, self.consecutive, self.streaks[ev["p"]])
            if fire and self.record is None:
                self.record = (ev["p"], ev["made"], ev["q"])
            if fire and not self.played_out:
                self.resigned = True
                self.n_searches, self.n_sims = k + 1, sum(e["budget"] for e in self.events[:k + 1])
                return rows[:ev["rows"]], -ev["p"], None
        return rows, w, passes


@functools.lru_cache(maxsize=None)
def resign_twin(base):
    return type("Resign" + base.__name__, (ResignTwin, base), {})


# ---------------------------------------------------------------- the two functions
def _c_step(q, threshold, consecutive, streak_in):
    out = C.c_int32(-7)
    fire = _lib.lib().bz_resign_step(C.c_float(q), C.c_float(threshold), consecutive, streak_in, C.byref(out))
    return out.value, fire


def test_resign_step_equals_the_restatement_on_every_streak_and_around_the_threshold():
    for thr in (np.float32(-0.9), np.float32(-0.2), np.float32(0.0), np.float32(1.0), np.float32(-1.0)):
        qs = [thr, np.nextafter(thr, np.float32(-2)), np.nextafter(thr, np.float32(2)), np.float32("nan"), np.float32("inf"),
              np.float32("-inf"), np.float32(1.0), np.float32(-1.0), np.float32(0.0)]
        for cons in (1, 2, 3, 255):
            for s_in in range(256):
                for q in qs:
                    s, fire = resign_step(q, thr, cons, s_in)
                    assert _c_step(q, thr, cons, s_in) == (s, int(fire)), (q, thr, cons, s_in)
    thr = np.float32(-0.9)
    assert _c_step(thr, thr, 1, 4) == (0, 0)  # a q equal to the threshold does not count ...
    assert _c_step(np.nextafter(thr, np.float32(-2)), thr, 1, 4) == (5, 1)  # ... the next float below it does
    assert _c_step(np.float32("nan"), thr, 1, 9) == (0, 0)  # a NaN q resets the streak
    assert _c_step(np.float32(-1.0), thr, 255, 254) == (255, 1) and _c_step(np.float32(-1.0), thr, 255, 255) == (255, 1)  # saturates
    assert _c_step(np.float32(-1.0), thr, 3, 1) == (2, 0) and _c_step(np.float32(-1.0), thr, 3, 2) == (3, 1)
    assert _c_step(np.float32("-inf"), thr, 2, 1) == (2, 1) and _c_step(np.float32("inf"), thr, 2, 1) == (0, 0)


def test_resign_step_refuses_bad_arguments_with_a_message():
    L = _lib.lib()
    out = C.c_int32()
    for cons, s_in, ptr in ((0, 0, C.byref(out)), (256, 0, C.byref(out)), (2, -1, C.byref(out)), (2, 256, C.byref(out)), (2, 0, None)):
        assert L.bz_resign_step(C.c_float(0), C.c_float(0), cons, s_in, ptr) == -1
        assert b"bz_resign_step" in L.bz_last_error()


def test_playout_draw_equals_the_restatement_on_the_twins_rng():
    L = _lib.lib()
    rng = np.random.default_rng(0)
    seeds = [0, 1, 3, 0xFFFFFFFFFFFFFFFF, C_CAP] + [int(x) for x in rng.integers(0, 1 << 63, 4)]
    gids = [0, 1, 7, 4095, (1 << 40) + 5] + [int(x) for x in rng.integers(0, 1 << 62, 3)]
    for seed in seeds + [C_RESIGN]:
        for gid in gids:
            for pq in (0, 1, 6554, 16384, 49152, 65535, 65536):
                got = L.bz_resign_playout(seed, gid, pq)
                assert got == int(played_out(seed, gid, pq)), (seed, gid, pq)
                if pq == 0:
                    assert got == 0  # no game is played out
                if pq == 65536:
                    assert got == 1  # every game is
    assert L.bz_resign_playout(0, 0, 65537) == -1 and b"bz_resign_playout" in L.bz_last_error()


def test_playout_count_is_the_pinned_one_and_the_draw_is_not_the_caps():
    L = _lib.lib()
    out = [L.bz_resign_playout(0, gid, 6554) for gid in range(4096)]
    assert sum(out) == PINNED_PLAYOUTS  # of 4096 games: a tenth
    cap = [L.bz_playout_cap_budget(0, gid, 0, 800, 100, 6554) == 800 for gid in range(4096)]  # the cap's draw at (seed, gid, 0)
    assert out != [int(c) for c in cap]
    assert sum(a != int(c) for a, c in zip(out, cap)) > 400  # independent tenths differ in about 0.18 of the games


PINNED_PLAYOUTS = 404


# ---------------------------------------------------------------- the twin
# the sizes tests/test_gpu_resign.py runs: (game, games, sims)
SIZES = [("reversi", 12, 24), ("ttt", 16, 40), ("reversi4", 8, 16), ("reversi6", 6, 30)]


@functools.lru_cache(maxsize=None)
def _played(game, n, sims, base_cls=Twin, seed=7, temp_moves=4, args=(), kw=()):
    """n games of a resignation twin, played once: the twins with their events and base games"""
    out = []
    for g in range(n):
        tw = resign_twin(base_cls)(game, "hash", *args, boards=boards(), resign=(-0.2, 2, 0), **dict(kw))
        tw.selfplay(g, sims, temp_moves, 0, seed)
        out.append(tw)
    return out


def _apply(tw, gid, seed, threshold, consecutive, playout_q, **kw):
    tw.threshold, tw.consecutive, tw.playout_q = f32(threshold), consecutive, playout_q
    return tw.apply(gid, seed, **kw)


def _same_rows(rows, ref):
    assert len(rows) == len(ref)
    for a, b in zip(rows, ref):
        assert a[0] == b[0] and a[1] == b[1] and a[3] == b[3] and a[4] == b[4]
        assert np.array_equal(np.asarray(a[2], np.float32).view(np.uint32), np.asarray(b[2], np.float32).view(np.uint32))


def test_the_hooks_see_every_search_of_every_kind_of_twin_once():
    """the mixin notes a search where the base twin plays its move: as many events as searches, with the base twin's own figures"""
    for base_cls, args, kw in ((Twin, (), {}), (Twin, (), {"reuse": True}), (KTwin, (), {"leaves": 4}), (KTwin, (), {"leaves": 2, "reuse": True}),
                               (CapTwin, (4, 16384), {}), (ForcedTwin, (2.0,), {"cap": (4, 32768)}), (SolverTwin, (), {"cap": (4, 32768)}),
                               (GumbelTwin, (), {"m": 4})):
        tw = resign_twin(base_cls)("reversi6", "hash", *args, boards=boards(), resign=(-0.2, 2, 65536), **kw)
        rows, w, _ = tw.selfplay(3, 16, 2, 0, 5)
        ref = base_cls("reversi6", "hash", *args, boards=boards(), **kw).selfplay(3, 16, 2, 0, 5)
        _same_rows(rows, ref[0])
        assert w == ref[1] and sum(e["full"] for e in tw.events) == len(rows)
        assert [e["made"] for e in tw.events] == sorted(set(e["made"] for e in tw.events)) and tw.events[0]["made"] == 0
        if hasattr(tw, "budgets"):
            assert [e["budget"] for e in tw.events] == tw.budgets
            assert {e["budget"] for e in tw.events} == {4, 16}
        for e in tw.events:
            assert -1.0 <= e["q"] <= 1.0
    tw = resign_twin(Twin)("reversi", "hash", boards=boards(), resign=(-0.2, 2, 65536))  # Twin.selfplay's own opening plies
    tw.selfplay(5, 8, 0, 1, 5)
    assert tw.events[0]["made"] == 2


@pytest.mark.parametrize("game,n,sims", SIZES)
def test_every_game_played_out_is_the_base_game_and_records_its_first_fire(game, n, sims):
    for g, tw in enumerate(_played(game, n, sims)):
        rows, w, ps = _apply(tw, g, 7, -0.2, 2, 65536)
        assert tw.played_out and not tw.resigned and (rows, w, ps) == tw.base and tw.n_searches == len(tw.events)
        streak, first = {1: 0, -1: 0}, None
        for ev in tw.events:  # the first fire, walked by hand
            streak[ev["p"]] = streak[ev["p"]] + 1 if ev["q"] < f32(-0.2) else 0
            if streak[ev["p"]] >= 2 and first is None:
                first = (ev["p"], ev["made"], ev["q"])
        assert tw.record == first


@pytest.mark.parametrize("game,n,sims", SIZES)
def test_no_game_played_out_gives_prefixes_and_a_loss_for_the_recorded_side(game, n, sims):
    n_res = 0
    for g, tw in enumerate(_played(game, n, sims)):
        rows, w, _ = _apply(tw, g, 7, -0.2, 2, 0)
        brows, bw, _ = tw.base
        assert not tw.played_out
        _same_rows(rows, brows[:len(rows)])
        if tw.resigned:
            n_res += 1
            side, made, q = tw.record
            assert w == -side and q < f32(-0.2) and len(rows) < len(brows) and tw.n_searches == len(rows) + 1
            assert all(w * r[3] == (-1 if r[3] == side else 1) for r in rows)  # z: a loss for the recorded side in every row
        else:
            assert tw.record is None and (rows, w) == (brows, bw)
    assert n_res > 0


def test_the_counts_the_gpu_cases_rely_on():
    """hash evaluator, seed 7, gids from 0, temp_moves 4, no openings: games that resign at (-0.2, 2) and at (-0.3, 2), and the
    false positives at (-0.2, 2) -- recorded sides that did not lose the base game"""
    res, res3, fps = [], [], []
    for game, n, sims in SIZES:
        tws = _played(game, n, sims)
        r = fp = 0
        for g, tw in enumerate(tws):
            _apply(tw, g, 7, -0.2, 2, 0)
            r += tw.resigned
            fp += tw.resigned and tw.base[1] != -tw.record[0]
        res.append(r)
        fps.append(fp)
        r3 = 0
        for g, tw in enumerate(tws):
            _apply(tw, g, 7, -0.3, 2, 0)
            r3 += tw.resigned
        res3.append(r3)
    assert res == [9, 4, 4, 6] and fps == [1, 2, 0, 0] and res3 == [5, 1, 4, 6], (res, fps, res3)


def _cap_game():
    """the game of test_under_the_cap_a_fast_search_leaves_the_streak_untouched: (twin, gid, seed)"""
    game, gid, seed, sims, fast = FAST_DECIDES
    tw = resign_twin(CapTwin)(game, "hash", fast, 32768, boards=boards(), resign=(-0.2, 2, 0))
    tw.selfplay(gid, sims, 2, 0, seed)
    return tw, gid, seed


# (game, gid, seed, sims, fast_sims), found by search over the twin's games: X's full searches at 8 and 10 moves are both below
# the threshold and so is the fast one at 6 moves -- counted, it would end the game one full search early
FAST_DECIDES = ("reversi4", 1, 0, 16, 4)


def test_under_the_cap_a_fast_search_leaves_the_streak_untouched():
    tw, gid, seed = _cap_game()
    right = _apply(tw, gid, seed, -0.2, 2, 0)
    rec, res, n = tw.record, tw.resigned, tw.n_searches
    wrong = _apply(tw, gid, seed, -0.2, 2, 0, fast_counts=True)
    assert {e["budget"] for e in tw.events} == {FAST_DECIDES[3], FAST_DECIDES[4]}
    # the two rules end this game differently: the fast searches between two full ones of a side decide it
    assert (right[1], len(right[0]), rec, res, n) != (wrong[1], len(wrong[0]), tw.record, tw.resigned, tw.n_searches)
    # and by hand: only full searches move a streak
    _apply(tw, gid, seed, -0.2, 2, 65536)
    streak, first = {1: 0, -1: 0}, None
    for ev in tw.events:
        if ev["full"]:
            streak[ev["p"]] = streak[ev["p"]] + 1 if ev["q"] < f32(-0.2) else 0
            if streak[ev["p"]] >= 2 and first is None:
                first = (ev["p"], ev["made"], ev["q"])
    assert tw.record == first == rec and tw.streaks == streak


# ---------------------------------------------------------------- buffer size and refusals
def test_resign_bytes_is_the_stated_layout():
    L = _lib.lib()
    up = lambda x: (x + 255) // 256 * 256  # noqa: E731
    for game in (0, 1, 2, 3):
        for B in (1, 4, 33, 64, 65, 4096, 16384):
            for rounds in (1, 3):
                cfg = _cfg(game, B, 8)
                cfg.rounds = rounds
                n = rounds * B
                assert L.bz_engine_resign_bytes(C.byref(cfg)) == up(2 * n) + up(n) + up(4 * n) + up(4 * n) + up(n)
    assert L.bz_engine_resign_bytes(C.byref(_cfg(1, 4, 8, flags=_lib.ENGINE_REUSE_SUBTREE))) == 5 * 256  # every config the engine accepts
    assert L.bz_engine_resign_bytes(C.byref(_cfg(1, 4, 8, K=8))) == 5 * 256
    assert L.bz_engine_resign_bytes(None) == -1 and b"bz_engine_resign_bytes" in L.bz_last_error()
    assert L.bz_engine_resign_bytes(C.byref(_cfg(sims=0))) == -1 and b"bz_engine_resign_bytes" in L.bz_last_error()
    assert L.bz_engine_resign_bytes(C.byref(_cfg(flags=1 << 13))) == -1 and b"bz_engine_resign_bytes" in L.bz_last_error()


def test_the_setter_and_the_reader_refuse_with_a_message():
    """(what needs no engine; a too small buffer and the ownership refusal need one: tests/test_gpu_resign.py)"""
    L = _lib.lib()
    buf = 1 << 20  # (an address the refusals never touch)
    for thr, cons, pq, ptr, word in ((float("nan"), 2, 0, buf, b"threshold"), (float("inf"), 2, 0, buf, b"threshold"),
                                     (-1.5, 2, 0, buf, b"threshold"), (1.0001, 2, 0, buf, b"threshold"), (-0.9, 0, 0, buf, b"consecutive"),
                                     (-0.9, 256, 0, buf, b"consecutive"), (-0.9, -1, 0, buf, b"consecutive"), (-0.9, 2, 65537, buf, b"playout_q"),
                                     (-0.9, 2, 0, buf + 128, b"256-byte aligned"), (-0.9, 2, 0, buf, b"null engine"),
                                     (-0.9, 2, 0, None, b"null engine")):
        assert L.bz_engine_set_resign(None, C.c_float(thr), cons, pq, ptr, 1 << 20, None) == _lib.BZ_EINVAL
        assert b"bz_engine_set_resign" in L.bz_last_error() and word in L.bz_last_error(), L.bz_last_error()
    assert L.bz_engine_resign_rows(None, None, None, None, None, None) == _lib.BZ_EINVAL
    assert b"bz_engine_resign_rows" in L.bz_last_error()


def test_the_abi_version_stays_and_the_header_documents_the_rule():
    import os
    assert _lib.lib().bz_abi_version() == 7
    h = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bz_abi.h")).read()
    assert "#define BZ_ABI_VERSION 7" in h and "#define BZ_RESIGN_KEY 0x%016XULL" % C_RESIGN in h
    for name in ("bz_engine_resign_bytes", "bz_engine_set_resign", "bz_engine_resign_rows", "bz_resign_step", "bz_resign_playout"):
        assert name + "(" in h, name


# ---------------------------------------------------------------- Python validation (no GPU needed)
@pytest.fixture
def _no_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("touched a device")
    monkeypatch.setattr(_lib, "require_gpu", no_device)
    monkeypatch.setattr(_lib, "lib", no_device)


def _everyone(match, **kw):
    from betazero_amd.engine import PipelinedSelfPlay, SelfPlayEngine, self_play
    with pytest.raises(ValueError, match=match):
        SelfPlayEngine("reversi", 4, 16, "uniform", **kw)
    with pytest.raises(ValueError, match=match):
        PipelinedSelfPlay("reversi", 4, 16, "uniform", streams=[None], pipelines=1, **kw)
    with pytest.raises(ValueError, match=match):
        self_play("reversi", 4, 16, **kw)


def test_python_refuses_every_bad_resign_before_touching_a_device(_no_device):
    from betazero_amd.engine import Resign, check_resign
    for bad in (float("nan"), float("inf"), -1.5, 1.5, 1e39, True, "x", None):
        with pytest.raises(ValueError, match="threshold"):
            check_resign(Resign(threshold=bad))
        _everyone("threshold", resign=Resign(threshold=bad))
    for bad in (0, 256, -1, 2.0, True, "2", None):
        with pytest.raises(ValueError, match="consecutive"):
            check_resign(Resign(consecutive=bad))
        _everyone("consecutive", resign=Resign(consecutive=bad))
    for bad in (-0.1, 1.5, float("nan"), True, "0.1", None):
        with pytest.raises(ValueError, match="playout_frac"):
            check_resign(Resign(playout_frac=bad))
        _everyone("playout_frac", resign=Resign(playout_frac=bad))
    for bad in ("yes", -0.9, (-0.9, 2, 0.1), {"threshold": -0.9}, 1):
        with pytest.raises(ValueError, match="resign must be"):
            check_resign(bad)
        _everyone("resign must be", resign=bad)
    for rs in (True, Resign()):
        with pytest.raises(ValueError, match="ownership"):
            check_resign(rs, ownership=True)
        _everyone("ownership", resign=rs, ownership=True)


def test_python_accepts_off_true_and_a_rule_and_maps_the_share_to_q():
    import betazero_amd as bz
    from betazero_amd.engine import Resign, check_resign
    assert bz.Resign is Resign and bz.check_resign is check_resign
    assert check_resign(None) is None and check_resign(False) is None and check_resign(None, ownership=True) is None
    assert check_resign(True) == Resign(float(np.float32(-0.9)), 2, 0.1)
    assert check_resign(Resign(np.float32(-0.5), np.int64(3), 1)) == Resign(-0.5, 3, 1.0)
    assert check_resign(Resign(-1, 1, 0)) == Resign(-1.0, 1, 0.0) and check_resign(Resign(1.0, 255, 1.0)).consecutive == 255
    assert [Resign(playout_frac=p).playout_q for p in (0.0, 0.1, 0.25, 1.0, 1e-6, 0.99999)] == [0, 6554, 16384, 65536, 0, 65535]


# ---------------------------------------------------------------- resign_stats
def test_resign_stats_arithmetic_on_hand_made_arrays():
    from betazero_amd.engine import _sum_resign_stats, resign_stats
    #                 resigned  resigned  out,lost  out,won   out,draw  out,none  unfinished  plain
    side = np.array([[1, -1, 1, -1, 1, 0, 1, 0]], np.int8)
    out = np.array([[0, 0, 1, 1, 1, 1, 1, 0]], bool)
    win = np.array([[-1, 1, -1, -1, 0, 1, 0, 1]], np.int8)
    ln = np.array([[5, 0, 9, 9, 9, 9, -1, 9]], np.int32)
    st = resign_stats(side, out, win, ln)
    assert st == {"n_finished": 7, "n_resigned": 2, "n_played_out": 4, "n_would_resign": 3, "n_false_positive": 2,
                  "false_positive_rate": 2 / 3}
    # a drawn game with a record is a false positive on its own
    one = resign_stats(np.array([1], np.int8), np.array([True]), np.array([0], np.int8), np.array([7]))
    assert one["n_false_positive"] == 1 and one["false_positive_rate"] == 1.0
    none = resign_stats(side[:, :2], out[:, :2], win[:, :2], ln[:, :2])
    assert none["n_would_resign"] == 0 and none["false_positive_rate"] is None and none["n_resigned"] == 2
    tot = _sum_resign_stats([st, none, one])
    assert tot["n_finished"] == 10 and tot["n_would_resign"] == 4 and tot["false_positive_rate"] == 3 / 4
    assert _sum_resign_stats([none, none])["false_positive_rate"] is None
