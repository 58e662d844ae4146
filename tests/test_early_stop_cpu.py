"""Exact early stop without a GPU: bz_early_stop_decided -- the function the kernels run -- against a plain
restatement, the stop twin (StopTwin: oracle.py_twin.Twin whose search checks the rule before every simulation s >= 1 of a slot
whose move is not sampled) against the plain twin along whole games, the buffer layout, and the ABI / Python validation.
tests/test_gpu_early_stop.py pins the engine to this twin."""
import ctypes as C
import inspect
import itertools
import os

import numpy as np
import pytest

from betazero_amd import _lib
from oracle.py_twin import Twin
from test_fpu_cpu import FpuTwin
from test_playout_cap_cpu import _cfg, boards


# ---------------------------------------------------------------- the rule, restated
def decided(N, left):
    """N the root edges' visits in ascending action order, left the simulations to go"""
    N = [int(x) for x in N]
    if sum(N) < 1:
        return False
    lead = N.index(max(N))  # the first maximum: the edge DESIGN.md 3.7 would play now
    for j, x in enumerate(N):
        if j == lead:
            continue
        if not (x + left < N[lead] or (x + left == N[lead] and j > lead)):
            return False
    return True


def c_decided(N, left):
    a = np.ascontiguousarray(N, dtype=np.uint32)
    return _lib.lib().bz_early_stop_decided(a.ctypes.data, len(a), left)


def visits(root):
    return [e["N"] for e in root["edges"]]


class Enough(Exception):
    """a stop twin has searched max_searches times"""


def stop_twin(Base):
    """Base (a Twin) with early stop: search() checks the rule before simulation s >= 1 while moves made >= temp_moves (moves made
    is noise_key[2], as selfplay() sets it; temp_moves is the one selfplay() was called with, or the attribute).  Every search
    appends {"stop_at", "N", "made", and the root as searched: "b", "p", "a", "W", "P"} to stops; root["stop_at"] is the search's
    own.  max_searches: selfplay() ends with Enough before search number max_searches + 1 (None: whole games)."""
    class _Stop(Base):
        temp_moves = 0
        max_searches = None

        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.stops = []

        def selfplay(self, gid, sims, temp_moves, *a, **k):
            self.temp_moves = temp_moves
            return super().selfplay(gid, sims, temp_moves, *a, **k)

        def search(self, b, p, sims):
            if self.max_searches is not None and len(self.stops) >= self.max_searches:
                raise Enough
            self._S, self._s, self._stop = sims, 0, None
            root = super().search(b, p, sims)
            root["stop_at"] = sims if self._stop is None else self._stop
            self.stops.append({"stop_at": root["stop_at"], "N": visits(root), "made": self.noise_key[2], "b": b, "p": p,
                               "a": [e["a"] for e in root["edges"]], "W": [e["W"] for e in root["edges"]],
                               "P": [e["P"] for e in root["edges"]]})
            return root

        def simulate(self, root):
            if self._stop is not None:
                return
            if self._s >= 1 and self.noise_key[2] >= self.temp_moves and decided(visits(root), self._S - self._s):
                self._stop = self._s
                return
            super().simulate(root)
            self._s += 1
    return _Stop


def snap_twin(Base):
    """Base that keeps, per search, the root's visits after every simulation: snaps[k][s] = N after s simulations of search k"""
    class _Snap(Base):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.snaps = []

        def search(self, b, p, sims):
            self._cur = []
            root = super().search(b, p, sims)
            self._cur.append(visits(root))
            self.snaps.append(self._cur)
            return root

        def simulate(self, root):
            self._cur.append(visits(root))
            super().simulate(root)
    return _Snap


StopTwin = stop_twin(Twin)
SnapTwin = snap_twin(Twin)


# ---------------------------------------------------------------- bz_early_stop_decided
def test_decided_equals_the_restatement_on_every_small_case():
    n_dec = 0
    for n in (1, 2, 3, 4):
        for N in itertools.product(range(7), repeat=n):
            for left in range(8):
                want = decided(N, left)
                assert c_decided(N, left) == int(want), (N, left)
                n_dec += want
    assert n_dec > 1000  # (both answers occur)


def test_decided_equals_the_restatement_on_random_vectors():
    rng = np.random.default_rng(25)
    seen = set()
    for _ in range(4000):
        n = int(rng.integers(1, 35))
        hi = int(rng.choice([3, 40, 800, 8189]))
        N = rng.integers(0, hi + 1, n)
        if rng.random() < 0.5:  # a clear leader, so that "decided" is not rare
            N[int(rng.integers(n))] = min(8189, int(N.max()) + int(rng.integers(0, hi + 1)))
        if rng.random() < 0.3:  # ... and a tie with it somewhere
            N[int(rng.integers(n))] = int(N.max())
        gap = int(np.sort(N)[-1] - (np.sort(N)[-2] if n > 1 else 0))
        for left in {0, 1, max(gap - 1, 0), gap, gap + 1, int(rng.integers(0, 8190))}:
            want = decided(N, left)
            assert c_decided(N, left) == int(want), (N.tolist(), left)
            seen.add(want)
    assert seen == {True, False}


def test_decided_ties_zero_left_empty_roots_and_one_edge():
    # a tie goes to the lower action: the trailing edge may tie only from above the leader
    assert c_decided([5, 3], 2) == 1 and decided([5, 3], 2)          # edge 1 can only tie, and it is the higher action
    assert c_decided([3, 5], 2) == 0 and not decided([3, 5], 2)      # edge 0 can tie, and a tie is its
    assert c_decided([3, 5], 1) == 1 and c_decided([5, 3], 3) == 0
    assert c_decided([2, 5, 3], 2) == 1 and c_decided([3, 5, 2], 2) == 0
    assert c_decided([4, 4], 0) == 1 and c_decided([4, 4], 1) == 0  # equal now: edge 0 is the leader, edge 1 needs one visit
    for N in ([1], [0, 1], [7, 7, 7], [0, 0, 9], [8189] * 34):        # left = 0 is always decided
        assert c_decided(N, 0) == 1 and decided(N, 0)
    for N in ([0], [0, 0, 0]):                                        # no simulation done: never
        assert c_decided(N, 0) == 0 and c_decided(N, 5) == 0 and not decided(N, 0)
    for left in (0, 1, 63, 8188, 0xFFFFFFFF):                         # one edge: decided from s = 1 on
        assert c_decided([1], left) == 1 and c_decided([0], left) == 0
    # n >= 2: never before the leader has as many visits as are left
    for s in range(1, 32):
        assert c_decided([s, 0], 64 - s) == 0 and c_decided([0, s], 64 - s) == 0
    assert c_decided([32, 0], 32) == 1 and c_decided([0, 32], 32) == 0 and c_decided([0, 33], 31) == 1


def test_decided_refuses_bad_arguments_with_a_message():
    L = _lib.lib()
    a = np.zeros(300, np.uint32)
    for ptr, n in ((None, 3), (a.ctypes.data, 0), (a.ctypes.data, -1), (a.ctypes.data, 256)):
        assert L.bz_early_stop_decided(ptr, n, 1) == -1
        assert b"bz_early_stop_decided" in L.bz_last_error() and b"1 .. 255" in L.bz_last_error()
    a[2] = 1 << 24
    assert L.bz_early_stop_decided(a.ctypes.data, 3, 1) == -1 and b"visit count" in L.bz_last_error()
    a[2] = (1 << 24) - 1
    assert L.bz_early_stop_decided(a.ctypes.data, 255, 0) == 1


# ---------------------------------------------------------------- the twin along whole games
def _game_pair(stop_cls, snap_cls, game, ev, gid, sims, temp_moves, openings, seed, **kw):
    st, pl = stop_cls(game, ev, boards=boards(), **kw), snap_cls(game, ev, boards=boards(), **kw)
    return st, pl, st.selfplay(gid, sims, temp_moves, openings, seed), pl.selfplay(gid, sims, temp_moves, openings, seed)


def _check_games(stop_cls, snap_cls, game, ev, sims, n_games, openings, temp_moves=0, seed=7, **kw):
    """the stop twin's games against the plain twin's -> (searches, stopped early, one-edge roots stopped at 1)"""
    n_search = n_early = n_single = 0
    for gid in range(n_games):
        st, pl, (rows_s, w_s, pass_s), (rows_p, w_p, pass_p) = _game_pair(stop_cls, snap_cls, game, ev, gid, sims, temp_moves, openings,
                                                                         seed, **kw)
        assert (w_s, pass_s) == (w_p, pass_p) and len(rows_s) == len(rows_p) == len(st.stops) == len(pl.snaps)
        for k, (rs, rp, rec, snaps) in enumerate(zip(rows_s, rows_p, st.stops, pl.snaps)):
            assert rs[0] == rp[0] and rs[1] == rp[1] and rs[3] == rp[3], (gid, k)  # the same position, the same mover
            assert rs[4] == rp[4], (gid, k)                                      # the same move
            s = rec["stop_at"]
            assert 1 <= s <= sims and rec["N"] == snaps[s], (gid, k)            # the plain twin's visits after stop_at simulations
            assert sum(rec["N"]) == s
            if rec["made"] < temp_moves:  # a sampled move depends on every visit: the whole budget
                assert s == sims
                continue
            assert decided(snaps[s], sims - s) and c_decided(snaps[s], sims - s) == 1
            for t in range(1, s):         # ... and at no earlier simulation index
                assert not decided(snaps[t], sims - t), (gid, k, t)
            # pi = N / stop_at in the row
            assert [float(x) for x in rs[2]] == [float(np.float32(n) / np.float32(s)) if n else 0.0
                                                 for n in _by_action(rec["N"], st, rs)], (gid, k)
            n_search += 1
            n_early += s < sims
            if len(rec["N"]) == 1:
                assert s == 1
                n_single += 1
            else:
                assert 2 * s >= sims  # never before half the budget
    return n_search, n_early, n_single


def _by_action(N, tw, row):
    """the visits by action: the edges are the row's legal actions in ascending order"""
    legal = _legal_actions(tw, row[0], row[1])
    assert len(legal) == len(N)
    by = dict(zip(legal, N))
    return [by.get(a, 0) for a in range(tw.na)]


def _legal_actions(tw, own, opp):
    if tw.game == "ttt":
        return [a for a in range(9) if not ((own | opp) >> a) & 1]
    lg = C.c_uint64()
    _lib.check(_lib.lib().bz_reversi_legal(own, opp, tw.size, C.byref(lg)))
    return [a for a in range(64) if (lg.value >> a) & 1] or [64]


CASES = [("ttt", "hash", 64, 16, 0), ("reversi4", "hash", 48, 8, 0), ("reversi", "hash", 48, 2, 1)]
_singles = {}


@pytest.mark.parametrize("game,ev,sims,n_games,openings", CASES)
def test_stop_twin_plays_the_plain_twins_games_and_stops_exactly_where_the_rule_first_holds(game, ev, sims, n_games, openings):
    n, early, single = _check_games(StopTwin, SnapTwin, game, ev, sims, n_games, openings)
    assert n > 0 and 2 * early >= n, (n, early)  # not vacuous: at least half of the searches stop before the budget
    _singles[game] = single
    if game == "ttt":  # the ninth move of a full tic-tac-toe game is a one-edge root
        assert single >= 1


def test_temp_moves_keeps_the_sampled_searches_whole():
    for gid in range(4):
        st = StopTwin("ttt", "hash", boards=boards())
        pl = Twin("ttt", "hash", boards=boards())
        rows_s, w_s, _ = st.selfplay(gid, 64, 2, 0, 7)
        rows_p, w_p, _ = pl.selfplay(gid, 64, 2, 0, 7)
        assert w_s == w_p and [r[4] for r in rows_s] == [r[4] for r in rows_p]
        assert [r["stop_at"] for r in st.stops[:2]] == [64, 64]
        assert any(r["stop_at"] < 64 for r in st.stops[2:])
    n, early, _ = _check_games(StopTwin, SnapTwin, "ttt", "hash", 64, 4, 0, temp_moves=2)
    assert early >= 1


def test_stop_twin_over_the_fpu_twin():
    n, early, _ = _check_games(stop_twin(FpuTwin), snap_twin(FpuTwin), "ttt", "hash", 64, 4, 0, fpu=(0.2, 0.1))
    assert n > 0 and 2 * early >= n


# ---------------------------------------------------------------- the buffer and the refusals: the C entry points
def test_early_stop_bytes_is_the_stated_layout():
    L = _lib.lib()
    for game in (0, 1, 2, 3):
        for B in (1, 4, 33, 64, 65, 4096, 16384):
            for sims in (2, 7, 800):
                assert L.bz_engine_early_stop_bytes(C.byref(_cfg(game, B, sims))) == (4 * B + 255) // 256 * 256 + 256
    assert L.bz_engine_early_stop_bytes(C.byref(_cfg(1, 4, 8, flags=_lib.ENGINE_EVAL_CACHE | _lib.ENGINE_EVAL_CACHE_CARRY))) == 512
    for cfg, word in ((_cfg(flags=_lib.ENGINE_REUSE_SUBTREE), b"subtree reuse"), (_cfg(K=2), b"leaves_per_step")):
        assert L.bz_engine_early_stop_bytes(C.byref(cfg)) == -1
        assert word in L.bz_last_error() and b"early stop" in L.bz_last_error()
    assert L.bz_engine_early_stop_bytes(None) == -1 and L.bz_engine_early_stop_bytes(C.byref(_cfg(sims=0))) == -1


def test_early_stop_check_accepts_and_refuses_with_a_message():
    L = _lib.lib()
    chk = lambda cfg: L.bz_engine_early_stop_check(C.byref(cfg))  # noqa: E731
    for game in (0, 1, 2, 3):
        assert chk(_cfg(game, 4, 8)) == 0 and chk(_cfg(game, 4096, 800)) == 0
    for flags in (0, _lib.ENGINE_EVAL_CACHE, _lib.ENGINE_EVAL_CACHE | _lib.ENGINE_EVAL_CACHE_CARRY):  # every cache mode
        assert chk(_cfg(flags=flags)) == 0
    noisy = _cfg()
    noisy.dirichlet_alpha, noisy.dirichlet_eps, noisy.temp_moves = 0.3, 0.25, 10
    assert chk(noisy) == 0
    for ek in range(8):  # every evaluator (the MLPs: tic-tac-toe)
        cfg = _cfg(game=0 if ek >= 6 else 1)
        cfg.eval_kind = ek
        assert chk(cfg) == 0
    for cfg, word in ((_cfg(flags=_lib.ENGINE_REUSE_SUBTREE), b"subtree reuse"), (_cfg(K=2), b"leaves_per_step"),
                      (_cfg(K=32), b"leaves_per_step")):
        assert chk(cfg) == _lib.BZ_EINVAL
        assert word in L.bz_last_error() and b"early stop" in L.bz_last_error(), L.bz_last_error()
    assert L.bz_engine_early_stop_check(None) == _lib.BZ_EINVAL and chk(_cfg(sims=0)) == _lib.BZ_EINVAL


def test_the_engine_entry_points_refuse_a_null_engine_with_a_message():
    """(an engine needs a GPU: the setters' refusals on a live engine are in tests/test_gpu_early_stop.py)"""
    L = _lib.lib()
    assert L.bz_engine_set_early_stop(None, 1, 1, None, 0, None) == _lib.BZ_EINVAL
    assert b"bz_engine_set_early_stop" in L.bz_last_error()
    assert L.bz_engine_stopped(None, None, None) == _lib.BZ_EINVAL
    assert b"bz_engine_stopped" in L.bz_last_error()


def test_the_abi_version_stays_and_the_header_documents_the_rule():
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bz_abi.h")).read()
    assert "#define BZ_ABI_VERSION 7" in hdr and _lib.lib().bz_abi_version() == 7 and _lib.ABI_VERSION == 7
    for name in ("bz_engine_early_stop_bytes", "bz_engine_early_stop_check", "bz_engine_set_early_stop", "bz_engine_stopped",
                 "bz_early_stop_decided"):
        assert f"{name}(" in hdr and name in _lib.ABI_SYMBOLS
    assert "DESIGN.md 3.25" in hdr
    assert C.sizeof(_lib.EngineCfg) == 80


# ---------------------------------------------------------------- Python validation (no GPU needed)
def _no_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("touched a device")
    monkeypatch.setattr(_lib, "require_gpu", no_device)
    monkeypatch.setattr(_lib, "lib", no_device)


def _everyone(es, **kw):
    """every public entry point that takes early_stop=, as thunks; kw: the other option under test"""
    from betazero_amd.arena import play_arena
    from betazero_amd.engine import SelfPlayEngine
    from betazero_amd.match import MatchPlayer, play_match
    from betazero_amd.players import MCTSPlayer
    out = [lambda: SelfPlayEngine("reversi", 4, 16, "uniform", early_stop=es, **kw)]
    if set(kw) <= {"leaves_per_step", "gumbel", "solver", "fpu", "eval_symmetry"}:  # (what players and matches take)
        ev = {"evaluator": "net_bf16", "net": _FakeNet()} if "eval_symmetry" in kw else {}
        out += [lambda: MCTSPlayer(1, sims=16, early_stop=es, **kw, **ev),
                lambda: play_match("reversi", 4, MatchPlayer(16, early_stop=es, **kw, **ev), MatchPlayer(16)),
                lambda: play_match("reversi", 4, MatchPlayer(16), MatchPlayer(16, early_stop=es, **kw, **ev))]
        if "eval_symmetry" not in kw:
            out.append(lambda: play_arena("reversi", 4, 16, early_stop=es, **kw))
    return out


class _FakeNet:
    max_batch = 1 << 20


REFUSED = [({"reuse_subtree": True}, "reuse_subtree"), ({"leaves_per_step": 2}, "leaves_per_step"), ({"gumbel": True}, "gumbel"),
           ({"playout_cap": "cap"}, "playout_cap"), ({"forced_playouts": True}, "forced_playouts"), ({"solver": True}, "solver"),
           ({"root_store": (16, 2)}, "root_store"), ({"surprise": True}, "surprise"), ({"search_value": True}, "search_value"),
           ({"ownership": True}, "ownership"), ({"resign": True}, "resign")]


@pytest.mark.parametrize("kw,word", REFUSED, ids=[w for _, w in REFUSED])
def test_python_refuses_every_refused_combination_before_touching_a_device(kw, word, monkeypatch):
    from betazero_amd.engine import EarlyStop, PlayoutCap
    _no_device(monkeypatch)
    if "playout_cap" in kw:
        kw = {"playout_cap": PlayoutCap(4, 0.25)}
    for es in (True, EarlyStop(), EarlyStop(host_exit=False)):
        thunks = _everyone(es, **kw)
        assert thunks
        for thunk in thunks:
            with pytest.raises(ValueError, match=f"early.stop.*{word}"):
                thunk()
    for off in (None, False):  # off: the other option alone passes validation (the next thing the engine does is the device)
        with pytest.raises(AssertionError, match="touched a device"):
            _everyone(off, **kw)[0]()


def test_python_refuses_bad_values_before_touching_a_device(monkeypatch):
    from betazero_amd.engine import EarlyStop
    _no_device(monkeypatch)
    for bad in ("yes", 1, 0, 0.5, (True,), {"host_exit": True}):
        for thunk in _everyone(bad):
            with pytest.raises(ValueError, match="early_stop must be"):
                thunk()
    for bad in (1, None, "no", 0.0):
        for thunk in _everyone(EarlyStop(host_exit=bad)):
            with pytest.raises(ValueError, match="host_exit must be a bool"):
                thunk()


ACCEPTED = [{}, {"fpu": True}, {"eval_symmetry": True}, {"dirichlet_alpha": 0.3, "dirichlet_eps": 0.25}, {"temp_moves": 4},
            {"eval_cache": True}, {"eval_cache": "carry"}, {"eval_cache": "search"}, {"eval_cache": False}, {"eval_cache": None},
            {"evaluator": "hash"}, {"evaluator": "external"}, {"evaluator": "net_f32"}, {"evaluator": "net_fp8"}, {"root_store": False}]


@pytest.mark.parametrize("kw", ACCEPTED, ids=[",".join(f"{k}={v}" for k, v in kw.items()) or "plain" for kw in ACCEPTED])
def test_python_accepts_every_accepted_combination(kw, monkeypatch):
    from betazero_amd.engine import EarlyStop, SelfPlayEngine, check_early_stop
    _no_device(monkeypatch)
    kw = dict(kw)
    ev = kw.pop("evaluator", "net_bf16" if "eval_symmetry" in kw else "uniform")
    for es in (True, EarlyStop(host_exit=False)):
        with pytest.raises(AssertionError, match="touched a device"):  # validation passed: the next thing is the device
            SelfPlayEngine("reversi", 4, 16, ev, early_stop=es, **kw)
        if set(kw) <= {"fpu", "eval_symmetry"}:
            thunks = _everyone(es, **kw)
            assert thunks[1]().early_stop == check_early_stop(es)  # (a player builds its engine at the first move)
            for thunk in thunks[2:]:
                with pytest.raises(AssertionError, match="touched a device"):
                    thunk()


def test_check_early_stop_values_and_the_entry_points_that_do_not_take_it():
    import betazero_amd as bz
    from betazero_amd.arena import play_arena
    from betazero_amd.engine import EarlyStop, PipelinedSelfPlay, SelfPlayEngine, check_early_stop, self_play
    from betazero_amd.match import MatchPlayer
    from betazero_amd.players import MCTSPlayer
    assert check_early_stop(None) is None and check_early_stop(False) is None
    assert check_early_stop(True) == EarlyStop(True) and EarlyStop().host_exit is True
    assert check_early_stop(EarlyStop(np.bool_(False))) == EarlyStop(False)
    assert bz.EarlyStop is EarlyStop and bz.check_early_stop is check_early_stop and "EarlyStop" in bz.__all__
    for fn in (SelfPlayEngine.__init__, MCTSPlayer.__init__, play_arena):
        assert inspect.signature(fn).parameters["early_stop"].default is None
    assert MatchPlayer().early_stop is None
    # self-play pipelines do not get the option: a shortened search changes pi
    for fn in (PipelinedSelfPlay.__init__, self_play):
        assert "early_stop" not in inspect.signature(fn).parameters
    with pytest.raises(ValueError, match="early_stop"):
        PipelinedSelfPlay("reversi", 4, 16, "uniform", streams=[None], early_stop=True)
    with pytest.raises(TypeError):
        self_play("ttt", 4, 16, early_stop=True)
    assert "early_stop" not in open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py")).read()
