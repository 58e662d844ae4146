"""First-play urgency reduction without a GPU: bz_fpu_mass / bz_fpu_value -- the functions the kernels run --
against a restatement in numpy float32 under every edge order tried, the FPU twin (FpuTwin: ForcedTwin, and through it CapTwin,
with the rule in simulate and the root's running value sum Wr) and its invariants, the buffer size and the ABI / Python
validation.  tests/test_gpu_fpu.py pins the engine to this twin."""
import ctypes as C
import inspect

import numpy as np
import pytest

from betazero_amd import _lib
from oracle.py_twin import Twin, f32
from test_forced_playouts_cpu import ForcedTwin, _score, forced_nf
from test_match_cpu import Side
from test_playout_cap_cpu import CapTwin, _cfg, boards

TWO24 = f32(16777216.0)
INV24 = f32(5.9604644775390625e-08)
NOISE = dict(dir_alpha=0.3, dir_eps=0.25)


def fpu_pq(P):
    """a visited edge's prior in units of 2^-24, truncated; NaN / negative / zero -> 0"""
    P = f32(P)
    return int(P * TWO24) if P > 0 else 0


def fpu_mass(N, P):
    return sum(fpu_pq(p) for n, p in zip(N, P) if n > 0)


def fpu_value(S, q_node, reduction):
    """DESIGN.md 3.20, one rounding per operation"""
    m = f32(S)  # (an int below 2^53 is exact in the double numpy converts through: one rounding, to nearest even)
    m = m * INV24
    m = np.sqrt(m)
    red = f32(reduction) * m
    return f32(q_node) - red


class FpuTwin(ForcedTwin):
    """ForcedTwin with first-play urgency reduction in simulate.  fpu = (reduction, root_reduction); k = None: no forced
    playouts (and no pruning); cap = (fast_sims, full_q) or None.  Wr, the root's running value sum, restarts with every
    search.  n_changed = walks in which the rule chose, at some level, another edge than the same walk would have chosen with
    q = 0 for the unvisited edges from the same statistics (the forced rule applied to both)."""

    def __init__(self, game, eval_kind, fpu=(0.2, 0.1), k=None, prune=True, cap=None, eval_fn=None, **kw):
        super().__init__(game, eval_kind, 1.0 if k is None else k, prune=prune and k is not None, cap=cap, eval_fn=eval_fn, **kw)
        self.forcing = k is not None
        self.r, self.r_root = f32(fpu[0]), f32(fpu[1])
        self.Wr, self.n_done, self.n_changed, self.n_walks, self.max_nodes = f32(0.0), 0, 0, 0, 0

    def search(self, b, p, sims):
        self.Wr, self.n_done, self._nodes = f32(0.0), 0, 0  # (new_node counts the root too)
        root = super().search(b, p, sims)
        self.max_nodes = max(self.max_nodes, self._nodes)
        return root

    def new_node(self, b, p):
        self._nodes = getattr(self, "_nodes", 0) + 1
        return super().new_node(b, p)

    def simulate(self, root):
        node, path, depth, changed = root, [], 0, False
        qx = self.Wr / f32(self.n_done) if self.n_done > 0 else f32(0.0)
        while True:
            if node["term"]:
                v = f32(node["tv"])
                break
            edges = node["edges"]
            sumN = sum(e["N"] for e in edges)
            sq = np.sqrt(f32(max(sumN, 1)))
            S = fpu_mass([e["N"] for e in edges], [e["P"] for e in edges])
            f = fpu_value(S, qx, self.r_root if depth == 0 else self.r)
            best, bests, own, plain = None, f32(-np.inf), None, None
            for e in edges:
                q = e["W"] / f32(e["N"]) if e["N"] > 0 else f
                s = _score(q, self.c, e["P"], sq, e["N"])
                s0 = _score(e["W"] / f32(e["N"]) if e["N"] > 0 else f32(0.0), self.c, e["P"], sq, e["N"])
                if own is None or s > own[1]:
                    own = (e, s)
                if node is root and self.forcing and self.force_on and e["N"] > 0 and f32(e["N"]) < forced_nf(self.k, e["P"], sumN):
                    s = s0 = f32(np.inf)
                if s > bests:
                    best, bests = e, s
                if plain is None or s0 > plain[1]:
                    plain = (e, s0)
            if node is root and best is not own[0]:
                self.n_overrides += 1
            changed = changed or best is not plain[0]
            path.append(best)
            if best["child"] is not None:
                qx = -(best["W"] / f32(best["N"]))  # the child's value for its mover, from the edge as the walk read it
                node, depth = best["child"], depth + 1
                continue
            ch = self.new_node(self.play(node["b"], node["p"], best["a"]), -node["p"])
            best["child"] = ch
            v = f32(ch["tv"]) if ch["term"] else self.expand(ch)
            break
        val = -v
        for e in reversed(path):
            e["N"] += 1
            e["W"] = f32(e["W"] + val)
            x, val = val, -val
        self.Wr = f32(self.Wr + x)  # what this simulation's backup added to its root edge's W
        self.n_done += 1
        self.n_walks += 1
        self.n_changed += changed


class FpuSide(Side):
    """a match side that searches with the FPU twin"""

    def __init__(self, sims, ev="uniform", fpu=(0.2, 0.1), eval_fn=None, c_puct=1.5):
        super().__init__(sims, ev, eval_fn=eval_fn, c_puct=c_puct)
        self.fpu = fpu

    def twin(self, game):
        if game not in self._tw:
            self._tw[game] = FpuTwin(game, self.ev, self.fpu, eval_fn=self.eval_fn, c_puct=self.c_puct, boards=boards())
        return self._tw[game]


# ---------------------------------------------------------------- the two functions
def _c_mass(N, P):
    n, p = np.asarray(N, np.uint32), np.asarray(P, np.float32)
    return int(_lib.lib().bz_fpu_mass(n.ctypes.data, p.ctypes.data, len(n)))


def _c_value(N, P, q, r):
    n, p = np.asarray(N, np.uint32), np.asarray(P, np.float32)
    return f32(_lib.lib().bz_fpu_value(n.ctypes.data, p.ctypes.data, len(n), C.c_float(q), C.c_float(r)))


def _same(a, b):
    return np.asarray(a, np.float32).view(np.uint32) == np.asarray(b, np.float32).view(np.uint32)


def test_mass_and_value_equal_the_restatement_on_random_edge_sets_in_every_order_tried():
    rng = np.random.default_rng(0)
    visited_some = partial = 0
    with np.errstate(all="ignore"):
        for trial in range(3000):
            n = int(rng.integers(1, 35))
            P = rng.dirichlet(np.full(n, float(rng.choice([0.1, 0.5, 2.0])))).astype(np.float32)
            N = rng.multinomial(int(rng.choice([0, 1, 3, 16, 200, 800])), rng.dirichlet(np.full(n, 0.3))).astype(np.uint32)
            q, r = f32(rng.uniform(-1, 1)), f32(rng.choice([0.0, 0.1, 0.2, 1.0, 3.0]))
            S = fpu_mass(N, P)
            want = fpu_value(S, q, r)
            assert _c_mass(N, P) == S and S < 1 << 30, (trial, N, P)
            assert _same(_c_value(N, P, q, r), want), (trial, N, P, q, r)
            for _ in range(3):  # an integer sum has no order
                o = rng.permutation(n)
                assert _c_mass(N[o], P[o]) == S and _same(_c_value(N[o], P[o], q, r), want)
            assert _c_mass(N[::-1].copy(), P[::-1].copy()) == S
            visited_some += 0 < S
            partial += 0 < int((N > 0).sum()) < n
    assert visited_some > 1000 and partial > 1000, (visited_some, partial)  # (a mass above 2^24: the edge cases below)


def test_mass_and_value_edge_cases_and_hand_computed_values():
    one, q = f32(1.0), f32(0.25)
    den = np.array([1], np.uint32).view(np.float32)[0]  # the smallest denormal
    nan = f32(np.nan)
    cases = {
        "no edge visited": ([0, 0, 0], [0.5, 0.25, 0.25], 0),
        "all visited": ([1, 2, 3], [0.5, 0.25, 0.25], 1 << 24),
        "P exactly 0": ([4, 1], [0.0, 1.0], 1 << 24),
        "P exactly 1": ([7], [1.0], 1 << 24),
        "P denormal": ([3, 2], [den, f32(1e-39)], 0),
        "P NaN": ([3, 2], [nan, 0.5], 1 << 23),
        "P negative": ([3, 2], [-0.5, 0.5], 1 << 23),
        "one unvisited edge": ([0], [1.0], 0),
        "a prior just below 2^-24": ([5], [f32(5.9e-8)], 0),
        "a prior of 2^-24": ([5], [INV24], 1),
    }
    with np.errstate(all="ignore"):
        for name, (N, P, S) in cases.items():
            assert fpu_mass(N, P) == S and _c_mass(N, P) == S, name
            for r in (0.0, 0.2, 1.5):
                assert _same(_c_value(N, P, q, r), fpu_value(S, q, r)), (name, r)
            if S == 0:  # m = 0: f is the node's own value
                assert _same(_c_value(N, P, q, 0.2), q), name
    # a mass just above 2^24 (a noised root's priors may sum to 1 + a few ulp): (float)S rounds to even
    N, P = [1, 1, 1], [f32(0.5), f32(0.5), f32(3 * 2.0 ** -24)]
    assert fpu_mass(N, P) == (1 << 24) + 3 and int(f32((1 << 24) + 3)) == (1 << 24) + 4
    assert _c_mass(N, P) == (1 << 24) + 3
    assert _same(_c_value(N, P, q, 0.2), fpu_value((1 << 24) + 3, q, 0.2))
    # hand-computed: P = (0.25, 0.5, 0.25), N = (2, 0, 1): S = 2^23, m = sqrt(0.5) -> f = 0.5 - 0.2 * 0.70710677 = 0.35857865
    assert fpu_mass([2, 0, 1], [0.25, 0.5, 0.25]) == 1 << 23
    got = _c_value([2, 0, 1], [0.25, 0.5, 0.25], 0.5, 0.2)
    assert _same(got, f32(0.5) - f32(0.2) * np.sqrt(f32(0.5))) and abs(float(got) - 0.35857865) < 1e-7
    # hand-computed: P = (0.25, 0.75), both visited: S = 2^24, m = 1 exactly -> f = q - r: -0.6 - 1.0 = -1.6 (no clamp)
    assert _same(_c_value([1, 5], [0.25, 0.75], -0.6, 1.0), f32(-0.6) - f32(1.0)) and float(_c_value([1, 5], [0.25, 0.75], -0.6, 1.0)) < -1.0
    # reduction 0: an unvisited child is worth exactly its parent
    assert _same(_c_value([1, 5, 0], [0.25, 0.5, 0.25], -0.6, 0.0), f32(-0.6))


def test_mass_and_value_refuse_bad_arguments_with_a_message():
    L = _lib.lib()
    N, P = np.array([1, 2], np.uint32), np.array([0.5, 0.5], np.float32)
    for args in ((None, P.ctypes.data, 2), (N.ctypes.data, None, 2), (N.ctypes.data, P.ctypes.data, 0), (N.ctypes.data, P.ctypes.data, 256)):
        assert L.bz_fpu_mass(*args) == 0xFFFFFFFF and b"bz_fpu_mass" in L.bz_last_error()
        assert np.isnan(L.bz_fpu_value(*args, C.c_float(0.0), C.c_float(0.2)))
    big = np.array([0.5, 3.0], np.float32)
    assert L.bz_fpu_mass(N.ctypes.data, big.ctypes.data, 2) == 0xFFFFFFFF and b"no prior" in L.bz_last_error()


# ---------------------------------------------------------------- the twin
GAMES = ["ttt", "reversi", "reversi4"]
SIMS = {"ttt": (40, 8), "reversi": (24, 6), "reversi4": (32, 8)}


@pytest.mark.parametrize("game", GAMES)
@pytest.mark.parametrize("ev", ["hash", "uniform"])
@pytest.mark.parametrize("noise", [False, True])
def test_twin_root_visits_equal_the_budget_and_the_rule_bites(game, ev, noise):
    """the inputs of the GPU file's self-play cases: sum N(root) = the budget after every search, at most sims + 1 nodes, and
    walks in which the rule chose another edge than plain PUCT would have from the same statistics"""
    sims, _ = SIMS[game]
    changed = walks = 0
    for gid in (0, 3, 5):
        tw = FpuTwin(game, ev, boards=boards(), **(NOISE if noise else {}))
        rows, w, _ = tw.selfplay(gid, sims, 4, 1, 3, slot=gid, stagger=3)
        assert w in (-1, 0, 1) and len(rows) == len(tw.log) == len(tw.budgets)
        assert tw.root_sums == tw.budgets == [sims] * len(rows) and tw.max_nodes <= sims + 1 and tw.n_overrides == 0
        for lg, row in zip(tw.log, rows):
            assert lg["Np"] == lg["N"] and sum(lg["N"]) == sims
            assert abs(sum(float(x) for x in row[2]) - 1.0) <= 1e-5
        changed, walks = changed + tw.n_changed, walks + tw.n_walks
    # Reversi 8x8 under the uniform evaluator is the one input on which the rule cannot bite at these sizes: every value is 0 (no
    # game ends inside 24 simulations), so f <= 0 only lowers unvisited edges that the u term still puts first.  The GPU file
    # therefore pairs the uniform evaluator with tic-tac-toe and Reversi 4x4, and Reversi 8x8 with the hash evaluator.
    assert changed < walks and (changed > 0 or (game, ev) == ("reversi", "uniform")), (changed, walks)


@pytest.mark.parametrize("game", GAMES)
def test_twin_under_the_cap_draws_the_cap_twins_budgets_and_uses_the_rule_in_fast_searches(game):
    sims, fast = SIMS[game]
    kinds, changed_fast = set(), 0
    for gid in (1, 4, 6):
        tw = FpuTwin(game, "hash", cap=(fast, 32768), boards=boards(), **NOISE)
        rows, w, _ = tw.selfplay(gid, sims, 3, 1, 9)
        assert len(rows) == sum(b == sims for b in tw.budgets) and tw.root_sums == tw.budgets
        # the budgets are a function of (seed, game id, moves made) alone: the cap twin's, move for move
        ref = CapTwin(game, "hash", fast, 32768, boards=boards(), **NOISE)
        ref.selfplay(gid, sims, 3, 1, 9)
        n = min(len(tw.budgets), len(ref.budgets))  # (the two games part; the draw of move t does not depend on the position)
        assert tw.budgets[:n] == ref.budgets[:n]
        kinds |= set(tw.budgets)
        for lg in tw.log:
            if lg["budget"] == fast:  # a fast search: the rule without noise on the same position
                one = FpuTwin(game, "hash", boards=boards())
                root = one.search(lg["b"], lg["p"], fast)
                assert lg["N"] == [e["N"] for e in root["edges"]] and lg["W"] == [e["W"] for e in root["edges"]]
                changed_fast += one.n_changed
    assert kinds == {sims, fast} and changed_fast > 0


@pytest.mark.parametrize("game", GAMES)
def test_twin_with_forced_playouts_still_forces_and_prunes(game):
    sims, _ = SIMS[game]
    overrides = differs = changed = 0
    for gid in (0, 3, 5):
        tw = FpuTwin(game, "hash", k=2.0, prune=True, boards=boards(), **NOISE)
        rows, w, _ = tw.selfplay(gid, sims, 4, 1, 3, slot=gid, stagger=3)
        overrides, changed = overrides + tw.n_overrides, changed + tw.n_changed
        differs += sum(lg["Np"] != lg["N"] for lg in tw.log)
        assert all(sum(lg["N"]) == sims for lg in tw.log)
    assert overrides > 0 and differs > 0 and changed > 0, (overrides, differs, changed)


@pytest.mark.parametrize("game", GAMES)
def test_zero_reductions_pick_plain_pucts_edge_at_a_root_whose_children_are_all_unvisited(game):
    """the only identity with the plain engine: reduction = root_reduction = 0 on the uniform evaluator -- at the first walk
    every child is unvisited, qx = 0 and m = 0, so f = 0 = plain PUCT's q.  (From the second walk on the root's value is
    generally not 0 and the searches part.)"""
    b = boards()[1]() if game == "ttt" else boards()[0](size=4 if game == "reversi4" else 8)
    tw, ref = FpuTwin(game, "uniform", (0.0, 0.0), boards=boards()), Twin(game, "uniform", boards=boards())
    ra, rb = tw.search(b, 1, 1), ref.search(b, 1, 1)
    assert [e["N"] for e in ra["edges"]] == [e["N"] for e in rb["edges"]] and tw.n_changed == 0
    assert sum(e["N"] for e in ra["edges"]) == 1


def test_wr_is_the_running_sum_in_simulation_order_not_the_sum_over_the_edges():
    """Wr adds one value per simulation; the sum over the root's edges adds the same values grouped by edge -- another order,
    so other roundings: the twin must keep the former"""
    differs = 0
    for gid in range(4):
        tw = FpuTwin("reversi", "hash", boards=boards())
        b = boards()[0](size=8)
        root = tw.search(b, 1, 64 + gid)
        s = f32(0.0)
        for e in root["edges"]:
            s = f32(s + e["W"])
        assert abs(float(s) - float(tw.Wr)) < 1e-4 and tw.n_done == 64 + gid
        differs += not _same(s, tw.Wr)
    assert differs > 0


# ---------------------------------------------------------------- the buffer and the refusals: the C entry points
def test_fpu_bytes_is_one_float_per_game_rounded_up_to_256():
    L = _lib.lib()
    for n, want in ((1, 256), (64, 256), (65, 512), (4096, 16384)):
        assert L.bz_engine_fpu_bytes(C.byref(_cfg(1, n, 16))) == want
    assert L.bz_engine_fpu_bytes(C.byref(_cfg(0, 64, 16))) == 256
    for cfg, word in ((_cfg(flags=_lib.ENGINE_REUSE_SUBTREE), b"subtree reuse"), (_cfg(K=2), b"leaves_per_step")):
        assert L.bz_engine_fpu_bytes(C.byref(cfg)) == -1
        assert word in L.bz_last_error() and b"first-play urgency" in L.bz_last_error()
    assert L.bz_engine_fpu_bytes(None) == -1 and L.bz_engine_fpu_bytes(C.byref(_cfg(sims=0))) == -1


def test_fpu_check_accepts_and_refuses_with_a_message():
    L = _lib.lib()
    chk = lambda cfg, r=0.2, r0=0.1: L.bz_engine_fpu_check(C.byref(cfg), C.c_float(r), C.c_float(r0))  # noqa: E731
    for game in (0, 1, 2, 3):
        assert chk(_cfg(game, 4, 8)) == 0 and chk(_cfg(game, 4096, 800), 0.0, 0.0) == 0  # (0 is a reduction, not "off")
    assert chk(_cfg(flags=_lib.ENGINE_EVAL_CACHE | _lib.ENGINE_EVAL_CACHE_CARRY)) == 0
    noisy = _cfg()
    noisy.dirichlet_alpha, noisy.dirichlet_eps = 0.3, 0.25
    assert chk(noisy) == 0
    for cfg, r, r0, word in ((_cfg(flags=_lib.ENGINE_REUSE_SUBTREE), 0.2, 0.1, b"subtree reuse"), (_cfg(K=2), 0.2, 0.1, b"leaves_per_step"),
                             (_cfg(K=32), 0.2, 0.1, b"leaves_per_step"), (_cfg(), -1.0, 0.1, b"finite"), (_cfg(), 0.2, -0.1, b"finite"),
                             (_cfg(), float("inf"), 0.1, b"finite"), (_cfg(), 0.2, float("inf"), b"finite"),
                             (_cfg(), float("nan"), 0.1, b"finite"), (_cfg(), 0.2, float("nan"), b"finite")):
        assert chk(cfg, r, r0) == _lib.BZ_EINVAL
        assert word in L.bz_last_error() and b"first-play urgency" in L.bz_last_error(), L.bz_last_error()
    assert L.bz_engine_fpu_check(None, C.c_float(0.2), C.c_float(0.1)) == _lib.BZ_EINVAL
    assert chk(_cfg(sims=0)) == _lib.BZ_EINVAL


def test_set_fpu_refuses_a_null_engine_with_a_message():
    """(an engine needs a GPU: the setter's refusals on a live engine are in tests/test_gpu_fpu.py)"""
    L = _lib.lib()
    assert L.bz_engine_set_fpu(None, 1, C.c_float(0.2), C.c_float(0.1), None, 0, None) == _lib.BZ_EINVAL
    assert b"bz_engine_set_fpu" in L.bz_last_error()


def test_the_abi_version_stays_and_the_header_documents_the_rule():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bz_abi.h")).read()
    assert _lib.lib().bz_abi_version() == 7
    for name in ("bz_engine_fpu_bytes", "bz_engine_fpu_check", "bz_engine_set_fpu", "bz_fpu_mass", "bz_fpu_value"):
        assert f"{name}(" in hdr and name in _lib.ABI_SYMBOLS
    assert "DESIGN.md 3.20" in hdr and "16777216" in hdr


# ---------------------------------------------------------------- Python validation (no GPU needed)
def _no_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("touched a device")
    monkeypatch.setattr(_lib, "require_gpu", no_device)
    monkeypatch.setattr(_lib, "lib", no_device)


def _everyone(fp, **kw):
    """every public entry point that takes fpu=, as thunks"""
    from betazero_amd.arena import play_arena
    from betazero_amd.engine import PipelinedSelfPlay, SelfPlayEngine, check_fpu, self_play
    from betazero_amd.match import MatchPlayer, play_match
    from betazero_amd.players import MCTSPlayer
    lps, gum = kw.get("leaves_per_step", 1), kw.get("gumbel")
    out = [lambda: SelfPlayEngine("reversi", 4, 16, "uniform", fpu=fp, **kw),
           lambda: PipelinedSelfPlay("reversi", 4, 16, "uniform", fpu=fp, streams=[None], **kw),
           lambda: self_play("ttt", 4, 16, fpu=fp, **kw),
           lambda: check_fpu(fp, kw.get("reuse_subtree", False), lps, gum)]
    if "reuse_subtree" not in kw:  # (players and matches have no subtree reuse)
        out += [lambda: MCTSPlayer(1, sims=16, fpu=fp, **kw),
                lambda: play_match("reversi", 4, MatchPlayer(16, fpu=fp, **kw), MatchPlayer(16)),
                lambda: play_match("reversi", 4, MatchPlayer(16), MatchPlayer(16, fpu=fp, **kw)),
                lambda: play_arena("reversi", 4, 16, fpu=fp, **kw)]
    return out


@pytest.mark.parametrize("bad", [-0.1, -2.0, float("nan"), float("inf"), 1e39, True, "0.2", None])
@pytest.mark.parametrize("field", ["reduction", "root_reduction"])
def test_python_refuses_a_bad_reduction_before_touching_a_device(bad, field, monkeypatch):
    from betazero_amd.engine import Fpu
    _no_device(monkeypatch)
    for thunk in _everyone(Fpu(**{field: bad})):
        with pytest.raises(ValueError, match=f"{field} must be"):
            thunk()


def test_python_refuses_bad_values_and_combinations_before_touching_a_device(monkeypatch):
    from betazero_amd.engine import Fpu
    _no_device(monkeypatch)
    for bad in ("yes", 0.2, 1, 0, (0.2, 0.1), {"reduction": 0.2}):
        for thunk in _everyone(bad):
            with pytest.raises(ValueError, match="fpu must be"):
                thunk()
    for fp in (True, Fpu(), Fpu(0.0, 0.0)):
        for kw, word in (({"reuse_subtree": True}, "reuse"), ({"leaves_per_step": 2}, "leaves_per_step"), ({"gumbel": True}, "Gumbel")):
            for thunk in _everyone(fp, **kw):
                with pytest.raises(ValueError, match=word):
                    thunk()


def test_python_accepts_off_true_and_a_config_everywhere():
    from betazero_amd.arena import play_arena
    from betazero_amd.engine import Fpu, PipelinedSelfPlay, SelfPlayEngine, check_fpu, self_play
    from betazero_amd.match import MatchPlayer
    from betazero_amd.players import MCTSPlayer
    assert check_fpu(None) is None and check_fpu(False) is None
    assert check_fpu(True) == Fpu(float(f32(0.2)), float(f32(0.1)))
    assert check_fpu(Fpu(np.float32(0.5), 0)) == Fpu(0.5, 0.0) and check_fpu(Fpu(0, 0)) == Fpu(0.0, 0.0)
    assert check_fpu(Fpu(1e-46, 0.1)).reduction == 0.0  # (rounds to 0 in float32: a valid reduction)
    for fn in (SelfPlayEngine.__init__, PipelinedSelfPlay.__init__, self_play, MCTSPlayer.__init__, play_arena):
        assert inspect.signature(fn).parameters["fpu"].default is None
    assert MatchPlayer().fpu is None and MatchPlayer(fpu=True).checked("reversi", 2, "a")[0] == "uniform"
