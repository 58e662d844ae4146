"""Forced playouts and policy target pruning without a GPU: bz_forced_prune -- the function the kernels run --
against a restatement in numpy float32, the invariants of the pruning, the forced twin (ForcedTwin: CapTwin with the forced
rule at the root and the pruned pi in its rows) and the ABI / Python validation.  tests/test_gpu_forced_playouts.py pins the
engine to this twin."""
import ctypes as C

import numpy as np
import pytest

from betazero_amd import _lib
from oracle.py_twin import Twin, f32, rng_draw
from test_playout_cap_cpu import CapTwin, _cfg, boards, cap_budget

TINY_K = 1e-6  # fsqrt(k P sum N) <= fsqrt(1e-6 * 8189) < 0.1: no edge is ever forced


def _score(q, c, P, sq, N):
    """DESIGN.md 3.3, one rounding per operation"""
    u = c * P
    u = u * sq
    u = u / (f32(1.0) + f32(N))
    return q + u


def forced_nf(k, P, sumN):
    t = f32(k) * f32(P)
    t = t * f32(sumN)
    return np.sqrt(t)


def forced_prune(N, W, P, c, k):
    """DESIGN.md 3.16 restated: the pruned visit counts N' of one root, edges in ascending action order"""
    c, k = f32(c), f32(k)
    sumN = sum(N)
    cs = max(range(len(N)), key=lambda i: (N[i], -i))  # max N, lowest action
    sq = np.sqrt(f32(max(sumN, 1)))
    with np.errstate(all="ignore"):
        ss = _score(f32(W[cs]) / f32(N[cs]) if N[cs] > 0 else f32(0.0), c, f32(P[cs]), sq, N[cs])
        out = list(N)
        for i in range(len(N)):
            if i == cs or N[i] == 0:
                continue
            nf = forced_nf(k, P[i], sumN)
            m = int(np.ceil(nf)) if nf < f32(N[i]) else N[i]
            q = f32(W[i]) / f32(N[i])
            for t in range(1, min(m, N[i]) + 1):
                if not (_score(q, c, f32(P[i]), sq, N[i] - t) < ss):
                    break
                out[i] = N[i] - t
            if out[i] < N[i] and out[i] <= 1:
                out[i] = 0
    return out


class ForcedTwin(CapTwin):
    """CapTwin with forced playouts: at the root of a full search an edge with 0 < N < fsqrt(k P sum N) scores +inf; a full
    search's row holds N' / sum N' (prune) or N / sum N.  cap = (fast_sims, full_q) or None (every search full).  After
    selfplay(): log = one dict per search (budget, root position, root N / W / P / actions, the pi and the action
    root_policy() reports), n_overrides = walks in which the forced rule took another edge than PUCT's own first maximum."""

    def __init__(self, game, eval_kind, k, prune=True, cap=None, eval_fn=None, **kw):
        fast, full_q = cap if cap is not None else (0, 65536)  # (full_q 65536: every draw is a full search)
        super().__init__(game, eval_kind, fast, full_q, eval_fn=eval_fn, **kw)
        self.k, self.prune, self.force_on, self.n_overrides, self.log = f32(k), prune, True, 0, []

    def simulate(self, root):
        node, path = root, []
        while True:
            if node["term"]:
                v = f32(node["tv"])
                break
            sumN = sum(e["N"] for e in node["edges"])
            sq = np.sqrt(f32(max(sumN, 1)))
            best, bests, own = None, f32(-np.inf), None
            for e in node["edges"]:
                q = e["W"] / f32(e["N"]) if e["N"] > 0 else f32(0.0)
                s = _score(q, self.c, e["P"], sq, e["N"])
                if own is None or s > own[1]:
                    own = (e, s)
                if node is root and self.force_on and e["N"] > 0 and f32(e["N"]) < forced_nf(self.k, e["P"], sumN):
                    s = f32(np.inf)
                if s > bests:
                    best, bests = e, s
            if node is root and best is not own[0]:
                self.n_overrides += 1
            path.append(best)
            if best["child"] is not None:
                node = best["child"]
                continue
            ch = self.new_node(self.play(node["b"], node["p"], best["a"]), -node["p"])
            best["child"] = ch
            v = f32(ch["tv"]) if ch["term"] else self.expand(ch)
            break
        val = -v
        for e in reversed(path):
            e["N"] += 1
            e["W"] = f32(e["W"] + val)
            val = -val

    def selfplay(self, gid, sims, temp_moves, openings, seed, slot=0, stagger=0):
        b, p, made = self.start(slot, gid, openings, seed, stagger)
        ex, passes = [], 0
        self.budgets, self.root_sums, self.log, self.n_overrides = [], [], [], 0
        while True:
            budget = cap_budget(seed, gid, made, sims, self.fast_sims, self.full_q)
            full = budget == sims
            self.noise_key, self.noise_on, self.force_on = (seed, gid, made), full, full
            before = self.n_overrides
            root = self.search(b, p, budget)
            edges = root["edges"]
            N = [e["N"] for e in edges]
            sumN = sum(N)
            self.budgets.append(budget)
            self.root_sums.append(sumN)
            if made < temp_moves:  # the move: DESIGN.md 3.7 over the raw N
                r = rng_draw(seed, gid, made) % sumN
                cum = 0
                for e in edges:
                    cum += e["N"]
                    if cum > r:
                        pick = e
                        break
            else:
                pick, bn = edges[0], 0
                for e in edges:
                    if e["N"] > bn:
                        pick, bn = e, e["N"]
            Np = forced_prune(N, [e["W"] for e in edges], [e["P"] for e in edges], self.c, self.k) if (full and self.prune) else N
            pi = [f32(0.0)] * self.na
            with np.errstate(all="ignore"):
                for e, n1 in zip(edges, Np):
                    pi[e["a"]] = f32(n1) / f32(sum(Np))
            self.log.append({"budget": budget, "b": b, "p": p, "a": [e["a"] for e in edges], "N": N, "Np": list(Np),
                             "W": [e["W"] for e in edges], "P": [e["P"] for e in edges], "pi": pi, "act": pick["a"],
                             "overrides": self.n_overrides - before})
            if full:
                own, opp = self.bits(b, p)
                ex.append((own, opp, pi, p, pick["a"]))
            b = self.play(b, p, pick["a"])
            p, made = -p, made + 1
            over, w = self.terminal(b)
            if over:
                return ex, w, passes
            if not self.moves(b, p):
                p, passes = -p, passes + 1


# ---------------------------------------------------------------- the pruning function
def _c_prune(N, W, P, c, k):
    n = len(N)
    a = np.asarray(N, np.uint32)
    w, p, out = np.asarray(W, np.float32), np.asarray(P, np.float32), np.full(n, 0xFFFFFFFF, np.uint32)
    rc = _lib.lib().bz_forced_prune(a.ctypes.data, w.ctypes.data, p.ctypes.data, n, C.c_float(c), C.c_float(k), out.ctypes.data)
    assert rc == 0, _lib.lib().bz_last_error()
    return [int(x) for x in out]


def _check_invariants(N, W, P, c, k, Np):
    sumN, cs = sum(N), max(range(len(N)), key=lambda i: (N[i], -i))
    assert Np[cs] == N[cs]
    for i in range(len(N)):
        m = int(min(np.ceil(forced_nf(k, P[i], sumN)), N[i]))
        assert Np[i] == 0 or N[i] - m <= Np[i] <= N[i], (i, N[i], Np[i], m)
        assert Np[i] != 1 or N[i] == 1, (i, N[i])  # a reduced child is never left with one visit
    assert sum(Np) >= N[cs]
    if sum(Np) > 0:
        pi = [f32(x) / f32(sum(Np)) for x in Np]
        assert abs(sum(float(x) for x in pi) - 1.0) <= len(N) * 2.0 ** -24  # half an ulp of a value below 1 per division
        # the played move is chosen from the raw N; even a tau = 0 choice over N' would be the same edge
        assert max(range(len(N)), key=lambda i: (Np[i], -i)) == cs


def _random_root(rng, n, total):
    """a root as a PUCT search leaves it, roughly: visits ~ multinomial(priors), W = N q with |q| <= 1"""
    P = rng.dirichlet(np.full(n, 0.5)).astype(np.float32)
    N = rng.multinomial(total, rng.dirichlet(np.full(n, 0.3)))
    W = (N * rng.uniform(-1, 1, n)).astype(np.float32)
    return [int(x) for x in N], [f32(x) for x in W], [f32(x) for x in P]


def test_prune_equals_the_restatement_on_random_roots():
    rng = np.random.default_rng(0)
    changed = zeroed = 0
    for trial in range(400):
        n = int(rng.integers(1, 35))
        total = int(rng.choice([1, 2, 5, 16, 64, 200, 800, 3000, 8189]))
        N, W, P = _random_root(rng, n, total)
        c, k = float(rng.choice([0.5, 1.5, 4.0])), float(rng.choice([0.25, 1.0, 2.0, 8.0, TINY_K]))
        want = forced_prune(N, W, P, c, k)
        assert _c_prune(N, W, P, c, k) == want, (trial, N, W, P, c, k)
        _check_invariants(N, W, P, c, k, want)
        changed += want != N
        zeroed += any(a > 0 and b == 0 for a, b in zip(N, want))
    assert changed > 50 and zeroed > 20, (changed, zeroed)  # the comparison is not one of untouched inputs


def test_prune_edge_cases_equal_the_restatement():
    one = f32(1.0)
    cases = {
        "a single edge": ([7], [f32(-3.0)], [one]),
        "a single unvisited edge": ([0], [f32(0.0)], [one]),
        "all N equal": ([5] * 6, [f32(x) for x in (-1, 0.5, 2, -3, 0, 1)], [f32(1 / 6)] * 6),
        "N = 0 edges": ([0, 9, 0, 3, 0, 1], [f32(x) for x in (0, 2, 0, -2, 0, -1)], [f32(x) for x in (.3, .2, .1, .2, .1, .1)]),
        "nothing visited": ([0, 0, 0], [f32(0)] * 3, [f32(x) for x in (.5, .25, .25)]),
        "a child reduced exactly to 1": ([20, 3], [f32(10.0), f32(-6.0)], [f32(0.5), f32(0.5)]),
        "P at 0 and at 1": ([30, 4, 2], [f32(3.0), f32(-4.0), f32(-2.0)], [f32(0.0), one, f32(0.0)]),
        "P = 1 on the most visited": ([4, 30, 2], [f32(-4.0), f32(3.0), f32(-2.0)], [f32(0.0), one, f32(0.0)]),
        "the largest sum": ([8000, 100, 60, 29], [f32(4000.0), f32(-50.0), f32(-60.0), f32(0.0)], [f32(x) for x in (.4, .3, .2, .1)]),
        "the largest sum on one edge": ([8189], [f32(100.0)], [one]),
        "k large enough to offer every visit": ([50, 40, 30], [f32(25.0), f32(-40.0), f32(-30.0)], [f32(x) for x in (.5, .3, .2)]),
    }
    assert sum(cases["the largest sum"][0]) == 8189
    for name, (N, W, P) in cases.items():
        for k in (2.0, 0.5, 1e4 if name.startswith("k large") else 8.0, TINY_K):
            want = forced_prune(N, W, P, 1.5, k)
            assert _c_prune(N, W, P, 1.5, k) == want, (name, k)
            _check_invariants(N, W, P, 1.5, k, want)
    # hand-checked: N = (20, 3), q = (0.5, -1), P = 0.5 each, c = 1.5, k = 2: sq = sqrt(23) ~ 4.80, s* = 0.5 + 3.60 / 21 ~ 0.67;
    # nf = sqrt(23) -> m = 5 > 3; the child's score with 2, 1, 0 visits in u is -1 + 3.60 / (3, 2, 1) = 0.20, 0.80 (>= s*): one
    # visit goes, 2 are left
    assert forced_prune([20, 3], [f32(10.0), f32(-3.0)], [f32(0.5), f32(0.5)], 1.5, 2.0) == [20, 2]
    # ... and with q = -2 (W = -6) the scores are -0.80, -0.20, 1.60: two visits go, 1 is left -> 0
    assert forced_prune([20, 3], [f32(10.0), f32(-6.0)], [f32(0.5), f32(0.5)], 1.5, 2.0) == [20, 0]
    assert _c_prune([20, 3], [10.0, -6.0], [0.5, 0.5], 1.5, 2.0) == [20, 0]
    assert forced_prune([20, 4], [f32(10.0), f32(-8.0)], [f32(0.5), f32(0.5)], 1.5, 0.16) == [20, 2]  # nf = sqrt(1.92): m = 2 stops it at 2


def test_prune_refuses_bad_arguments_with_a_message():
    L = _lib.lib()
    N, W, P, out = np.array([3, 1], np.uint32), np.zeros(2, np.float32), np.full(2, 0.5, np.float32), np.zeros(2, np.uint32)
    ptr = lambda a: a.ctypes.data  # noqa: E731
    for args in ((None, ptr(W), ptr(P), 2, 1.5, 2.0, ptr(out)), (ptr(N), ptr(W), ptr(P), 0, 1.5, 2.0, ptr(out)),
                 (ptr(N), ptr(W), ptr(P), 256, 1.5, 2.0, ptr(out)), (ptr(N), ptr(W), ptr(P), 2, 1.5, 0.0, ptr(out)),
                 (ptr(N), ptr(W), ptr(P), 2, 1.5, -1.0, ptr(out)), (ptr(N), ptr(W), ptr(P), 2, 1.5, float("inf"), ptr(out)),
                 (ptr(N), ptr(W), ptr(P), 2, 1.5, float("nan"), ptr(out)), (ptr(N), ptr(W), ptr(P), 2, 1.5, 2.0, None)):
        assert L.bz_forced_prune(*args) == _lib.BZ_EINVAL
        assert b"bz_forced_prune" in L.bz_last_error()
    big = np.array([3, 16384], np.uint32)
    assert L.bz_forced_prune(ptr(big), ptr(W), ptr(P), 2, 1.5, 2.0, ptr(out)) == _lib.BZ_EINVAL and b"16383" in L.bz_last_error()


# ---------------------------------------------------------------- the twin
GAMES = ["ttt", "reversi", "reversi4"]
SIMS = {"ttt": (40, 8), "reversi": (24, 6), "reversi4": (32, 8)}
NOISE = dict(dir_alpha=0.3, dir_eps=0.25)


def _same_rows(rows, ref):
    assert len(rows) == len(ref)
    for a, b in zip(rows, ref):
        assert a[0] == b[0] and a[1] == b[1] and a[3] == b[3] and a[4] == b[4]
        assert np.array_equal(np.asarray(a[2], np.float32).view(np.uint32), np.asarray(b[2], np.float32).view(np.uint32))


@pytest.mark.parametrize("game", GAMES)
@pytest.mark.parametrize("ev", ["hash", "uniform"])
@pytest.mark.parametrize("noise", [False, True])
def test_twin_with_a_tiny_k_forces_nothing_and_equals_the_plain_twin(game, ev, noise):
    """k so small that nf < 1 for every edge: no edge is ever forced, so the search -- and with prune off every row, bit for bit
    -- is the plain twin's.  With prune on the rule still offers m = ceil(nf) = 1 visit of every other child to the pruning
    (DESIGN.md 3.16), so there the games, moves and raw statistics are the plain twin's and every N' is N, N - 1 or 0."""
    sims, fast = SIMS[game]
    kw = NOISE if noise else {}
    for gid in (2, 7):
        ref, rw, rps = Twin(game, ev, boards=boards(), **kw).selfplay(gid, sims, 3, 1, 5)
        tw = ForcedTwin(game, ev, TINY_K, prune=False, boards=boards(), **kw)
        rows, w, ps = tw.selfplay(gid, sims, 3, 1, 5)
        assert (w, ps) == (rw, rps) and tw.n_overrides == 0
        _same_rows(rows, ref)
        tp = ForcedTwin(game, ev, TINY_K, prune=True, boards=boards(), **kw)
        prow, w, ps = tp.selfplay(gid, sims, 3, 1, 5)
        assert (w, ps) == (rw, rps) and tp.n_overrides == 0 and len(prow) == len(ref)
        for a, b, lg, lg0 in zip(prow, ref, tp.log, tw.log):
            assert a[0] == b[0] and a[1] == b[1] and a[3] == b[3] and a[4] == b[4] and lg["N"] == lg0["N"]
            assert all(n1 in (n0, n0 - 1, 0) for n0, n1 in zip(lg["N"], lg["Np"]))
        # under the cap too: the cap twin's games
        cref = CapTwin(game, ev, fast, 32768, boards=boards(), **kw)
        crow, cw, _ = cref.selfplay(gid, sims, 3, 1, 5)
        tc = ForcedTwin(game, ev, TINY_K, prune=False, cap=(fast, 32768), boards=boards(), **kw)
        rows, w, _ = tc.selfplay(gid, sims, 3, 1, 5)
        assert w == cw and tc.budgets == cref.budgets and tc.n_overrides == 0
        _same_rows(rows, crow)


@pytest.mark.parametrize("game", GAMES)
@pytest.mark.parametrize("ev", ["hash", "uniform"])
def test_twin_forces_prunes_and_keeps_the_moves_of_the_unpruned_search(game, ev):
    """k = 2 with noise: the forced rule overrides PUCT, the pruned pi differs from the raw one and some child is pruned to 0
    -- counted, so that neither this test nor the GPU file's equalities (same cases) are vacuous; pruning changes pi alone"""
    sims, _ = SIMS[game]
    overrides = differs = zeroed = 0
    for gid in (0, 3, 5):
        tw = ForcedTwin(game, ev, 2.0, prune=True, boards=boards(), **NOISE)
        rows, w, ps = tw.selfplay(gid, sims, 4, 1, 3, slot=gid, stagger=3)
        raw = ForcedTwin(game, ev, 2.0, prune=False, boards=boards(), **NOISE)
        rrows, rw, rps = raw.selfplay(gid, sims, 4, 1, 3, slot=gid, stagger=3)
        assert (w, ps) == (rw, rps) and len(rows) == len(rrows) == len(tw.log)
        overrides += tw.n_overrides
        for a, b, lg, lg0 in zip(rows, rrows, tw.log, raw.log):
            assert a[0] == b[0] and a[1] == b[1] and a[3] == b[3] and a[4] == b[4]  # positions, mover, the played move
            assert lg["N"] == lg0["N"] and lg["W"] == lg0["W"] and lg0["Np"] == lg0["N"] and sum(lg["N"]) == sims
            _check_invariants(lg["N"], lg["W"], lg["P"], 1.5, 2.0, lg["Np"])
            assert abs(sum(float(x) for x in a[2]) - 1.0) <= 1e-6  # (a tau = 1 move may be a child whose pi was pruned to 0)
            differs += lg["Np"] != lg["N"]
            zeroed += any(n0 > 0 and n1 == 0 for n0, n1 in zip(lg["N"], lg["Np"]))
            assert (lg["Np"] != lg["N"]) == (not np.array_equal(np.asarray(a[2], np.float32), np.asarray(b[2], np.float32)))
    assert overrides > 0 and differs > 0 and zeroed > 0, (overrides, differs, zeroed)


@pytest.mark.parametrize("game", GAMES)
def test_twin_under_the_cap_forces_in_full_searches_only(game):
    sims, fast = SIMS[game]
    kinds, overrides = set(), 0
    for gid in (1, 4, 6):
        tw = ForcedTwin(game, "hash", 2.0, cap=(fast, 32768), boards=boards(), **NOISE)
        rows, w, _ = tw.selfplay(gid, sims, 3, 1, 9)
        assert len(rows) == sum(b == sims for b in tw.budgets) and tw.root_sums == tw.budgets
        kinds |= set(tw.budgets)
        for lg in tw.log:
            if lg["budget"] == fast:  # a fast search: plain PUCT without noise on the same position, its pi the raw one
                root = Twin(game, "hash", boards=boards()).search(lg["b"], lg["p"], fast)
                assert lg["overrides"] == 0 and lg["Np"] == lg["N"] == [e["N"] for e in root["edges"]]
                assert lg["W"] == [e["W"] for e in root["edges"]] and lg["P"] == [e["P"] for e in root["edges"]]
            else:
                overrides += lg["overrides"]
    assert kinds == {sims, fast} and overrides > 0
    # every search fast: the cap twin's game, nothing forced, no rows
    tw = ForcedTwin(game, "hash", 2.0, cap=(fast, 0), boards=boards(), **NOISE)
    rows, w, _ = tw.selfplay(2, sims, 3, 1, 5)
    ref = CapTwin(game, "hash", fast, 0, boards=boards(), **NOISE)
    _, rw, _ = ref.selfplay(2, sims, 3, 1, 5)
    assert rows == [] and w == rw and tw.n_overrides == 0 and tw.budgets == ref.budgets


# ---------------------------------------------------------------- refusals: the C entry points
def test_forced_playouts_check_accepts_and_refuses_with_a_message():
    L = _lib.lib()
    chk = lambda cfg, k: L.bz_engine_forced_playouts_check(C.byref(cfg), C.c_float(k))  # noqa: E731
    for game in (0, 1, 2, 3):
        assert chk(_cfg(game, 4, 8), 2.0) == 0 and chk(_cfg(game, 4096, 800), 0.5) == 0
    assert chk(_cfg(flags=_lib.ENGINE_EVAL_CACHE | _lib.ENGINE_EVAL_CACHE_CARRY), 2.0) == 0  # the cache is allowed
    noisy = _cfg()
    noisy.dirichlet_alpha, noisy.dirichlet_eps = 0.3, 0.25
    assert chk(noisy, 2.0) == 0 and chk(_cfg(), 0.0) == 0  # (k = 0 is "off": nothing to refuse)
    for cfg, k, word in ((_cfg(flags=_lib.ENGINE_REUSE_SUBTREE), 2.0, b"subtree reuse"), (_cfg(K=2), 2.0, b"leaves_per_step"),
                         (_cfg(K=32), 2.0, b"leaves_per_step"), (_cfg(), -1.0, b"finite"), (_cfg(), float("inf"), b"finite"),
                         (_cfg(), float("nan"), b"finite")):
        assert chk(cfg, k) == _lib.BZ_EINVAL
        assert word in L.bz_last_error() and b"forced playouts" in L.bz_last_error(), L.bz_last_error()
    assert L.bz_engine_forced_playouts_check(None, C.c_float(2.0)) == _lib.BZ_EINVAL
    assert chk(_cfg(sims=0), 2.0) == _lib.BZ_EINVAL


def test_set_forced_playouts_refuses_a_null_engine_with_a_message():
    """(an engine needs a GPU: the setter's refusals on a live engine are in tests/test_gpu_forced_playouts.py)"""
    L = _lib.lib()
    assert L.bz_engine_set_forced_playouts(None, C.c_float(2.0), 1, None) == _lib.BZ_EINVAL
    assert b"bz_engine_set_forced_playouts" in L.bz_last_error()


# ---------------------------------------------------------------- Python validation (no GPU needed)
def _no_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("touched a device")
    monkeypatch.setattr(_lib, "require_gpu", no_device)
    monkeypatch.setattr(_lib, "lib", no_device)


@pytest.mark.parametrize("bad", [0, 0.0, -2.0, float("nan"), float("inf"), 1e39, 1e-46, True, "2", None])
def test_python_refuses_a_bad_k_before_touching_a_device(bad, monkeypatch):
    from betazero_amd.engine import ForcedPlayouts, PipelinedSelfPlay, SelfPlayEngine, check_forced_playouts, self_play
    _no_device(monkeypatch)
    fp = ForcedPlayouts(bad)
    with pytest.raises(ValueError, match="k must be"):
        check_forced_playouts(fp)
    with pytest.raises(ValueError, match="k must be"):
        SelfPlayEngine("reversi", 4, 16, "uniform", forced_playouts=fp)
    with pytest.raises(ValueError, match="k must be"):
        PipelinedSelfPlay("reversi", 4, 16, "uniform", forced_playouts=fp, streams=[None])
    with pytest.raises(ValueError, match="k must be"):
        self_play("ttt", 4, 16, forced_playouts=fp)


def test_python_refuses_bad_values_and_combinations_before_touching_a_device(monkeypatch):
    from betazero_amd.engine import ForcedPlayouts, PipelinedSelfPlay, SelfPlayEngine, check_forced_playouts, self_play
    _no_device(monkeypatch)
    for bad in ("yes", 2.0, 2, (2.0, True), {"k": 2.0}):
        with pytest.raises(ValueError, match="forced_playouts must be"):
            check_forced_playouts(bad)
        with pytest.raises(ValueError, match="forced_playouts must be"):
            SelfPlayEngine("ttt", 4, 16, "uniform", forced_playouts=bad)
    for bad in (1, 0, None, "no"):
        with pytest.raises(ValueError, match="prune"):
            check_forced_playouts(ForcedPlayouts(2.0, bad))
    for fp in (True, ForcedPlayouts(), ForcedPlayouts(0.5, False)):
        for kw, word in (({"reuse_subtree": True}, "reuse"), ({"leaves_per_step": 2}, "leaves_per_step"), ({"gumbel": True}, "Gumbel")):
            with pytest.raises(ValueError, match=word):
                SelfPlayEngine("reversi", 4, 16, "uniform", forced_playouts=fp, **kw)
            with pytest.raises(ValueError, match=word):
                PipelinedSelfPlay("reversi", 4, 16, "uniform", forced_playouts=fp, streams=[None], **kw)
            with pytest.raises(ValueError, match=word):
                self_play("reversi", 4, 16, forced_playouts=fp, **kw)


def test_python_accepts_off_true_and_a_config_and_does_not_offer_it_to_players():
    import inspect

    from betazero_amd.arena import play_arena
    from betazero_amd.engine import ForcedPlayouts, check_forced_playouts
    from betazero_amd.match import MatchPlayer
    from betazero_amd.players import MCTSPlayer
    assert check_forced_playouts(None) is None and check_forced_playouts(False) is None
    assert check_forced_playouts(True) == ForcedPlayouts(2.0, True)
    assert check_forced_playouts(ForcedPlayouts(np.float32(0.5), np.bool_(False))) == ForcedPlayouts(0.5, False)
    assert check_forced_playouts(ForcedPlayouts(1)) == ForcedPlayouts(1.0, True)
    # a training-data tool: players and matches search at full strength
    for fn in (MCTSPlayer, MatchPlayer, play_arena):
        assert "forced_playouts" not in inspect.signature(fn).parameters
