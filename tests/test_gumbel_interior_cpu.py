"""Gumbel interior selection without a GPU: the rule for one node restated in numpy float32 and pinned to
bz_gumbel_interior_pick bit for bit, GumbelFullTwin -- the Gumbel twin of tests/test_gumbel_cpu.py with the rule below the root
-- its invariants, that the rule really chooses other edges than PUCT, the buffer-size function and the Python validation.
tests/test_gpu_gumbel_interior.py pins the engine to this twin."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from betazero_amd import _lib
from oracle.py_twin import expf_spec, f32, logf_spec
from test_gumbel_cpu import FLT_MIN, ONE, ZERO, GumbelTwin, _cfg, boards, game_roots
from test_match_cpu import Side

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ("n_sims", "n_path_nodes", "n_child_scored", "n_edges_backed", "n_expanded", "n_child_written", "n_env_steps")


def interior_rule(N, W, P, v, mvi, vs):
    """DESIGN.md 3.21, depth >= 1, n > 1: (p [n], sc [n], the chosen edge) from a node's N / W / P in edge order and its own
    value v -- every expression one float32 operation in the written order, sums in ascending edge order"""
    n = len(N)
    v, mvi, vs = f32(v), f32(mvi), f32(vs)
    S, nmax = int(sum(int(x) for x in N)), int(max(int(x) for x in N))
    pf = [f32(p) if f32(p) > FLT_MIN else FLT_MIN for p in P]
    sp, spq = ZERO, ZERO
    for i in range(n):
        if N[i] > 0:
            q = f32(f32(W[i]) / f32(N[i]))
            sp = f32(sp + pf[i])
            t = f32(pf[i] * q)
            spq = f32(spq + t)
    wq = f32(spq / sp) if sp > 0 else ZERO
    if S == 0:
        vmix = v
    else:
        t = f32(f32(S) * wq)
        a = f32(v + t)
        b = f32(f32(S) + ONE)
        vmix = f32(a / b)
    cq = [f32(f32(W[i]) / f32(N[i])) if N[i] > 0 else vmix for i in range(n)]
    lo = hi = cq[0]
    for c in cq[1:]:
        lo = c if c < lo else lo
        hi = c if c > hi else hi
    d = f32(hi - lo)
    d = f32(1e-8) if d < f32(1e-8) else d
    s = f32(mvi + f32(nmax))
    s = f32(s * vs)
    x = []
    for i in range(n):
        sg = f32(s * f32(f32(cq[i] - lo) / d))
        x.append(f32(logf_spec(pf[i]) + sg))
    m = x[0]
    for xi in x[1:]:
        m = xi if xi > m else m
    e = [expf_spec(f32(xi - m)) for xi in x]
    ssum = ZERO
    for t in e:
        ssum = f32(ssum + t)
    p = [f32(t / ssum) for t in e]
    den = f32(ONE + f32(S))
    sc = [f32(p[i] - f32(f32(N[i]) / den)) for i in range(n)]
    pick, bests = 0, sc[0]
    for i in range(1, n):
        if sc[i] > bests:
            pick, bests = i, sc[i]
    return p, sc, pick


class GumbelFullTwin(GumbelTwin):
    """GumbelTwin with the interior rule of DESIGN.md 3.21 below the root (interior="gumbel"; "puct": GumbelTwin unchanged).
    Every expanded node keeps the value it was expanded with in node["v"].  n_interior counts the interior selections among
    n > 1 edges, n_changed those where PUCT would have taken another edge from the same statistics, max_n the most edges such a
    selection had; cnt are the engine's work counters for the searches run so far; n_evals the evaluations."""

    def __init__(self, game, eval_kind, interior="gumbel", **kw):
        super().__init__(game, eval_kind, **kw)
        assert interior in ("puct", "gumbel")
        self.interior, self.n_interior, self.n_changed, self.n_evals, self.max_n = interior, 0, 0, 0, 0
        self.cnt = dict.fromkeys(COUNTERS, 0)

    def expand(self, node):
        v = super().expand(node)
        node["v"] = f32(v)
        self.n_evals += 1
        self.cnt["n_expanded"] += 1
        self.cnt["n_child_written"] += len(node["edges"])
        return v

    def puct_pick(self, node):
        sumN = sum(e["N"] for e in node["edges"])
        sq = np.sqrt(f32(max(sumN, 1)))
        best, bests = None, f32(-np.inf)
        for e in node["edges"]:
            q = e["W"] / f32(e["N"]) if e["N"] > 0 else f32(0.0)
            u = self.c * e["P"]
            u = u * sq
            u = u / (f32(1.0) + f32(e["N"]))
            s = q + u
            if s > bests:
                best, bests = e, s
        return best

    def interior_pick(self, node, n_in):
        es = node["edges"]
        if len(es) == 1:  # a forced pass
            return es[0]
        assert sum(e["N"] for e in es) == n_in - 1  # the identity of DESIGN.md 3.3 the kernel relies on
        _, _, i = interior_rule([e["N"] for e in es], [e["W"] for e in es], [e["P"] for e in es], node["v"], self.mvi, self.vs)
        self.n_interior += 1
        self.max_n = max(self.max_n, len(es))
        self.n_changed += es[i] is not self.puct_pick(node)
        return es[i]

    def simulate_g(self, root, k, sims):
        if self.interior == "puct":
            return super().simulate_g(root, k, sims)
        node, path = root, []
        self.cnt["n_sims"] += 1
        self.cnt["n_path_nodes"] += 1
        while True:
            if node["term"]:
                v = f32(node["tv"])
                break
            self.cnt["n_child_scored"] += len(node["edges"])
            best = self.root_pick(root, k, sims) if node is root else self.interior_pick(node, path[-1]["N"])
            path.append(best)
            self.cnt["n_path_nodes"] += 1
            if best["child"] is not None:
                node = best["child"]
                continue
            ch = self.new_node(self.play(node["b"], node["p"], best["a"]), -node["p"])
            best["child"] = ch
            self.cnt["n_env_steps"] += 1
            v = f32(ch["tv"]) if ch["term"] else self.expand(ch)
            break
        self.cnt["n_edges_backed"] += len(path)
        val = -v
        for e in reversed(path):
            e["N"] += 1
            e["W"] = f32(e["W"] + val)
            val = -val


class GfullSide(Side):
    """a match side (tests/test_match_cpu.py) that searches with GumbelFullTwin"""

    def twin(self, game):
        if game not in self._tw:
            g = self.gumbel
            self._tw[game] = GumbelFullTwin(game, self.ev, interior=g.interior, m=g.max_considered, scale=g.scale,
                                            maxvisit_init=g.maxvisit_init, value_scale=g.value_scale, eval_fn=self.eval_fn,
                                            c_puct=self.c_puct, boards=boards())
        return self._tw[game]


# ---------------------------------------------------------------- the rule for one node against the library
def lib_pick(N, W, P, v, mvi=50.0, vs=0.1):
    N, W, P = np.asarray(N, np.uint32), np.asarray(W, np.float32), np.asarray(P, np.float32)
    n = len(N)
    p, sc = np.zeros(n, np.float32), np.zeros(n, np.float32)
    i = _lib.lib().bz_gumbel_interior_pick(N.ctypes.data, W.ctypes.data, P.ctypes.data, n, C.c_float(v), C.c_float(mvi), C.c_float(vs),
                                           p.ctypes.data, sc.ctypes.data)
    return p, sc, i


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def _same(N, W, P, v, mvi=50.0, vs=0.1):
    p, sc, i = lib_pick(N, W, P, v, mvi, vs)
    tp, tsc, ti = interior_rule(list(N), list(W), list(P), v, mvi, vs)
    assert np.array_equal(_bits(p), _bits(tp)), (N, W, P, v, p, tp)
    assert np.array_equal(_bits(sc), _bits(tsc)), (N, W, P, v, sc, tsc)
    assert i == ti, (N, W, P, v, i, ti)
    return p, sc, i


def _random_node(rng, n):
    N = rng.integers(0, 801, n).astype(np.uint32)
    N[rng.random(n) < 0.4] = 0
    W = (rng.uniform(-1, 1, n) * N).astype(np.float32)
    lg = rng.normal(0, 2, n)
    P = (np.exp(lg - lg.max()) / np.exp(lg - lg.max()).sum()).astype(np.float32)
    return N, W, P, np.float32(rng.uniform(-1, 1))


def test_library_equals_the_numpy_rule_on_random_nodes():
    rng = np.random.default_rng(0)
    picks = set()
    for t in range(400):
        n = 2 + t % 33  # 2 .. 34
        N, W, P, v = _random_node(rng, n)
        mvi, vs = ((50.0, 0.1), (0.0, 1.0), (10.0, 0.5))[t % 3]
        picks.add(_same(N, W, P, v, mvi, vs)[2] > 0)
    assert picks == {False, True}


def test_hand_checked_three_edge_node():
    # N = [2, 0, 1], W = [1, 0, -0.5], P = [0.5, 0.25, 0.25], v_X = 0.2, maxvisit_init 50, value_scale 0.1:
    #   q = [0.5, -, -0.5]; sp = 0.5 + 0.25 = 0.75; spq = 0.25 - 0.125 = 0.125; wq = 1/6; S = 3
    #   vmix = (0.2 + 3/6) / 4 = 0.175; cq = [0.5, 0.175, -0.5]; lo = -0.5, hi = 0.5, d = 1; s = (50 + 2) 0.1 = 5.2
    #   sigma = 5.2 [1, 0.675, 0] = [5.2, 3.51, 0]; lp = [-0.693147, -1.386294, -1.386294]; x = [4.506853, 2.123706, -1.386294]
    #   e = exp(x - 4.506853) = [1, 0.092260, 0.002758]; sum 1.095018; p = [0.913227, 0.084254, 0.002519]
    #   den = 4; r = [0.5, 0, 0.25]; sc = [0.413227, 0.084254, -0.247481] -> edge 0
    p, sc, i = _same([2, 0, 1], [1.0, 0.0, -0.5], [0.5, 0.25, 0.25], 0.2)
    assert np.allclose(p, [0.913227, 0.084254, 0.002519], atol=2e-6) and np.allclose(sc, [0.413227, 0.084254, -0.247481], atol=2e-6)
    assert i == 0
    # N_0 = 9 with W_0 = 0 (q_0 = 0): S = 10, spq = -0.125, wq = -1/6, vmix = (0.2 - 10/6) / 11 = -0.13333; lo = -0.5, hi = 0,
    # d = 0.5; s = 5.9; sigma_1 = 5.9 (0.36667 / 0.5) = 4.3267; x = [5.2069, 2.9404, -1.3863]; p ~ [0.905, 0.094, 0.001];
    # r_0 = 9/11 = 0.818: sc_0 ~ 0.087 < sc_1 ~ 0.094 -- edge 0's visit share has caught up, the unvisited edge 1 lags the most
    p, sc, i = _same([9, 0, 1], [0.0, 0.0, -0.5], [0.5, 0.25, 0.25], 0.2)
    assert i == 1 and abs(sc[0] - 0.087) < 2e-3 and abs(sc[1] - 0.094) < 2e-3


def test_edge_cases_equal_the_rule_and_behave_as_stated():
    rng = np.random.default_rng(1)
    # n = 1: the forced pass
    p, sc, i = lib_pick([5], [1.0], [1.0], 0.3)
    assert i == 0 and p[0] == 1.0
    # all N = 0: every cq is v_X, d clamps to 1e-8, sigma is 0 everywhere: p = softmax(lp) by the sequence of DESIGN.md 3.5
    for n in (2, 9, 17, 34):
        _, _, P, v = _random_node(rng, n)
        p, sc, i = _same(np.zeros(n, np.uint32), np.zeros(n, np.float32), P, v)
        lp = [logf_spec(x if x > FLT_MIN else FLT_MIN) for x in P]
        m = max(lp)
        e = [expf_spec(f32(x - m)) for x in lp]
        s = ZERO
        for t in e:
            s = f32(s + t)
        assert np.array_equal(_bits(p), _bits([f32(t / s) for t in e])) and np.array_equal(_bits(sc), _bits(p))
        assert i == int(np.argmax(p))
    # one visited child
    for n in (2, 16, 17, 33):
        N, W, P, v = _random_node(rng, n)
        k = int(rng.integers(n))
        N[:] = 0
        W[:] = 0
        N[k], W[k] = 3, -1.5
        _same(N, W, P, v)
    # all q equal (d clamps): sigma is 0 again
    N, W, P, v = _random_node(rng, 20)
    N[:] = 4
    W[:] = 2.0
    p, _, _ = _same(N, W, P, v)
    p0, _, _ = _same(np.zeros(20, np.uint32), np.zeros(20, np.float32), P, v)
    assert np.array_equal(_bits(p), _bits(p0))
    # a prior at FLT_MIN, one below it (floored) and a zero
    N, W, P, v = _random_node(rng, 12)
    P[3], P[4], P[7] = FLT_MIN, np.float32(1e-40), 0.0
    N[3], N[4], N[7] = 2, 0, 1
    W[3], W[4], W[7] = 1.0, 0.0, -1.0
    _same(N, W, P, v)
    # sigma's scale at its extremes
    _same(*_random_node(rng, 34), mvi=0.0, vs=0.0)
    _same(*_random_node(rng, 34), mvi=800.0, vs=1.0)


def test_library_refuses_bad_arguments():
    L = _lib.lib()
    a = np.zeros(4, np.float32)
    n = np.zeros(4, np.uint32)
    for args in ((None, a.ctypes.data, a.ctypes.data, 4), (n.ctypes.data, None, a.ctypes.data, 4), (n.ctypes.data, a.ctypes.data, a.ctypes.data, 0),
                 (n.ctypes.data, a.ctypes.data, a.ctypes.data, 65)):
        assert L.bz_gumbel_interior_pick(*args, C.c_float(0.0), C.c_float(50.0), C.c_float(0.1), None, None) == -1
        assert b"bz_gumbel_interior_pick" in L.bz_last_error()
    assert L.bz_gumbel_interior_pick(n.ctypes.data, a.ctypes.data, a.ctypes.data, 4, C.c_float(0.0), C.c_float(50.0), C.c_float(0.1), None, None) == 0


# ---------------------------------------------------------------- the twin
GAMES = ["ttt", "reversi", "reversi6", "reversi4"]


@pytest.mark.parametrize("game", GAMES)
@pytest.mark.parametrize("ev", ["hash", "uniform"])
def test_twin_invariants(game, ev):
    for m in (1, 4, 16):
        for sims in (8, 32):
            for (b, p, _, _) in game_roots(game, 2, seed=sims + m):
                tw = GumbelFullTwin(game, ev, m=m, boards=boards())
                root = tw.search(b, p, sims, True, (3, 5, 0))
                es = root["edges"]
                assert sum(e["N"] for e in es) == sims

                def count(node):
                    return 1 + sum(count(e["child"]) for e in (node["edges"] or []) if e["child"] is not None)
                assert count(root) <= sims + 1
                pi, pick = tw.decide(root)
                # n divisions by the same sum, each within half an ulp of its quotient, and the float32 sum of the results
                assert abs(float(np.sum(np.asarray(pi, np.float64))) - 1.0) <= len(es) * 2.0 ** -24
                assert pick["N"] == max(e["N"] for e in es)
                assert tw.cnt["n_sims"] == sims and tw.cnt["n_expanded"] == tw.n_evals


def _nwp(root):
    return [(e["N"], _bits(e["W"]).item(), _bits(e["P"]).item()) for e in root["edges"]]


VISIBLE_ROOTS = [(game, seed) for game in GAMES for seed in (7,)]


def test_the_rule_chooses_other_edges_than_puct_and_changes_root_statistics():
    changed, interior, differ = 0, 0, 0
    for game, seed in VISIBLE_ROOTS:
        for (b, p, _, _) in game_roots(game, 2, seed=seed):
            tw = GumbelFullTwin(game, "hash", m=16, boards=boards())
            root = tw.search(b, p, 32)
            changed, interior = changed + tw.n_changed, interior + tw.n_interior
            differ += _nwp(root) != _nwp(GumbelTwin(game, "hash", m=16, boards=boards()).search(b, p, 32))
    assert interior > 0 and changed > 0 and differ > 0, (interior, changed, differ)


@pytest.mark.parametrize("game", GAMES)
def test_interior_puct_is_the_gumbel_twin_bit_for_bit(game):
    for (b, p, _, _) in game_roots(game, 2, seed=3):
        for noise in (False, True):
            a = GumbelFullTwin(game, "hash", interior="puct", m=4, boards=boards())
            ra = a.search(b, p, 32, noise, (1, 2, 0))
            g = GumbelTwin(game, "hash", m=4, boards=boards())
            rg = g.search(b, p, 32, noise, (1, 2, 0))
            assert _nwp(ra) == _nwp(rg) and a.n_interior == 0
            assert np.array_equal(_bits(a.policy(ra)[0]), _bits(g.policy(rg)[0])) and a.policy(ra)[1] == g.policy(rg)[1]
    a = GumbelFullTwin(game, "hash", interior="puct", m=4, boards=boards()).selfplay(5, 16, 4, 1, 11, slot=3, stagger=3)
    g = GumbelTwin(game, "hash", m=4, boards=boards()).selfplay(5, 16, 4, 1, 11, slot=3, stagger=3)
    assert a[1:] == g[1:] and [r[:2] + r[3:] for r in a[0]] == [r[:2] + r[3:] for r in g[0]]
    assert np.array_equal(_bits([r[2] for r in a[0]]), _bits([r[2] for r in g[0]]))


# ---------------------------------------------------------------- buffer size and refusals
def test_interior_bytes_is_the_stated_layout():
    L = _lib.lib()
    rnd = lambda x: (x + 255) // 256 * 256  # noqa: E731
    for game in (0, 1, 2, 3):
        for B in (1, 4, 33, 4096):
            for sims in (1, 7, 800, 8189):
                assert L.bz_engine_gumbel_interior_bytes(C.byref(_cfg(game, B, sims))) == rnd(B * (sims + 2) * 4), (game, B, sims)
    assert L.bz_engine_gumbel_interior_bytes(C.byref(_cfg(1, 4, 8, flags=_lib.ENGINE_EVAL_CACHE | _lib.ENGINE_EVAL_CACHE_CARRY))) == 256


def test_interior_bytes_refuses_the_refused_combinations_with_a_message():
    L = _lib.lib()
    for cfg, word in ((_cfg(flags=_lib.ENGINE_REUSE_SUBTREE), b"subtree reuse"), (_cfg(K=2), b"leaves_per_step"),
                      (_cfg(eps=0.25), b"Dirichlet"), (_cfg(sims=0), b"")):
        assert L.bz_engine_gumbel_interior_bytes(C.byref(cfg)) == -1
        assert b"bz_engine_gumbel_interior_bytes" in L.bz_last_error() and word in L.bz_last_error(), L.bz_last_error()
    assert L.bz_engine_gumbel_interior_bytes(None) == -1


# ---------------------------------------------------------------- Python validation (no GPU needed)
@pytest.mark.parametrize("bad", ["PUCT", "", "full", None, 1, True, b"gumbel"])
def test_python_refuses_a_bad_interior_before_touching_a_device(bad, monkeypatch):
    from betazero_amd.arena import play_arena
    from betazero_amd.engine import GumbelConfig, PipelinedSelfPlay, SelfPlayEngine, check_gumbel, self_play
    from betazero_amd.match import MatchPlayer, play_match
    from betazero_amd.players import MCTSPlayer

    def no_device(*a, **k):
        raise AssertionError("touched a device")
    monkeypatch.setattr(_lib, "require_gpu", no_device)
    monkeypatch.setattr(_lib, "lib", no_device)
    g = GumbelConfig(interior=bad)
    with pytest.raises(ValueError, match="interior"):
        check_gumbel(g)
    with pytest.raises(ValueError, match="interior"):
        SelfPlayEngine("reversi", 4, 16, "uniform", gumbel=g)
    with pytest.raises(ValueError, match="interior"):
        MCTSPlayer(1, 16, gumbel=g)
    with pytest.raises(ValueError, match="interior"):
        PipelinedSelfPlay("reversi", 4, 16, "uniform", gumbel=g, streams=[None])
    with pytest.raises(ValueError, match="interior"):
        self_play("ttt", 4, 16, gumbel=g)
    with pytest.raises(ValueError, match="interior"):
        play_arena("ttt", 4, 16, gumbel=g)
    with pytest.raises(ValueError, match="interior"):
        play_match("reversi", 4, MatchPlayer(sims=8, evaluator="hash", gumbel=g), MatchPlayer(sims=8, evaluator="hash"))


def test_python_accepts_the_two_interiors_and_keeps_the_default():
    from betazero_amd.engine import GumbelConfig, check_gumbel
    assert GumbelConfig().interior == "puct" and check_gumbel(True) == GumbelConfig(16, 1.0, 50.0, 0.1, "puct")
    assert check_gumbel(GumbelConfig(4, interior="gumbel")) == GumbelConfig(4, 1.0, 50.0, 0.1, "gumbel")
    # everything Gumbel root search refuses stays refused with the interior rule
    for kw in (dict(reuse_subtree=True), dict(leaves_per_step=2), dict(dirichlet_eps=0.25)):
        with pytest.raises(ValueError):
            check_gumbel(GumbelConfig(interior="gumbel"), **kw)


def test_python_refuses_what_refuses_gumbel_with_the_interior_rule_too():
    from betazero_amd.engine import ForcedPlayouts, Fpu, GumbelConfig, PlayoutCap, check_forced_playouts, check_fpu, check_playout_cap
    g = GumbelConfig(interior="gumbel")
    with pytest.raises(ValueError, match="Gumbel"):
        check_playout_cap(PlayoutCap(4, 0.25), 16, gumbel=g)
    with pytest.raises(ValueError, match="Gumbel"):
        check_forced_playouts(ForcedPlayouts(2.0), gumbel=g)
    with pytest.raises(ValueError, match="Gumbel"):
        check_fpu(Fpu(), gumbel=g)


def test_az_loop_refuses_gumbel_interior_without_gumbel():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "az_loop.py"), "--gumbel-interior", "--iters", "1"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and "--gumbel-interior" in out.stderr and "--gumbel" in out.stderr, out.stderr[-500:]
