"""Gumbel root search without a GPU: the Gumbel twin -- root rule, completed Q, sigma, the move and the
improved policy exactly as the spec states them, built on oracle.py_twin.Twin -- its invariants, the considered-visit table
against a restatement of mctx's sequence, and the ABI / Python validation.  tests/test_gpu_gumbel.py pins the engine to
this twin."""
import ctypes as C
import math

import numpy as np
import pytest

from betazero_amd import _lib
from oracle.py_twin import Twin, expf_spec, f32, logf_spec, rng_noise, u01_spec
from test_leaf_parallel_cpu import KTwin, boards

FLT_MIN = f32(2.0 ** -126)
ZERO, ONE = f32(0.0), f32(1.0)


def mctx_considered_visits(n_considered, sims):
    """mctx's get_sequence_of_considered_visits (seq_halving.py), restated"""
    if n_considered <= 1:
        return list(range(sims))
    log2max = int(math.ceil(math.log2(n_considered)))
    seq, visits, num = [], [0] * n_considered, n_considered
    while len(seq) < sims:
        extra = max(1, int(sims / (log2max * num)))
        for _ in range(extra):
            seq.extend(visits[:num])
            for i in range(num):
                visits[i] += 1
        num = max(2, num // 2)
    return seq[:sims]


_T = {}


def considered(n_considered, sims):
    key = (n_considered, sims)
    if key not in _T:
        _T[key] = mctx_considered_visits(n_considered, sims)
    return _T[key]


class GumbelTwin(Twin):
    """Twin with Gumbel root search: the root's edge by the considered-visit rule, PUCT below, the move and
    pi' from the final statistics.  eval_fn(own, opp) -> (logits [NA] f32, value f32) replaces the synthetic evaluators.
    `trace` records (k, T[n_c][k], N of the edge taken) for every root visit of the last search."""

    def __init__(self, game, eval_kind, m=16, scale=1.0, maxvisit_init=50.0, value_scale=0.1, eval_fn=None, **kw):
        super().__init__(game, eval_kind, **kw)
        self.m, self.scale, self.mvi, self.vs = m, f32(scale), f32(maxvisit_init), f32(value_scale)
        self.eval_fn, self.trace = eval_fn, []

    start = KTwin.start  # (openings, then the bench's stagger plies)

    def evaluate(self, b, p):
        if self.eval_fn is None:
            return super().evaluate(b, p)
        return self.eval_fn(*self.bits(b, p))

    # ---- per search, after the root's expansion
    def prepare(self, root, v_root, noise, key):
        seed, gid, ply = key
        root["v_root"] = f32(v_root)
        for i, e in enumerate(root["edges"]):
            e["lp"] = logf_spec(e["P"] if e["P"] > FLT_MIN else FLT_MIN)
            g = ZERO
            if noise:
                u = u01_spec(rng_noise(seed ^ 0x6A09E667F3BCC908, gid, ply, i))
                y = logf_spec(u)
                y = -y
                y = logf_spec(y)
                g = f32(self.scale * f32(-y))
            e["base"] = f32(g + e["lp"])

    # ---- completed Q and sigma from the root's current statistics
    def sigma(self, root):
        es = root["edges"]
        S, nmax = sum(e["N"] for e in es), max(e["N"] for e in es)
        sp, spq = ZERO, ZERO
        for e in es:
            if e["N"] > 0:
                q = f32(e["W"] / f32(e["N"]))
                pf = e["P"] if e["P"] > FLT_MIN else FLT_MIN
                sp = f32(sp + pf)
                t = f32(pf * q)
                spq = f32(spq + t)
        wq = f32(spq / sp) if sp > 0 else ZERO
        if S == 0:
            vmix = root["v_root"]
        else:
            t = f32(f32(S) * wq)
            a = f32(root["v_root"] + t)
            b = f32(f32(S) + ONE)
            vmix = f32(a / b)
        cq = [f32(e["W"] / f32(e["N"])) if e["N"] > 0 else vmix for e in es]
        lo = hi = cq[0]
        for c in cq[1:]:
            lo = c if c < lo else lo
            hi = c if c > hi else hi
        d = f32(hi - lo)
        d = f32(1e-8) if d < f32(1e-8) else d
        s = f32(self.mvi + f32(nmax))
        s = f32(s * self.vs)
        return [f32(s * f32(f32(c - lo) / d)) for c in cq], nmax

    def root_pick(self, root, k, sims):
        es = root["edges"]
        cv = considered(min(self.m, len(es)), sims)[k]
        sig, _ = self.sigma(root)
        best, bests = None, None
        for e, sg in zip(es, sig):
            if e["N"] != cv:
                continue
            sc = f32(e["base"] + sg)
            if best is None or sc > bests:
                best, bests = e, sc
        assert best is not None, (k, cv, [e["N"] for e in es])
        self.trace.append((k, cv, best["N"]))
        return best

    def simulate_g(self, root, k, sims):
        node, path = root, []
        while True:
            if node["term"]:
                v = f32(node["tv"])
                break
            if node is root:
                best = self.root_pick(root, k, sims)
            else:
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

    def search(self, b, p, sims, noise=False, key=(0, 0, 0)):
        root = self.new_node(b, p)
        assert not root["term"]
        v = self.expand(root)
        self.prepare(root, v, noise, key)
        self.trace = []
        for k in range(sims):
            self.simulate_g(root, k, sims)
        return root

    def decide(self, root):
        """(pi' over the root's edges in edge order, the played edge)"""
        es = root["edges"]
        sig, nmax = self.sigma(root)
        x = [f32(e["lp"] + sg) for e, sg in zip(es, sig)]
        m = x[0]
        for xi in x[1:]:
            m = xi if xi > m else m
        ex = [expf_spec(f32(xi - m)) for xi in x]
        s = ZERO
        for t in ex:
            s = f32(s + t)
        pi = [f32(t / s) for t in ex]
        pick, bests = None, None
        for e, sg in zip(es, sig):
            if e["N"] == nmax:
                sc = f32(e["base"] + sg)
                if pick is None or sc > bests:
                    pick, bests = e, sc
        return pi, pick

    def policy(self, root):
        """pi' at the actions (0 elsewhere) and the move's action: what bz_engine_root_policy returns"""
        pi_e, pick = self.decide(root)
        pi = np.zeros(self.na, np.float32)
        for e, x in zip(root["edges"], pi_e):
            pi[e["a"]] = x
        return pi, pick["a"]

    def selfplay(self, gid, sims, temp_moves, openings, seed, slot=0, stagger=0):
        b, p, made = self.start(slot, gid, openings, seed, stagger)
        ex, passes = [], 0
        while True:
            root = self.search(b, p, sims, made < temp_moves and self.scale > 0, (seed, gid, made))
            pi, a = self.policy(root)
            own, opp = self.bits(b, p)
            ex.append((own, opp, list(pi), p, a))
            b = self.play(b, p, a)
            p, made = -p, made + 1
            over, w = self.terminal(b)
            if over:
                return ex, w, passes
            if not self.moves(b, p):
                p, passes = -p, passes + 1


def game_roots(game, n_roots, seed):
    """a few positions along a pseudo-random game: (board object, mover, own, opp)"""
    tw = Twin(game, "uniform", boards=boards())
    rng = np.random.default_rng(seed)
    b = tw.TicTacToeBoard() if tw.game == "ttt" else tw.ReversiBoard(size=tw.size)
    p, out = 1, []
    while len(out) < n_roots and not tw.terminal(b)[0]:
        mv = tw.moves(b, p)
        if not mv:
            p = -p
            continue
        own, opp = tw.bits(b, p)
        out.append((b, p, own, opp))
        for _ in range(3 if game != "ttt" else 1):  # (a few plies apart)
            if tw.terminal(b)[0]:
                break
            mv = tw.moves(b, p)
            if not mv:
                p = -p
                continue
            b, p = tw.play(b, p, mv[int(rng.integers(len(mv)))]), -p
    return out


# ---------------------------------------------------------------- the considered-visit table
def _lib_T(nc, sims):
    out = (C.c_uint16 * sims)()
    assert _lib.lib().bz_gumbel_considered_visits(nc, sims, out) == _lib.BZ_OK
    return list(out)


HAND_ROWS = {(4, 8): [0, 0, 0, 0, 1, 1, 2, 2], (3, 7): [0, 0, 0, 1, 1, 2, 2], (2, 5): [0, 0, 1, 1, 2], (1, 4): [0, 1, 2, 3],
             (9, 20): [0] * 9 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5], (16, 32): [0] * 16 + [1] * 8 + [2, 2, 2, 2, 3, 3, 3, 3]}


def test_considered_visits_hand_checked_rows():
    for (nc, sims), row in HAND_ROWS.items():
        assert mctx_considered_visits(nc, sims) == row, (nc, sims)
        assert _lib_T(nc, sims) == row, (nc, sims)


def test_considered_visits_equal_mctx_sequence():
    rng = np.random.default_rng(0)
    sims_list = sorted(set([1, 2, 3, 7, 16, 32, 100, 200, 300] + [int(x) for x in rng.integers(1, 301, 24)]))
    for nc in range(1, 65):
        for sims in sims_list:
            assert _lib_T(nc, sims) == mctx_considered_visits(nc, sims), (nc, sims)
    for nc in (1, 2, 3, 4, 5, 16, 33, 64):
        for sims in (800, 8189):
            assert _lib_T(nc, sims) == mctx_considered_visits(nc, sims), (nc, sims)


def test_considered_visits_refuses_bad_arguments():
    L = _lib.lib()
    out = (C.c_uint16 * 16)()
    for nc, sims in ((0, 4), (65, 4), (4, 0), (4, 8190)):
        assert L.bz_gumbel_considered_visits(nc, sims, out) == _lib.BZ_EINVAL
        assert b"n_considered" in L.bz_last_error()


# ---------------------------------------------------------------- buffer size and refusals
def _cfg(game=1, B=4, sims=8, flags=0, K=1, eps=0.0):
    return _lib.EngineCfg(game, B, sims, 0, 1.5, 0, 0, 1, 64, 0, 0, 0, B, flags | ((K - 1) << _lib.ENGINE_LEAVES_SHIFT),
                          0.3 if eps > 0 else 0.0, eps, 0)


def test_gumbel_bytes_is_the_stated_layout():
    L = _lib.lib()
    rnd = lambda x: (x + 255) // 256 * 256  # noqa: E731
    for game, maxch in ((0, 9), (1, 34), (2, 34), (3, 34)):
        for B in (1, 4, 33, 4096):
            for sims in (1, 7, 800, 8189):
                for m in (1, 2, 16, 64):
                    got = L.bz_engine_gumbel_bytes(C.byref(_cfg(game, B, sims)), m)
                    assert got == rnd(m * sims * 2) + rnd(B * maxch * 4) + rnd(B * 4), (game, B, sims, m)
    # the evaluation cache is allowed
    assert L.bz_engine_gumbel_bytes(C.byref(_cfg(1, 4, 8, flags=_lib.ENGINE_EVAL_CACHE | _lib.ENGINE_EVAL_CACHE_CARRY)), 16) > 0


def test_gumbel_bytes_refuses_bad_m_and_the_refused_combinations_with_a_message():
    L = _lib.lib()
    for m in (0, -1, 65, 1000):
        assert L.bz_engine_gumbel_bytes(C.byref(_cfg()), m) == -1
        assert b"max_considered" in L.bz_last_error()
    for cfg, word in ((_cfg(flags=_lib.ENGINE_REUSE_SUBTREE), b"subtree reuse"), (_cfg(K=2), b"leaves_per_step"),
                      (_cfg(K=32), b"leaves_per_step"), (_cfg(eps=0.25), b"Dirichlet")):
        assert L.bz_engine_gumbel_bytes(C.byref(cfg), 16) == -1
        assert word in L.bz_last_error(), L.bz_last_error()
    assert L.bz_engine_gumbel_bytes(None, 16) == -1


# ---------------------------------------------------------------- the twin
GAMES = ["ttt", "reversi", "reversi6", "reversi4"]


@pytest.mark.parametrize("game", GAMES)
@pytest.mark.parametrize("ev", ["uniform", "hash"])
@pytest.mark.parametrize("m", [1, 2, 4, 16])
def test_twin_invariants(game, ev, m):
    for sims in (1, 7, 32, 200):
        for noise in (False, True):
            for (b, p, _, _) in game_roots(game, 2, seed=sims + m):
                tw = GumbelTwin(game, ev, m=m, boards=boards())
                root = tw.search(b, p, sims, noise, (3, 5, 0))
                es = root["edges"]
                assert sum(e["N"] for e in es) == sims
                T = considered(min(m, len(es)), sims)
                assert [t[0] for t in tw.trace] == list(range(sims))
                assert all(cv == T[k] and n == cv for k, cv, n in tw.trace)
                pi, pick = tw.decide(root)
                assert abs(float(np.sum(np.asarray(pi, np.float64))) - 1.0) <= 1e-6
                assert pick["N"] == max(e["N"] for e in es)
                assert all(x >= 0 for x in pi)


@pytest.mark.parametrize("game", GAMES)
def test_twin_m1_without_noise_spends_every_visit_on_the_highest_prior(game):
    for ev in ("uniform", "hash"):
        for (b, p, _, _) in game_roots(game, 3, seed=1):
            tw = GumbelTwin(game, ev, m=1, scale=0.0, boards=boards())
            root = tw.search(b, p, 32, True, (1, 2, 0))  # (scale 0: no noise even when asked)
            es = root["edges"]
            top = max(range(len(es)), key=lambda i: (es[i]["P"], -i))
            assert [e["N"] for e in es] == [32 if i == top else 0 for i in range(len(es))]
            assert tw.decide(root)[1] is es[top]


def test_twin_noise_changes_base_and_only_base():
    b, p, _, _ = game_roots("reversi", 1, seed=0)[0]
    a = GumbelTwin("reversi", "hash", boards=boards()).search(b, p, 1, False)
    n = GumbelTwin("reversi", "hash", boards=boards()).search(b, p, 1, True, (7, 3, 0))
    assert all(x["lp"] == y["lp"] and x["P"] == y["P"] for x, y in zip(a["edges"], n["edges"]))
    assert all(x["base"] == x["lp"] for x in a["edges"])
    assert any(x["base"] != y["base"] for x, y in zip(a["edges"], n["edges"]))


@pytest.mark.parametrize("game", GAMES)
def test_twin_selfplay_rows(game):
    tw = GumbelTwin(game, "hash", m=4, boards=boards())
    rows, w, _ = tw.selfplay(5, 16, 4, 1, 11, slot=3, stagger=3)
    assert w in (-1, 0, 1) and rows
    for own, opp, pi, mover, a in rows:
        assert abs(sum(float(x) for x in pi) - 1.0) <= 1e-6 and pi[a] > 0


def ttt_arena_never_loses(sims, m=16):
    """the Gumbel twin (uniform evaluator, no noise) against every optimal reply of a perfect tic-tac-toe player, with
    either colour: True iff no line of play loses for the twin"""
    import betazero_amd as bz
    memo = {}

    def score(b, to_move):  # perfect play value for `to_move`
        key = (b.bits(1), b.bits(-1), to_move)
        if key not in memo:
            over, w = b.is_game_over()
            if over:
                memo[key] = w * to_move
            else:
                memo[key] = max(-score(b.make_move(r, c, to_move), -to_move) for r, c in b.generate_possible_moves())
        return memo[key]

    tw = GumbelTwin("ttt", "uniform", m=m, boards=boards())

    def play(b, to_move, mcts):
        over, w = b.is_game_over()
        if over:
            return w * mcts >= 0
        if to_move == mcts:
            _, a = tw.policy(tw.search(b, to_move, sims))
            return play(b.make_move(a // 3, a % 3, to_move), -to_move, mcts)
        best = max(-score(b.make_move(r, c, to_move), -to_move) for r, c in b.generate_possible_moves())
        return all(play(b.make_move(r, c, to_move), -to_move, mcts) for r, c in b.generate_possible_moves()
                   if -score(b.make_move(r, c, to_move), -to_move) == best)
    return play(bz.TicTacToeBoard(), 1, 1) and play(bz.TicTacToeBoard(), 1, -1)


# the smallest count found that holds (m = 16): 200, 400, 800 and 1600 each lose a line; tests/test_gpu_gumbel.py pins the
# engine's arena at this count
ARENA_SIMS = 3200


def test_twin_never_loses_at_tictactoe_at_the_pinned_sims():
    assert ttt_arena_never_loses(ARENA_SIMS)


# ---------------------------------------------------------------- Python validation (no GPU needed)
@pytest.mark.parametrize("bad", [0, 65, 2.0, True, -1, "4", None])
def test_python_refuses_bad_max_considered_before_touching_a_device(bad, monkeypatch):
    from betazero_amd.arena import play_arena
    from betazero_amd.engine import GumbelConfig, PipelinedSelfPlay, SelfPlayEngine, check_gumbel, self_play
    from betazero_amd.players import MCTSPlayer

    def no_device(*a, **k):
        raise AssertionError("touched a device")
    monkeypatch.setattr(_lib, "require_gpu", no_device)
    monkeypatch.setattr(_lib, "lib", no_device)
    g = GumbelConfig(max_considered=bad)
    with pytest.raises(ValueError, match="max_considered"):
        check_gumbel(g)
    with pytest.raises(ValueError, match="max_considered"):
        SelfPlayEngine("reversi", 4, 16, "uniform", gumbel=g)
    with pytest.raises(ValueError, match="max_considered"):
        MCTSPlayer(1, 16, gumbel=g)
    with pytest.raises(ValueError, match="max_considered"):
        PipelinedSelfPlay("reversi", 4, 16, "uniform", gumbel=g, streams=[None])
    with pytest.raises(ValueError, match="max_considered"):
        self_play("ttt", 4, 16, gumbel=g)
    with pytest.raises(ValueError, match="max_considered"):
        play_arena("ttt", 4, 16, gumbel=g)


def test_python_refuses_bad_floats_and_combinations_before_touching_a_device(monkeypatch):
    from betazero_amd.engine import GumbelConfig, PipelinedSelfPlay, SelfPlayEngine, check_gumbel, self_play
    from betazero_amd.players import MCTSPlayer

    def no_device(*a, **k):
        raise AssertionError("touched a device")
    monkeypatch.setattr(_lib, "require_gpu", no_device)
    monkeypatch.setattr(_lib, "lib", no_device)
    for name in ("scale", "maxvisit_init", "value_scale"):
        for bad in (-0.5, float("nan"), float("inf"), True, "1"):
            with pytest.raises(ValueError, match=name):
                check_gumbel(GumbelConfig(**{name: bad}))
            with pytest.raises(ValueError, match=name):
                SelfPlayEngine("ttt", 4, 16, "uniform", gumbel=GumbelConfig(**{name: bad}))
    for bad in ("yes", 1, 16, {"max_considered": 4}):
        with pytest.raises(ValueError, match="gumbel"):
            check_gumbel(bad)
    for kw, word in (({"reuse_subtree": True}, "reuse"), ({"leaves_per_step": 2}, "leaves_per_step"),
                     ({"dirichlet_alpha": 0.3, "dirichlet_eps": 0.25}, "Dirichlet")):
        with pytest.raises(ValueError, match=word):
            SelfPlayEngine("reversi", 4, 16, "uniform", gumbel=True, **kw)
        with pytest.raises(ValueError, match=word):
            PipelinedSelfPlay("reversi", 4, 16, "uniform", gumbel=True, streams=[None], **kw)
        with pytest.raises(ValueError, match=word):
            self_play("reversi", 4, 16, gumbel=True, **kw)
    with pytest.raises(ValueError, match="leaves_per_step"):
        MCTSPlayer(1, 16, gumbel=True, leaves_per_step=4)


def test_python_accepts_off_true_and_a_config():
    from betazero_amd.engine import GumbelConfig, check_gumbel
    assert check_gumbel(None) is None and check_gumbel(False) is None
    assert check_gumbel(True) == GumbelConfig(16, 1.0, 50.0, 0.1)
    assert check_gumbel(GumbelConfig(np.int64(4), 0, 10, 1)) == GumbelConfig(4, 0.0, 10.0, 1.0)
