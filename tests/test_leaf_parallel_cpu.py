"""Leaf-parallel MCTS without a GPU: the K-walk twin -- virtual loss, the collision rule and the
sum-of-visits definition exactly as the spec states them, built on oracle.py_twin.Twin -- its invariants, and the
ABI / Python validation of leaves_per_step.  tests/test_gpu_leaf_parallel.py pins the engine to this twin."""
import ctypes as C

import numpy as np
import pytest

from betazero_amd import _lib
from oracle.py_twin import Twin, f32, rng_draw

ONE = f32(1.0)


class KTwin(Twin):
    """Twin with `leaves` = K walks per step.  K = 1 is Twin itself (its simulate(), no virtual loss).
    eval_fn(own, opp) -> (logits [NA] f32, value f32) replaces the synthetic evaluators (a net's per-position forward).
    Every edge keeps the list of values its backups added ("bk"), and n_collisions counts the walks that collided."""

    def __init__(self, game, eval_kind, leaves=1, eval_fn=None, **kw):
        super().__init__(game, eval_kind, **kw)
        self.K, self.eval_fn, self.n_collisions = leaves, eval_fn, 0

    def evaluate(self, b, p):
        if self.eval_fn is None:
            return super().evaluate(b, p)
        return self.eval_fn(*self.bits(b, p))

    def expand(self, node):
        v = super().expand(node)
        node["v"] = v  # what a collision with this node backs up
        for e in node["edges"]:
            e["bk"] = []
        return v

    def _walk(self, root, root_sum):
        """one walk with the PUCT rule on the current statistics (pending visits included); leaves its virtual loss"""
        node, path, sumN = root, [], root_sum
        while True:
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
            ch = best["child"]
            if ch is None:
                ch = self.new_node(self.play(node["b"], node["p"], best["a"]), -node["p"])
                best["child"] = ch
                kind = "term" if ch["term"] else "eval"
                break
            if ch["term"]:
                kind = "term"
                break
            if ch["edges"] is None:  # created by an earlier walk of this step, not expanded yet
                kind = "collide"
                self.n_collisions += 1
                break
            sumN = best["N"] - 1  # N(edge into X) - 1, pending visits included
            node = ch
        for e in path:
            e["N"] += 1
            e["W"] = f32(e["W"] - ONE)
        return kind, ch, path

    def run(self, root, sims, base=0):
        """sims simulations from an expanded root; base = root_base (subtree reuse: N of the edge into the kept root - 1)"""
        if self.K == 1:
            for _ in range(sims):
                self._sim1(root)
            return
        done = 0
        while done < sims:
            kp = min(self.K, sims - done)
            walks = [self._walk(root, done + j + base) for j in range(kp)]
            for kind, node, _ in walks:  # expand the new leaves in ascending j
                if kind == "eval":
                    self.expand(node)
            for kind, node, path in walks:  # then back up the paths in ascending j
                v = f32(node["tv"]) if kind == "term" else node["v"]
                val = -v
                for e in reversed(path):
                    e["W"] = f32(f32(e["W"] + ONE) + val)
                    e.setdefault("bk", []).append(float(val))
                    val = -val
            done += kp

    def _sim1(self, root):
        """Twin.simulate with the backed-up values recorded (same arithmetic)"""
        node, path = root, []
        while True:
            if node["term"]:
                v = f32(node["tv"])
                break
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
            e.setdefault("bk", []).append(float(val))
            val = -val

    def search(self, b, p, sims):
        root = self.new_node(b, p)
        assert not root["term"]
        self.expand(root)
        self.root_noise(root)
        self.run(root, sims)
        return root

    def start(self, slot, gid, openings, seed, stagger):
        """the start position of a self-play game: openings (gid % 12), then the bench's stagger plies (slot % stagger)"""
        b = self.TicTacToeBoard() if self.game == "ttt" else self.ReversiBoard(size=self.size)
        p, made = 1, 0
        if self.game == "reversi" and openings and self.size == 8:
            k = gid % 12
            for pick in (k // 3, k % 3):
                b = self.play(b, p, self.moves(b, p)[pick])
                p, made = -p, made + 1
        if stagger > 0:
            b2, p2, m2, ok = b, p, made, True
            for k in range(slot % stagger):
                if self.terminal(b2)[0]:
                    ok = False
                    break
                mv = self.moves(b2, p2)
                if not mv:
                    p2 = -p2
                    continue
                a = mv[rng_draw(seed ^ 0x5AFEC0DE, slot, k) % len(mv)]
                b2, p2, m2 = self.play(b2, p2, a), -p2, m2 + 1
            if ok and not self.terminal(b2)[0]:
                if not self.moves(b2, p2):
                    p2 = -p2
                b, p, made = b2, p2, m2
        return b, p, made

    def selfplay(self, gid, sims, temp_moves, openings, seed, slot=0, stagger=0, on_search=None):
        """Twin.selfplay with K walks per step (and the stagger of the bench); on_search(root, base) after every search"""
        b, p, made = self.start(slot, gid, openings, seed, stagger)
        ex, passes = [], 0
        kept, kept_base = None, 0
        while True:
            self.noise_key = (seed, gid, made)
            if kept is not None:
                root, base = kept, kept_base
                self.root_noise(root)
                self.run(root, sims, base)
            else:
                root, base = self.search(b, p, sims), 0
            if on_search is not None:
                on_search(root, base)
            sumN = sum(e["N"] for e in root["edges"])
            pi = [f32(0.0)] * self.na
            for e in root["edges"]:
                pi[e["a"]] = f32(e["N"]) / f32(sumN)
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
            own, opp = self.bits(b, p)
            ex.append((own, opp, pi, p, pick["a"]))
            b = self.play(b, p, pick["a"])
            p, made = -p, made + 1
            over, w = self.terminal(b)
            if over:
                return ex, w, passes
            keep_node, keep_N = pick["child"], pick["N"]
            if not self.moves(b, p):
                p, passes = -p, passes + 1
                if keep_node is not None:
                    pe = keep_node["edges"][0]
                    keep_node, keep_N = pe["child"], pe["N"]
            ok = self.reuse and keep_node is not None and keep_N + sims + 2 <= 4 * (sims + 2)
            kept, kept_base = (keep_node, keep_N - 1) if ok else (None, 0)


def boards():
    import betazero_amd as bz
    return (bz.ReversiBoard, bz.TicTacToeBoard)


def _edges(root):
    out, stack = [], [root]
    while stack:
        n = stack.pop()
        for e in n["edges"] or []:
            out.append(e)
            if e["child"] is not None:
                stack.append(e["child"])
    return out


def _nodes(root):
    n, stack = 0, [root]
    while stack:
        x = stack.pop()
        n += 1
        stack.extend(e["child"] for e in x["edges"] or [] if e["child"] is not None)
    return n


def check_invariants(root, sims, base, root_sum0):
    """after a K > 1 search: the root's visits add up to sims + what it had, no virtual loss is left in any W (W is the
    fp64 sum of its backups within fp32 rounding; N is their number), the tree grew by at most one node per walk"""
    assert sum(e["N"] for e in root["edges"]) == sims + root_sum0
    for e in _edges(root):
        bk = e.get("bk", [])
        assert e["N"] == len(bk), (e["N"], len(bk))
        ref = float(np.sum(np.asarray(bk, np.float64)))
        tol = 4.0 * (len(bk) + 1) * (len(bk) + 2) * 2.0 ** -24
        assert abs(float(e["W"]) - ref) <= tol, (float(e["W"]), ref)
    return True


# ---------------------------------------------------------------- the twin
def _root_board(tw, game):
    import betazero_amd as bz
    if game == "ttt":
        return bz.TicTacToeBoard(), 1
    return bz.ReversiBoard(size=tw.size), 1


def _dump(root):
    return [(e["a"], e["N"], float(e["W"]).hex(), float(e["P"]).hex()) for e in root["edges"]]


GAMES = ["ttt", "reversi", "reversi6", "reversi4"]


@pytest.mark.parametrize("game", GAMES)
@pytest.mark.parametrize("ev", ["uniform", "hash"])
def test_k1_twin_is_the_twin_bit_for_bit(game, ev):
    sims = 60 if game == "ttt" else 40
    a, b = Twin(game, ev, boards=boards()), KTwin(game, ev, leaves=1, boards=boards())
    bd, p = _root_board(a, game)
    assert _dump(a.search(bd, p, sims)) == _dump(b.search(bd, p, sims))
    for kw in ({"dir_alpha": 0.3, "dir_eps": 0.25}, {"reuse": True}, {"dir_alpha": 1.0, "dir_eps": 0.5, "reuse": True}):
        a, b = Twin(game, ev, boards=boards(), **kw), KTwin(game, ev, leaves=1, boards=boards(), **kw)
        ra, rb = a.selfplay(3, 12, 2, 1, 7), b.selfplay(3, 12, 2, 1, 7)
        assert ra[1:] == rb[1:] and len(ra[0]) == len(rb[0])
        for x, y in zip(ra[0], rb[0]):
            assert x[:2] == y[:2] and x[3:] == y[3:] and [float(v).hex() for v in x[2]] == [float(v).hex() for v in y[2]]


# (collides: the twin's walks meet a pending node at least once -- the cases exercise the collision rule)
SEARCH_CASES = [("ttt", "uniform", 32, 100, True), ("ttt", "hash", 3, 50, False), ("reversi", "hash", 8, 101, True),
                ("reversi", "uniform", 32, 100, True), ("reversi6", "hash", 8, 50, True), ("reversi4", "hash", 8, 101, True),
                ("reversi4", "uniform", 3, 80, False)]


@pytest.mark.parametrize("game,ev,K,sims,collides", SEARCH_CASES)
def test_k_walk_search_invariants_and_collisions(game, ev, K, sims, collides):
    tw = KTwin(game, ev, leaves=K, boards=boards())
    bd, p = _root_board(tw, game)
    root = tw.search(bd, p, sims)
    check_invariants(root, sims, 0, 0)
    assert _nodes(root) <= sims + 1
    assert (tw.n_collisions > 0) == collides


@pytest.mark.parametrize("game,K", [("ttt", 8), ("reversi", 4), ("reversi6", 8), ("reversi4", 3)])
@pytest.mark.parametrize("kw", [{}, {"dir_alpha": 0.3, "dir_eps": 0.25}, {"reuse": True},
                                {"dir_alpha": 1.0, "dir_eps": 0.5, "reuse": True}], ids=["plain", "noise", "reuse", "both"])
def test_k_walk_selfplay_invariants(game, K, kw):
    tw = KTwin(game, "hash", leaves=K, boards=boards(), **kw)
    sims = 24 if game == "reversi" else 30
    seen = {"n": 0, "kept": 0}

    def on_search(root, base):
        before = getattr(on_search, "pre", 0)
        check_invariants(root, sims, base, before)
        seen["n"] += 1
        seen["kept"] += base > 0
    # the kept root's children visits before the new search: measured by wrapping run()
    orig = tw.run

    def run(root, s, base=0):
        on_search.pre = sum(e["N"] for e in root["edges"])
        orig(root, s, base)
    tw.run = run
    ex, w, _ = tw.selfplay(5, sims, 4, 1, 11, slot=3, stagger=4, on_search=on_search)
    assert seen["n"] == len(ex) and w in (-1, 0, 1)
    if kw.get("reuse"):
        assert seen["kept"] > 0


def test_k_walk_twin_first_step_spreads_over_the_root_by_virtual_loss():
    """TTT, uniform, K = 9 from the empty board: the first step's 9 walks spread over the 9 root edges by virtual loss alone
    (a visited edge's q is -1 until its backup), so no walk collides, and every W comes back to exactly 0"""
    tw = KTwin("ttt", "uniform", leaves=9, boards=boards())
    bd, p = _root_board(tw, "ttt")
    root = tw.search(bd, p, 9)
    assert [e["N"] for e in root["edges"]] == [1] * 9 and tw.n_collisions == 0
    assert all(float(e["W"]) == 0.0 for e in root["edges"])  # (W - 1) + 1 + 0: uniform value 0


def one_move_position(seed=0):
    """a Reversi position whose mover has exactly one legal move, leading to a non-terminal child: (board, mover, child,
    child's mover) -- both walks of a K = 2 step must take that move, and the second meets the first one's pending node"""
    import betazero_amd as bz
    tw = KTwin("reversi", "hash", boards=boards())
    rng = np.random.default_rng(seed)
    while True:
        b, p = bz.ReversiBoard(), 1
        while not tw.terminal(b)[0]:
            mv = tw.moves(b, p)
            if not mv:
                p = -p
                continue
            if len(mv) == 1:
                ch = tw.play(b, p, mv[0])
                if not tw.terminal(ch)[0] and tw.moves(ch, -p):
                    return b, p, ch, -p
            b, p = tw.play(b, p, mv[int(rng.integers(len(mv)))]), -p


def hand_checked_collision_w(v):
    """the root edge's W after one K = 2 step over a single legal move, by the rules of DESIGN.md 3.12: walk 0 leaves
    W = 0 - 1, walk 1 collides at the pending child and leaves W = -2; both back up the child's value v as val = -v,
    each as (W + 1) + val"""
    w = f32(f32(0.0) - ONE)
    w = f32(w - ONE)
    w = f32(f32(w + ONE) + f32(-v))
    return f32(f32(w + ONE) + f32(-v))


def test_k_walk_twin_collision_backs_up_the_pending_nodes_value():
    from oracle.py_twin import eval_hash
    b, p, ch, q = one_move_position()
    tw = KTwin("reversi", "hash", leaves=2, boards=boards())
    root = tw.search(b, p, 2)
    own, opp = tw.bits(ch, q)
    v = eval_hash(own, opp, 65)[1]
    assert v != 0 and tw.n_collisions == 1
    (e,) = root["edges"]
    assert e["N"] == 2 and e["child"]["v"] == v
    assert float(e["W"]).hex() == float(hand_checked_collision_w(v)).hex(), (float(e["W"]), float(hand_checked_collision_w(v)))


# ---------------------------------------------------------------- ABI and Python validation (no GPU needed)
def _cfg(K=1, flags=0, game=1, B=4, sims=8):
    return _lib.EngineCfg(game, B, sims, 0, 1.5, 0, 0, 1, 64, 0, 0, 0, B, flags | ((K - 1) << _lib.ENGINE_LEAVES_SHIFT),
                          0.0, 0.0, 0)


# bz_engine_workspace_bytes of the engine before leaves_per_step existed, key "game,B,sims,eval_kind,flags": a K = 1
# workspace is byte for byte that size (the flag bits are 0, and n_collisions lives outside the per-wave counter slots)
K1_BYTES = {
    "0,1,8,0,0": 13312, "0,1,800,0,6": 152832, "0,1,50,1,1": 84736, "0,4,8,0,0": 29184,
    "0,4,800,0,6": 586752, "0,4,50,1,1": 315136, "0,33,8,0,0": 198912, "0,33,800,0,6": 4798976,
    "0,33,50,1,1": 2556928, "0,4096,8,0,0": 23938304, "0,4096,800,0,6": 594887936, "0,4096,50,1,1": 316638464,
    "1,1,8,0,0": 34560, "1,1,800,3,6": 992512, "1,1,50,1,1": 268288, "1,4,8,0,0": 113664,
    "1,4,800,3,6": 3943424, "1,4,50,1,1": 1049344, "1,33,8,0,0": 892928, "1,33,800,3,6": 32485376,
    "1,33,50,1,1": 8610048, "1,4096,8,0,0": 110052608, "1,4096,800,3,6": 4031268096, "1,4096,50,1,1": 1067943168,
    "2,1,8,0,0": 34560, "2,1,800,3,6": 992512, "2,1,50,1,1": 268288, "2,4,8,0,0": 113664,
    "2,4,800,3,6": 3943424, "2,4,50,1,1": 1049344, "2,33,8,0,0": 892928, "2,33,800,3,6": 32485376,
    "2,33,50,1,1": 8610048, "2,4096,8,0,0": 110052608, "2,4096,800,3,6": 4031268096, "2,4096,50,1,1": 1067943168,
    "3,1,8,0,0": 34560, "3,1,800,3,6": 992512, "3,1,50,1,1": 268288, "3,4,8,0,0": 113664,
    "3,4,800,3,6": 3943424, "3,4,50,1,1": 1049344, "3,33,8,0,0": 892928, "3,33,800,3,6": 32485376,
    "3,33,50,1,1": 8610048, "3,4096,8,0,0": 110052608, "3,4096,800,3,6": 4031268096, "3,4096,50,1,1": 1067943168,
}


def _cfg_k(key, K):
    game, B, sims, ev, flags = (int(x) for x in key.split(","))
    return _lib.EngineCfg(game, B, sims, ev, 1.5, 0, 0, 1, 64, 0, 0, 0, B, flags | ((K - 1) << _lib.ENGINE_LEAVES_SHIFT),
                          0.0, 0.0, 0)


def test_workspace_at_k1_is_exactly_the_size_it_was():
    L = _lib.lib()
    for key, want in K1_BYTES.items():
        assert L.bz_engine_workspace_bytes(C.byref(_cfg_k(key, 1))) == want, key


def test_workspace_accepts_every_k_and_grows_by_the_stated_bytes():
    L = _lib.lib()
    assert _lib.ENGINE_LEAVES_SHIFT == 8 and _lib.ENGINE_LEAVES_MASK == 31 << 8
    assert _lib.COUNTER_NAMES[10] == "n_collisions"
    rnd = lambda x: (x + 255) // 256 * 256  # noqa: E731  (every array starts at a multiple of 256 bytes)
    for key, base in K1_BYTES.items():
        game, B, sims, ev, flags = (int(x) for x in key.split(","))
        if sims != 8 or B == 4096:
            continue
        na, maxd = (9, 16) if game == 0 else (65, 128)
        for K in range(1, 33):
            got = L.bz_engine_workspace_bytes(C.byref(_cfg_k(key, K)))
            assert got > 0, (key, K, L.bz_last_error())
            # paths [B][K][maxd] x 16 B, leaf records [B][K] x 32 B (K > 1), rows K*B of leaf_kind (1), leaf_own /
            # leaf_opp / c_own / c_opp (8 each), logits (4 NA), value (4)
            def arrays(k):
                return (rnd(maxd * k * B * 16) + (rnd(k * B * 32) if k > 1 else 0) + rnd(k * B) + 4 * rnd(k * B * 8) +
                        rnd(k * B * na * 4) + rnd(k * B * 4))
            assert got - base == arrays(K) - arrays(1), (key, K)


def test_workspace_refuses_flag_bits_above_12_with_a_message():
    L = _lib.lib()
    for bit in range(13, 32):
        assert L.bz_engine_workspace_bytes(C.byref(_cfg(1, flags=1 << bit))) == -1
        assert b"bit 12" in L.bz_last_error() and b"flags" in L.bz_last_error()
    for bit in range(0, 13):  # the bits below stay what they were
        assert L.bz_engine_workspace_bytes(C.byref(_cfg(1, flags=1 << bit))) > 0


@pytest.mark.parametrize("bad", [0, 33, 2.0, True, -1, "4", None])
def test_python_refuses_bad_leaves_per_step_before_touching_a_device(bad, monkeypatch):
    from betazero_amd.engine import PipelinedSelfPlay, SelfPlayEngine, check_leaves_per_step, self_play
    from betazero_amd.players import MCTSPlayer
    from betazero_amd.arena import play_arena

    def no_device(*a, **k):
        raise AssertionError("touched a device")
    monkeypatch.setattr(_lib, "require_gpu", no_device)
    monkeypatch.setattr(_lib, "lib", no_device)
    with pytest.raises(ValueError, match="leaves_per_step"):
        check_leaves_per_step(bad)
    with pytest.raises(ValueError, match="leaves_per_step"):
        SelfPlayEngine("reversi", 4, 16, "uniform", leaves_per_step=bad)
    with pytest.raises(ValueError, match="leaves_per_step"):
        MCTSPlayer(1, 16, leaves_per_step=bad)
    with pytest.raises(ValueError, match="leaves_per_step"):
        PipelinedSelfPlay("reversi", 4, 16, "uniform", leaves_per_step=bad, streams=[None])
    with pytest.raises(ValueError, match="leaves_per_step"):
        self_play("ttt", 4, 16, leaves_per_step=bad)
    with pytest.raises(ValueError, match="leaves_per_step"):
        play_arena("ttt", 4, 16, leaves_per_step=bad)


def test_python_accepts_every_k_from_1_to_32():
    from betazero_amd.engine import check_leaves_per_step
    assert [check_leaves_per_step(k) for k in range(1, 33)] == list(range(1, 33))
    assert check_leaves_per_step(np.int64(8)) == 8
