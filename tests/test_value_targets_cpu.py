"""Search-value targets without a GPU: bz_root_value and bz_value_targets_segment -- the functions the kernels
run -- against restatements in numpy float32 (what tests/test_gpu_value_targets.py pins the kernels to), the value twins (the
existing feature twins, keeping every searched root and giving a q per recorded row) and the ABI / Python validation."""
import ctypes as C

import numpy as np
import pytest

from betazero_amd import _lib
from oracle.py_twin import Twin, f32
from test_forced_playouts_cpu import ForcedTwin
from test_gumbel_cpu import GumbelTwin
from test_playout_cap_cpu import CapTwin, _cfg, boards

ONE, ZERO = f32(1.0), f32(0.0)


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


# ---------------------------------------------------------------- restatements
def root_value(N, W):
    """sW = 0, sW = sW + W_i in edge order (one binary32 add each), sN = sum N_i (integer),
    q = sN > 0 ? sW / float(sN) : 0"""
    sW, sN = f32(0.0), 0
    with np.errstate(all="ignore"):
        for n, w in zip(N, W):
            sW = f32(sW + f32(w))
            sN += int(n)
        return f32(sW / f32(sN)) if sN > 0 else f32(0.0)


def vt_twin(q, z, mover, lam, q_mix):
    """the value targets of S segments of the same length at once: q f32, z, mover int [S, T]; lam, q_mix f32 [S] (or
    scalars).  Every line is one binary32 operation per element, in the order DESIGN.md 3.18 writes them."""
    q = np.atleast_2d(np.asarray(q, np.float32))
    z, m = np.atleast_2d(np.asarray(z, np.int64)), np.atleast_2d(np.asarray(mover, np.int64))
    S, T = q.shape
    lam = np.broadcast_to(np.asarray(lam, np.float32), (S,)).astype(np.float32)
    q_mix = np.broadcast_to(np.asarray(q_mix, np.float32), (S,)).astype(np.float32)
    with np.errstate(all="ignore"):
        c = np.where(q != q, ZERO, np.where(q < -ONE, -ONE, np.where(q > ONE, ONE, q))).astype(np.float32)
        A = np.where(m == 1, c, -c).astype(np.float32)
        G = np.zeros((S, T), np.float32)
        G[:, T - 1] = (m[:, T - 1] * z[:, T - 1]).astype(np.float32)
        for t in range(T - 2, -1, -1):
            a = (ONE - lam).astype(np.float32)
            a = (a * A[:, t + 1]).astype(np.float32)
            b = (lam * G[:, t + 1]).astype(np.float32)
            G[:, t] = (a + b).astype(np.float32)
        cc = (ONE - q_mix).astype(np.float32)[:, None]
        cc = (cc * G).astype(np.float32)
        d = (q_mix[:, None] * A).astype(np.float32)
        Tt = (cc + d).astype(np.float32)
        Tt = np.where(Tt < -ONE, -ONE, np.where(Tt > ONE, ONE, Tt)).astype(np.float32)
        return np.where(m == 1, Tt, -Tt).astype(np.float32)


def segment_starts(game, ply):
    """row i starts a segment iff i == 0, game[i] != game[i-1] or ply[i] <= ply[i-1]"""
    game, ply = np.asarray(game), np.asarray(ply)
    s = np.ones(len(game), bool)
    s[1:] = (game[1:] != game[:-1]) | (ply[1:] <= ply[:-1])
    return s


def value_targets_twin(q, z, mover, game, ply, lam, q_mix, max_segment=1024):
    """bz_value_targets in numpy: (vt f32 [n], the status word = segments longer than max_segment, which keep (float)z)"""
    n = len(q)
    vt, long_segments = np.asarray(z, np.float32).copy(), 0
    if n == 0:
        return vt, 0
    bounds = list(np.nonzero(segment_starts(game, ply))[0]) + [n]
    for a, b in zip(bounds[:-1], bounds[1:]):
        if b - a > max_segment:
            long_segments += 1
        else:
            vt[a:b] = vt_twin(q[a:b], z[a:b], mover[a:b], lam, q_mix)[0]
    return vt, long_segments


# ---------------------------------------------------------------- the value twins
class _Value:
    """mixin over a feature twin: keeps every searched root by its position (root_noise() / Gumbel's prepare() see every
    root a search starts from).  A played-from root is never simulated again, so once the game is over its edges hold the
    statistics the search left: the q of the row recorded there."""

    def _keep(self, root):
        if root["edges"] is None:
            return
        if not hasattr(self, "roots"):
            self.roots = {}
        self.roots[self.bits(root["b"], root["p"])] = root

    def root_noise(self, root):
        self._keep(root)
        super().root_noise(root)

    def prepare(self, root, *a, **k):
        self._keep(root)
        super().prepare(root, *a, **k)

    def row_q(self, row):
        edges = self.roots[(row[0], row[1])]["edges"]  # (a position occurs once in a game)
        return root_value([e["N"] for e in edges], [e["W"] for e in edges])

    def q_rows(self, rows):
        return np.array([self.row_q(r) for r in rows], np.float32)


def ValueTwin(base):
    return type("Value" + base.__name__, (_Value, base), {})


def _selfplay(cls, kind, game, g, sims, temp_moves, openings, seed, base, noise, cap, reuse):
    kw = dict(boards=boards(), **(dict(dir_alpha=0.3, dir_eps=0.25) if noise else {}))
    if kind == "plain":
        tw = cls(Twin)(game, "hash", reuse=reuse, **kw)
        return tw, tw.selfplay(base + g, sims, temp_moves, openings, seed)
    if kind == "cap":
        tw = cls(CapTwin)(game, "hash", cap[0], cap[1], **kw)
    elif kind == "forced":
        tw = cls(ForcedTwin)(game, "hash", 2.0, prune=True, cap=cap, **kw)
    else:
        tw = cls(GumbelTwin)(game, "hash", **kw)
    return tw, tw.selfplay(base + g, sims, temp_moves, openings, seed, slot=g)


def value_games(kind, game, n, sims, temp_moves=0, openings=0, seed=0, base=0, noise=False, cap=None, reuse=False):
    """n games of a value twin: [(rows, q [len(rows)], winner)].  kind: "plain" | "cap" | "forced" | "gumbel"."""
    out = []
    for g in range(n):
        tw, (rows, w, _) = _selfplay(ValueTwin, kind, game, g, sims, temp_moves, openings, seed, base, noise, cap, reuse)
        out.append((rows, tw.q_rows(rows), w))
    return out


# ---------------------------------------------------------------- bz_root_value
def _c_q(N, W):
    n, w, out = np.asarray(N, np.uint32), np.asarray(W, np.float32), C.c_float(-7.0)
    assert _lib.lib().bz_root_value(n.ctypes.data, w.ctypes.data, len(n), C.addressof(out)) == 0, _lib.lib().bz_last_error()
    return f32(out.value)


def test_root_value_equals_the_restatement_on_random_roots():
    rng = np.random.default_rng(0)
    inside = 0
    for trial in range(3000):
        n = int(rng.integers(1, 66))
        N = rng.integers(0, int(rng.choice([2, 30, 800])), n).astype(np.uint32)
        W = ((rng.random(n) * 2 - 1) * N).astype(np.float32)  # |W_i| <= N_i, as a search leaves them
        if trial % 9 == 0:
            W[rng.integers(0, n)] = f32(rng.choice([np.nan, np.inf, -np.inf, 1e30]))  # carried, not cleaned: the targets clean
        want, got = root_value(N, W), _c_q(N, W)
        assert _bits(got) == _bits(want), (trial, N, W, got, want)
        inside += bool(abs(got) <= 1)
    assert inside > 2500


def test_root_value_edge_cases():
    for n in (1, 9, 34, 65):
        assert _bits(_c_q(np.zeros(n, np.uint32), np.full(n, 0.5, np.float32))) == _bits(0.0)  # no visit: 0, whatever W holds
    assert _bits(_c_q([7], [-3.5])) == _bits(-0.5)                                          # the one-edge root (a forced pass)
    assert _bits(_c_q([1], [1.0])) == _bits(1.0) and _bits(_c_q([3], [-3.0])) == _bits(-1.0)
    assert _bits(_c_q([1, 2], [0.25, 0.5])) == _bits(f32(0.75) / f32(3.0))                  # hand-checked
    # the sum is sequential from 0.0f in edge order: 2^24 + 1 + 1 stays 2^24, 1 + 1 + 2^24 is 2^24 + 2
    big = f32(2.0 ** 24)
    assert _bits(_c_q([1, 0, 0], [big, 1, 1])) == _bits(big) and _bits(_c_q([1, 0, 0], [1, 1, big])) == _bits(big + f32(2.0))


def test_root_value_refuses_bad_arguments_with_a_message():
    L = _lib.lib()
    n, w, out = np.ones(2, np.uint32), np.ones(2, np.float32), C.c_float()
    for args in ((None, w.ctypes.data, 2, C.addressof(out)), (n.ctypes.data, None, 2, C.addressof(out)),
                 (n.ctypes.data, w.ctypes.data, 0, C.addressof(out)), (n.ctypes.data, w.ctypes.data, 256, C.addressof(out)),
                 (n.ctypes.data, w.ctypes.data, 2, None)):
        assert L.bz_root_value(*args) == _lib.BZ_EINVAL and b"bz_root_value" in L.bz_last_error()


# ---------------------------------------------------------------- bz_value_targets_segment
def _c_segment(q, z, mover, lam, q_mix):
    q, z, m = np.ascontiguousarray(q, np.float32), np.ascontiguousarray(z, np.int8), np.ascontiguousarray(mover, np.int8)
    vt = np.full(len(q) + 2, -7.0, np.float32)
    rc = _lib.lib().bz_value_targets_segment(q.ctypes.data, z.ctypes.data, m.ctypes.data, len(q), C.c_float(lam), C.c_float(q_mix),
                                             vt.ctypes.data)
    assert rc == 0, _lib.lib().bz_last_error()
    assert (vt[len(q):] == -7.0).all()  # nothing written behind the segment
    return vt[:len(q)]


def _segments(rng, S, T):
    """S random segments of T rows: movers with repeats (passes), z consistent with one winner, q with NaN, +-inf, +-1 and
    values outside [-1, 1] among ordinary ones"""
    m = np.where(rng.random((S, T)) < 0.5, 1, -1).astype(np.int8)
    alt = np.where((np.arange(T) % 2 == 0)[None, :], 1, -1).astype(np.int8) * np.where(rng.random((S, 1)) < 0.5, 1, -1).astype(np.int8)
    m = np.where(rng.random((S, 1)) < 0.5, alt, m).astype(np.int8)  # half of them strictly alternating
    w = rng.integers(-1, 2, (S, 1))
    z = (m * w).astype(np.int8)
    q = (rng.random((S, T)) * 2 - 1).astype(np.float32)
    special = np.array([np.nan, np.inf, -np.inf, 1.0, -1.0, 1.5, -3.0, 0.0, -0.0, 1e-40], np.float32)
    hit = rng.random((S, T)) < 0.15
    q[hit] = special[rng.integers(0, len(special), int(hit.sum()))]
    q[rng.random(S) < 0.05] = ONE  # saturated games
    fixed = np.array([0.0, 0.5, 0.8, 1.0], np.float32)
    lam = np.where(rng.random(S) < 0.5, fixed[rng.integers(0, 4, S)], rng.random(S).astype(np.float32)).astype(np.float32)
    q_mix = np.where(rng.random(S) < 0.5, fixed[rng.integers(0, 4, S)], rng.random(S).astype(np.float32)).astype(np.float32)
    return q, z, m, lam, q_mix


def test_segment_equals_the_numpy_twin_on_20000_random_segments():
    rng = np.random.default_rng(1)
    total = 0
    for T in range(1, 61):
        S = 334
        q, z, m, lam, q_mix = _segments(rng, S, T)
        want = vt_twin(q, z, m, lam, q_mix)
        assert (np.abs(want) <= 1).all()
        for s in range(S):
            got = _c_segment(q[s], z[s], m[s], float(lam[s]), float(q_mix[s]))
            assert np.array_equal(_bits(got), _bits(want[s])), (T, s, q[s], z[s], m[s], lam[s], q_mix[s], got, want[s])
            assert (np.abs(got) <= 1).all()
        total += S
    assert total >= 20000


def test_the_two_identities_hold_exactly():
    """lam = 1, q_mix = 0: vt == (float)z on every row, by value (a drawn game gives -0.0 for mover -1);
    lam = 0, q_mix = 1: vt == the cleaned q"""
    rng = np.random.default_rng(2)
    for T in (1, 2, 3, 17, 60):
        q, z, m, _, _ = _segments(rng, 200, T)
        with np.errstate(all="ignore"):
            clean = np.where(q != q, ZERO, np.clip(q, -1, 1)).astype(np.float32)
        for s in range(200):
            got = _c_segment(q[s], z[s], m[s], 1.0, 0.0)
            assert np.array_equal(got, z[s].astype(np.float32)), (T, s, got, z[s])
            got = _c_segment(q[s], z[s], m[s], 0.0, 1.0)
            assert np.array_equal(got, clean[s]), (T, s, got, clean[s])
        assert np.array_equal(vt_twin(q, z, m, 1.0, 0.0), z.astype(np.float32)) and np.array_equal(vt_twin(q, z, m, 0.0, 1.0), clean)


def test_segment_hand_checked_and_refusals():
    # three rows, movers +1 -1 +1, +1 wins: A = (0.5, -0.25, 0.75) from q = (0.5, 0.25, 0.75); lam = 0.5, q_mix = 0:
    # G2 = 1, G1 = 0.5 * 0.75 + 0.5 * 1 = 0.875, G0 = 0.5 * -0.25 + 0.5 * 0.875 = 0.3125; vt = (G0, -G1, G2)
    got = _c_segment([0.5, 0.25, 0.75], [1, -1, 1], [1, -1, 1], 0.5, 0.0)
    assert np.array_equal(got, np.array([0.3125, -0.875, 1.0], np.float32))
    # q_mix = 0.5 at lam = 1: the average of z and q
    got = _c_segment([0.5, 0.25, 0.75], [1, -1, 1], [1, -1, 1], 1.0, 0.5)
    assert np.array_equal(got, np.array([0.75, -0.375, 0.875], np.float32))
    L = _lib.lib()
    q, z, vt = np.zeros(4, np.float32), np.ones(4, np.int8), np.zeros(4, np.float32)
    ok = [q.ctypes.data, z.ctypes.data, z.ctypes.data, 4, C.c_float(0.5), C.c_float(0.5), vt.ctypes.data]
    assert L.bz_value_targets_segment(*ok) == 0
    for i, bad in ((0, None), (1, None), (2, None), (6, None), (3, 0), (3, 1025), (3, -1), (4, C.c_float(-0.01)), (4, C.c_float(1.01)),
                   (4, C.c_float(float("nan"))), (5, C.c_float(-0.01)), (5, C.c_float(2.0)), (5, C.c_float(float("nan"))),
                   (4, C.c_float(float("inf")))):
        args = list(ok)
        args[i] = bad
        assert L.bz_value_targets_segment(*args) == _lib.BZ_EINVAL and b"bz_value_targets_segment" in L.bz_last_error(), (i, bad)


def test_value_targets_twin_splits_segments_where_the_issue_says():
    game = np.array([5, 5, 5, 6, 6, 6, 6, 6])
    ply = np.array([0, 1, 3, 0, 2, 2, 1, 4])  # a fast search's row is simply absent (1 -> 3); equal and falling plies split
    assert list(segment_starts(game, ply)) == [True, False, False, True, False, True, True, False]
    rng = np.random.default_rng(3)
    q, m = (rng.random(8) * 2 - 1).astype(np.float32), np.where(rng.random(8) < 0.5, 1, -1).astype(np.int8)
    z = m.copy()
    vt, status = value_targets_twin(q, z, m, game, ply, 0.5, 0.25)
    assert status == 0
    for a, b in ((0, 3), (3, 5), (5, 6), (6, 8)):
        assert np.array_equal(_bits(vt[a:b]), _bits(_c_segment(q[a:b], z[a:b], m[a:b], 0.5, 0.25)))
    vt, status = value_targets_twin(q, z, m, np.zeros(8), np.arange(8), 0.5, 0.25, max_segment=7)
    assert status == 1 and np.array_equal(vt, z.astype(np.float32))


# ---------------------------------------------------------------- the twins
def _plain_rows(kind, game, sims, **kw):
    """the rows of the feature twin WITHOUT the mixin: the mixin observes only"""
    return _selfplay(lambda base: base, kind, game, 0, sims, kw.get("temp_moves", 0), 0, 5, 3, kw.get("noise", False), kw.get("cap"),
                     kw.get("reuse", False))[1][0]


@pytest.mark.parametrize("kind,kw", [("plain", {}), ("plain", {"noise": True}), ("plain", {"noise": True, "reuse": True}),
                                     ("cap", {"cap": (4, 32768), "noise": True}), ("forced", {"noise": True}),
                                     ("gumbel", {"temp_moves": 3})])
@pytest.mark.parametrize("game,sims", [("ttt", 24), ("reversi4", 16)])
def test_value_twin_observes_only_and_gives_a_q_per_row(kind, kw, game, sims):
    rows, q, w = value_games(kind, game, 1, sims, seed=5, base=3, **kw)[0]
    ref = _plain_rows(kind, game, sims, **kw)
    assert len(rows) == len(ref) == len(q)
    for a, b in zip(rows, ref):
        assert a[0] == b[0] and a[1] == b[1] and a[3] == b[3] and a[4] == b[4] and np.array_equal(_bits(a[2]), _bits(b[2]))
    assert (np.abs(q) <= 1).all() and (q != 0).any() and np.isfinite(q).all()


def test_value_twin_q_is_of_the_raw_visits_of_the_searched_root():
    """a full search's root has sum N = sims (plus what subtree reuse carried over), and the q is W over exactly those visits"""
    tw, (rows, w, _) = _selfplay(ValueTwin, "plain", "reversi4", 0, 16, 0, 0, 9, 2, False, None, False)
    for r in rows:
        edges = tw.roots[(r[0], r[1])]["edges"]
        assert sum(e["N"] for e in edges) == 16
        assert _bits(tw.row_q(r)) == _bits(root_value([e["N"] for e in edges], [e["W"] for e in edges]))
    tw, (rows, w, _) = _selfplay(ValueTwin, "plain", "reversi4", 0, 16, 0, 0, 9, 2, True, None, True)
    assert any(sum(e["N"] for e in tw.roots[(r[0], r[1])]["edges"]) > 16 for r in rows)  # carried visits are included
    # forced playouts: the q is of the raw visits, not of the pruned ones the row's pi holds
    tw, (rows, w, _) = _selfplay(ValueTwin, "forced", "reversi4", 0, 16, 0, 0, 7, 0, True, None, False)
    differs = 0
    for r in rows:
        edges = tw.roots[(r[0], r[1])]["edges"]
        sumN = sum(e["N"] for e in edges)
        differs += any(_bits(f32(e["N"]) / f32(sumN)) != _bits(r[2][e["a"]]) for e in edges)
    assert differs > 0


# ---------------------------------------------------------------- buffer size, ABI and Python validation
def test_search_value_bytes_is_the_stated_layout_and_the_abi_refuses_bad_arguments():
    L = _lib.lib()
    al = lambda x: (x + 255) // 256 * 256  # noqa: E731
    for game in (0, 1, 2, 3):
        for B in (1, 4, 33, 64, 4096):
            for rounds in (1, 3):
                cfg = _cfg(game, B, 8)
                cfg.rounds, cfg.t_max = rounds, 9 if game == 0 else 64
                assert L.bz_engine_search_value_bytes(C.byref(cfg)) == al(rounds * B * cfg.t_max * 4), (game, B, rounds)
    # nothing the engine accepts is refused: subtree reuse, K > 1, the caches
    for cfg in (_cfg(flags=_lib.ENGINE_REUSE_SUBTREE), _cfg(K=8), _cfg(flags=_lib.ENGINE_EVAL_CACHE | _lib.ENGINE_EVAL_CACHE_CARRY)):
        assert L.bz_engine_search_value_bytes(C.byref(cfg)) > 0
    assert L.bz_engine_search_value_bytes(None) == -1 and b"bz_engine_search_value_bytes" in L.bz_last_error()
    assert L.bz_engine_search_value_bytes(C.byref(_cfg(sims=9000))) == -1
    assert L.bz_engine_set_search_value(None, None, 0, None) == _lib.BZ_EINVAL and b"bz_engine_set_search_value" in L.bz_last_error()
    assert L.bz_engine_pack_search_value(None, None, 1, 0, None) == _lib.BZ_EINVAL and b"bz_engine_pack_search_value" in L.bz_last_error()
    assert L.bz_abi_version() == 7
    # bz_value_targets: every refusal comes before a launch (this host has no GPU to launch on)
    a = np.zeros(4, np.int64)
    p = a.ctypes.data
    ok = [p, p, p, p, p, 4, C.c_float(1.0), C.c_float(0.0), p, p, None]
    for i, bad in ((5, -1), (5, (1 << 26) + 1), (6, C.c_float(-0.5)), (6, C.c_float(1.5)), (6, C.c_float(float("nan"))),
                   (7, C.c_float(-0.5)), (7, C.c_float(1.5)), (7, C.c_float(float("nan"))), (9, None), (9, p + 4), (0, None), (1, None),
                   (2, None), (3, None), (4, None), (8, None)):
        args = list(ok)
        args[i] = bad
        assert L.bz_value_targets(*args) == _lib.BZ_EINVAL and b"bz_value_targets" in L.bz_last_error(), (i, bad)
    assert L.bz_value_targets(*(ok[:5] + [(1 << 26) + 1] + ok[6:])) == _lib.BZ_EINVAL and b"2^26" in L.bz_last_error()
    # bz_train_heads_vt: bz_train_heads' refusals, plus the slot
    assert L.bz_train_heads_vt(None, None, None, 64, 64, 64, None, None, None, None, None, None, None) == _lib.BZ_EINVAL
    assert b"bz_train_heads_vt" in L.bz_last_error()
    hp = _lib.TrainHeadParams(*([p] * 10))
    assert L.bz_train_heads_vt(p, p, None, 64, 64, 64, C.byref(hp), p, p, p, p, p, None) == _lib.BZ_EINVAL   # no slot
    assert L.bz_train_heads_vt(p, p, p, 6, 64, 64, C.byref(hp), p, p, p, p, p, None) == _lib.BZ_EINVAL      # n not a multiple of 4
    assert L.bz_train_heads_vt(p, p, p, 64, 96, 64, C.byref(hp), p, p, p, p, p, None) == _lib.BZ_EINVAL     # width
    assert L.bz_train_heads_vt(p, p, p, 64, 64, 65, C.byref(hp), p, p, p, p, p, None) == _lib.BZ_EINVAL     # value_hidden
    assert C.sizeof(_lib.TrainBatch) == 48


def _examples(n, seed=0, **have):
    from betazero_amd.engine import Examples
    g = np.random.default_rng(seed)
    extra = {f: g.random(n).astype(np.float32) for f in ("kl", "q", "vt") if have.get(f)}
    return Examples(g.integers(0, 2 ** 62, n).astype(np.uint64), g.integers(0, 2 ** 62, n).astype(np.uint64),
                    g.random((n, 65)).astype(np.float32), g.integers(-1, 2, n).astype(np.int8), np.ones(n, np.int8),
                    np.zeros(n, np.uint8), np.arange(n), np.zeros(n, np.int32), 8, **extra)


def test_examples_carry_q_and_vt_through_concat_select_and_the_host_round_trip():
    import torch
    from betazero_amd.engine import DeviceExamples, Examples, concat_device_examples, concat_examples
    from betazero_amd.train import select_rows
    a, b = _examples(5, 1, q=True, vt=True), _examples(3, 2, q=True, vt=True)
    bare, only_q, with_kl = _examples(4, 3), _examples(4, 4, q=True), _examples(4, 5, kl=True, q=True, vt=True)
    # the two fields are the last ones, after kl, and default to None: positional constructions keep working
    pos = Examples(*[getattr(bare, f) for f in ("own", "opp", "pi", "z", "mover", "act", "game", "ply", "size")])
    assert pos.kl is None and pos.q is None and pos.vt is None
    pos = Examples(*[getattr(with_kl, f) for f in ("own", "opp", "pi", "z", "mover", "act", "game", "ply", "size", "kl", "q", "vt")])
    assert pos.kl is with_kl.kl and pos.q is with_kl.q and pos.vt is with_kl.vt
    ab = concat_examples([a, b])
    assert np.array_equal(ab.q, np.concatenate([a.q, b.q])) and np.array_equal(ab.vt, np.concatenate([a.vt, b.vt])) and ab.kl is None
    cc = concat_examples([bare, bare])
    assert cc.q is None and cc.vt is None
    oq = concat_examples([only_q, only_q])
    assert oq.q is not None and oq.vt is None
    for parts, field in (([a, bare], "q"), ([only_q, a], "vt"), ([with_kl, a], "kl")):  # a mixture raises, per field
        with pytest.raises(ValueError, match=rf"carry {field} "):
            concat_examples(parts)
    da, db, dbare, doq = (DeviceExamples.from_host(x, "cpu") for x in (a, b, bare, only_q))
    assert da.q.dtype == torch.float32 and da.vt.dtype == torch.float32 and dbare.q is None and dbare.vt is None and doq.vt is None
    dab = concat_device_examples([da, db])
    assert np.array_equal(dab.q.numpy(), ab.q) and np.array_equal(dab.vt.numpy(), ab.vt) and concat_device_examples([dbare, dbare]).q is None
    for parts, field in (([dbare, da], "q"), ([doq, da], "vt")):
        with pytest.raises(ValueError, match=rf"carry {field} "):
            concat_device_examples(parts)
    idx = torch.tensor([7, 0, 0, 3])
    sel = select_rows(dab, idx)
    assert np.array_equal(sel.q.numpy(), ab.q[[7, 0, 0, 3]]) and np.array_equal(sel.vt.numpy(), ab.vt[[7, 0, 0, 3]])
    assert select_rows(dbare, torch.tensor([1])).q is None and select_rows(doq, torch.tensor([1])).vt is None
    back = dab.cpu()
    assert np.array_equal(back.q, ab.q) and np.array_equal(back.vt, ab.vt) and back.q.dtype == np.float32 and dbare.cpu().q is None


def test_python_refuses_a_search_value_that_is_no_bool_before_touching_a_device(monkeypatch):
    from betazero_amd import engine

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(_lib, "require_gpu", no_device)
    monkeypatch.setattr(_lib, "lib", no_device)
    for bad in (1, "yes", None, 0.5):
        with pytest.raises(ValueError, match="search_value"):
            engine.SelfPlayEngine("reversi", 4, 8, search_value=bad)
        with pytest.raises(ValueError, match="search_value"):
            engine.PipelinedSelfPlay("reversi", 4, 8, pipelines=1, streams=[None], search_value=bad)
        with pytest.raises(ValueError, match="search_value"):
            engine.self_play("reversi", 4, 8, search_value=bad)


def test_value_targets_refuses_bad_arguments_before_touching_a_device(monkeypatch):
    from betazero_amd import value_targets as vtm
    from betazero_amd.engine import DeviceExamples

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(_lib, "lib", no_device)
    with_q, without = DeviceExamples.from_host(_examples(4, q=True), "cpu"), DeviceExamples.from_host(_examples(4), "cpu")
    with pytest.raises(ValueError, match="no q"):
        vtm.value_targets(without)
    for bad in (-0.01, 1.01, float("nan"), "0.5", None, True):
        with pytest.raises(ValueError, match="lam"):
            vtm.value_targets(with_q, lam=bad)
        with pytest.raises(ValueError, match="q_mix"):
            vtm.value_targets(with_q, q_mix=bad)
    with pytest.raises(ValueError, match="GPU"):
        vtm.value_targets(with_q)  # valid arguments, host tensors: refused too, still before any library call
    with pytest.raises(ValueError, match="GPU"):
        vtm.value_targets(_examples(4, q=True))  # host Examples


def test_the_training_entry_points_refuse_a_missing_vt_before_touching_a_device():
    from betazero_amd.engine import DeviceExamples
    from betazero_amd.train import train_step
    ex = DeviceExamples.from_host(_examples(4, q=True), "cpu")
    with pytest.raises(ValueError, match="vt"):
        train_step(None, None, ex, value_targets=True)
