"""Policy surprise weighting without a GPU: bz_surprise_kl and bz_surprise_count -- the functions the kernels
run -- against restatements in numpy float32, the resampler's numpy twin (what tests/test_gpu_surprise.py pins the kernels to),
the surprise twins (the existing feature twins, keeping the root's raw prior and giving a kl per recorded row) and the ABI /
Python validation."""
import ctypes as C

import numpy as np
import pytest

from betazero_amd import _lib
from oracle.py_twin import M64, Twin, f32, logf_spec, mix64, rng_draw
from test_forced_playouts_cpu import ForcedTwin
from test_gumbel_cpu import GumbelTwin
from test_playout_cap_cpu import CapTwin, _cfg, boards

FLT_MIN = f32(1.17549435e-38)
C_SURPRISE = 0x7375727072697365
KL_MAX, W_MAX, Q30, Q24 = f32(128.0), f32(2.0 ** 30), f32(2.0 ** 30), f32(2.0 ** 24)


# ---------------------------------------------------------------- restatements
def surprise_kl(pi, P):
    """sum over the edges with pi > 0 of pi * (logf(pi) - logf(max(P, FLT_MIN))), one rounding per operation,
    then negative / NaN -> 0.  A NaN prior is carried as a NaN (logf_spec is defined on normal positive numbers only)."""
    kl = f32(0.0)
    with np.errstate(all="ignore"):
        for p, q in zip(pi, P):
            p, q = f32(p), f32(q)
            if not (p > 0):
                continue
            q = FLT_MIN if q < FLT_MIN else q
            lq = logf_spec(q) if q == q else q
            t = f32(logf_spec(p) - lq)
            t = f32(p * t)
            kl = f32(kl + t)
    return kl if kl > 0 else f32(0.0)


def hash_pos(own, opp):
    return mix64(((own * 0x9E3779B97F4A7C15) & M64) ^ mix64((opp + 0x632BE59BD9B4E019) & M64))


def surprise_clean(kl):
    k = f32(kl) if f32(kl) > 0 else f32(0.0)
    return k if k < KL_MAX else KL_MAX


def surprise_mean(kls):
    """the exact integer mean: q_i = (u64)(kl_i * 2^30), mean = float(double(sum q) / (double(n) * 2^30))"""
    s = sum(int(f32(surprise_clean(k) * Q30)) for k in kls)
    return f32(float(s) / (float(len(kls)) * 2.0 ** 30))


def surprise_weight(kl, mean, u):
    mean, u = f32(mean), f32(u)
    if not (mean > 0):
        return f32(1.0)
    t = f32(f32(1.0) - u)
    t = f32(t * f32(surprise_clean(kl) / mean))
    w = f32(u + t)
    return w if w < W_MAX else W_MAX


def surprise_draw(seed, game, ply, own, opp):
    """24 bits keyed by (seed ^ C_SURPRISE, game id, ply) and the position: the row's content, never its index"""
    h = rng_draw((seed ^ C_SURPRISE) & M64, game & M64, ply & 0xFFFFFFFF)
    return mix64(h ^ hash_pos(own, opp)) >> 40


def surprise_count(kl, mean, u, seed, game, ply, own, opp):
    w = surprise_weight(kl, mean, u)
    fl = np.floor(w)
    fr = f32(w - fl)
    return int(fl) + (1 if surprise_draw(seed, game, ply, own, opp) < int(f32(fr * Q24)) else 0)


# ---- the same, vectorised over rows (uint64 arrays wrap silently): the resampler's twin
def _mix64_v(x):
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xFF51AFD7ED558CCD)
    x = x ^ (x >> np.uint64(33))
    x = x * np.uint64(0xC4CEB9FE1A85EC53)
    return x ^ (x >> np.uint64(33))


def resample_twin(kl, game, ply, own, opp, u, seed, idx_cap=None):
    """bz_surprise_resample in numpy: (counts int32 [n], idx int64 -- row i count_i times, ascending, cut at idx_cap --, sum
    count, dropped entries, mean)"""
    kl = np.asarray(kl, np.float32)
    n = len(kl)
    with np.errstate(all="ignore"):
        k = np.where(kl > 0, kl, f32(0.0)).astype(np.float32)
        k = np.where(k < KL_MAX, k, KL_MAX).astype(np.float32)
        s = int((k * Q30).astype(np.uint64).sum(dtype=np.uint64))
        mean = f32(float(s) / (float(n) * 2.0 ** 30)) if n else f32(0.0)
        if mean > 0:
            t = f32(f32(1.0) - f32(u))
            w = (f32(u) + (t * (k / mean).astype(np.float32)).astype(np.float32)).astype(np.float32)
            w = np.where(w < W_MAX, w, W_MAX).astype(np.float32)
        else:
            w = np.ones(n, np.float32)
        fl = np.floor(w)
        thr = ((w - fl).astype(np.float32) * Q24).astype(np.float32).astype(np.uint32)
        g, p = np.asarray(game, np.int64).view(np.uint64), np.asarray(ply, np.int32).view(np.uint32).astype(np.uint64)
        o, q = np.asarray(own, np.uint64), np.asarray(opp, np.uint64)
        h = _mix64_v(np.uint64((seed ^ C_SURPRISE) & M64) * np.uint64(0x9E3779B97F4A7C15) + g)
        h = _mix64_v(h ^ (p * np.uint64(0xBF58476D1CE4E5B9) + np.uint64(0x94D049BB133111EB)))
        hp = _mix64_v(o * np.uint64(0x9E3779B97F4A7C15) ^ _mix64_v(q + np.uint64(0x632BE59BD9B4E019)))
        draw = (_mix64_v(h ^ hp) >> np.uint64(40)).astype(np.uint32)
    count = (fl.astype(np.int64) + (draw < thr)).astype(np.int32)
    idx = np.repeat(np.arange(n, dtype=np.int64), count)
    total = int(count.sum(dtype=np.int64))
    cap = total if idx_cap is None else idx_cap
    return count, idx[:cap], total, max(0, total - cap), mean


# ---------------------------------------------------------------- the surprise twins
class _Surprise:
    """mixin over a feature twin: keeps every searched root's raw prior -- as the expansion stored it, before root_noise()
    rewrites it (Gumbel: before prepare() reads it) -- by the root's position, and gives the kl of recorded rows"""

    def _keep(self, root):
        if root["edges"] is None:
            return
        if not hasattr(self, "raw"):
            self.raw = {}
        self.raw[self.bits(root["b"], root["p"])] = ([e["a"] for e in root["edges"]], [f32(e["P"]) for e in root["edges"]])

    def root_noise(self, root):
        self._keep(root)
        super().root_noise(root)

    def prepare(self, root, *a, **k):
        self._keep(root)
        super().prepare(root, *a, **k)

    def row_kl(self, row):
        acts, prior = self.raw[(row[0], row[1])]  # (a position occurs once in a game)
        return surprise_kl([row[2][a] for a in acts], prior)

    def kl_rows(self, rows):
        return np.array([self.row_kl(r) for r in rows], np.float32)


def SurpriseTwin(base):
    return type("Surprise" + base.__name__, (_Surprise, base), {})


def surprise_games(kind, game, n, sims, temp_moves=0, openings=0, seed=0, base=0, noise=False, cap=None, reuse=False):
    """n games of a surprise twin: [(rows, kl [len(rows)], winner)].  kind: "plain" | "cap" | "forced" | "gumbel"."""
    kw = dict(boards=boards(), **(dict(dir_alpha=0.3, dir_eps=0.25) if noise else {}))
    out = []
    for g in range(n):
        if kind == "plain":
            tw = SurpriseTwin(Twin)(game, "hash", reuse=reuse, **kw)
            rows, w, _ = tw.selfplay(base + g, sims, temp_moves, openings, seed)
        elif kind == "cap":
            tw = SurpriseTwin(CapTwin)(game, "hash", cap[0], cap[1], **kw)
            rows, w, _ = tw.selfplay(base + g, sims, temp_moves, openings, seed, slot=g)
        elif kind == "forced":
            tw = SurpriseTwin(ForcedTwin)(game, "hash", 2.0, prune=True, cap=cap, **kw)
            rows, w, _ = tw.selfplay(base + g, sims, temp_moves, openings, seed, slot=g)
        else:
            tw = SurpriseTwin(GumbelTwin)(game, "hash", **kw)
            rows, w, _ = tw.selfplay(base + g, sims, temp_moves, openings, seed, slot=g)
        out.append((rows, tw.kl_rows(rows), w))
    return out


# ---------------------------------------------------------------- bz_surprise_kl
def _c_kl(pi, P):
    a, b, out = np.asarray(pi, np.float32), np.asarray(P, np.float32), C.c_float(-1.0)
    assert _lib.lib().bz_surprise_kl(a.ctypes.data, b.ctypes.data, len(a), C.addressof(out)) == 0, _lib.lib().bz_last_error()
    return f32(out.value)


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def test_kl_equals_the_restatement_on_random_pairs():
    rng = np.random.default_rng(0)
    positive = 0
    for trial in range(3000):
        n = int(rng.integers(1, 66))
        pi = rng.dirichlet(np.full(n, float(rng.choice([0.05, 0.3, 1.0])))).astype(np.float32)
        pi[rng.random(n) < 0.3] = 0  # unvisited edges
        P = rng.dirichlet(np.full(n, float(rng.choice([0.05, 0.3, 1.0])))).astype(np.float32)
        if trial % 7 == 0:
            P[rng.integers(0, n)] = f32(rng.choice([0.0, 1e-39, 1e-45, 1.17549435e-38]))  # at and below FLT_MIN
        want = surprise_kl(pi, P)
        got = _c_kl(pi, P)
        assert _bits(got) == _bits(want), (trial, pi, P, got, want)
        assert got >= 0
        positive += got > 0
    assert positive > 2000


def test_kl_edge_cases():
    one = f32(1.0)
    assert _bits(_c_kl([one], [one])) == _bits(0.0)                         # the forced-pass root: one edge, P = 1
    for n in (2, 9, 34, 65):
        p = np.random.default_rng(n).dirichlet(np.ones(n)).astype(np.float32)
        assert _bits(_c_kl(p, p)) == _bits(0.0)                             # pi == P: every term is p * (x - x)
    assert _bits(_c_kl([0, 0, 0], [0.2, 0.3, 0.5])) == _bits(0.0)           # nothing recorded
    nan = f32(np.nan)
    for pi, P in (([one], [nan]), ([0.5, 0.5], [nan, 0.5]), ([0.25, 0.75], [0.5, nan]), ([0.5, 0.5], [nan, nan])):
        assert _bits(_c_kl(pi, P)) == _bits(0.0) and _bits(surprise_kl(pi, P)) == _bits(0.0)
    assert _c_kl([0.0, 1.0], [nan, 0.5]) > 0                                # a NaN prior under pi = 0 is never read
    # P below FLT_MIN is floored there: 87.3 = ln(1 / FLT_MIN) bounds a row's kl
    for tiny in (0.0, 1e-45, 1e-39):
        got = _c_kl([one], [tiny])
        assert _bits(got) == _bits(surprise_kl([one], [tiny])) and 87.0 < got < 87.5
    # hand-checked: pi = (1/2, 1/2), P = (1/4, 3/4): 0.5 ln 2 + 0.5 ln(2/3) = 0.14384
    assert abs(float(_c_kl([0.5, 0.5], [0.25, 0.75])) - 0.143841) < 1e-5


def test_kl_refuses_bad_arguments_with_a_message():
    L = _lib.lib()
    a, out = np.ones(2, np.float32), C.c_float()
    for args in ((None, a.ctypes.data, 2, C.addressof(out)), (a.ctypes.data, None, 2, C.addressof(out)),
                 (a.ctypes.data, a.ctypes.data, 0, C.addressof(out)), (a.ctypes.data, a.ctypes.data, 256, C.addressof(out)),
                 (a.ctypes.data, a.ctypes.data, 2, None)):
        assert L.bz_surprise_kl(*args) == _lib.BZ_EINVAL and b"bz_surprise_kl" in L.bz_last_error()


# ---------------------------------------------------------------- bz_surprise_count
def _c_count(kl, mean, u, seed, game, ply, own, opp):
    out = C.c_int32(-1)
    rc = _lib.lib().bz_surprise_count(C.c_float(kl), C.c_float(mean), C.c_float(u), seed, game, ply, own, opp, C.byref(out))
    assert rc == 0, _lib.lib().bz_last_error()
    return out.value


def test_count_equals_the_restatement_and_is_floor_or_floor_plus_one():
    rng = np.random.default_rng(1)
    ups = 0
    for trial in range(4000):
        kl = f32(rng.choice([0.0, 1e-9, 0.01, 0.3, 2.0, 87.0, 500.0, -1.0, np.nan]) * rng.random())
        mean = f32(rng.choice([0.0, 1e-9, 0.05, 0.4, 3.0]) * rng.random())
        u = f32(rng.choice([0.0, 0.25, 0.5, 1.0, rng.random()]))
        seed, game, own, opp = (int(rng.integers(0, 2 ** 63)) for _ in range(4))
        ply = int(rng.integers(0, 64))
        want = surprise_count(kl, mean, u, seed, game, ply, own, opp)
        got = _c_count(kl, mean, u, seed, game, ply, own, opp)
        assert got == want, (trial, kl, mean, u, got, want)
        w = surprise_weight(kl, mean, u)
        assert got in (int(np.floor(w)), int(np.floor(w)) + 1)
        if w == np.floor(w):
            assert got == int(w)
        ups += got > int(np.floor(w))
    assert 500 < ups < 3500


def test_count_is_one_at_uniform_frac_one_and_at_mean_zero():
    rng = np.random.default_rng(2)
    for _ in range(500):
        kl, mean = f32(rng.random() * 5), f32(rng.random() + 1e-3)
        key = [int(rng.integers(0, 2 ** 63)) for _ in range(2)] + [int(rng.integers(0, 64))] + [int(rng.integers(0, 2 ** 63)) for _ in range(2)]
        assert _c_count(kl, mean, 1.0, *key) == 1
        assert _c_count(kl, 0.0, 0.5, *key) == 1 and _c_count(kl, 0.0, 0.0, *key) == 1


def test_rows_that_differ_only_in_own_draw_independently():
    """frac(w) = 0.5 (u = 0.5, kl = 2 mean: w = 1.5): two rows that differ only in `own` -- a row and one of its D4 copies --
    are two fair coins, so they disagree about half the time"""
    rng = np.random.default_rng(3)
    differ = ones = 0
    for i in range(4096):
        seed, game, own, own2, opp = (int(rng.integers(0, 2 ** 63)) for _ in range(5))
        ply = int(rng.integers(0, 64))
        a = _c_count(2.0, 1.0, 0.5, seed, game, ply, own, opp)
        b = _c_count(2.0, 1.0, 0.5, seed, game, ply, own2, opp)
        assert a == surprise_count(2.0, 1.0, 0.5, seed, game, ply, own, opp) and {a, b} <= {1, 2}
        differ += a != b
        ones += a == 1
    assert 0.4 < differ / 4096 < 0.6 and 0.4 < ones / 4096 < 0.6, (differ, ones)


def test_count_does_not_depend_on_anything_but_the_rows_content_and_refuses_a_bad_uniform_frac():
    L = _lib.lib()
    out = C.c_int32()
    for u in (-0.1, 1.5, float("nan")):
        assert L.bz_surprise_count(C.c_float(1.0), C.c_float(1.0), C.c_float(u), 0, 0, 0, 0, 0, C.byref(out)) == _lib.BZ_EINVAL
        assert b"uniform_frac" in L.bz_last_error()
    assert L.bz_surprise_count(C.c_float(1.0), C.c_float(1.0), C.c_float(0.5), 0, 0, 0, 0, 0, None) == _lib.BZ_EINVAL
    # a negative game id (int64) and a large ply are keyed as their unsigned bit patterns
    assert _c_count(0.75, 0.5, 0.5, 9, -5, 63, 1, 2) == surprise_count(0.75, 0.5, 0.5, 9, -5, 63, 1, 2)


def test_resample_twin_equals_the_scalar_restatement():
    rng = np.random.default_rng(4)
    for n in (1, 7, 300):
        kl = (rng.random(n) * rng.choice([0.0, 1e-3, 1.0, 30.0], n)).astype(np.float32)
        game, ply = rng.integers(0, 2 ** 40, n), rng.integers(0, 64, n).astype(np.int32)
        own, opp = rng.integers(0, 2 ** 63, n).astype(np.uint64), rng.integers(0, 2 ** 63, n).astype(np.uint64)
        for u in (0.0, 0.5, 1.0):
            count, idx, total, dropped, mean = resample_twin(kl, game, ply, own, opp, u, 77)
            assert _bits(mean) == _bits(surprise_mean(kl))
            want = [surprise_count(kl[i], mean, u, 77, int(game[i]), int(ply[i]), int(own[i]), int(opp[i])) for i in range(n)]
            assert list(count) == want and total == sum(want) and dropped == 0
            assert np.array_equal(idx, np.repeat(np.arange(n), want))
            if u == 1.0:
                assert np.array_equal(idx, np.arange(n))
        assert np.array_equal(resample_twin(np.zeros(n), game, ply, own, opp, 0.5, 1)[1], np.arange(n))  # mean 0: every row once
        _, cut, total, dropped, _ = resample_twin(kl, game, ply, own, opp, 0.5, 77, idx_cap=max(0, idx.size - 1))
        assert dropped == total - cut.size and cut.size == max(0, idx.size - 1)


def test_the_mean_is_the_exact_integer_mean():
    assert surprise_mean([0.5, 0.25, 0.0]) == f32(0.25)
    assert surprise_mean([2.0 ** -31] * 5) == 0                      # below the quantum: nothing surprising anywhere
    assert surprise_mean([np.nan, -1.0, 1.0]) == f32(1 / 3)           # cleaned first
    assert surprise_mean([500.0]) == KL_MAX
    kls = np.random.default_rng(5).random(1000).astype(np.float32)
    assert surprise_mean(kls) == surprise_mean(kls[::-1])            # order-independent by construction


# ---------------------------------------------------------------- the twins
def _plain_rows(kind, game, sims, **kw):
    """the rows of the feature twin WITHOUT the mixin: the mixin observes only"""
    b = dict(boards=boards(), **(dict(dir_alpha=0.3, dir_eps=0.25) if kw.get("noise") else {}))
    if kind == "plain":
        return Twin(game, "hash", **b).selfplay(3, sims, kw.get("temp_moves", 0), 0, 5)[0]
    if kind == "cap":
        return CapTwin(game, "hash", *kw["cap"], **b).selfplay(3, sims, kw.get("temp_moves", 0), 0, 5, slot=0)[0]
    if kind == "forced":
        return ForcedTwin(game, "hash", 2.0, prune=True, cap=kw.get("cap"), **b).selfplay(3, sims, kw.get("temp_moves", 0), 0, 5, slot=0)[0]
    return GumbelTwin(game, "hash", **b).selfplay(3, sims, kw.get("temp_moves", 0), 0, 5, slot=0)[0]


@pytest.mark.parametrize("kind,kw", [("plain", {}), ("plain", {"noise": True}), ("cap", {"cap": (4, 32768), "noise": True}),
                                     ("forced", {"noise": True}), ("gumbel", {"temp_moves": 3})])
def test_surprise_twin_observes_only_and_gives_a_kl_per_row(kind, kw):
    rows, kl, _ = surprise_games(kind, "ttt", 1, 24, seed=5, base=3, **kw)[0]
    ref = _plain_rows(kind, "ttt", 24, **kw)
    assert len(rows) == len(ref) == len(kl)
    for a, b in zip(rows, ref):
        assert a[0] == b[0] and a[1] == b[1] and a[3] == b[3] and a[4] == b[4] and np.array_equal(_bits(a[2]), _bits(b[2]))
    assert (kl >= 0).all() and (kl > 0).any() and np.isfinite(kl).all()


def test_surprise_twin_reads_the_prior_before_the_noise():
    """with Dirichlet noise the search's edges hold P' = (1 - eps) P + eps eta; the kl is against the raw P: equal to the kl
    computed from the noise-free expansion of the same positions, different from the one against P'"""
    tw = SurpriseTwin(Twin)("reversi4", "hash", boards=boards(), dir_alpha=0.3, dir_eps=0.25)
    noised, roots = {}, {}
    orig = Twin.root_noise

    def spy(self, root):
        orig(self, root)
        key = self.bits(root["b"], root["p"])
        noised[key], roots[key] = [f32(e["P"]) for e in root["edges"]], (root["b"], root["p"])
    Twin.root_noise = spy
    try:
        rows, _, _ = tw.selfplay(2, 16, 0, 0, 9)
    finally:
        Twin.root_noise = orig
    clean = Twin("reversi4", "hash", boards=boards())
    differs = 0
    for r in rows:
        key = (r[0], r[1])
        acts, prior = tw.raw[key]
        node = clean.new_node(*roots[key])
        clean.expand(node)  # the expansion's softmax of the position, whatever the noise did afterwards
        assert acts == [e["a"] for e in node["edges"]] and np.array_equal(_bits(prior), _bits([e["P"] for e in node["edges"]]))
        differs += any(_bits(x) != _bits(y) for x, y in zip(prior, noised[key]))
    assert differs > 0
    kl_raw = tw.kl_rows(rows)
    kl_noised = np.array([surprise_kl([r[2][a] for a in tw.raw[(r[0], r[1])][0]], noised[(r[0], r[1])]) for r in rows], np.float32)
    assert not np.array_equal(_bits(kl_raw), _bits(kl_noised))


def test_surprise_twin_under_subtree_reuse_and_a_forced_pass_root():
    rows, kl, _ = surprise_games("plain", "reversi4", 3, 16, seed=1, reuse=True)[1]
    assert len(rows) == len(kl) > 0 and (kl >= 0).all()
    # a one-edge root (the pass): pi = (1), P = (1): kl = 0
    assert surprise_kl([f32(1.0)], [f32(1.0)]) == 0


# ---------------------------------------------------------------- buffer size and Python validation
def test_surprise_bytes_is_the_stated_layout():
    L = _lib.lib()
    al = lambda x: (x + 255) // 256 * 256  # noqa: E731
    for game, maxch in ((0, 9), (1, 34), (2, 34), (3, 34)):
        for B in (1, 4, 33, 64, 4096):
            for rounds in (1, 3):
                cfg = _cfg(game, B, 8)
                cfg.rounds, cfg.t_max = rounds, 9 if game == 0 else 64
                want = al(B * maxch * 4) + al(B * 8) + al(rounds * B * cfg.t_max * 4)
                assert L.bz_engine_surprise_bytes(C.byref(cfg)) == want, (game, B, rounds)
    # nothing the engine accepts is refused: subtree reuse, K > 1, the caches, Dirichlet noise
    for cfg in (_cfg(flags=_lib.ENGINE_REUSE_SUBTREE), _cfg(K=8), _cfg(flags=_lib.ENGINE_EVAL_CACHE | _lib.ENGINE_EVAL_CACHE_CARRY)):
        assert L.bz_engine_surprise_bytes(C.byref(cfg)) > 0
    assert L.bz_engine_surprise_bytes(None) == -1 and b"bz_engine_surprise_bytes" in L.bz_last_error()
    bad = _cfg(sims=9000)
    assert L.bz_engine_surprise_bytes(C.byref(bad)) == -1
    assert L.bz_engine_set_surprise(None, None, 0, None) == _lib.BZ_EINVAL and b"bz_engine_set_surprise" in L.bz_last_error()
    assert L.bz_engine_pack_surprise(None, None, 1, 0, None) == _lib.BZ_EINVAL
    assert L.bz_surprise_resample_workspace_bytes(-1) == -1 and L.bz_surprise_resample_workspace_bytes((1 << 26) + 1) == -1
    assert L.bz_surprise_resample_workspace_bytes(0) == 256 and L.bz_surprise_resample_workspace_bytes(1) == 768
    assert L.bz_surprise_resample_workspace_bytes(1 << 26) == 256 + (1 << 16) * 12
    assert L.bz_surprise_resample(None, None, None, None, None, (1 << 26) + 1, C.c_float(0.5), 0, None, 0, None, None, 0, None, None) == _lib.BZ_EINVAL
    assert b"2^26" in L.bz_last_error()


def _examples(n, kl=True, seed=0):
    from betazero_amd.engine import Examples
    g = np.random.default_rng(seed)
    return Examples(g.integers(0, 2 ** 62, n).astype(np.uint64), g.integers(0, 2 ** 62, n).astype(np.uint64),
                    g.random((n, 65)).astype(np.float32), g.integers(-1, 2, n).astype(np.int8), np.ones(n, np.int8),
                    np.zeros(n, np.uint8), np.arange(n), np.zeros(n, np.int32), 8, **({"kl": g.random(n).astype(np.float32)} if kl else {}))


def test_examples_carry_kl_through_concat_select_and_the_host_round_trip():
    from betazero_amd.engine import DeviceExamples, Examples, concat_device_examples, concat_examples
    from betazero_amd.train import select_rows
    a, b, c = _examples(5, seed=1), _examples(3, seed=2), _examples(4, kl=False)
    assert c.kl is None and Examples(*[getattr(c, f) for f in ("own", "opp", "pi", "z", "mover", "act", "game", "ply", "size")]).kl is None
    ab = concat_examples([a, b])
    assert np.array_equal(ab.kl, np.concatenate([a.kl, b.kl])) and len(ab) == 8
    assert concat_examples([c, c]).kl is None
    with pytest.raises(ValueError, match="kl"):
        concat_examples([a, c])
    da, db, dc = (DeviceExamples.from_host(x, "cpu") for x in (a, b, c))
    assert da.kl.dtype.is_floating_point and dc.kl is None
    dab = concat_device_examples([da, db])
    assert np.array_equal(dab.kl.numpy(), ab.kl) and concat_device_examples([dc, dc]).kl is None
    with pytest.raises(ValueError, match="kl"):
        concat_device_examples([dc, da])
    import torch
    idx = torch.tensor([7, 0, 0, 3])
    sel = select_rows(dab, idx)
    assert np.array_equal(sel.kl.numpy(), ab.kl[[7, 0, 0, 3]]) and np.array_equal(sel.own.numpy().view(np.uint64), ab.own[[7, 0, 0, 3]])
    assert select_rows(dc, torch.tensor([1])).kl is None
    back = dab.cpu()
    assert np.array_equal(back.kl, ab.kl) and back.kl.dtype == np.float32 and dc.cpu().kl is None


def test_surprise_resample_refuses_bad_arguments_before_touching_a_device(monkeypatch):
    from betazero_amd import surprise
    from betazero_amd.engine import DeviceExamples

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(_lib, "lib", no_device)
    with_kl, without = DeviceExamples.from_host(_examples(4), "cpu"), DeviceExamples.from_host(_examples(4, kl=False), "cpu")
    with pytest.raises(ValueError, match="no kl"):
        surprise.surprise_resample(without)
    for u in (-0.01, 1.01, float("nan"), "0.5", None, True):
        with pytest.raises(ValueError, match="uniform_frac"):
            surprise.surprise_resample(with_kl, uniform_frac=u)
    with pytest.raises(ValueError, match="GPU"):
        surprise.surprise_resample(with_kl)  # valid arguments, host tensors: refused too, still before any library call


def test_python_refuses_a_surprise_that_is_no_bool_before_touching_a_device(monkeypatch):
    from betazero_amd import engine

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(_lib, "require_gpu", no_device)
    for bad in (1, "yes", None, 0.5):
        with pytest.raises(ValueError, match="surprise"):
            engine.SelfPlayEngine("reversi", 4, 8, surprise=bad)
