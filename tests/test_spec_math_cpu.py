"""The float primitives of csrc/bz_math.h as the HOST build computes them (bz_spec_probe, where = host):
equal to their independent restatements (oracle/py_twin.py, oracle/bz_oracle.c) bit for bit, to IEEE for sqrt and division,
accurate against float64 numpy, and still what tests/golden/spec_math.npz recorded.  tests/test_gpu_spec_math.py pins the
gfx950 build to the same fixture.  Runs on CPU; "equal" = the same bits, every NaN counted as one value."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import oracle as orc
from oracle import spec_math as sm

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import py_twin  # noqa: E402

G = os.path.join(os.path.dirname(__file__), "golden")
f32, u32, u64 = np.float32, np.uint32, np.uint64


def _pat(*bits):
    return np.array(bits, u32).view(f32)


def _around(x, k=1):
    """the float32 x and its k neighbours on either side"""
    b = int(np.array([x], f32).view(u32)[0])
    return _pat(*range(b - k, b + k + 1))


def _expf_ties():
    """the arguments around which n = floor(x * 1.44269504f + 0.5f) of expf_spec steps from n - 1 to n, n = 0, -1, -63, -125"""
    return np.concatenate([_around(f32((n - 0.5) / 1.44269504), 2) for n in (0, -1, -63, -125)])


NANS = _pat(0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001)  # quiet and signalling, positive and negative
# the edge list, shared with tests/test_gpu_spec_math.py
EDGES = np.concatenate([
    _pat(0x00000000, 0x80000000),                          # +-0
    _pat(0x00000001, 0x007FFFFF),                          # the smallest and the largest denormal
    _around(_pat(0x00800000)[0]),                          # FLT_MIN and its neighbours
    _around(f32(1.0)),
    _around(f32(1.41421356)),                              # the branch in logf_spec
    _around(f32(-87.0)), np.array([-87.3], f32),           # the cut-off of expf_spec
    _expf_ties(),
    _pat(0x7F7FFFFF, 0x7F800000, 0xFF800000),              # FLT_MAX, +-inf
    NANS,
])
# fdiv, additionally: quotients in the denormal range (exact, rounded, rounding up to FLT_MIN, underflow to 0) and around
# the overflow edge (just below, FLT_MAX exactly, rounding to inf)
FDIV_EXTRA = np.array([
    (_pat(0x00800000)[0], 2.0), (_pat(0x00800000)[0], 3.0), (_pat(0x00800001)[0], 2.0), (_pat(0x00FFFFFF)[0], 2.0),
    (1e-30, 1e10), (1.0, _pat(0x7F7FFFFF)[0]), (3.0, _pat(0x7F7FFFFF)[0]), (_pat(0x00000001)[0], 2.0), (_pat(0x00000003)[0], 2.0),
    (_pat(0x00000001)[0], 3.0), (1e-20, 1e25), (1e-20, 1e26),
    (_pat(0x7F7FFFFF)[0], 1.0), (_pat(0x7F7FFFFF)[0], _pat(0x3F7FFFFF)[0]), (_pat(0x7F7FFFFF)[0], _pat(0x3F800001)[0]),
    (_pat(0x7F7FFFFF)[0], 0.5), (1e20, 1e-18), (1e20, 1e-19), (_pat(0x7F000000)[0], _pat(0x3EFFFFFF)[0]), (-1e20, 1e-19),
], f32)


def _mix64(x):
    x = np.asarray(x, u64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> u64(33); x *= u64(0xFF51AFD7ED558CCD)
        x ^= x >> u64(33); x *= u64(0xC4CEB9FE1A85EC53)
        x ^= x >> u64(33)
    return x


def counter_u64(n, key):
    """n 64-bit words from a counter, the same on every run"""
    return _mix64(np.arange(n, dtype=u64) + u64(key << 40))


def fdiv_pairs():
    """the edge list crossed with itself, the denormal / overflow extras, and 2^20 counter-generated pairs of patterns"""
    w = counter_u64(1 << 20, 1)
    ea, eb = np.meshgrid(EDGES, EDGES, indexing="ij")
    a = np.concatenate([ea.ravel(), FDIV_EXTRA[:, 0], (w >> u64(32)).astype(u32).view(f32)])
    b = np.concatenate([eb.ravel(), FDIV_EXTRA[:, 1], w.astype(u32).view(f32)])
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def gamma_inputs():
    """alpha in {1, 0.5, 0.3, 0.03} x 64 edges x 4096 (game, ply) pairs -> alpha float32 [n], (seed, game, ply, edge) uint64 [n][4]"""
    w = counter_u64(4096, 2)
    alpha, edge, j = np.meshgrid(np.array([1.0, 0.5, 0.3, 0.03], f32), np.arange(64, dtype=u64), np.arange(4096), indexing="ij")
    j = j.ravel()
    key = np.stack([np.full(j.size, 3, u64), w[j] >> u64(20), w[j] & u64(63), edge.ravel()], axis=1)
    return np.ascontiguousarray(alpha.ravel()), np.ascontiguousarray(key)


def same(a, b):
    return np.array_equal(sm.canon(a), sm.canon(b))


def first_difference(x, a, b):
    d = np.nonzero(sm.canon(a) != sm.canon(b))[0]
    return None if d.size == 0 else (d.size, int(d[0]), x[d[0]], hex(int(a.view(u32)[d[0]])), hex(int(b.view(u32)[d[0]])))


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(os.path.join(G, "spec_math.npz")))


# ---------------------------------------------------------------- 1. host build == the restatements
def _samples():
    rng = np.random.default_rng(5)
    neg = -np.concatenate([rng.random(2000, dtype=f32) * f32(87.5), rng.random(1000, dtype=f32) * f32(4.0),
                           f32(2.0) ** rng.integers(-40, 0, 500).astype(f32)]).astype(f32)
    pos = np.concatenate([rng.random(2000, dtype=f32) + f32(1e-7),
                          (f32(2.0) ** rng.integers(-126, 128, 1500).astype(f32) * (1 + rng.random(1500, dtype=f32))).astype(f32)])
    return neg, pos


def test_host_expf_equals_twin_and_oracle():
    """expf_spec on its domain (x <= 0, NaN): the numpy twin and the C oracle restate the host build bit for bit"""
    neg, _ = _samples()
    edges = EDGES[(EDGES <= 0) | np.isnan(EDGES)]
    assert edges.size >= 30 and np.isnan(edges).sum() == 4
    x = np.concatenate([neg, edges])
    got = sm.host_map("expf_spec", x)
    with np.errstate(all="ignore"):
        twin = np.array([py_twin.expf_spec(v) for v in x], f32)
        oracle = np.array([orc.expf(v) for v in x], f32)
    assert first_difference(x, got, twin) is None and first_difference(x, got, oracle) is None
    # the tie arguments of the edge list do straddle the step of n they are there for
    for n in (0, -1, -63, -125):
        t = _around(f32((n - 0.5) / 1.44269504), 2) * f32(1.44269504)
        assert set(np.floor(t + f32(0.5)).tolist()) == {n - 1, n}, n


def test_host_tanhf_equals_oracle():
    rng = np.random.default_rng(6)
    x = np.concatenate([(rng.random(3000, dtype=f32) - f32(0.5)) * f32(24.0), (rng.random(1000, dtype=f32) - f32(0.5)) * f32(1e-3), EDGES])
    got = sm.host_map("tanhf_spec", x)
    assert first_difference(x, got, np.array([orc.tanhf(v) for v in x], f32)) is None


def test_host_logf_equals_twin_and_oracle():
    """logf_spec on positive finite inputs (normals: its domain; denormals: the same bit manipulation everywhere)"""
    _, pos = _samples()
    edges = EDGES[(EDGES > 0) & np.isfinite(EDGES)]
    x = np.concatenate([pos, edges])
    got = sm.host_map("logf_spec", x)
    assert first_difference(x, got, np.array([py_twin.logf_spec(v) for v in x], f32)) is None
    assert first_difference(x, got, np.array([orc.logf(v) for v in x], f32)) is None


def test_host_u01_hashes_and_gamma_equal_twin_and_oracle():
    w = counter_u64(3000, 3)
    bits = np.concatenate([w, np.array([0, (1 << 64) - 1, 1 << 41, (1 << 41) - 1, ((1 << 23) - 1) << 41], u64)])
    got = sm.host_map("u01_spec", bits)
    assert same(got, np.array([py_twin.u01_spec(int(b)) for b in bits], f32))
    assert got.min() == f32(0.5 / 8388608.0) and got.max() == f32(1.0) - f32(0.5 / 8388608.0)   # inside (0, 1)
    # hash_logit / hash_value: the hash evaluator of the twin and of the oracle, position by position
    own, opp = counter_u64(40, 4), counter_u64(40, 5)
    for o, p in zip(own.tolist(), opp.tolist()):
        h = py_twin.mix64(((o * 0x9E3779B97F4A7C15) & py_twin.M64) ^ py_twin.mix64((p + 0x632BE59BD9B4E019) & py_twin.M64))
        hh = np.full(65, h, u64)
        lg = sm.host_map("hash_logit", hh, np.arange(65, dtype=u64))
        v = sm.host_map("hash_value", hh[:1])
        olg, ov = orc.eval_hash(o, p, 65)
        tlg, tv = py_twin.eval_hash(o, p, 65)
        assert same(lg, olg) and same(v, np.array([ov], f32))
        assert same(lg, np.array(tlg, f32)) and same(v, np.array([tv], f32))
    alpha, key = gamma_inputs()
    g = sm.host_map("gamma_spec", alpha, key)
    assert np.isfinite(g).all() and (g >= 0).all()
    for a in (1.0, 0.5, 0.3, 0.03):
        assert abs(g[alpha == f32(a)].mean() - a) < 0.01 * max(a, 0.2)    # 262,144 variates of mean alpha, variance alpha
    for i in np.linspace(0, alpha.size - 1, 1500).astype(int).tolist():
        a, (s, gid, ply, e) = alpha[i], key[i].tolist()
        assert g[i].view(u32) == orc.gamma(a, s, gid, ply, e).view(u32), (i, a, key[i])
        if i % 5 == 0:
            assert g[i].view(u32) == py_twin.gamma_spec(a, s, gid, ply, e).view(u32), (i, a, key[i])


# ---------------------------------------------------------------- 2. host build vs IEEE
def sqrt_inputs():
    """the edge list; every integer 1 .. 8189 (sq of the PUCT selection, the LDS table of k_tree_step); 2^20 products
    (k P) SigmaN, k in {0.5, 2, 1e-6}, P a softmax of hash logits, SigmaN in 1 .. 8189 (the argument of forced_nf)"""
    n = 1 << 20
    h = counter_u64(n // 64, 6)
    q = _mix64((h[:, None] + np.arange(64, dtype=u64)[None, :] * u64(0xD6E8FEB86659FD93)))
    lg = ((q >> u64(40)).astype(np.int64) - (1 << 23)).astype(np.float64) / 4194304.0
    p = np.exp(lg - lg.max(axis=1, keepdims=True))
    p = (p / p.sum(axis=1, keepdims=True)).astype(f32).ravel()
    i = np.arange(n, dtype=np.int64)
    k = np.array([0.5, 2.0, 1e-6], f32)[i % 3]
    sn = (1 + (i * 2654435761) % 8189).astype(f32)
    return np.concatenate([EDGES, np.arange(1, 8190, dtype=f32), (k * p) * sn])


def test_host_fsqrt_and_fdiv_are_ieee():
    """tolerance 0 against numpy's float32 sqrt and division (correctly rounded), NaN compares as NaN"""
    x = sqrt_inputs()
    with np.errstate(all="ignore"):
        assert first_difference(x, sm.host_map("fsqrt", x), np.sqrt(x)) is None
        a, b = fdiv_pairs()
        assert a.size == EDGES.size ** 2 + len(FDIV_EXTRA) + (1 << 20)
        q = a / b
        assert first_difference(np.stack([a, b], 1), sm.host_map("fdiv", a, b), q) is None
    # the extras do land where they are meant to
    qe = q[EDGES.size ** 2:EDGES.size ** 2 + len(FDIV_EXTRA)]
    sub = (np.abs(qe) < _pat(0x00800000)[0]) & (qe != 0)
    assert sub.sum() >= 6 and (qe == 0).sum() >= 1 and np.isinf(qe).sum() >= 3 and (np.abs(qe) == _pat(0x7F7FFFFF)[0]).sum() >= 1


# ---------------------------------------------------------------- 3. accuracy against float64 numpy
# the worst cases measured over the entire domains
WORST = {"expf_spec": 0xC26FCD57, "logf_spec": 0x403324E4, "tanhf_spec": 0x3F9FB2D5}


def _accuracy_chunks(op):
    ch = sm.spread(sm.ACCURACY[op])
    for c in sm.chunks(sm.ACCURACY[op]):
        if c[0] <= WORST[op] < c[1] and c not in ch:
            ch.append(c)
    return ch


@pytest.mark.parametrize("op", list(sm.ACCURACY))
def test_accuracy_against_float64(op, fixture):
    """bounds: expf_spec relative error <= 1e-7 on [-87, 0]; logf_spec |err| <= 1e-7 max(1, |ln x|) on positive normals;
    tanhf_spec absolute error <= 1e-7 on every finite input.  Checked on 16 chunks of 2^24 patterns spread over the domain, on
    the chunk of the worst case, and on the exhaustive maximum the fixture recorded (the host build is bit-reproducible: the
    margin is for the float64 reference's own last digit only)."""
    with ThreadPoolExecutor(4) as ex:
        got = list(ex.map(lambda c: sm.chunk_max_error(op, *c), _accuracy_chunks(op)))
    worst, at = max(got, key=lambda r: (r[0], -r[1]))
    rec, rec_at = float(fixture[op + "_max_err"]), int(fixture[op + "_max_at"])
    print(op, "max error on the sampled chunks %.4e at 0x%08X; exhaustive (fixture) %.4e at 0x%08X" % (worst, at, rec, rec_at))
    assert worst <= sm.BOUND[op] and rec <= sm.BOUND[op]
    # the sampled chunks include the worst case's: they reproduce the recorded maximum
    assert at == rec_at == WORST[op] and worst == rec


# ---------------------------------------------------------------- 4. the fixture is not stale
@pytest.mark.parametrize("op", list(sm.SWEEPS))
def test_fixture_checksums_are_the_host_builds(op, fixture):
    """16 of the fixture's chunk checksums, spread over the op's sweep domain, re-derived from the host build"""
    allc = sm.chunks(sm.SWEEPS[op])
    assert fixture[op + "_lo"].tolist() == [c[0] for c in allc] and fixture[op + "_hi"].tolist() == [c[1] for c in allc]
    pick = sm.spread(sm.SWEEPS[op])
    assert len(pick) == 16
    with ThreadPoolExecutor(4) as ex:
        got = list(ex.map(lambda c: int(sm.host_sweep(op, *c)[0]), pick))
    assert got == [int(fixture[op + "_sum"][allc.index(c)]) for c in pick]


def test_sweep_checksum_is_what_the_header_says():
    """the checksum against its definition in numpy, on ranges that straddle chunk borders and hold NaNs"""
    for op, lo, hi in (("fsqrt", 0x7F7FFF00, 0x80000100), ("tanhf_spec", 0x00FFFFF0, 0x01000010), ("expf_spec", 0xFEFFFFFF, 0xFF800001)):
        x = sm.patterns(lo, hi)
        y = sm.canon(sm.host_map(op, x)).astype(u64)
        term = _mix64((np.arange(lo, hi, dtype=u64) << u64(32)) | y)
        want = [int(term[(np.arange(lo, hi) >> 24) == c].sum(dtype=u64)) for c in range(lo >> 24, ((hi - 1) >> 24) + 1)]
        assert sm.host_sweep(op, lo, hi).tolist() == want


# ---------------------------------------------------------------- 5. NaN in, NaN out
def test_nan_in_nan_out():
    """run-time NaNs through the probe (the conversion (int)n of expf_spec is undefined for a NaN: the NaN path is explicit)"""
    for op in ("expf_spec", "tanhf_spec"):
        assert np.isnan(sm.host_map(op, NANS)).all(), op
    assert np.isnan(sm.host_map("fsqrt", NANS)).all() and np.isnan(sm.host_map("fdiv", NANS, np.ones(4, f32))).all()
    assert np.isnan(orc.expf(np.nan)) and np.isnan(orc.tanhf(np.nan)) and np.isnan(py_twin.expf_spec(np.nan))


def test_probe_refuses_bad_arguments():
    from betazero_amd import _lib
    L, out = _lib.lib(), np.zeros(4, u64)
    assert L.bz_spec_probe(9, 0, 0, out.ctypes.data, None, 1, 0, 0, out.ctypes.data, None) == _lib.BZ_EINVAL
    assert L.bz_spec_probe(0, 2, 0, out.ctypes.data, None, 1, 0, 0, out.ctypes.data, None) == _lib.BZ_EINVAL
    assert L.bz_spec_probe(4, 0, 0, out.ctypes.data, None, 1, 0, 0, out.ctypes.data, None) == _lib.BZ_EINVAL      # fdiv without b
    assert L.bz_spec_probe(4, 0, 1, None, None, 0, 0, 16, out.ctypes.data, None) == _lib.BZ_EINVAL                # fdiv has no sweep
    assert L.bz_spec_probe(3, 0, 1, None, None, 0, 16, 16, out.ctypes.data, None) == _lib.BZ_EINVAL               # empty range
    assert L.bz_spec_probe(3, 0, 1, None, None, 0, 0, (1 << 32) + 1, out.ctypes.data, None) == _lib.BZ_EINVAL
    assert L.bz_spec_probe(3, 0, 1, None, None, 0, 0, 16, None, None) == _lib.BZ_EINVAL
