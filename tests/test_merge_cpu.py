"""Position averaging without a GPU: bz_merge_group -- the function the kernels run -- against a twin written
here with Python integers (what tests/test_gpu_merge.py pins the kernels to), the refusals of the C entry points, of
merge_positions / merged_repeats and of tools/az_loop.py, and the ABI.  "Equal" = bit for bit."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from betazero_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT, KL = 32, 24  # the fixed-point bits of pi / value / q and of kl


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ---------------------------------------------------------------- the twin
def fix(x, lo, hi, k):
    """(int64)(x * 2^k), truncating, as a Python integer; None when x is NaN or outside [lo, hi]"""
    x = np.float32(x)
    if not (lo <= x <= hi):
        return None
    return int(x * np.float32(2.0 ** k))  # (the product is exact in binary32; int() truncates)


def mean(S, n, k):
    """M = floor((2 S + n) / (2 n)) in integers, then (float)((double)M * 2^-k)"""
    return np.float32(np.float64((2 * S + n) // (2 * n)) * 2.0 ** -k)


def group_twin(pi, val, q=None, kl=None):
    """one group's rows (pi [n, NA]; val, q, kl [n]) -> (pi, vt, z, q, kl, bad) of the merged row"""
    pi, val = np.asarray(pi, np.float32), np.asarray(val, np.float32)
    n, na = pi.shape
    S, bad = [0] * (na + 3), 0
    for r in range(n):
        f = [fix(x, 0.0, 1.0, UNIT) for x in pi[r]] + [fix(val[r], -1.0, 1.0, UNIT), 0 if q is None else fix(q[r], -1.0, 1.0, UNIT),
                                                       0 if kl is None else fix(kl[r], 0.0, 128.0, KL)]
        if any(x is None for x in f):
            bad += 1
            continue
        S = [a + b for a, b in zip(S, f)]
    z = (S[na] > 0) - (S[na] < 0)
    if n == 1:
        return pi[0].copy(), val[0], z, None if q is None else np.float32(q[0]), None if kl is None else np.float32(kl[0]), bad
    return (np.array([mean(s, n, UNIT) for s in S[:na]], np.float32), mean(S[na], n, UNIT), z,
            None if q is None else mean(S[na + 1], n, UNIT), None if kl is None else mean(S[na + 2], n, KL), bad)


def merge_twin(ex):
    """merge_positions on host Examples in plain Python: (columns of the merged rows as a dict, counts, bad rows).  Groups in
    the order of their first occurrence; mover, act, game, ply of the first occurrence."""
    groups = {}
    for i, key in enumerate(zip(ex.own.tolist(), ex.opp.tolist())):
        groups.setdefault(key, []).append(i)
    val = np.asarray(ex.z, np.float32) if ex.vt is None else np.asarray(ex.vt, np.float32)
    na = ex.pi.shape[1]
    out = {k: [] for k in ("own", "opp", "pi", "z", "mover", "act", "game", "ply", "vt", "q", "kl")}
    count, bad = [], 0
    for rows in groups.values():
        pi, vt, z, q, kl, b = group_twin(ex.pi[rows], val[rows], None if ex.q is None else ex.q[rows], None if ex.kl is None else ex.kl[rows])
        h = rows[0]
        for k, v in (("own", ex.own[h]), ("opp", ex.opp[h]), ("pi", pi), ("z", z), ("mover", ex.mover[h]), ("act", ex.act[h]),
                     ("game", ex.game[h]), ("ply", ex.ply[h]), ("vt", vt), ("q", q), ("kl", kl)):
            out[k].append(v)
        count.append(len(rows))
        bad += b
    cols = {"own": np.array(out["own"], np.uint64), "opp": np.array(out["opp"], np.uint64),
            "pi": np.array(out["pi"], np.float32).reshape(-1, na), "z": np.array(out["z"], np.int8),
            "mover": np.array(out["mover"], np.int8), "act": np.array(out["act"], np.uint8), "game": np.array(out["game"], np.int64),
            "ply": np.array(out["ply"], np.int32), "vt": np.array(out["vt"], np.float32),
            "q": None if ex.q is None else np.array(out["q"], np.float32), "kl": None if ex.kl is None else np.array(out["kl"], np.float32)}
    return cols, np.array(count, np.int32), bad


# ---------------------------------------------------------------- bz_merge_group
def _c_group(pi, z, vt=None, q=None, kl=None):
    pi = np.ascontiguousarray(pi, np.float32)
    n, na = pi.shape
    z = np.ascontiguousarray(z, np.int8)
    opt = [None if a is None else np.ascontiguousarray(a, np.float32) for a in (vt, q, kl)]
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    po = np.full(na + 2, -7.0, np.float32)
    vo, qo, ko, zo, bad = C.c_float(-7.0), C.c_float(-7.0), C.c_float(-7.0), C.c_int8(-7), C.c_int32(-7)
    rc = _lib.lib().bz_merge_group(pi.ctypes.data, p(opt[0]), z.ctypes.data, p(opt[1]), p(opt[2]), n, na, po.ctypes.data, C.addressof(vo),
                                   C.addressof(zo), C.addressof(qo), C.addressof(ko), C.addressof(bad))
    assert rc == 0, _lib.lib().bz_last_error()
    assert (po[na:] == -7.0).all()  # nothing written behind the row
    return (po[:na], np.float32(vo.value), zo.value, None if q is None else np.float32(qo.value),
            None if kl is None else np.float32(ko.value), bad.value)


def _same(got, want):
    assert np.array_equal(_bits(got[0]), _bits(want[0])), (got[0], want[0])
    assert _bits(got[1]) == _bits(want[1]) and got[2] == want[2] and got[5] == want[5], (got[1:], want[1:])
    for g, w in zip(got[3:5], want[3:5]):
        assert (g is None and w is None) or _bits(g) == _bits(w), (g, w)


def _random_group(g, n, na, vt=True, q=True, kl=True, sparse=False):
    """n rows of one position: pi rows that sum to 1 in fp32 arithmetic (with exact zeros, and whole zero columns when sparse),
    z in {-1, 0, 1}, vt / q in [-1, 1], kl in [0, 128]"""
    pi = g.random((n, na)).astype(np.float32) ** 3
    pi[g.random((n, na)) < 0.3] = 0.0
    if sparse:
        pi[:, g.random(na) < 0.6] = 0.0
    pi[:, 0] += np.float32(1e-3)  # (no all-zero row)
    pi = (pi / pi.sum(1, keepdims=True, dtype=np.float32)).astype(np.float32)
    z = g.integers(-1, 2, n).astype(np.int8)
    return (pi, z, (g.random(n) * 2 - 1).astype(np.float32) if vt else None, (g.random(n) * 2 - 1).astype(np.float32) if q else None,
            (g.random(n) * g.choice([0.01, 3.0, 128.0])).astype(np.float32) if kl else None)


def _val(z, vt):
    return np.asarray(z, np.float32) if vt is None else vt


@pytest.mark.parametrize("na", [9, 65])
@pytest.mark.parametrize("n", [1, 2, 3, 1000])
def test_group_equals_the_python_integer_twin(na, n):
    g = np.random.default_rng(100 * na + n)
    for trial in range(3 if n == 1000 else 40):
        have = [bool(trial & 1), bool(trial & 2), bool(trial & 4)]  # vt / q / kl given and absent
        pi, z, vt, q, kl = _random_group(g, n, na, *have, sparse=trial % 5 == 0)
        _same(_c_group(pi, z, vt, q, kl), group_twin(pi, _val(z, vt), q, kl))


@pytest.mark.parametrize("na", [9, 65])
def test_a_single_row_is_copied_verbatim(na):
    """values the fixed point would truncate -- pi far below 2^-32's grid, denormals, -0.0 -- come back as they went in"""
    g = np.random.default_rng(na)
    pi = (g.random((1, na)) * 2.0 ** -g.integers(0, 60, (1, na))).astype(np.float32)
    pi[0, :4] = [1e-12, 2.0 ** -40, 1e-45, -0.0]
    vt, q, kl = np.array([-3e-11], np.float32), np.array([2.0 ** -35], np.float32), np.array([1e-9], np.float32)
    z = np.array([1], np.int8)
    got = _c_group(pi, z, vt, q, kl)
    assert np.array_equal(_bits(got[0]), _bits(pi[0])) and _bits(got[1]) == _bits(vt[0]) and _bits(got[3]) == _bits(q[0])
    assert _bits(got[4]) == _bits(kl[0]) and got[2] == 0 and got[5] == 0   # z = the sign of the value SUM: -3e-11 * 2^32 truncates to 0
    _same(got, group_twin(pi, vt, q, kl))
    for zz in (-1, 0, 1):  # without vt the value input is (float)z
        got = _c_group(pi, [zz])
        assert got[1] == np.float32(zz) and got[2] == zz and got[3] is None and got[4] is None
        _same(got, group_twin(pi, np.array([zz], np.float32)))


@pytest.mark.parametrize("na", [9, 65])
def test_two_rows_round_half_up_also_for_negative_sums(na):
    u = np.float32(2.0 ** -32)
    pi = np.zeros((2, na), np.float32)
    pi[0, 0], pi[1, 0] = 5 * u, 6 * u          # sum 11: 5.5 -> 6
    pi[0, 1], pi[1, 1] = 0.5, 0.5 + 2.0 ** -24  # the mean needs a bit more than binary32 has: the one rounding, double -> float
    pi[0, 2], pi[1, 2] = 1.0, 1.0
    vt = np.array([-3 * u, -2 * u], np.float32)  # sum -5: -2.5 -> -2 (half up), not -3
    q = np.array([-3 * u, -4 * u], np.float32)   # sum -7: -3.5 -> -3
    kl = np.array([128.0, 127.0], np.float32)
    got = _c_group(pi, [0, 0], vt, q, kl)
    assert got[0][0] == 6 * u and got[0][2] == 1.0 and got[1] == -2 * u and got[3] == -3 * u and got[4] == np.float32(127.5) and got[2] == -1
    assert got[0][1] == np.float32(0.5 + 2.0 ** -25) and not got[0][3:].any()
    _same(got, group_twin(pi, vt, q, kl))
    got = _c_group(pi, [1, -1])  # z +1 and -1: the mean value is 0, and so is its sign
    assert got[1] == 0.0 and got[2] == 0
    got = _c_group(pi, [-1, 0])  # -0.5 exactly
    assert got[1] == -0.5 and got[2] == -1


@pytest.mark.parametrize("na", [9, 65])
def test_a_permuted_group_gives_the_same_bits(na):
    g = np.random.default_rng(7 + na)
    pi, z, vt, q, kl = _random_group(g, 257, na)
    want = _c_group(pi, z, vt, q, kl)
    for _ in range(5):
        p = g.permutation(257)
        _same(_c_group(pi[p], z[p], vt[p], q[p], kl[p]), want)


def test_bad_rows_are_reported_and_not_summed():
    g = np.random.default_rng(3)
    pi, z, vt, q, kl = _random_group(g, 12, 9)
    clean = [0, 1, 2, 4, 6, 8, 10]
    pi[3, 2], pi[5, 0], pi[7, 8] = np.nan, -1e-9, 1.0 + 2.0 ** -23
    vt[9], q[11], kl[3] = 2.0, -np.inf, 129.0     # (row 3 holds two bad values: one row)
    got = _c_group(pi, z, vt, q, kl)
    want = group_twin(pi, vt, q, kl)
    assert got[5] == want[5] == 5
    _same(got, want)
    # ... the sums are those of the clean rows, over the group's 12 rows
    S = sum(fix(x, 0, 1, UNIT) for x in pi[clean, 1])
    assert _bits(got[0][1]) == _bits(mean(S, 12, UNIT))
    for bad in (np.nan, np.inf, 1.5, -1.5):
        assert _c_group(pi[:1], z[:1], np.array([bad], np.float32))[5] == 1
    assert _c_group(pi[:1], z[:1], None, None, np.array([-0.5], np.float32))[5] == 1


def test_group_refuses_bad_arguments_with_a_message():
    L = _lib.lib()
    pi, z, out = np.zeros((2, 9), np.float32), np.zeros(2, np.int8), np.zeros(16, np.float32)
    p, o = pi.ctypes.data, out.ctypes.data
    ok = [p, p, z.ctypes.data, p, p, 2, 9, o, o, o, o, o, o]
    assert L.bz_merge_group(*ok) == 0
    for i, bad in ((0, None), (2, None), (7, None), (8, None), (9, None), (12, None), (10, None), (11, None), (5, 0), (5, -1),
                   (5, (1 << 26) + 1), (6, 8), (6, 10), (6, 64), (6, 66), (6, 0)):
        args = list(ok)
        args[i] = bad
        assert L.bz_merge_group(*args) == _lib.BZ_EINVAL and b"bz_merge_group" in L.bz_last_error(), (i, bad)
    args = list(ok)
    args[1] = args[3] = args[4] = args[10] = args[11] = None  # vt, q, kl absent: their outputs may be absent too
    assert L.bz_merge_group(*args) == 0


def test_workspace_bytes_and_the_device_entry_point_refuse_before_a_launch():
    L = _lib.lib()
    for na in (9, 65):
        for n in (0, 1, 63, 4099, 1 << 26):
            assert L.bz_merge_workspace_bytes(n, na) == (n * (na + 3) * 8 + 255) // 256 * 256
    for n, na in ((-1, 9), ((1 << 26) + 1, 65), (4, 10), (4, 0)):
        assert L.bz_merge_workspace_bytes(n, na) == -1 and b"bz_merge_workspace_bytes" in L.bz_last_error()
    a = np.zeros(96, np.int64)
    p = a.ctypes.data + ((-a.ctypes.data) & 255)  # 256-byte aligned, as the workspace must be
    rows = _lib.MergeRows(*([p] * 11))
    ok = [C.byref(rows), 4, 9, p, p, p, p, p, p, p, 1 << 20, C.byref(rows), p, None]
    # n == 0: nothing is launched and no pointer is looked at
    assert L.bz_merge_positions(None, 0, 9, None, None, None, None, None, None, None, 0, None, None, None) == _lib.BZ_OK
    for i, bad in ((1, -1), (1, (1 << 26) + 1), (2, 8), (2, 64), (0, None), (11, None), (3, None), (4, None), (5, None), (6, None),
                   (7, None), (8, None), (9, None), (9, p + 8), (12, None), (12, p + 4)):
        args = list(ok)
        args[i] = bad
        assert L.bz_merge_positions(*args) == _lib.BZ_EINVAL and b"bz_merge_positions" in L.bz_last_error(), (i, bad)
    args = list(ok)
    args[10] = 8
    assert L.bz_merge_positions(*args) == _lib.BZ_ENOMEM and b"too small" in L.bz_last_error()
    for field in ("own", "pi", "z", "ply"):
        broken = _lib.MergeRows(*([p] * 11))
        setattr(broken, field, None)
        assert L.bz_merge_positions(C.byref(broken), *ok[1:]) == _lib.BZ_EINVAL
        assert L.bz_merge_positions(*ok[:11], C.byref(broken), *ok[12:]) == _lib.BZ_EINVAL
    no_vt_out = _lib.MergeRows(*([p] * 11))
    no_vt_out.vt = None
    assert L.bz_merge_positions(*ok[:11], C.byref(no_vt_out), *ok[12:]) == _lib.BZ_EINVAL
    no_q_out = _lib.MergeRows(*([p] * 11))
    no_q_out.q = None
    assert L.bz_merge_positions(*ok[:11], C.byref(no_q_out), *ok[12:]) == _lib.BZ_EINVAL


def test_the_abi_version_stays_7_and_the_new_symbols_are_declared_and_bound(tmp_path):
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "bz_abi.h")).read()
    assert "#define BZ_ABI_VERSION 7 " in hdr and L.bz_abi_version() == 7 and _lib.ABI_VERSION == 7
    for name in ("bz_merge_workspace_bytes", "bz_merge_positions", "bz_merge_group"):
        assert f"{name}(" in hdr and name in _lib.ABI_SYMBOLS and hasattr(L, name)
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "bz_abi.h"\nint main(void) { printf("%zu %zu %zu\\n", sizeof(bz_merge_rows), '
                   "sizeof(bz_engine_cfg), sizeof(bz_train_batch)); return 0; }\n")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "s"), str(src)])
    sizes = [int(x) for x in subprocess.check_output([str(tmp_path / "s")]).split()]
    assert sizes == [C.sizeof(_lib.MergeRows), 80, 48] and sizes[0] == 88


# ---------------------------------------------------------------- the twin itself
def _examples(n, na=9, seed=0, pool=5, vt=False, q=False, kl=False, own=False):
    """n rows whose boards are drawn from a pool of `pool` positions (repeats are certain for n > pool)"""
    from betazero_amd.engine import Examples
    g = np.random.default_rng(seed)
    boards = g.integers(0, 2 ** 63, (pool, 2)).astype(np.uint64)
    boards[0] = (0, 0)                         # the empty board
    boards[-1] = (2 ** 64 - 1, 2 ** 63)        # the sign bit set: int64 views are negative
    pick = g.integers(0, pool, n)
    pi, z, vtc, qc, klc = _random_group(g, max(n, 1), na, vt, q, kl)
    cut = lambda a: None if a is None else a[:n]  # noqa: E731
    return Examples(boards[pick, 0].copy(), boards[pick, 1].copy(), pi[:n], z[:n], np.where(g.random(n) < 0.5, 1, -1).astype(np.int8),
                    g.integers(0, na, n).astype(np.uint8), g.integers(0, 1000, n).astype(np.int64), g.integers(0, 60, n).astype(np.int32),
                    3 if na == 9 else 8, kl=cut(klc), q=cut(qc), vt=cut(vtc),
                    fown=boards[pick, 0].copy() if own else None, fopp=boards[pick, 1].copy() if own else None)


def test_merge_twin_groups_by_first_occurrence_and_uses_the_c_function_per_group():
    ex = _examples(200, 9, seed=1, pool=7, vt=True, q=True, kl=True)
    cols, count, bad = merge_twin(ex)
    assert bad == 0 and count.sum() == 200 and len(count) == 7 and count.max() > 1
    keys = list(zip(ex.own.tolist(), ex.opp.tolist()))
    firsts = sorted(keys.index(k) for k in set(keys))
    assert [keys[i] for i in firsts] == list(zip(cols["own"].tolist(), cols["opp"].tolist()))
    assert np.array_equal(cols["game"], ex.game[firsts]) and np.array_equal(cols["ply"], ex.ply[firsts])
    assert np.array_equal(cols["mover"], ex.mover[firsts]) and np.array_equal(cols["act"], ex.act[firsts])
    for d, k in enumerate(zip(cols["own"].tolist(), cols["opp"].tolist())):
        rows = [i for i, kk in enumerate(keys) if kk == k]
        got = _c_group(ex.pi[rows], ex.z[rows], ex.vt[rows], ex.q[rows], ex.kl[rows])
        _same(got, (cols["pi"][d], cols["vt"][d], cols["z"][d], cols["q"][d], cols["kl"][d], 0))
    assert np.abs(cols["pi"].sum(1, dtype=np.float64) - 1).max() < 1e-5


# ---------------------------------------------------------------- Python: argument errors before any device call
def test_merge_positions_refuses_bad_arguments_before_touching_a_device(monkeypatch):
    from betazero_amd import merge
    from betazero_amd.engine import DeviceExamples

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(_lib, "lib", no_device)
    monkeypatch.setattr(_lib, "require_gpu", no_device)
    with pytest.raises(ValueError, match="ownership"):
        merge.merge_positions(_examples(8, own=True))
    with pytest.raises(ValueError, match="ownership"):
        merge.merge_positions(DeviceExamples.from_host(_examples(8, 65, own=True), "cpu"))
    with pytest.raises(ValueError, match="GPU"):
        merge.merge_positions(DeviceExamples.from_host(_examples(8), "cpu"))  # valid rows on no GPU
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="return_counts"):
            merge.merge_positions(_examples(8), return_counts=bad)
    with pytest.raises(ValueError, match="Examples"):
        merge.merge_positions(np.zeros(4))
    wide = _examples(8)
    wide.pi = np.zeros((8, 10), np.float32)
    with pytest.raises(ValueError, match="pi must be"):
        merge.merge_positions(wide)

    class TooMany(DeviceExamples):
        def __len__(self):
            return (1 << 26) + 1
    with pytest.raises(ValueError, match=r"2\^26"):
        merge.merge_positions(TooMany(**vars(DeviceExamples.from_host(_examples(8), "cpu"))))
    # no rows: an empty result of the same type with vt set, and no device either
    out, cnt = merge.merge_positions(_examples(0, 65), return_counts=True)
    assert len(out) == 0 and out.vt.shape == (0,) and out.vt.dtype == np.float32 and cnt.shape == (0,) and cnt.dtype == np.int32
    dout = merge.merge_positions(DeviceExamples.from_host(_examples(0), "cpu"))
    assert isinstance(dout, DeviceExamples) and len(dout) == 0 and dout.vt.shape == (0,)
    import betazero_amd as bz
    assert bz.merge_positions is merge.merge_positions and bz.merged_repeats is merge.merged_repeats
    assert "merge_positions" in bz.__all__ and "merged_repeats" in bz.__all__


def test_merged_repeats_counts_and_refusals():
    import torch
    from betazero_amd.merge import merged_repeats
    count = torch.tensor([1, 2, 3, 4, 1023, 1024], dtype=torch.int32)
    assert merged_repeats(count).tolist() == [0, 1, 2, 3, 4, 5] and merged_repeats(count, "constant").dtype == torch.int64
    log = merged_repeats(count, "log")
    assert log.dtype == torch.int64 and torch.bincount(log).tolist() == [1, 2, 2, 3, 10, 11]
    assert log.tolist() == sorted(log.tolist())
    assert torch.bincount(merged_repeats(np.array([1 << 26, 1], np.int32), "log")).tolist() == [27, 1]
    assert merged_repeats(torch.zeros(0, dtype=torch.int32), "log").numel() == 0
    for bad in ("linear", "LOG", None, 2):
        with pytest.raises(ValueError, match="policy"):
            merged_repeats(count, bad)
    for bad in (count.float(), count[None], [1, 2], 5):
        with pytest.raises(ValueError, match="count"):
            merged_repeats(bad, "log")


# ---------------------------------------------------------------- the loop's refusals
@pytest.mark.parametrize("flags,words", [(["--merge-positions", "--ownership"], ("--merge-positions", "--ownership")),
                                         (["--merge-positions", "--merge-weight", "log", "--surprise"], ("--merge-weight log", "--surprise")),
                                         (["--merge-weight", "log"], ("--merge-weight", "--merge-positions")),
                                         (["--merge-positions", "--merge-weight", "linear"], ("--merge-weight", "linear"))])
def test_az_loop_refuses_what_the_merge_does_not_combine_with(flags, words):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "az_loop.py"), "--iters", "1", *flags],
                         capture_output=True, text=True, timeout=300)  # (an argument error: before any device is touched)
    assert out.returncode == 2 and all(w in out.stderr for w in words), out.stderr[-500:]
