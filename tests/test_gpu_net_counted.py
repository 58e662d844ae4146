"""The device-count net forwards -- bz_net_forward_counted and bz_net_forward_sym_counted, the only forwards an engine ever
calls -- against net_forward_ref of tests/test_net_numerics_cpu.py, bit for bit on exact nets, at every geometry the launch
code can pick: the three f32 kernels, the bf16 tower at C = 64 / 128 / 256 in its latency and throughput shapes (at C = 128
and 261 rows under all three adaptive modes and both tile maps), the fp8 tower; each plain, under one fixed symmetry that is
not the identity and under the hashed one.  include/bz_abi.h promises for them: rows below the count are the host-count
forward's bits, rows from the count on are never written, a count of 0 touches nothing, and a count above max_n is clamped
to max_n.

Buffers: own, opp, logits and value have max_n + GUARD rows and the forwards get their [:max_n] views; the outputs are
filled with a sentinel bit pattern first.  A launch is ceil(max_n / P) workgroups of P <= 8 rows, so whatever the count says
no row index >= max_n + 7 can be reached: every access stays inside the allocations.  Every row is compared -- rows below
the count with the reference, all others (the guard rows included) with the sentinel -- on integer views; nothing here has
a tolerance.

The symmetric expectations come from the plain reference on the transformed boards (test_gpu_symmetry's numpy twin), gathered
through sym_action_map, with the row's symmetry from sym_index: never from the symmetric kernels.

The reference asserts its own exactness.  The board set here (boards(285, seed=269) with repeated positions dropped, 269
rows), the value conv of _exact() and the net fp8 (128, 2, 64) are not among the configurations test_gpu_net_numerics.py
runs: every (net, form) below was run through _ref(.., dev="cpu") on the CPU first -- all exact, all rows distinct."""
import os
import re

import numpy as np
import pytest
import torch

from betazero_amd.symmetry import sym_action_map, sym_index
from test_gpu_symmetry import _twin_boards
from test_net_numerics_cpu import boards, exact_net, flat_params, net_forward_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
T1 = int(re.search(r"constexpr int kAdaptT1 = (\d+);", open(os.path.join(ROOT, "betazero_amd", "csrc", "bz_net.hip")).read()).group(1))
GUARD = 8                   # rows behind max_n: one more than the last workgroup of any shape (P <= 8) can reach
ROWS = 261 + GUARD          # one board set for every geometry: a geometry of max_n rows takes the first max_n + GUARD
NET_SEED, HASH_SEED, FIXED = 1, 7, 3    # (FIXED = 3: a quarter turn, which is not its own inverse)
SENT = 0x7FC5A5A5           # the outputs' fill: a NaN no forward produces
FORMS = ("plain", "fixed", "hash")
OVER = (1, 7, None)         # over-counts: max_n + 1, max_n + 7, 2^31 - 1

# (mode, C, NB, VH, max_n, P = rows per workgroup): the kernel and shape the launch code picks (bz_net.hip)
GEOMS = [
    ("f32", 32, 1, 64, 37, 1),      # k_stem / k_conv_f32 / k_heads: one block per row
    ("f32", 64, 1, 33, 37, 1),
    ("bf16", 64, 1, 33, 251, 2),    # TwS64
    ("bf16", 64, 1, 33, 261, 8),    # Tw<64>
    ("bf16", 128, 1, 64, 251, 1),   # TwS128 (a buffer of at most 256 rows: no adaptive pair)
    ("bf16", 256, 1, 33, 251, 1),   # TwS256
    ("bf16", 256, 1, 33, 261, 2),   # Tw<256>
    ("fp8", 128, 1, 64, 7, 4),      # k_tower_fp8 / k_sym_fp8
    ("fp8", 128, 1, 64, 261, 4),
    ("fp8", 128, 0, 64, 261, 4),
    ("fp8", 128, 2, 64, 261, 4),
]
# bf16, C = 128, max_n = 261: the shape follows the adaptive mode and the count (P = 1 or 4), the plain throughput kernel the tile map
ADAPTIVE = [("bf16", 128, 1, 64, 261), ("bf16", 128, 0, 33, 261), ("bf16", 128, 2, 64, 261)]
VARIANTS = {"plain": [(m, t) for m in (0, 1, 2) for t in (0, 1)], "fixed": [(m, 1) for m in (0, 1, 2)], "hash": [(m, 1) for m in (0, 1, 2)]}


def _gid(g):
    return f"{g[0]}-C{g[1]}-NB{g[2]}-n{g[4]}"


_BOARDS, _REFS, _NETS, _BUFS = {}, {}, {}, {}


def _boards():
    if not _BOARDS:
        own, opp = boards(ROWS + 16, seed=ROWS)     # the golden games repeat a few positions: every position once, in order
        keep = np.sort(np.unique(np.stack([own, opp], 1), axis=0, return_index=True)[1])[:ROWS]
        assert keep.size == ROWS
        _BOARDS.update(own=own[keep], opp=opp[keep])
    return _BOARDS["own"], _BOARDS["opp"]


def _row_syms(form, n):
    """the symmetry every one of the first n rows is evaluated under"""
    own, opp = _boards()
    if form == "fixed":
        return np.full(n, FIXED)
    return np.array([sym_index(HASH_SEED, int(o), int(p)) for o, p in zip(own[:n], opp[:n])])


def _exact(mode, C, NB, VH):
    """exact_net(.., seed = NET_SEED).  On the bf16 and f32 nets its value conv gives all zeros (C = 128, 256) or sums in the
    hundreds (C = 64), so the value is one constant or +-1 on every row; here that conv is |val_w| 2^-7 with no bias -- still
    exact, which the reference asserts -- and the value differs from row to row (asserted in _ref; the scale is the one of
    2^-6 .. 2^-10 at which that holds for every net and form here).  The fp8 nets stay."""
    P = exact_net(C, NB, VH, mode, NET_SEED)
    if mode != "fp8":
        P["val_w"] = P["val_w"].abs() * 2.0 ** -7
        P["val_w"][0, 0] = 2.0 ** -7
        P["val_b"] = torch.zeros(1, dtype=torch.float64)
    return P


def _params(mode, C, NB, VH, dev):
    return {k: t.to(dev) for k, t in _exact(mode, C, NB, VH).items()}


def _ref(mode, C, NB, VH, form, dev=DEV):
    """(logits bits [n, 65], value bits [n]) the form must give on the first n board rows (n = 261; 37 for f32, whose
    geometries need no more), computed once and never changed.  The reference asserts its own exactness; its logit rows
    differ from one another (asserted here), so no shifted or repeated row can pass for the right one."""
    key = (mode, C, NB, VH, form)
    if key not in _REFS:
        n = 37 if mode == "f32" else 261
        own, opp = _boards()
        own, opp = own[:n], opp[:n]
        P = _params(mode, C, NB, VH, dev)
        if form == "plain":
            lg, v = net_forward_ref(own, opp, P, mode)
            lg = lg.cpu().numpy()
        else:
            s, rows = _row_syms(form, n), np.arange(n)
            if form == "hash":  # the first 7 rows (the smallest geometry) meet several symmetries, 261 rows all eight
                assert len(set(s[:7].tolist())) > 2 and (n < 100 or len(set(s.tolist())) == 8)
            town = np.stack([_twin_boards(own, 8, k) for k in range(8)])[s, rows]
            topp = np.stack([_twin_boards(opp, 8, k) for k in range(8)])[s, rows]
            lt, v = net_forward_ref(town, topp, P, mode)
            tau = np.stack([sym_action_map(8, k) for k in range(8)]).astype(np.int64)    # [8, 65]
            lg = np.take_along_axis(lt.cpu().numpy(), tau[s], axis=1)                    # logit j of row i = lt[i, tau_s(j)]
        lg = np.ascontiguousarray(lg.astype(np.float32)).view(np.uint32)
        v = np.ascontiguousarray(v.cpu().numpy().astype(np.float32)).view(np.uint32)
        # the rows differ from one another in their logits, and on the bf16 and f32 nets no two rows that one workgroup can
        # hold (P <= 8: up to 7 apart, 8 taken) have the same value: a value from a neighbouring row, or from the clamped
        # last row of a partial workgroup, cannot pass.  The fp8 nets' values repeat (some tens of distinct ones in 261
        # rows; they are asserted not to be one constant, over the first 7 rows too), so there the logits say which row
        # is which and the sentinel where the value lands.
        assert np.unique(lg, axis=0).shape[0] == n, key
        if mode == "fp8":
            assert np.unique(v).size > 1 and np.unique(v[:7]).size > 1, key
        else:
            assert all((v[d:] != v[:-d]).all() for d in range(1, 9)), key
        _REFS[key] = (lg, v)
    return _REFS[key]


def _net(mode, C, NB, VH):
    key = (mode, C, NB, VH)
    if key not in _NETS:
        from betazero_amd.net import DeviceNet
        _NETS[key] = DeviceNet(C, NB, VH, flat_params(_exact(mode, C, NB, VH)), 261)
    return _NETS[key]


class _Buffers:
    """own / opp / logits / value of max_n + GUARD rows and the count, on the device"""

    def __init__(self, max_n):
        own, opp = _boards()
        dev = lambda a: torch.as_tensor(np.asarray(a[:max_n + GUARD], dtype=np.uint64).view(np.int64)).to(DEV)  # noqa: E731
        self.max_n = max_n
        self.own, self.opp = dev(own), dev(opp)
        self.lg = torch.empty((max_n + GUARD, 65), dtype=torch.int32, device=DEV)
        self.v = torch.empty((max_n + GUARD,), dtype=torch.int32, device=DEV)
        self.count = torch.zeros(1, dtype=torch.int32, device=DEV)

    def fill(self):
        self.lg.fill_(SENT)
        self.v.fill_(SENT)

    def launch(self, dn, mode, form, count):
        """the count written by a device op on the stream, then the forward on the [:max_n] views: no host synchronisation"""
        m = self.max_n
        self.count.fill_(count)
        sym = {"plain": None, "fixed": FIXED, "hash": "hash"}[form]
        dn.forward_counted(self.own[:m], self.opp[:m], self.count, self.lg[:m].view(torch.float32), self.v[:m].view(torch.float32),
                           bf16=mode != "f32", fp8=mode == "fp8", symmetry=sym, size=8, seed=HASH_SEED)

    def read(self):
        return self.lg.cpu().numpy().view(np.uint32), self.v.cpu().numpy().view(np.uint32)


def _bufs(max_n):
    if max_n not in _BUFS:
        _BUFS[max_n] = _Buffers(max_n)
    return _BUFS[max_n]


def _check(out, ref, lo, hi, what):
    """rows [lo, hi) are the reference's bits, every row from hi on (up to the last guard row) holds the sentinel"""
    (lg, v), (rl, rv) = out, ref
    bad = np.argwhere(lg[lo:hi] != rl[lo:hi])
    assert bad.size == 0, (what, "logits differ from the reference", len(bad), (bad[:5] + [lo, 0]).tolist())
    bad = np.flatnonzero(v[lo:hi] != rv[lo:hi])
    assert bad.size == 0, (what, "values differ from the reference", len(bad), (bad[:5] + lo).tolist())
    rows = np.flatnonzero((lg[hi:] != SENT).any(axis=1) | (v[hi:] != SENT))
    assert rows.size == 0, (what, "rows written at or above the count", (rows + hi).tolist())


def _counts(max_n, *Ps):
    """0, 1, P - 1, P, P + 1, the first row of the last workgroup and the row before it, max_n - 1, max_n"""
    c = {0, 1, max_n - 1, max_n}
    for P in Ps:
        last = (max_n - 1) // P * P
        c |= {P - 1, P, P + 1, last - 1, last}
    return sorted(x for x in c if 0 <= x <= max_n)


def _expected_tally(adaptive, n):
    shape = None if n <= 0 else ("latency" if adaptive == 2 or (adaptive == 1 and n <= T1) else "throughput")
    return {k: int(k == shape) for k in ("latency", "middle", "throughput")}


def _over(max_n, k):
    return 2 ** 31 - 1 if k is None else max_n + k


# ---------------------------------------------------------------- every geometry but the adaptive one
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_counted_rows_are_the_reference_and_no_other_row_is_written(geom, form):
    mode, C, NB, VH, max_n, P = geom
    dn, B, ref = _net(mode, C, NB, VH), _bufs(max_n), _ref(mode, C, NB, VH, form)
    for n in _counts(max_n, P):
        B.fill()
        B.launch(dn, mode, form, n)
        _check(B.read(), ref, 0, n, (_gid(geom), form, n))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_a_count_above_max_n_is_clamped_to_max_n(geom, form):
    mode, C, NB, VH, max_n, P = geom
    dn, B, ref = _net(mode, C, NB, VH), _bufs(max_n), _ref(mode, C, NB, VH, form)
    for k in OVER:
        B.fill()
        B.launch(dn, mode, form, _over(max_n, k))
        _check(B.read(), ref, 0, max_n, (_gid(geom), form, _over(max_n, k)))


def _stale_rows(dn, B, mode, form, ref, what):
    """count a, then -- no refill, no host synchronisation -- a smaller count b written by a device op: rows [b, a) keep the
    first launch's bits; then a count above a writes the new rows"""
    max_n = B.max_n
    a, b = max(2, 2 * max_n // 3), max(1, max_n // 3)
    B.fill()
    B.launch(dn, mode, form, a)
    B.launch(dn, mode, form, b)
    _check(B.read(), ref, 0, a, (what, form, "counts", a, b))
    B.launch(dn, mode, form, max_n)
    _check(B.read(), ref, 0, max_n, (what, form, "counts", a, b, max_n))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("geom", GEOMS, ids=_gid)
def test_a_smaller_count_in_stream_order_leaves_the_stale_rows(geom, form):
    mode, C, NB, VH, max_n, P = geom
    _stale_rows(_net(mode, C, NB, VH), _bufs(max_n), mode, form, _ref(mode, C, NB, VH, form), _gid(geom))


# ---------------------------------------------------------------- bf16, C = 128, 261 rows: the shape follows mode and count
def _variant(dn, adaptive, tile_map):
    dn.set_adaptive_shape(adaptive)
    dn.set_tile_map(tile_map)


def _vid(v):
    return f"mode{v[0]}-map{v[1]}"


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("geom", ADAPTIVE, ids=_gid)
def test_adaptive_geometry_rows_tally_and_equal_bits_in_every_mode_and_tile_map(geom, form):
    mode, C, NB, VH, max_n = geom
    dn, B, ref = _net(mode, C, NB, VH), _bufs(max_n), _ref(mode, C, NB, VH, form)
    try:
        for n in sorted({*_counts(max_n, 1, 4), T1 - 1, T1, T1 + 1}):
            first = None
            for adaptive, tile_map in VARIANTS[form]:
                what = (_gid(geom), form, _vid((adaptive, tile_map)), n)
                _variant(dn, adaptive, tile_map)
                dn.shape_tally()
                B.fill()
                B.launch(dn, mode, form, n)
                tally = dn.shape_tally()
                out = B.read()
                _check(out, ref, 0, n, what)
                assert tally == _expected_tally(adaptive, n), (what, tally)
                if first is None:
                    first = out
                assert np.array_equal(out[0], first[0]) and np.array_equal(out[1], first[1]), what
    finally:
        _variant(dn, 1, 1)


# (the tile map does not reach the symmetric kernels: they run once per mode)
FORM_VARIANTS = [(f, v) for f in FORMS for v in VARIANTS[f]]
_fvid = lambda fv: f"{fv[0]}-{_vid(fv[1])}"  # noqa: E731


@pytest.mark.parametrize("form_variant", FORM_VARIANTS, ids=_fvid)
@pytest.mark.parametrize("geom", ADAPTIVE, ids=_gid)
def test_adaptive_geometry_clamps_a_count_above_max_n(geom, form_variant):
    """the tally is what max_n rows call for: the latency shape in mode 2, else (261 > kAdaptT1) the throughput shape"""
    form, variant = form_variant
    mode, C, NB, VH, max_n = geom
    dn, B, ref = _net(mode, C, NB, VH), _bufs(max_n), _ref(mode, C, NB, VH, form)
    try:
        _variant(dn, *variant)
        for k in OVER:
            what = (_gid(geom), form, _vid(variant), _over(max_n, k))
            dn.shape_tally()
            B.fill()
            B.launch(dn, mode, form, _over(max_n, k))
            tally = dn.shape_tally()
            _check(B.read(), ref, 0, max_n, what)
            assert tally == _expected_tally(variant[0], max_n), (what, tally)
    finally:
        _variant(dn, 1, 1)


@pytest.mark.parametrize("form_variant", FORM_VARIANTS, ids=_fvid)
def test_adaptive_geometry_smaller_count_in_stream_order_leaves_the_stale_rows(form_variant):
    """in mode 1 the first two launches (174 and 87 rows) run the latency shape and the third (261) the throughput shape"""
    form, variant = form_variant
    mode, C, NB, VH, max_n = ADAPTIVE[0]
    dn = _net(mode, C, NB, VH)
    try:
        _variant(dn, *variant)
        _stale_rows(dn, _bufs(max_n), mode, form, _ref(mode, C, NB, VH, form), (_gid(ADAPTIVE[0]), _vid(variant)))
    finally:
        _variant(dn, 1, 1)
