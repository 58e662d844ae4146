"""The batch-API kernels -- k_reversi_step / _legal / _score, k_ttt_step (csrc/bz_env.hip), k_reversi_minimax
(csrc/bz_arena.hip), k_augment_d4 and the dedupe (betazero_amd/augment.py) -- against the oracle's rule functions and plain
Python, at every board size, every kind of action byte, past the grid cap of 2048 blocks, to the minimax kernel's full stack
depth and on inputs with real duplicates.  The references live in tests/test_batch_kernels_cpu.py; every comparison is exact."""
import os

import numpy as np
import pytest
import torch

from betazero_amd import _lib
from oracle import oracle as orc
from test_batch_kernels_cpu import (STEP_N, STRIDE_POOL, _dict_first, _scalar, check_step_coverage, minimax_cases,
                                    step_pool, ttt_step_pool, wide_rows)

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"


def _dev_u64(a):
    return torch.as_tensor(np.asarray(a, dtype=np.uint64).view(np.int64)).to(DEV)


def _dev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a).astype(dtype))).to(DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


# ---------------------------------------------------------------- env step
STEP_OUT = ("own_next", "opp_next", "legal_next", "status", "winner")


def _reversi_step(own, opp, act, size):
    """one launch of bz_reversi_step_batch_sized -> the five outputs as numpy arrays, in STEP_OUT's order"""
    n = len(own)
    o, p, a = _dev_u64(own), _dev_u64(opp), _dev(act, np.uint8)
    on, pn, lg = (torch.full((n,), -1, dtype=torch.int64, device=DEV) for _ in range(3))  # (no output is all ones: a row
    st = torch.full((n,), 0xEE, dtype=torch.uint8, device=DEV)                             # left unwritten shows)
    w = torch.full((n,), 0x55, dtype=torch.int8, device=DEV)
    _lib.check(_lib.lib().bz_reversi_step_batch_sized(o.data_ptr(), p.data_ptr(), a.data_ptr(), n, size, on.data_ptr(),
                                                      pn.data_ptr(), lg.data_ptr(), st.data_ptr(), w.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return _u64(on), _u64(pn), _u64(lg), st.cpu().numpy(), w.cpu().numpy()


def _assert_step_rows(got, pool, idx, what):
    """every output of every row; on a mismatch the first failing row is named with its inputs"""
    for name, g in zip(STEP_OUT, got):
        e = pool[name][idx]
        if not np.array_equal(g, e):
            r = int(np.flatnonzero(g != e)[0])
            i = int(np.asarray(idx)[r]) if not isinstance(idx, slice) else r
            raise AssertionError(f"{what}: {name} row {r} (pool row {i}): got {int(g[r]):#x}, expected {int(e[r]):#x}; own "
                                 f"{int(pool['own'][i]):#018x} opp {int(pool['opp'][i]):#018x} action {int(pool['act'][i])} "
                                 f"kind {int(pool['kind'][i])}")


@pytest.mark.parametrize("size", range(1, 9))
def test_reversi_step_every_size_every_action_kind_all_five_outputs(size):
    """20,000 random well-formed positions per size (all stones inside the size x size region, a few stones to a full board)
    with action bytes of every kind -- half of them drawn from 0..255 -- against the oracle's rules: stones after the move in
    the next mover's view, next legal mask, status and winner.  An illegal action (a byte above 64, a cell outside the
    region, an occupied cell, an empty cell that flips nothing, a pass while a move exists) leaves the position unchanged and
    reports the mover's own legal mask, ILLEGAL and winner 0.  The kernel's ray tables are 8x8 tables: a ray that runs out of
    a small board must stay harmless.  Then the same pool at n = 1, 2, 3, 5, 7, 130 (the ragged tail, with a small-board
    `valid`), every class of row taking its turn in the tail."""
    pool = step_pool(size)
    check_step_coverage(pool)
    got = _reversi_step(pool["own"], pool["opp"], pool["act"], size)
    _assert_step_rows(got, pool, slice(None), f"size {size}, n = {STEP_N}")
    # one row of every (status, kind) class that occurs, rotated so that each of them lands in the tail rows
    cls = pool["status"].astype(np.int64) * 8 + pool["kind"]
    sel = np.array([int(np.flatnonzero(cls == c)[0]) for c in np.unique(cls)])
    for n in (1, 2, 3, 5, 7, 130):
        for k in range(len(sel)):
            idx = np.resize(np.roll(sel, -k), n)
            got = _reversi_step(pool["own"][idx], pool["opp"][idx], pool["act"][idx], size)
            _assert_step_rows(got, pool, idx, f"size {size}, n = {n}, rotation {k}")


@pytest.mark.parametrize("size", [8, 6])
def test_reversi_step_second_grid_stride_trip_and_tail(size):
    """grid_for caps the grid at 2048 blocks of 256 lanes x 4 games: n = 2,097,152 + 5 * 1024 + 3 takes a second trip of the
    grid-stride loop (five blocks of it) and the ragged tail.  A pool of 4099 rows (a prime) with the oracle's outputs is
    tiled to n, so that a lane reading or writing one stride off meets another row."""
    pool = step_pool(size)
    n = 2_097_152 + 5 * 1024 + 3
    idx = np.resize(np.arange(STRIDE_POOL), n)
    got = _reversi_step(pool["own"][idx], pool["opp"][idx], pool["act"][idx], size)
    for name, g in zip(STEP_OUT, got):
        assert np.array_equal(g, pool[name][idx]), (name, int(np.flatnonzero(g != pool[name][idx])[0]))


def test_reversi_legal_and_score_second_grid_stride_trip():
    """k_reversi_legal and k_reversi_score hold one position per lane: n = 524,288 + 1,027 is their second trip.  The score
    is checked for the winner and both counts (orc.reversi_score on the pool rows)."""
    pool = step_pool(8)
    n = 524_288 + 1027
    idx = np.resize(np.arange(STRIDE_POOL), n)
    own, opp = pool["own"][:STRIDE_POOL], pool["opp"][:STRIDE_POOL]
    sc = [orc.reversi_score(int(a), int(b)) for a, b in zip(own, opp)]
    exp_w = np.array([s[0] for s in sc], dtype=np.int8)
    exp_c = np.array([s[1] for s in sc], dtype=np.uint8)
    assert set(exp_w.tolist()) == {-1, 0, 1}
    o, p = _dev_u64(own[idx]), _dev_u64(opp[idx])
    lg = torch.full((n,), -1, dtype=torch.int64, device=DEV)  # (a full mask is no legal mask: an unwritten row shows)
    _lib.check(_lib.lib().bz_reversi_legal_batch(o.data_ptr(), p.data_ptr(), n, lg.data_ptr(), _stream()))
    w = torch.full((n,), 0x55, dtype=torch.int8, device=DEV)
    cn = torch.full((n, 2), 0xEE, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.lib().bz_reversi_score_batch(o.data_ptr(), p.data_ptr(), n, w.data_ptr(), cn.data_ptr(), _stream()))
    torch.cuda.synchronize()
    assert np.array_equal(_u64(lg), pool["legal"][idx])
    assert np.array_equal(w.cpu().numpy(), exp_w[idx])
    assert np.array_equal(cn.cpu().numpy(), exp_c[idx])


def _ttt_step(rows):
    n = len(rows)
    own, opp = _dev(rows[:, 0], np.int16), _dev(rows[:, 1], np.int16)
    act, tm = _dev(rows[:, 2], np.uint8), _dev(rows[:, 3], np.int8)
    on, pn, lg = (torch.full((n,), -1, dtype=torch.int16, device=DEV) for _ in range(3))
    st = torch.full((n,), 0xEE, dtype=torch.uint8, device=DEV)
    w = torch.full((n,), 0x55, dtype=torch.int8, device=DEV)
    _lib.check(_lib.lib().bz_ttt_step_batch(own.data_ptr(), opp.data_ptr(), act.data_ptr(), tm.data_ptr(), n, on.data_ptr(),
                                            pn.data_ptr(), lg.data_ptr(), st.data_ptr(), w.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return np.stack([t.cpu().numpy().astype(np.int64) for t in (on, pn, lg, st, w)], 1)


def test_ttt_step_every_output_and_second_grid_stride_trip():
    """every position of ttt_exhaustive.npz x (9 cells and one byte above 8), all five outputs against the oracle's rules
    (an illegal action changes nothing and reports the mover's own empty cells), once as it is and once tiled to
    n = 524,288 + 1,027: the second trip of k_ttt_step's grid-stride loop"""
    rows, exp = ttt_step_pool()
    assert (exp[:, 3] == _lib.ST_ILLEGAL).sum() > 5000 and (exp[:, 3] == _lib.ST_TERMINAL).sum() > 1000
    got = _ttt_step(rows)
    assert np.array_equal(got, exp), int(np.flatnonzero((got != exp).any(1))[0])
    n = 524_288 + 1027
    idx = np.resize(np.arange(len(rows)), n)
    got = _ttt_step(rows[idx])
    assert np.array_equal(got, exp[idx]), int(np.flatnonzero((got != exp[idx]).any(1))[0])


# ---------------------------------------------------------------- minimax
def _minimax_batch(rows, size, depth, active=None):
    """rows: sequence of (self, other) -> (move, score) int64 arrays from one launch of k_reversi_minimax"""
    n = len(rows)
    s, o = _dev_u64([r[0] for r in rows]), _dev_u64([r[1] for r in rows])
    act = None if active is None else _dev(active, np.uint8)
    mv = torch.full((n,), 99, dtype=torch.int8, device=DEV)
    sc = torch.full((n,), 9999, dtype=torch.int16, device=DEV)
    _lib.check(_lib.lib().bz_reversi_minimax_batch(s.data_ptr(), o.data_ptr(), None if act is None else act.data_ptr(), n, size,
                                                   depth, mv.data_ptr(), sc.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return mv.cpu().numpy().astype(np.int64), sc.cpu().numpy().astype(np.int64)


def _by_size_depth(rows):
    groups = {}
    for r in rows:
        groups.setdefault((r[0], r[1]), []).append(r[2:])
    return groups


def test_reversi_minimax_kernel_depths_0_to_8_vs_the_python_reference():
    """k_reversi_minimax at every depth its per-lane stack holds (0..8), sizes 4 / 6 / 8, against _minimax_ref: late positions
    for depths 5..8, positions anywhere in the game for 0..4, both colours, positions where `self` has no move (None, -1000)
    and finished ones.  One launch per size and depth; move and score are equal."""
    rows, nodes = minimax_cases()
    print(f"minimax cases: {len(rows)} rows, reference nodes {nodes}, None {sum(r[4] == -1 for r in rows)}, "
          f"+-1000 {sum(abs(r[5]) == 1000 for r in rows)}")
    for (size, depth), g in sorted(_by_size_depth(rows).items()):
        mv, sc = _minimax_batch(g, size, depth)
        exp_mv, exp_sc = np.array([r[2] for r in g]), np.array([r[3] for r in g])
        assert np.array_equal(mv, exp_mv) and np.array_equal(sc, exp_sc), (size, depth, mv.tolist(), exp_mv.tolist(),
                                                                            sc.tolist(), exp_sc.tolist())


def test_reversi_minimax_kernel_wide_set_vs_the_scalar_entry_point():
    """a few thousand rows over every size and depth, device against bz_reversi_minimax (the host build of the same source,
    itself held to the Python reference on the CPU): lanes, stack and batch handling rather than the rule"""
    n_rows = 0
    for (size, depth), g in sorted(_by_size_depth(wide_rows()).items()):
        exp = np.array([_scalar(s, o, size, depth) for s, o in g], dtype=np.int64)
        mv, sc = _minimax_batch(g, size, depth)
        bad = np.flatnonzero((mv != exp[:, 0]) | (sc != exp[:, 1]))
        assert len(bad) == 0, (size, depth, len(g), int(bad[0]), hex(g[bad[0]][0]), hex(g[bad[0]][1]), int(mv[bad[0]]),
                               int(sc[bad[0]]), exp[bad[0]].tolist())
        n_rows += len(g)
    print("wide set rows", n_rows)
    assert n_rows >= 2000


@pytest.mark.parametrize("size,depth", [(4, 8), (6, 6), (8, 5)])
def test_reversi_minimax_kernel_ragged_batches_and_active_mask(size, depth):
    """n = 1, 63, 64, 65 and 200 against the 64-lane blocks, without a mask and with every third row switched off: a row
    that is off reports move -1 and score 0, a row that is on is what it is without the mask"""
    late = [(s, o) for sz, d, s, o in wide_rows() if sz == size and size * size - bin(s | o).count("1") <= 8][:200]
    assert len(late) == 200
    exp = np.array([_scalar(s, o, size, depth) for s, o in late], dtype=np.int64)
    assert len(set(exp[:, 0].tolist())) > 5
    for n in (1, 63, 64, 65, 200):
        rows = late[200 - n:]  # (the last rows: another row leads every batch)
        mv, sc = _minimax_batch(rows, size, depth)
        assert np.array_equal(mv, exp[200 - n:, 0]) and np.array_equal(sc, exp[200 - n:, 1]), n
        on = (np.arange(n) % 3 != 2) if n > 1 else np.zeros(1, bool)
        mv, sc = _minimax_batch(rows, size, depth, active=on)
        assert np.array_equal(mv, np.where(on, exp[200 - n:, 0], -1)) and np.array_equal(sc, np.where(on, exp[200 - n:, 1], 0)), n
    mv, sc = _minimax_batch(late[:1], size, depth, active=np.ones(1, bool))
    assert (int(mv[0]), int(sc[0])) == tuple(exp[0].tolist())


def test_reversi_minimax_kernel_refuses_depth_9():
    t = torch.zeros(4, dtype=torch.int64, device=DEV)
    mv = torch.empty(4, dtype=torch.int8, device=DEV)
    sc = torch.empty(4, dtype=torch.int16, device=DEV)
    L = _lib.lib()
    assert L.bz_reversi_minimax_batch(t.data_ptr(), t.data_ptr(), None, 4, 8, 9, mv.data_ptr(), sc.data_ptr(), _stream()) == _lib.BZ_EINVAL
    assert L.bz_reversi_minimax_batch(t.data_ptr(), t.data_ptr(), None, 4, 8, -1, mv.data_ptr(), sc.data_ptr(), _stream()) == _lib.BZ_EINVAL
    assert L.bz_reversi_minimax_batch(t.data_ptr(), t.data_ptr(), None, 4, 5, 2, mv.data_ptr(), sc.data_ptr(), _stream()) == _lib.BZ_EINVAL


# ---------------------------------------------------------------- augmentation and dedupe
def _cells(bits):
    return ((np.asarray(bits, np.uint64)[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)


def _bits(cells):
    return (cells.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(1, dtype=np.uint64)


def _augment_input():
    """1,003 rows at 8x8 with na = 65: random rows; rows whose boards and pi are symmetric under one or more of the transforms
    (several of their eight copies coincide); rows that are transform t of an earlier row; rows equal to an earlier one in
    the boards with pi one ULP away; `act` over 0..64 and distinct z / mover / game / ply / kl / q / vt per row"""
    from betazero_amd.engine import Examples
    maps = np.load(os.path.join(G, "augment.npz"))["maps8"].astype(np.int64)
    rng = np.random.default_rng(8)
    n = 1003
    own = rng.integers(0, 2**63, n, dtype=np.int64).astype(np.uint64) * np.uint64(2) + rng.integers(0, 2, n).astype(np.uint64)
    opp = rng.integers(0, 2**63, n, dtype=np.int64).astype(np.uint64) * np.uint64(2) + rng.integers(0, 2, n).astype(np.uint64)
    co, cp = _cells(own), _cells(opp) & (1 - _cells(own))
    pi = rng.random((n, 65)).astype(np.float32)
    gens = [(1,), (2,), (4,), (6,), (3,), (1, 2), (6, 4), (1, 6)]  # generators of subgroups of D4, up to the whole group
    n_sym = n_tr = n_ulp = 0
    for i in range(200, n):
        r = rng.random()
        if r < 0.3:  # close the row under a subgroup: OR of the boards, maximum of pi (exact in any order)
            a, b, p = co[i].copy(), cp[i].copy(), pi[i, :64].copy()
            gen = gens[int(rng.integers(len(gens)))]
            for _ in range(8):  # (an orbit has at most 8 elements: the closure is reached well before)
                for t in gen:
                    a, b, p = a | a[maps[t]], b | b[maps[t]], np.maximum(p, p[maps[t]])
            co[i], cp[i], pi[i, :64] = a, b & (1 - a), p
            assert all(np.array_equal(co[i], co[i][maps[t]]) and np.array_equal(pi[i, :64], pi[i, :64][maps[t]]) for t in gen)
            n_sym += 1
        elif r < 0.55:  # transform t of an earlier row
            j, t = int(rng.integers(0, i)), int(rng.integers(1, 8))
            co[i], cp[i], pi[i, :64], pi[i, 64] = co[j][maps[t]], cp[j][maps[t]], pi[j, :64][maps[t]], pi[j, 64]
            n_tr += 1
        elif r < 0.7:   # the boards of an earlier row, pi one ULP away in one column (the pass column included)
            j, c = int(rng.integers(0, i)), int(rng.integers(65))
            co[i], cp[i], pi[i] = co[j], cp[j], pi[j]
            pi[i, c] = np.nextafter(pi[i, c], np.float32(2))
            n_ulp += 1
    act = rng.integers(0, 65, n).astype(np.uint8)
    act[::17] = 64
    ex = Examples(_bits(co), _bits(cp), pi, rng.integers(-1, 2, n).astype(np.int8), rng.choice([-1, 1], n).astype(np.int8), act,
                  rng.permutation(n).astype(np.int64), rng.integers(0, 60, n).astype(np.int32), 8,
                  kl=rng.random(n).astype(np.float32), q=rng.random(n).astype(np.float32), vt=rng.random(n).astype(np.float32))
    return ex, maps, (n_sym, n_tr, n_ulp)


def test_augment_8x8_maps_act_dedupe_and_carry_over_on_rows_with_real_duplicates():
    """dedupe=False: boards and pi are the index maps of augment.npz["maps8"], the pass column stays, `act` is the mapped
    cell and 64 stays 64.  dedupe=True: the kept rows are the first-occurrence list of a Python dict over (own, opp, pi
    bytes) in insertion order -- on an input where copies of one row coincide (symmetric rows), where rows are transforms of
    earlier rows and where rows one ULP apart must stay -- and z / mover / game / ply / kl / q / vt are those of source row
    keep // 8.  The kernel's key8 separates exactly the distinct contents of this input (else every training step pays
    extra dedupe passes)."""
    from betazero_amd.augment import augment_examples
    from betazero_amd.engine import DeviceExamples
    ex, maps, made = _augment_input()
    n = len(ex)
    co, cp = _cells(ex.own), _cells(ex.opp)
    inv = np.argsort(maps, 1)  # out[j] = x[m[j]]: the stone (or the one-hot act) of cell a lands on j with m[j] == a
    e_own = np.stack([_bits(co[:, maps[t]]) for t in range(8)], 1).reshape(-1)
    e_opp = np.stack([_bits(cp[:, maps[t]]) for t in range(8)], 1).reshape(-1)
    e_pi = np.stack([np.concatenate([ex.pi[:, :64][:, maps[t]], ex.pi[:, 64:]], 1) for t in range(8)], 1).reshape(8 * n, 65)
    e_act = np.stack([np.where(ex.act == 64, 64, inv[t][np.minimum(ex.act, 63)]) for t in range(8)], 1).reshape(-1)
    full = augment_examples(ex, dedupe=False)
    assert len(full) == 8 * n
    assert np.array_equal(full.own, e_own) and np.array_equal(full.opp, e_opp)
    assert np.array_equal(full.pi.view(np.uint32), e_pi.view(np.uint32))
    assert np.array_equal(full.act, e_act) and (full.act[ex.act.repeat(8) == 64] == 64).all() and (ex.act == 64).sum() >= 59
    src = np.arange(8 * n) // 8
    for f in ("z", "mover", "game", "ply", "kl", "q", "vt"):
        assert np.array_equal(getattr(full, f), getattr(ex, f)[src]), f
    keep = np.array(_dict_first(e_own, e_opp, e_pi))
    within = sum(len({(int(a), int(b), p.tobytes()) for a, b, p in zip(e_own[8 * i:8 * i + 8], e_opp[8 * i:8 * i + 8], e_pi[8 * i:8 * i + 8])})
                 for i in range(n))
    print(f"augment input: {n} rows ({made[0]} symmetric, {made[1]} transforms of earlier rows, {made[2]} one ULP away), "
          f"{8 * n} copies, {within} distinct within their own row, {len(keep)} distinct in all")
    assert within < 7 * n - 300 and len(keep) < within - 800  # duplicates beyond the reference's 5 = 7 pair, and across rows
    for out in (augment_examples(ex, dedupe=True), augment_examples(DeviceExamples.from_host(ex, DEV), dedupe=True).cpu()):
        assert len(out) == len(keep)
        assert np.array_equal(out.own, e_own[keep]) and np.array_equal(out.opp, e_opp[keep])
        assert np.array_equal(out.pi.view(np.uint32), e_pi[keep].view(np.uint32)) and np.array_equal(out.act, e_act[keep])
        for f in ("z", "mover", "game", "ply", "kl", "q", "vt"):
            assert np.array_equal(getattr(out, f), getattr(ex, f)[keep // 8]), f
    # the content key, from the kernel itself
    d = DeviceExamples.from_host(ex, DEV)
    own8, opp8, key8 = (torch.empty(8 * n, dtype=torch.int64, device=DEV) for _ in range(3))
    pi8 = torch.empty((8 * n, 65), dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().bz_augment_d4_batch(d.own.data_ptr(), d.opp.data_ptr(), d.pi.data_ptr(), n, 8, 65, own8.data_ptr(),
                                              opp8.data_ptr(), pi8.data_ptr(), key8.data_ptr(), _stream()))
    torch.cuda.synchronize()
    key8 = key8.cpu().numpy()
    assert len(np.unique(key8)) == len(keep)
    assert len(np.unique(key8[keep])) == len(keep)  # and equal contents share their key


def test_augment_zero_rows_in_zero_rows_out():
    """no finished game yet (an early az_loop iteration): host Examples and DeviceExamples with no rows come back with no
    rows, every field of the right type and shape"""
    from betazero_amd.augment import augment_examples
    from betazero_amd.engine import DeviceExamples, Examples
    z = lambda dt, *shape: np.zeros((0,) + shape, dtype=dt)  # noqa: E731
    for size, na in ((8, 65), (3, 9)):
        ex = Examples(z(np.uint64), z(np.uint64), z(np.float32, na), z(np.int8), z(np.int8), z(np.uint8), z(np.int64), z(np.int32),
                      size, kl=z(np.float32))
        for dedupe in (True, False):
            out = augment_examples(ex, dedupe=dedupe)
            assert isinstance(out, Examples) and len(out) == 0 and out.pi.shape == (0, na) and out.act.dtype == np.uint8
            assert out.kl.shape == (0,) and out.q is None and out.size == size
            dout = augment_examples(DeviceExamples.from_host(ex, DEV), dedupe=dedupe)
            assert isinstance(dout, DeviceExamples) and len(dout) == 0 and tuple(dout.pi.shape) == (0, na)
            assert dout.own.device.type == "cuda" and dout.own.dtype == torch.int64


def test_augment_carries_every_column_that_rides_with_the_source_row():
    """3 tic-tac-toe rows with every optional column: the eight copies of row i have its z / mover / game / ply / kl / q / vt /
    count (dedupe=False: row 8 i + t; dedupe=True: whichever copies are kept -- kl, distinct per row, names the source); the
    ownership target goes through the kernel with its position (here fown = own, fopp = opp: equal after every transform)"""
    from betazero_amd.augment import augment_examples
    from betazero_amd.engine import DeviceExamples, Examples
    from betazero_amd.examples import COLUMNS
    own = np.array([0b000010001, 0b100000000, 0b000000000], np.uint64)   # the first row is symmetric under the main diagonal
    opp = np.array([0b000000000, 0b000010010, 0b000010000], np.uint64)
    pi = np.zeros((3, 9), np.float32)
    pi[0, [2, 6]], pi[1, [0, 2, 3]], pi[2, :4] = 0.5, (0.5, 0.25, 0.25), 0.25
    ex = Examples(own, opp, pi, np.array([1, -1, 0], np.int8), np.array([1, -1, -1], np.int8), np.array([2, 0, 3], np.uint8),
                  np.array([7, 7, 2**40], np.int64), np.array([2, 3, 1], np.int32), 3, kl=np.array([0.5, 0.25, 0.125], np.float32),
                  q=np.array([-0.5, 0.75, 0.1], np.float32), vt=np.array([1.0, -0.25, 0.3], np.float32), fown=own.copy(), fopp=opp.copy(),
                  count=np.array([1, 5, 2**20], np.int32))
    assert all(getattr(ex, c.name) is not None for c in COLUMNS)
    rides = ("z", "mover", "game", "ply", "kl", "q", "vt", "count")
    for rows in (ex, DeviceExamples.from_host(ex, DEV)):
        full = augment_examples(rows, dedupe=False)
        kept = augment_examples(rows, dedupe=True)
        assert type(full) is type(rows) and type(kept) is type(rows)
        if rows is not ex:
            full, kept = full.cpu(), kept.cpu()
        assert len(full) == 24 and 3 < len(kept) < 24   # the symmetric row loses copies, no row loses all
        for f in rides:
            a, b = getattr(full, f), getattr(ex, f)
            assert a.dtype == b.dtype and np.array_equal(a, np.repeat(b, 8)), f
        src = np.array([{0.5: 0, 0.25: 1, 0.125: 2}[float(v)] for v in kept.kl])
        assert sorted(set(src.tolist())) == [0, 1, 2] and (np.diff(src) >= 0).all()
        for f in rides:
            a, b = getattr(kept, f), getattr(ex, f)
            assert a.dtype == b.dtype and np.array_equal(a, b[src]), f
        for out in (full, kept):
            assert out.fown.dtype == np.uint64 and np.array_equal(out.fown, out.own) and np.array_equal(out.fopp, out.opp)
            assert all(getattr(out, c.name) is not None for c in COLUMNS)
