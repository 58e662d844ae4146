"""Reanalysis without a GPU: reanalyse_rows, the refusals of Reanalyser.run / reanalyse() (they come before any
engine is built, so they are reachable on a host without a device), the argument checks of the two ABI entry points, and
reanalyse_twin -- the Python twin tests/test_gpu_reanalyse.py holds the device path to, built on the oracle's search as it is."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest
import torch

from betazero_amd import _lib
from betazero_amd.engine import Examples
from betazero_amd.reanalyse import reanalyse, reanalyse_rows
from oracle import oracle as orc

ORC_GAME = {3: orc.GAME_TTT, 8: orc.GAME_REVERSI, 6: orc.GAME_REVERSI6, 4: orc.GAME_REVERSI4}


def f32(x):
    return np.float32(x)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- the twin
def root_targets(N, W, P):
    """(pi [na], q, kl) of one searched root from the oracle's root statistics by action: pi = float32(N) / float32(sum N) at
    the root's edges, q = bz_root_value and kl = bz_surprise_kl over the edges in ascending action order.  The edges are the
    actions with P > 0 or N > 0: an edge with neither (a prior that underflowed and was never visited) adds +0 to both sums
    of q and is skipped by kl (pi = 0), so leaving it out changes no bit."""
    L = _lib.lib()
    ed = np.nonzero((P > 0) | (N > 0))[0]
    n, w, p = np.ascontiguousarray(N[ed], np.uint32), np.ascontiguousarray(W[ed], np.float32), np.ascontiguousarray(P[ed], np.float32)
    pi = np.zeros(N.shape[0], np.float32)
    pi[ed] = n.astype(np.float32) / f32(n.sum(dtype=np.uint64))
    q, kl = C.c_float(), C.c_float()
    _lib.check(L.bz_root_value(n.ctypes.data, w.ctypes.data, len(ed), C.addressof(q)))
    pe = np.ascontiguousarray(pi[ed])
    _lib.check(L.bz_surprise_kl(pe.ctypes.data, p.ctypes.data, len(ed), C.addressof(kl)))
    return pi, f32(q.value), f32(kl.value)


def reanalyse_twin(ex, rows, sims, eval_kind, net=None):
    """what Reanalyser.run(ex, rows) leaves in the refreshed columns under plain PUCT, from host Examples: (pi, q, kl) -- copies
    of ex's columns (q / kl: None where ex has none) with the rows `rows` (None = all) replaced by root_targets of
    oracle.mcts_search from the row's position.  One search per distinct position: a row is a function of its position."""
    pi = ex.pi.copy()
    q = None if ex.q is None else ex.q.copy()
    kl = None if ex.kl is None else ex.kl.copy()
    seen = {}
    for r in (range(len(ex)) if rows is None else (int(v) for v in rows)):
        key = (int(ex.own[r]), int(ex.opp[r]), int(ex.mover[r]))
        if key not in seen:
            N, W, P, _ = orc.mcts_search(ORC_GAME[ex.size], *key, sims, eval_kind, net=net)
            seen[key] = root_targets(N, W, P)
        pi[r] = seen[key][0][:pi.shape[1]]
        if q is not None:
            q[r] = seen[key][1]
        if kl is not None:
            kl[r] = seen[key][2]
    return pi, q, kl


def oracle_examples(size, n_games, sims, eval_kind, **cols):
    """host Examples of n_games oracle self-play games (4 sampled moves each, so that the games differ), with recorded q / kl
    columns of a recognisable constant where asked for (cols: q=True, kl=True, vt=True, count=True)"""
    g = [orc.selfplay_game(ORC_GAME[size], i, sims, eval_kind, 4, 0, 7) for i in range(n_games)]
    cat = lambda k: np.concatenate([r[k] for r in g])  # noqa: E731
    n = len(cat("own"))
    extra = {k: (np.full(n, 3, np.int32) if k == "count" else np.full(n, -0.75, np.float32)) for k, on in cols.items() if on}
    return Examples(own=cat("own"), opp=cat("opp"), pi=cat("pi"), z=cat("z"), mover=cat("mover"), act=cat("act"),
                    game=np.concatenate([np.full(len(r["own"]), i, np.int64) for i, r in enumerate(g)]),
                    ply=np.concatenate([np.arange(len(r["own"]), dtype=np.int32) for r in g]), size=size, **extra)


def test_the_twin_is_a_function_of_the_position_whatever_the_rows():
    ex = oracle_examples(3, 3, 8, orc.EVAL_HASH, q=True, kl=True)
    n = len(ex)
    pi, q, kl = reanalyse_twin(ex, None, 32, orc.EVAL_HASH)
    assert not np.array_equal(_bits(pi), _bits(ex.pi)) and (q != f32(-0.75)).all() and (kl != f32(-0.75)).all()
    assert np.allclose(pi.sum(1), 1.0, atol=1e-6) and (kl >= 0).all() and (np.abs(q) <= 1).all()
    rng = np.random.default_rng(0)
    perm = rng.permutation(n)
    dup = np.concatenate([perm, perm[:5], perm[::-1]])
    for rows in (perm, dup):
        p2, q2, k2 = reanalyse_twin(ex, rows, 32, orc.EVAL_HASH)
        assert np.array_equal(_bits(p2), _bits(pi)) and np.array_equal(_bits(q2), _bits(q)) and np.array_equal(_bits(k2), _bits(kl))
    # a subset leaves the other rows as they were
    sub = perm[: n // 2]
    p3, q3, k3 = reanalyse_twin(ex, sub, 32, orc.EVAL_HASH)
    rest = np.setdiff1d(np.arange(n), sub)
    assert np.array_equal(_bits(p3[sub]), _bits(pi[sub])) and np.array_equal(_bits(p3[rest]), _bits(ex.pi[rest]))
    assert np.array_equal(_bits(q3[rest]), _bits(ex.q[rest])) and np.array_equal(_bits(k3[sub]), _bits(kl[sub]))
    # pi is float32(N) / float32(sum N): at 32 simulations every entry is a multiple of 1 / 32 up to one rounding
    assert np.array_equal(_bits(pi), _bits(np.round(pi * 32).astype(np.float32) / f32(32)))


# ---------------------------------------------------------------- reanalyse_rows
def test_reanalyse_rows_is_a_sorted_distinct_draw_of_the_stated_size():
    for n, frac in ((1000, 0.25), (37, 0.5), (5, 0.3), (1, 1.0), (0, 0.5)):
        a = reanalyse_rows(n, frac, 3, (2, 1))
        assert a.dtype == torch.int64 and a.device.type == "cpu" and a.dim() == 1
        assert len(a) == int(round(frac * n))
        assert torch.equal(a, torch.unique(a)) and (len(a) == 0 or (int(a[0]) >= 0 and int(a[-1]) < n))
        assert torch.equal(a, reanalyse_rows(n, frac, 3, (2, 1)))


def test_reanalyse_rows_depends_on_seed_and_key_and_covers_the_ends():
    a = reanalyse_rows(1000, 0.25, 3, (2, 1))
    for other in (reanalyse_rows(1000, 0.25, 3, (2, 2)), reanalyse_rows(1000, 0.25, 3, (3, 1)), reanalyse_rows(1000, 0.25, 4, (2, 1)),
                  reanalyse_rows(1000, 0.25, 3, 2)):
        assert not torch.equal(a, other)
    assert len(reanalyse_rows(1000, 0.0, 0, 0)) == 0
    assert torch.equal(reanalyse_rows(1000, 1.0, 0, 0), torch.arange(1000))
    assert torch.equal(reanalyse_rows(1000, 1, 5, (9, 9)), torch.arange(1000))


@pytest.mark.parametrize("frac", [-0.01, 1.01, float("nan"), float("inf"), None, "0.5", True])
def test_reanalyse_rows_refuses_a_fraction_outside_0_1(frac):
    with pytest.raises(ValueError, match="frac"):
        reanalyse_rows(10, frac, 0, 0)


# ---------------------------------------------------------------- refusals, before an engine exists
def test_run_refuses_before_an_engine_is_built():
    """on a host without a device the engine itself raises RuntimeError (tests/test_abi.py): a ValueError here was raised
    before it was built.  With a device the same refusals leave the examples untouched."""
    ex = oracle_examples(3, 2, 8, orc.EVAL_HASH, q=True, kl=True)
    n = len(ex)
    before = dataclasses.replace(ex, pi=ex.pi.copy(), q=ex.q.copy(), kl=ex.kl.copy())
    ok = torch.arange(n, dtype=torch.int64)
    with pytest.raises(ValueError, match="board size"):
        reanalyse(ex, ok, sims=8, game="reversi")
    with pytest.raises(ValueError, match="count"):
        reanalyse(dataclasses.replace(ex, count=np.ones(n, np.int32)), ok, sims=8)
    with pytest.raises(ValueError, match="vt"):
        reanalyse(dataclasses.replace(ex, vt=np.zeros(n, np.float32)), ok, sims=8)
    with pytest.raises(ValueError, match="vt"):
        reanalyse(dataclasses.replace(ex, vt=np.zeros(n, np.float32)), None, sims=8, update_q=True)
    for bad in (torch.tensor([0, n], dtype=torch.int64), torch.tensor([-1, 0], dtype=torch.int64)):
        with pytest.raises(ValueError, match="outside 0"):
            reanalyse(ex, bad, sims=8)
    for bad in (ok.to(torch.int32), ok.to(torch.float32), ok.numpy(), list(range(n)), ok.reshape(1, -1)):
        with pytest.raises(ValueError, match="int64"):
            reanalyse(ex, bad, sims=8)
    with pytest.raises(ValueError, match="live on"):
        reanalyse(ex, ok.to("meta"), sims=8)
    with pytest.raises(ValueError, match="unknown game"):
        reanalyse(ex, ok, sims=8, game="chess")
    for k in ("pi", "q", "kl"):
        assert np.array_equal(_bits(getattr(ex, k)), _bits(getattr(before, k)))


@pytest.mark.skipif(_lib.lib().bz_device_count() > 0, reason="CPU-only check")
def test_vt_with_update_q_off_passes_the_checks_and_reaches_the_engine():
    ex = oracle_examples(3, 1, 8, orc.EVAL_HASH, q=True, vt=True)
    with pytest.raises(RuntimeError, match="no HIP device"):
        reanalyse(ex, None, sims=8, update_q=False)


# ---------------------------------------------------------------- the ABI
def test_the_abi_entry_points_refuse_bad_arguments_with_a_message():
    L = _lib.lib()
    one = np.zeros(4, np.uint64)
    p = one.ctypes.data
    assert L.bz_engine_reanalyse_load(None, p, p, p, 4, None, 0, 1, 1, None) == _lib.BZ_EINVAL
    assert b"bz_engine_reanalyse_load" in L.bz_last_error()
    assert L.bz_engine_reanalyse_store(None, p, None, None, 4, None, 0, 1, None) == _lib.BZ_EINVAL
    assert b"bz_engine_reanalyse_store" in L.bz_last_error()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bz_abi.h")).read()
    assert "#define BZ_ENGINE_ERR_REANALYSE_ROW 32" in hdr
