"""Reanalysis on the GPU: Reanalyser.run -- k_reanalyse_load, bz_engines_search, k_reanalyse_store -- against the
oracle's search through reanalyse_twin (plain PUCT: uniform, hash and the exact bf16 net), against the engine's own public path
set_roots -> search -> root_policy / root_stats in every search mode it accepts, and held to what its docstring promises: nothing
but the refreshed columns of the named rows moves, the chunking and the order of the rows do not matter, new weights in the
shared net take effect, refusals leave the examples alone, and tools/az_loop.py --reanalyse-frac resumed from a checkpoint is
the uninterrupted run.  The rows are recorded by a short self-play inside each test.  "Equal" = bit for bit; nothing here has a
tolerance."""
import ctypes as C
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from betazero_amd import _lib
from oracle import oracle as orc
from test_reanalyse_cpu import reanalyse_twin, root_targets

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORC_EVAL = {"uniform": orc.EVAL_UNIFORM, "hash": orc.EVAL_HASH, "net_bf16": orc.EVAL_NET_BF16}
COLUMNS = ("own", "opp", "pi", "z", "mover", "act", "game", "ply", "kl", "q", "vt", "fown", "fopp")


def _raw(t):
    """a tensor's bytes, on the host"""
    return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu()


def _f32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


RECORD_SIMS = 8   # fewer than any reanalysis below: a recorded row's targets are never what its reanalysis gives


def _record(game, n_games, evaluator, rows, net=None, vt=False, sims=RECORD_SIMS, tail=False):
    """the first (tail: the last) `rows` rows of a short self-play (4 sampled moves per game, so that the games differ), with the
    recorded kl and q columns -- and a made-up vt column where asked for"""
    from betazero_amd.engine import SelfPlayEngine
    from betazero_amd.train import select_rows
    eng = SelfPlayEngine(game, n_games, sims, evaluator, net=net, temp_moves=4, seed=5, surprise=True, search_value=True)
    eng.run_iteration()
    ex = eng.device_examples()
    assert len(ex) >= rows, (len(ex), rows)
    ex = select_rows(ex, torch.arange(rows, device=DEV) + (len(ex) - rows if tail else 0))
    if vt:
        ex.vt = torch.linspace(-1, 1, rows, device=DEV)
    return ex


def _clone(ex):
    return dataclasses.replace(ex, **{k: getattr(ex, k).clone() for k in COLUMNS if getattr(ex, k) is not None})


def _same(a, b, cols=COLUMNS, rows=None):
    for k in cols:
        x, y = getattr(a, k), getattr(b, k)
        assert (x is None) == (y is None), k
        if x is not None:
            assert torch.equal(_raw(x if rows is None else x[rows]), _raw(y if rows is None else y[rows])), k


def _equals_twin(ex, twin):
    pi, q, kl = twin
    h = ex.cpu()
    assert np.array_equal(_f32(h.pi), _f32(pi)), np.nonzero((_f32(h.pi) != _f32(pi)).any(1))[0]
    assert np.array_equal(_f32(h.q), _f32(q)), np.nonzero(_f32(h.q) != _f32(q))[0]
    assert np.array_equal(_f32(h.kl), _f32(kl)), np.nonzero(_f32(h.kl) != _f32(kl))[0]


# ---------------------------------------------------------------- 1. against the oracle, plain PUCT
@pytest.mark.parametrize("evaluator", ["uniform", "hash"])
def test_tic_tac_toe_three_chunks_with_a_tail_equal_the_oracle(evaluator):
    """21 rows in chunks of 8 on two engines: 8, 8 and a tail of 5 (three idle slots), the third chunk alone in its round (the
    other engine sits it out).  The fused tic-tac-toe search."""
    from betazero_amd.reanalyse import Reanalyser
    ex = _record("ttt", 8, evaluator, 21)
    twin = reanalyse_twin(ex.cpu(), None, 32, ORC_EVAL[evaluator])
    before = _clone(ex)
    out = Reanalyser("ttt", 32, evaluator, batch=8, pipelines=2).run(ex)
    assert (out["rows"], out["chunks"]) == (21, 3) and "n_sims" in out["counters"]
    _equals_twin(ex, twin)
    _same(ex, before, [c for c in COLUMNS if c not in ("pi", "q", "kl")])
    assert not torch.equal(_raw(ex.pi), _raw(before.pi))


def test_reversi_unsorted_rows_with_a_duplicate_equal_the_oracle():
    from betazero_amd.reanalyse import Reanalyser
    ex = _record("reversi", 2, "hash", 40)
    rng = np.random.default_rng(3)
    pick = rng.permutation(40)[:25]
    rows = np.concatenate([pick[:10], pick[3:4], pick[10:], pick[:1]])   # 27 indices: unsorted, two of them twice
    twin = reanalyse_twin(ex.cpu(), rows, 16, orc.EVAL_HASH)
    before = _clone(ex)
    out = Reanalyser("reversi", 16, "hash", batch=16, pipelines=2).run(ex, torch.as_tensor(rows, dtype=torch.int64, device=DEV))
    assert (out["rows"], out["chunks"]) == (27, 2)
    _equals_twin(ex, twin)
    rest = torch.as_tensor(np.setdiff1d(np.arange(40), rows), device=DEV)
    _same(ex, before, COLUMNS, rest)
    assert not torch.equal(_raw(ex.pi[torch.as_tensor(pick, device=DEV)]), _raw(before.pi[torch.as_tensor(pick, device=DEV)]))


def test_reversi6_with_the_exact_bf16_net_equals_the_oracle():
    from betazero_amd.reanalyse import Reanalyser
    from test_gpu_search_net import _dn, _net
    P, on = _net("bf16", 64, 1)
    dn = _dn(P, 8)
    ex = _record("reversi6", 2, "net_bf16", 10, net=dn)
    twin = reanalyse_twin(ex.cpu(), None, 16, orc.EVAL_NET_BF16, net=on)
    out = Reanalyser("reversi6", 16, "net_bf16", net=dn, batch=4, pipelines=2).run(ex)
    assert (out["rows"], out["chunks"]) == (10, 3)
    _equals_twin(ex, twin)


# ---------------------------------------------------------------- 2. against the engine's own public path, every mode
def _engine_targets(game, sims, evaluator, net, ex, opts, info=None):
    """(pi, q, kl) of every row of ex from ONE SelfPlayEngine of len(ex) slots with the same options: set_roots -> search ->
    root_policy() for pi, root_stats() with bz_root_value / bz_surprise_kl on the host for q and kl"""
    from betazero_amd.engine import SelfPlayEngine
    h = ex.cpu()
    n = len(h)
    eng = SelfPlayEngine(game, n, sims, evaluator, net=net, **opts)
    eng.set_roots(h.own, h.opp, h.mover)
    eng.search()
    eng.status()
    pi, act = eng.root_policy()
    N, W, P = eng.root_stats()
    assert (act >= 0).all()
    q, kl = np.zeros(n, np.float32), np.zeros(n, np.float32)
    L = _lib.lib()
    if info is not None:   # what the mode tests ask about the search itself: the raw visits, and what the solver decided
        info.update(N=N, n_decided=eng.proven()[2]["n_decided"] if opts.get("solver") else None)
    for g in range(n):
        _, q[g], _ = root_targets(N[g], W[g], P[g])          # (q is of the raw statistics whatever pi is)
        ed = np.nonzero((P[g] > 0) | (N[g] > 0))[0]
        a, b, out = np.ascontiguousarray(pi[g][ed]), np.ascontiguousarray(P[g][ed]), C.c_float()
        _lib.check(L.bz_surprise_kl(a.ctypes.data, b.ctypes.data, len(ed), C.addressof(out)))
        kl[g] = out.value
    return pi, q, kl


def _modes():
    from betazero_amd.engine import ForcedPlayouts, Fpu, GumbelConfig
    from betazero_amd.symmetry import EvalSymmetry
    return {"gumbel": dict(gumbel=GumbelConfig()), "gumbel_interior": dict(gumbel=GumbelConfig(interior="gumbel")),
            "fpu": dict(fpu=Fpu()), "forced_pruned": dict(forced_playouts=ForcedPlayouts(2.0, True)), "solver": dict(solver=True),
            "eval_symmetry": dict(eval_symmetry=EvalSymmetry(77)), "leaves_4": dict(leaves_per_step=4)}


@pytest.mark.parametrize("mode", ["gumbel", "gumbel_interior", "fpu", "forced_pruned", "solver", "eval_symmetry", "leaves_4"])
def test_every_accepted_mode_equals_the_engines_public_path(mode):
    """Reversi 8x8, 16 simulations, 20 rows in chunks of 8 against one engine of 20 slots.  The hash evaluator -- except under
    the evaluation symmetry, which the synthetic evaluators refuse: there the exact bf16 net (64 channels, one block).  Every
    mode is shown to have been at work on these rows: its visits are not the plain search's on some row; where the mode has a
    pi of its own (Gumbel, forced playouts with pruning) that pi is not the raw N / sum N on some row; the solver -- on the
    LAST 20 rows of the games, where there is something to prove -- decided nodes.  (The solver is held to that alone: its pi
    is N / sum N by definition, and a proof changes the visits only where a later walk would have entered the decided edge --
    at 16 simulations on these rows none does: 25 nodes decided, the visits of all 20 rows the plain search's.)"""
    from betazero_amd.reanalyse import Reanalyser
    opts = _modes()[mode]
    evaluator, net = "hash", None
    if mode == "eval_symmetry":
        from test_gpu_search_net import _dn, _net
        evaluator, net = "net_bf16", _dn(_net("bf16", 64, 1)[0], 32)
    ex = _record("reversi", 2, "hash", 20, tail=mode == "solver")
    info, plain = {}, {}
    pi, q, kl = _engine_targets("reversi", 16, evaluator, net, ex, opts, info)
    _engine_targets("reversi", 16, evaluator, net, ex, {}, plain)
    N = info["N"]
    raw = N.astype(np.float32) / N.sum(1, keepdims=True).astype(np.float32)
    moved, own_pi = int((N != plain["N"]).any(1).sum()), int((_f32(pi) != _f32(raw)).any(1).sum())
    print(f"{mode}: rows whose visits differ from the plain search's {moved} / 20, rows whose pi is not N / sum N {own_pi} / 20, "
          f"edges the solver decided {info['n_decided']}")
    assert moved > 0 or mode == "solver"
    assert (own_pi > 0) == (mode in ("gumbel", "gumbel_interior", "forced_pruned"))
    assert mode != "solver" or info["n_decided"] > 0
    before = _clone(ex)
    out = Reanalyser("reversi", 16, evaluator, net=net, batch=8, pipelines=2, **opts).run(ex)
    assert (out["rows"], out["chunks"]) == (20, 3)
    _equals_twin(ex, (pi, q, kl))
    assert not torch.equal(_raw(ex.pi), _raw(before.pi))


# ---------------------------------------------------------------- 3. nothing else moves
def test_nothing_but_the_refreshed_columns_of_the_named_rows_moves():
    from betazero_amd.reanalyse import Reanalyser
    ex = _record("reversi", 2, "hash", 30, vt=True)
    ex.fown, ex.fopp = ex.own.clone(), ex.opp.clone()   # (any bits: columns the run has no business with)
    before = _clone(ex)
    rows = torch.tensor([29, 3, 4, 17, 8, 3, 11, 0, 21], dtype=torch.int64, device=DEV)
    rest = torch.as_tensor(np.setdiff1d(np.arange(30), rows.cpu().numpy()), device=DEV)
    r = Reanalyser("reversi", 16, "hash", batch=4, pipelines=2)
    with pytest.raises(ValueError, match="vt"):
        r.run(ex, rows)          # update_q defaults to True: vt would go stale
    _same(ex, before)
    r.run(ex, rows, update_q=False)
    _same(ex, before, [c for c in COLUMNS if c not in ("pi", "kl")])     # q and vt included
    _same(ex, before, ("pi", "kl"), rest)
    named = torch.unique(rows)
    assert not torch.equal(_raw(ex.pi[named]), _raw(before.pi[named])) and not torch.equal(_raw(ex.kl[named]), _raw(before.kl[named]))
    # without the kl and q columns only pi is written
    bare = dataclasses.replace(_clone(before), kl=None, q=None, vt=None)
    r.run(bare, rows)
    assert torch.equal(_raw(bare.pi), _raw(ex.pi)) and bare.kl is None and bare.q is None
    # and with update_q the q column follows the twin while everything else is as above
    withq = dataclasses.replace(_clone(before), vt=None)
    r.run(withq, rows)
    twin = reanalyse_twin(dataclasses.replace(before, vt=None).cpu(), rows.cpu().numpy(), 16, orc.EVAL_HASH)
    _equals_twin(withq, twin)


# ---------------------------------------------------------------- 4. the chunking does not matter
def test_chunking_pipelines_and_repetition_do_not_matter():
    from betazero_amd.reanalyse import Reanalyser
    ex = _record("reversi", 2, "hash", 23)
    a, b = _clone(ex), _clone(ex)
    ra = Reanalyser("reversi", 16, "hash", batch=8, pipelines=1)
    ra.run(a)
    Reanalyser("reversi", 16, "hash", batch=5, pipelines=2).run(b)
    _same(a, b)
    assert not torch.equal(_raw(a.pi), _raw(ex.pi))
    again = _clone(a)
    ra.run(again)
    _same(again, a)
    perm = torch.as_tensor(np.random.default_rng(1).permutation(23), dtype=torch.int64, device=DEV)
    c = _clone(ex)
    ra.run(c, torch.cat([perm, perm[:7]]))
    _same(c, a)


def test_strided_views_of_rows_are_read_as_the_indices_they_show():
    """rows = base[::2] (stride 2) and a scalar expanded to 5 entries (stride 0, one element of storage): the named rows equal the
    twin, every other row equals the clone"""
    from betazero_amd.reanalyse import Reanalyser
    ex = _record("reversi", 2, "hash", 30)
    before = _clone(ex)
    base = torch.tensor([7, 1, 22, 2, 3, 4, 15, 5, 0, 6, 29, 8, 11, 9, 18, 10, 26], dtype=torch.int64, device=DEV)
    view = base[::2]
    assert not view.is_contiguous() and view.numel() == 9
    named = view.cpu().numpy()
    r = Reanalyser("reversi", 16, "hash", batch=4, pipelines=2)
    out = r.run(ex, view)
    assert (out["rows"], out["chunks"]) == (9, 3)
    _equals_twin(ex, reanalyse_twin(before.cpu(), named, 16, orc.EVAL_HASH))
    _same(ex, before, COLUMNS, torch.as_tensor(np.setdiff1d(np.arange(30), named), device=DEV))
    assert not torch.equal(_raw(ex.pi[view]), _raw(before.pi[view]))
    one = _clone(before)
    r.run(one, torch.tensor([13], dtype=torch.int64, device=DEV).expand(5))
    _equals_twin(one, reanalyse_twin(before.cpu(), [13], 16, orc.EVAL_HASH))
    _same(one, before, COLUMNS, torch.as_tensor(np.setdiff1d(np.arange(30), [13]), device=DEV))


# ---------------------------------------------------------------- 5. a weight update takes effect
def test_new_weights_in_the_shared_net_take_effect():
    """run, refresh_device_net with another net's weights, run again on the same Reanalyser: the second run is a fresh
    Reanalyser's on a net built from the vector the refresh pushed (its bf16-rounded copy of the module), not the first run's"""
    from betazero_amd.net import DeviceNet
    from betazero_amd.reanalyse import Reanalyser
    from betazero_amd.train import refresh_device_net
    from test_gpu_search_net import _dn, _net
    from test_net_numerics_cpu import to_module
    from test_search_net_cpu import VH
    (PA, _), (PB, _) = _net("bf16", 64, 1, 1), _net("bf16", 64, 1, 2)
    dn = _dn(PA, 8)
    ex = _record("reversi6", 2, "net_bf16", 10, net=dn)
    r = Reanalyser("reversi6", 16, "net_bf16", net=dn, batch=4, pipelines=2)
    first = _clone(ex)
    r.run(first)
    flat = refresh_device_net(dn, to_module(PB, torch.float32))
    second = _clone(ex)
    r.run(second)
    fresh = _clone(ex)
    Reanalyser("reversi6", 16, "net_bf16", net=DeviceNet(64, 1, VH, flat, 8), batch=4, pipelines=2).run(fresh)
    _same(second, fresh)
    assert not torch.equal(_raw(second.pi), _raw(first.pi))
    _same(second, ex, [c for c in COLUMNS if c not in ("pi", "q", "kl")])


# ---------------------------------------------------------------- 6. refusals
def test_an_index_out_of_range_is_refused_with_the_examples_untouched():
    from betazero_amd.reanalyse import Reanalyser
    ex = _record("ttt", 4, "hash", 12)
    before = _clone(ex)
    r = Reanalyser("ttt", 16, "hash", batch=8, pipelines=2)
    for bad in ([0, 12], [-1, 3], [2 ** 40]):
        with pytest.raises(ValueError, match="outside 0"):
            r.run(ex, torch.tensor(bad, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="int64"):
        r.run(ex, torch.tensor([0], dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="live on"):
        r.run(ex, torch.tensor([0], dtype=torch.int64))
    with pytest.raises(ValueError, match="board size"):
        Reanalyser("reversi", 16, "hash", batch=8, pipelines=1).run(ex)
    with pytest.raises(ValueError, match="count"):
        r.run(dataclasses.replace(ex, count=torch.ones(12, dtype=torch.int32, device=DEV)))
    _same(ex, before)
    # the kernel's own guard, past the Python check: the slot stays idle, the error bit is raised, nothing is written
    e, st = r.engines[0], torch.cuda.current_stream()
    L = _lib.lib()
    rows = torch.tensor([1, 12, 2, -5], dtype=torch.int64, device=DEV)
    _lib.check(L.bz_engine_reanalyse_load(e.h, ex.own.data_ptr(), ex.opp.data_ptr(), ex.mover.data_ptr(), 12, rows.data_ptr(), 0, 4, 1, st.cuda_stream))
    _, _, _, state = e.positions()
    assert list(state) == [0, 1, 0, 1, 1, 1, 1, 1]
    e.search()
    _lib.check(L.bz_engine_reanalyse_store(e.h, ex.pi.data_ptr(), ex.q.data_ptr(), ex.kl.data_ptr(), 12, rows.data_ptr(), 0, 4, st.cuda_stream))
    with pytest.raises(RuntimeError, match="reanalyse row index out of range"):
        e.status()
    keep = torch.tensor([r_ for r_ in range(12) if r_ not in (1, 2)], device=DEV)
    _same(ex, before, COLUMNS, keep)
    twin = reanalyse_twin(before.cpu(), [1, 2], 16, orc.EVAL_HASH)
    _equals_twin(ex, twin)
    cols = (ex.own.data_ptr(), ex.opp.data_ptr(), ex.mover.data_ptr())
    for n_rows, first, count in ((12, 0, 9), (12, 0, -1), (12, -1, 4), (-1, 0, 4)):   # count outside 0 .. 8, negative first / n_rows
        assert L.bz_engine_reanalyse_load(e.h, *cols, n_rows, None, first, count, 1, st.cuda_stream) == _lib.BZ_EINVAL
        assert L.bz_engine_reanalyse_store(e.h, ex.pi.data_ptr(), None, None, n_rows, None, first, count, st.cuda_stream) == _lib.BZ_EINVAL
    assert L.bz_engine_reanalyse_load(e.h, None, cols[1], cols[2], 12, None, 0, 4, 1, st.cuda_stream) == _lib.BZ_EINVAL
    assert L.bz_engine_reanalyse_store(e.h, None, None, None, 12, None, 0, 4, st.cuda_stream) == _lib.BZ_EINVAL


def test_a_terminal_row_raises_and_the_other_rows_are_still_written():
    from betazero_amd.reanalyse import Reanalyser
    ex = _record("ttt", 4, "hash", 12)
    # row 5 by hand: a full board without a line (X O X / X O O / O X X), X = own, nobody to move
    x = 0b110001101
    ex.own[5], ex.opp[5], ex.mover[5] = x, 0x1FF & ~x, 1
    before = _clone(ex)
    others = [r for r in range(12) if r != 5]
    twin = reanalyse_twin(before.cpu(), others, 16, orc.EVAL_HASH)
    r = Reanalyser("ttt", 16, "hash", batch=8, pipelines=2)
    with pytest.raises(RuntimeError, match="terminal root"):
        r.run(ex)
    _equals_twin(ex, twin)                      # row 5 keeps what it had, every other row is the twin's
    _same(ex, before, COLUMNS, torch.tensor([5], device=DEV))
    # the flag does not outlive the run that raised it
    good = _clone(before)
    r.run(good, torch.tensor(others, dtype=torch.int64, device=DEV))
    _equals_twin(good, twin)


# ---------------------------------------------------------------- 7. the loop
SMALL = ["--games", "64", "--sims", "16", "--channels", "64", "--blocks", "1", "--arena-games", "16", "--arena-sims", "8", "--depth", "1",
         "--final-depths", "", "--batch", "64"]   # tests/test_gpu_checkpoint.py's shape
TIMING = ("seconds", "self_play_s", "games_per_s", "train_s", "reanalyse_s")
NEW_KEYS = ("reanalysed_rows", "reanalyse_s", "reanalyse_argmax_changed")


def _loop(*flags):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "az_loop.py"), *SMALL, *flags], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    return [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]


def _untimed(d):
    if isinstance(d, dict):
        return {k: _untimed(v) for k, v in d.items() if k not in TIMING}
    return [_untimed(v) for v in d] if isinstance(d, list) else d


def test_az_loop_with_reanalysis_resumed_from_a_checkpoint_is_the_uninterrupted_run(tmp_path):
    """three iterations in one process against two, a checkpoint, and one more in a second process: the same lines, weights
    hashes and saved net.  Rows are reanalysed from the second iteration on (the first has no older slot: it is the iteration
    of a run without reanalysis), and with --reanalyse-frac 0 the loop prints what it prints without the flag."""
    flags = ["--reanalyse-frac", "0.5", "--surprise", "--value-lambda", "0.9"]
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    whole = _loop(*flags, "--iters", "3", "--checkpoint", str(a / "run.ckpt"), "--save-net", str(a / "net.pt"))
    first = _loop(*flags, "--iters", "2", "--checkpoint", str(b / "run.ckpt"))
    second = _loop(*flags, "--iters", "3", "--resume", str(b / "run.ckpt"), "--checkpoint", str(b / "run.ckpt"), "--save-net", str(b / "net.pt"))
    its = lambda lines: [d for d in lines if d.get("what") == "iteration"]  # noqa: E731
    assert [d["iter"] for d in its(whole)] == [1, 2, 3] and [d["iter"] for d in its(first)] == [1, 2] and [d["iter"] for d in its(second)] == [3]
    for x, y in zip(its(whole), its(first) + its(second)):
        assert x["weights_hash"] == y["weights_hash"], (x["iter"], x["weights_hash"], y["weights_hash"])
        assert _untimed(x) == _untimed(y), x["iter"]
    assert _untimed(whole) == _untimed(first + its(second))
    assert open(a / "net.pt", "rb").read() == open(b / "net.pt", "rb").read()
    rows = [d["reanalysed_rows"] for d in its(whole)]
    assert rows[0] == 0 and rows[1] > 0 and rows[2] > rows[1], rows          # one older slot, then two
    assert all(0.0 <= d["reanalyse_argmax_changed"] <= 1.0 for d in its(whole)) and its(whole)[1]["reanalyse_argmax_changed"] > 0
    # off: the flag at 0 is the loop without the flag, and neither prints a reanalysis key
    off = _loop("--reanalyse-frac", "0", "--surprise", "--value-lambda", "0.9", "--iters", "2")
    assert _untimed(off) == _untimed(_loop("--surprise", "--value-lambda", "0.9", "--iters", "2"))   # whole lines, timings apart
    assert not any(k in d for d in off for k in NEW_KEYS)
    # the first iteration reanalyses nothing, so it is the first iteration of the loop without reanalysis; the second is not
    strip = lambda d: {k: v for k, v in _untimed(d).items() if k not in NEW_KEYS}  # noqa: E731
    assert strip(its(whole)[0]) == strip(its(off)[0]) and [strip(d) for d in whole[:2]] == [strip(d) for d in off[:2]]
    assert its(whole)[1]["weights_hash"] != its(off)[1]["weights_hash"]
    # a resumed run may not change the two flags
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "az_loop.py"), *SMALL, "--surprise", "--value-lambda", "0.9", "--reanalyse-frac",
                          "0.25", "--iters", "3", "--resume", str(b / "run.ckpt")], capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "--reanalyse-frac differs" in bad.stderr
