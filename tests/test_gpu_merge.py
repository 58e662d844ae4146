"""Position averaging on the GPU: merge_positions -- torch grouping, k_merge_zero / k_merge_reduce /
k_merge_finish -- against the Python-integer twin of tests/test_merge_cpu.py, bit for bit in every column and in the counts.
k_merge_reduce walks the sorted rows in chunks of 64 (a workgroup takes 64 rows at NA = 65 and 8 x 64 at NA = 9): the shapes
below put groups inside a chunk, across one and many chunk boundaries, and exactly between two boundaries."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from betazero_amd.engine import DeviceExamples, Examples
from betazero_amd.merge import merge_positions, merged_repeats
from test_merge_cpu import _bits, _examples, _random_group, merge_twin

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOISE = dict(dirichlet_alpha=0.3, dirichlet_eps=0.25)
FLOATS, INTS = ("pi", "vt", "q", "kl"), ("own", "opp", "z", "mover", "act", "game", "ply")


def _equals_twin(got, count, want, want_count):
    """host Examples + counts against merge_twin's columns: every column, bit for bit"""
    assert np.array_equal(np.asarray(count), want_count) and len(got) == len(want_count)
    for k in INTS:
        a, b = getattr(got, k), want[k]
        assert a.dtype == b.dtype and np.array_equal(a, b), (k, np.nonzero(a != b)[0][:8])
    for k in FLOATS:
        a, b = getattr(got, k), want[k]
        assert (a is None) == (b is None), k
        if a is not None:
            assert a.dtype == np.float32 and a.shape == b.shape, (k, a.shape, b.shape)
            assert np.array_equal(_bits(a), _bits(b)), (k, np.argwhere(_bits(a) != _bits(b))[:8])


def _merge_and_check(ex):
    """merge on the device, compare with the twin, check the properties every result has; -> (merged host Examples, counts)"""
    want, want_count, bad = merge_twin(ex)
    assert bad == 0
    out, count = merge_positions(DeviceExamples.from_host(ex, DEV), return_counts=True)
    assert isinstance(out, DeviceExamples) and out.pi.is_cuda and count.is_cuda and count.dtype == torch.int32 and out.size == ex.size
    got, count = out.cpu(), count.cpu().numpy()
    _equals_twin(got, count, want, want_count)
    n = len(ex)
    assert int(count.sum()) == n and (count >= 1).all()
    keys = list(zip(ex.own.tolist(), ex.opp.tolist()))
    firsts = sorted({k: i for i, k in reversed(list(enumerate(keys)))}.values())
    assert [keys[i] for i in firsts] == list(zip(got.own.tolist(), got.opp.tolist()))  # the order of the first occurrences
    if n:  # NA * 2^-32 from the truncation plus the input rows' own fp32 rounding
        assert np.abs(got.pi.sum(1, dtype=np.float64) - 1).max() < 1e-5
    return got, count


# ---------------------------------------------------------------- synthetic rows
@pytest.mark.parametrize("na", [9, 65])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 4099])
def test_merged_rows_equal_the_twin_in_every_column(na, n):
    have = dict(vt=n % 2 == 1, q=n % 4 < 2, kl=n in (63, 64, 4099))  # every column given at some size and absent at another
    ex = _examples(n, na, seed=n + na, pool=max(1, min(n // 3, 40)), **have)
    got, count = _merge_and_check(ex)
    if n > 3:
        assert count.max() > 1 and len(got) < n
    again, count2 = merge_positions(DeviceExamples.from_host(ex, DEV), return_counts=True)  # run to run: the same bits
    assert np.array_equal(_bits(again.pi.cpu().numpy()), _bits(got.pi)) and np.array_equal(count2.cpu().numpy(), count)
    assert merged_repeats(count2).tolist() == list(range(len(got)))
    assert torch.bincount(merged_repeats(count2, "log"), minlength=len(got)).tolist() == [c.bit_length() for c in count.tolist()]


@pytest.mark.parametrize("na", [9, 65])
def test_one_group_and_no_repeat_at_all(na):
    ex = _examples(700, na, seed=3, pool=1, vt=True, q=True, kl=True)  # one position: eleven chunks, one output row
    got, count = _merge_and_check(ex)
    assert count.tolist() == [700]
    ex = _examples(300, na, seed=4, q=True)
    ex.own = np.random.default_rng(5).permutation(300).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)  # all distinct
    got, count = _merge_and_check(ex)
    assert (count == 1).all() and len(got) == 300
    for k in ("own", "opp", "z", "mover", "act", "game", "ply"):  # the window comes back as it went in ...
        assert np.array_equal(getattr(got, k), getattr(ex, k)), k
    assert np.array_equal(_bits(got.pi), _bits(ex.pi)) and np.array_equal(_bits(got.q), _bits(ex.q)) and got.kl is None
    assert np.array_equal(got.vt, ex.z.astype(np.float32))  # ... plus vt = (float)z


def _layout(na, seed):
    """rows whose SORTED order is known (own ascending, all below 2^63): 64 single rows [0, 64), a group of 3000 rows
    [64, 3064) -- it starts on a chunk boundary and crosses 46 more --, a group of 8 rows [3064, 3072) that ends on one, a group
    of 64 rows [3072, 3136) that is exactly one chunk, a group of 128 rows [3136, 3264) that is exactly two, 30 single rows and
    a group of 2 rows, 3 times, so that pairs stand inside chunks; then everything interleaved by a random permutation"""
    sizes = [1] * 64 + [3000, 8, 64, 128] + ([1] * 30 + [2]) * 3
    own = np.repeat(np.arange(1, len(sizes) + 1, dtype=np.uint64) * np.uint64(1000), sizes)
    n = len(own)
    g = np.random.default_rng(seed)
    pi, z, vt, q, kl = _random_group(g, n, na)
    ex = Examples(own, np.full(n, 77, np.uint64), pi, z, np.where(g.random(n) < 0.5, 1, -1).astype(np.int8),
                  g.integers(0, na, n).astype(np.uint8), g.integers(0, 1000, n).astype(np.int64), g.integers(0, 60, n).astype(np.int32),
                  3 if na == 9 else 8, kl=kl, q=q, vt=vt)
    return ex, g.permutation(n), sizes


def _take(ex, p):
    return Examples(ex.own[p], ex.opp[p], ex.pi[p], ex.z[p], ex.mover[p], ex.act[p], ex.game[p], ex.ply[p], ex.size,
                    kl=None if ex.kl is None else ex.kl[p], q=None if ex.q is None else ex.q[p], vt=None if ex.vt is None else ex.vt[p])


@pytest.mark.parametrize("na", [9, 65])
def test_a_3000_row_group_among_single_rows_and_groups_that_start_and_end_on_chunk_boundaries(na):
    ex, p, sizes = _layout(na, 11 + na)
    ex = _take(ex, p)
    got, count = _merge_and_check(ex)
    assert sorted(count.tolist()) == sorted(sizes)


@pytest.mark.parametrize("na", [9, 65])
def test_shuffled_rows_give_the_same_merged_set(na):
    ex = _examples(1500, na, seed=21, pool=60, vt=True, q=True, kl=True)
    a, ca = merge_positions(DeviceExamples.from_host(ex, DEV), return_counts=True)
    p = np.random.default_rng(22).permutation(1500)
    sh = _take(ex, p)
    b, cb = merge_positions(DeviceExamples.from_host(sh, DEV), return_counts=True)
    a, b, ca, cb = a.cpu(), b.cpu(), ca.cpu().numpy(), cb.cpu().numpy()
    keys = list(zip(sh.own.tolist(), sh.opp.tolist()))
    assert list(zip(b.own.tolist(), b.opp.tolist())) == [keys[i] for i in sorted({k: i for i, k in reversed(list(enumerate(keys)))}.values())]
    where = {k: d for d, k in enumerate(zip(a.own.tolist(), a.opp.tolist()))}
    at = np.array([where[k] for k in zip(b.own.tolist(), b.opp.tolist())])
    assert sorted(at.tolist()) == list(range(len(a)))  # the same positions, in the order of the new first occurrences
    for k in ("pi", "vt", "q", "kl"):
        assert np.array_equal(_bits(getattr(b, k)), _bits(getattr(a, k)[at])), k
    assert np.array_equal(b.z, a.z[at]) and np.array_equal(cb, ca[at])


def test_bad_rows_raise_at_the_one_wait_and_name_the_count():
    ex = _examples(500, 65, seed=31, pool=20, vt=True)
    ex.pi[17, 3] = np.nan
    ex.vt[17] = 2.0       # the same row: one row
    with pytest.raises(RuntimeError, match=r"merge_positions: 1 row"):
        merge_positions(DeviceExamples.from_host(ex, DEV))
    ex.vt[400], ex.pi[401, 64] = -np.inf, -0.25
    with pytest.raises(RuntimeError, match=r"merge_positions: 3 row"):
        merge_positions(DeviceExamples.from_host(ex, DEV))
    assert merge_twin(ex)[2] == 3


def test_ownership_rows_are_refused_and_host_examples_come_back_as_host_examples():
    with pytest.raises(ValueError, match="ownership"):
        merge_positions(DeviceExamples.from_host(_examples(64, 65, own=True), DEV))
    ex = _examples(900, 9, seed=41, pool=30, vt=True, kl=True)
    host, hc = merge_positions(ex, return_counts=True)
    dev, dc = merge_positions(DeviceExamples.from_host(ex, DEV), return_counts=True)
    assert isinstance(host, Examples) and isinstance(hc, np.ndarray) and hc.dtype == np.int32 and host.own.dtype == np.uint64
    want, want_count, _ = merge_twin(ex)
    _equals_twin(host, hc, want, want_count)
    _equals_twin(dev.cpu(), dc.cpu().numpy(), want, want_count)
    assert isinstance(merge_positions(ex), Examples)
    empty = merge_positions(DeviceExamples.from_host(_examples(0, 65), DEV))
    assert len(empty) == 0 and empty.vt.is_cuda and empty.vt.shape == (0,)


# ---------------------------------------------------------------- real rows
def test_tic_tac_toe_self_play_rows_merge_and_the_augmented_empty_board_is_one_row():
    from betazero_amd.augment import augment_examples
    from betazero_amd.engine import self_play
    ex = self_play("ttt", 64, 16, evaluator="hash", seed=3, temp_moves=4, search_value=True, **NOISE)[3]
    assert (ex.own[ex.ply == 0] == 0).all() and (ex.opp[ex.ply == 0] == 0).all() and int((ex.ply == 0).sum()) == 64
    got, count = _merge_and_check(ex)
    assert len(got) < len(ex) and got.own[0] == 0 and got.opp[0] == 0 and count[0] == 64  # every game's first row: the empty board
    first = ex.pi[ex.ply == 0]
    assert len({r.tobytes() for r in first}) > 1               # (the noise: the rows being merged do differ)
    assert abs(float(got.vt[0]) - ex.z[ex.ply == 0].mean()) < 1e-6 and got.q is not None
    aug = augment_examples(DeviceExamples.from_host(ex, DEV), dedupe=True)
    m, mc = merge_positions(aug, return_counts=True)
    host = aug.cpu()
    want, want_count, bad = merge_twin(host)
    _equals_twin(m.cpu(), mc.cpu().numpy(), want, want_count)
    empty = int(((host.own == 0) & (host.opp == 0)).sum())
    assert bad == 0 and int(mc[0]) == empty and 64 < empty <= 8 * 64 and len(m) < len(aug)
    raw = augment_examples(DeviceExamples.from_host(ex, DEV), dedupe=False)   # every symmetric image kept: 8 x 64 rows, one position
    r, rc = merge_positions(raw, return_counts=True)
    assert int(rc[0]) == 8 * 64 and int(rc.sum()) == 8 * len(ex) and len(r) == len(m)


def test_two_graphed_steps_on_merged_reversi_rows():
    from betazero_amd.engine import self_play
    from betazero_amd.net import PolicyValueNet
    from betazero_amd.train import GraphedTrainStep
    ex = self_play("reversi", 64, 16, evaluator="hash", seed=5, temp_moves=6, openings=1, **NOISE)[3]
    data, count = merge_positions(DeviceExamples.from_host(ex, DEV), return_counts=True)
    assert 64 < len(data) < len(ex) and int(count.max()) > 1 and data.vt is not None
    vt = data.vt.cpu().numpy()
    assert (np.abs(vt) <= 1).all() and (vt != np.round(vt)).any()   # averaged outcomes: no longer +-1
    torch.manual_seed(0)
    step = GraphedTrainStep(PolicyValueNet(64, 4, 64, fused_tower=True).cuda(), lr=1e-3, batch=64, value_targets=True)
    gen = torch.Generator(device=DEV).manual_seed(0)
    rep = merged_repeats(count, "log")
    losses = [step(data, rep[torch.randint(0, len(rep), (64,), device=DEV, generator=gen)]) for _ in range(2)]
    step.check()
    assert np.isfinite(torch.stack(losses).cpu().numpy()).all()


@pytest.mark.parametrize("weight", ["constant", "log"])
def test_az_loop_runs_two_iterations_with_merged_positions(weight):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "az_loop.py"), "--iters", "2", "--games", "64", "--sims", "16",
                          "--merge-positions", "--merge-weight", weight, "--channels", "64", "--blocks", "1",
                          "--arena-games", "16", "--arena-sims", "8", "--depth", "1", "--final-depths", ""],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    its = [d for d in (json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")) if d.get("what") == "iteration"]
    assert [d["iter"] for d in its] == [1, 2]
    for d in its:
        m = d["merge"]
        assert m["weight"] == weight and 0 < m["rows_after"] < m["rows_before"] and m["largest_group"] > 1, d
        assert 0 < m["share_rows_in_groups"] <= 1 and d["train_rows"] == m["rows_after"] and np.isfinite(d["loss_last_tenth"]).all(), d
