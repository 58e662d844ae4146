"""The tower's workgroup shape follows the device-side row count ("the head of a move"): a device-count
forward over a throughput-sized buffer runs the latency shape up to kAdaptT1 rows and the throughput shape above it.
Whatever shape runs, every row is the same bits (adaptive off = the throughput shape always, what every such launch ran
before), rows from the count on are never written, a count of 0 runs nothing, and the per-net tally (kept by the launch
that did the work) names the shape the count calls for.  Then the same through the engine: a pool just above the
threshold, whose searches cross both tiers, gives identical games, rows, root statistics and counters either way.
Nothing here has a tolerance."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_N = 2048
SENTINEL = -12345.0
T1 = int(re.search(r"constexpr int kAdaptT1 = (\d+);", open(os.path.join(ROOT, "betazero_amd", "csrc", "bz_net.hip")).read()).group(1))
COUNTS = (0, 1, 3, 4, 5, T1 - 1, T1, T1 + 1, 2047, 2048)
_STATE = {}


def _setup():
    """the net (128 channels, one block, VH = 64, random bf16-rounded weights: the shapes differ in geometry only) and
    fixture F1's positions tiled to MAX_N rows, built once"""
    if not _STATE:
        from betazero_amd.net import DeviceNet, PolicyValueNet
        torch.manual_seed(11)
        net = DeviceNet.from_module(PolicyValueNet(128, 1, 64).round_to_bf16_(), MAX_N)
        d = np.load(os.path.join(ROOT, "tests", "golden", "reversi_random_games.npz"))["rows"]
        d = d[d[:, 1] == 8]
        idx = np.arange(MAX_N) % len(d)
        own = torch.from_numpy(d[idx, 2].astype(np.uint64).view(np.int64)).cuda()
        opp = torch.from_numpy(d[idx, 3].astype(np.uint64).view(np.int64)).cuda()
        _STATE.update(net=net, own=own, opp=opp, count=torch.zeros(1, dtype=torch.int32, device="cuda"))
    return _STATE["net"], _STATE["own"], _STATE["opp"], _STATE["count"]


def _counted(net, own, opp, count, n, mode, symmetry=None):
    """(logits bits, value bits, tally) of one device-count forward of n rows into sentinel-filled buffers"""
    net.set_adaptive_shape(mode)
    net.shape_tally()
    count.fill_(n)
    lg = torch.full((MAX_N, 65), SENTINEL, dtype=torch.float32, device="cuda")
    v = torch.full((MAX_N,), SENTINEL, dtype=torch.float32, device="cuda")
    net.forward_counted(own, opp, count, lg, v, symmetry=symmetry, seed=7)
    tally = net.shape_tally()
    net.set_adaptive_shape(1)
    return lg.cpu().numpy().view(np.uint32), v.cpu().numpy().view(np.uint32), tally


def _expected_tally(n, adaptive):
    shape = None if n == 0 else ("latency" if adaptive and n <= T1 else "throughput")
    return {k: int(k == shape) for k in ("latency", "middle", "throughput")}


def _check(n, symmetry):
    net, own, opp, count = _setup()
    sent = np.float32(SENTINEL).view(np.uint32)
    lg1, v1, t1 = _counted(net, own, opp, count, n, 1, symmetry)
    lg0, v0, t0 = _counted(net, own, opp, count, n, 0, symmetry)
    assert t1 == _expected_tally(n, True), (n, t1)
    assert t0 == _expected_tally(n, False), (n, t0)
    assert np.array_equal(lg1[:n], lg0[:n]) and np.array_equal(v1[:n], v0[:n]), n
    for lg, v in ((lg1, v1), (lg0, v0)):
        assert (lg[n:] == sent).all() and (v[n:] == sent).all(), n          # rows from the count on: untouched
        assert not (lg[:n] == sent).any() and not (v[:n] == sent).any(), n  # rows below it: all written
    return lg1, v1


@pytest.mark.parametrize("n", COUNTS)
def test_counted_forward_is_the_same_bits_in_either_shape(n):
    lg, v = _check(n, None)
    if n in (5, T1):  # and they are the rows of the host-count forward (its own shape choice: latency up to 256 rows)
        net, own, opp, _ = _setup()
        hl, hv = net.forward(own[:n].contiguous(), opp[:n].contiguous())
        assert np.array_equal(hl.cpu().numpy().view(np.uint32), lg[:n]) and np.array_equal(hv.cpu().numpy().view(np.uint32), v[:n])


@pytest.mark.parametrize("n", (5, T1, T1 + 1))
def test_counted_symmetric_forward_is_the_same_bits_in_either_shape(n):
    lg, v = _check(n, "hash")
    net, own, opp, _ = _setup()
    hl, hv = net.forward(own[:n].contiguous(), opp[:n].contiguous(), symmetry="hash", seed=7)
    assert np.array_equal(hl.cpu().numpy().view(np.uint32), lg[:n]) and np.array_equal(hv.cpu().numpy().view(np.uint32), v[:n])


def _selfplay(net, mode, B, moves):
    from betazero_amd.engine import SelfPlayEngine
    net.set_adaptive_shape(mode)
    net.shape_tally()
    eng = SelfPlayEngine("reversi", B, 32, "net_bf16", net=net, temp_moves=8, openings=1, seed=3, stagger=58, rounds=2,
                         eval_cache=True)
    eng.reset_games()
    stats = []
    for _ in range(moves):
        eng.search()
        stats.append([a.copy() for a in eng.root_stats()])
        eng.play(True)
    eng.status()
    out = {"positions": eng.positions(), "examples": eng.examples(), "stats": stats, "counters": eng.counters()}
    out["tally"] = net.shape_tally()
    net.set_adaptive_shape(1)
    return out


def test_selfplay_is_identical_with_the_shape_adapting_and_not():
    """B just above the threshold: the root evaluation and the dense simulations run the throughput shape, the head of
    every later move -- where the carried-over evaluations serve most slots -- the latency shape"""
    net, _, _, _ = _setup()
    B, moves = T1 + 32, 3
    on, off = _selfplay(net, 1, B, moves), _selfplay(net, 0, B, moves)
    print("tally on", on["tally"], "off", off["tally"], "counters", on["counters"], "rows", len(on["examples"]))
    assert on["counters"] == off["counters"]
    assert on["counters"]["n_cache_hits_prev"] > 0 and on["counters"]["n_net_leaves"] > 0
    for a, b in zip(on["positions"], off["positions"]):
        assert np.array_equal(a, b)
    for sa, sb in zip(on["stats"], off["stats"]):
        for a, b in zip(sa, sb):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    ea, eb = on["examples"], off["examples"]
    assert len(ea) == len(eb)
    for f in ("own", "opp", "pi", "z", "mover", "act", "game", "ply"):
        assert np.array_equal(getattr(ea, f), getattr(eb, f)), f
    assert on["tally"]["latency"] > 0 and on["tally"]["throughput"] > 0, on["tally"]    # a launch of each tier
    assert off["tally"]["latency"] == 0 and off["tally"]["middle"] == on["tally"]["middle"] == 0
    assert off["tally"]["throughput"] == on["tally"]["latency"] + on["tally"]["throughput"]  # the same launches did work
