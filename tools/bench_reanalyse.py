#!/usr/bin/env python3
"""Reanalysis on one MI355X: what refreshing a window of recorded rows costs, and what the fused load / store
kernels buy over the same refresh written with the pieces that were public before them.

Two arms, interleaved in one process on the SAME engines and streams, one warm-up each, then REPS timed repeats each:

  fused   Reanalyser.run: k_reanalyse_load, bz_engines_search, k_reanalyse_store -- indices and targets never leave the device,
          no temporary
  torch   per chunk: a torch gather of the chunk's boards and movers (padded to the engine's slots), bz_engine_set_roots,
          bz_engines_search, bz_engine_root_policy into a [B, NA] temporary (root_policy_dev), index_copy_ into pi

at az_loop's default shape (64x4 bf16 net, 64 simulations, two engines of 1024 slots) and at bench.py's (128x6 bf16 net; 64 and
800 simulations, two engines of 2048 slots).  The rows are recorded by one self-play iteration with the same net; they carry pi
only, so both arms write the same column, and the two results must be the same bits (asserted).  As context, on the same engines
at the same simulations: the self-play searches/s (reset_games, then PLIES moves of bz_engines_step -- search and play -- with
every game still running), and the searches alone (bz_engines_search on one round of loaded roots: no load, no store, no play).
Medians and the spread (min .. max) of the repeats; one JSON object per line on stdout.

    python tools/bench_reanalyse.py [--quick] [--shapes az,bench64,bench800] [--rows N] [--out profiles/reanalyse_bench.jsonl]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from betazero_amd import _lib  # noqa: E402
from betazero_amd.engine import PipelinedSelfPlay  # noqa: E402
from betazero_amd.net import DeviceNet, PolicyValueNet  # noqa: E402
from betazero_amd.reanalyse import Reanalyser  # noqa: E402


def _arg(name, default, conv=str):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


QUICK = "--quick" in sys.argv
OUT = _arg("--out", None)
DEV = "cuda:0"
REPS = 5
# name: (what, channels, blocks, slots per engine, simulations, rows refreshed per repeat)
SHAPES = {"az": ("az_loop defaults", 64, 4, 1024, 64, 32768), "bench64": ("bench.py shape, 64 simulations", 128, 6, 2048, 64, 32768),
          "bench800": ("bench.py shape, 800 simulations", 128, 6, 2048, 800, 16384)}
if QUICK:
    SHAPES = {"az": ("az_loop defaults (quick)", 64, 4, 256, 16, 1024)}
PICK = _arg("--shapes", ",".join(SHAPES)).split(",")
ROWS = _arg("--rows", None, int)
lines = []


def emit(row):
    lines.append(row)
    print(json.dumps(row), flush=True)


def record(dnet, games, rows):
    """`rows` recorded rows (pi only) of one 16-simulation self-play iteration with the net: the positions a window holds"""
    sp = PipelinedSelfPlay("reversi", games, 16, "net_bf16", dnet, pipelines=2, temp_moves=10, openings=1, seed=1,
                           dirichlet_alpha=0.3, dirichlet_eps=0.25)
    sp.run_iteration()
    ex = sp.device_examples()
    del sp
    assert len(ex) >= rows, (len(ex), rows)
    # spread over the plies: every rows-th of the recorded rows would favour nothing, a prefix would favour early games' slots
    idx = torch.linspace(0, len(ex) - 1, rows, device=DEV).to(torch.int64)
    from betazero_amd.train import select_rows
    return select_rows(ex, idx)


def torch_refresh(r, ex):
    """Reanalyser.run(ex) for pi, written with set_roots / root_policy and torch's gather and index_copy_"""
    L = _lib.lib()
    n, B, P = len(ex), r.batch, r.pipelines
    chunks = (n + B - 1) // B
    cur = torch.cuda.current_stream()
    for st in r.streams:
        st.wait_stream(cur)
    sts = (C.c_void_p * P)(*[st.cuda_stream for st in r.streams])
    keep = []
    for c0 in range(0, chunks, P):
        live = [i for i in range(P) if c0 + i < chunks]
        idxs = {}
        for i in live:
            with torch.cuda.stream(r.streams[i]):
                first = (c0 + i) * B
                idx = torch.arange(first, min(n, first + B), device=DEV)
                own, opp, tm = (torch.zeros(B, dtype=t.dtype, device=DEV) for t in (ex.own, ex.opp, ex.mover))
                own[:len(idx)], opp[:len(idx)], tm[:len(idx)] = ex.own[idx], ex.opp[idx], ex.mover[idx]
                _lib.check(L.bz_engine_set_roots(r.engines[i].h, own.data_ptr(), opp.data_ptr(), tm.data_ptr(), r.streams[i].cuda_stream))
                idxs[i] = idx
                keep.append((own, opp, tm))
        _lib.check(L.bz_engines_search((C.c_void_p * P)(*[r.engines[i].h if i in live else None for i in range(P)]), sts, P, r.run_ahead))
        for i in live:
            with torch.cuda.stream(r.streams[i]):
                pi, _ = r.engines[i].root_policy_dev()
                ex.pi.index_copy_(0, idxs[i], pi[:len(idxs[i])])
                keep.append(pi)
    for i in range(min(P, chunks)):
        with torch.cuda.stream(r.streams[i]):
            r.engines[i].status()
        cur.wait_stream(r.streams[i])
    del keep


def search_only(r, ex):
    """the searches of one round alone: both engines' roots loaded outside the timed region -> seconds per round"""
    L = _lib.lib()
    P, B, n = r.pipelines, r.batch, len(ex)
    for i in range(P):
        _lib.check(L.bz_engine_reanalyse_load(r.engines[i].h, ex.own.data_ptr(), ex.opp.data_ptr(), ex.mover.data_ptr(), n, None, i * B,
                                              min(B, n - i * B), 1, r.streams[i].cuda_stream))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _lib.check(L.bz_engines_search((C.c_void_p * P)(*[e.h for e in r.engines]), (C.c_void_p * P)(*[st.cuda_stream for st in r.streams]), P,
                                   r.run_ahead))
    torch.cuda.synchronize()
    return time.perf_counter() - t0


PLIES = 8   # no game of Reversi is over before its ninth move: every slot searches at every one of them


def self_play(r):
    """the same engines playing: PLIES moves of every slot from the start position -> seconds"""
    L = _lib.lib()
    P = r.pipelines
    for e, st in zip(r.engines, r.streams):
        with torch.cuda.stream(st):
            e.reset_games()
    hs, sts = (C.c_void_p * P)(*[e.h for e in r.engines]), (C.c_void_p * P)(*[st.cuda_stream for st in r.streams])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(PLIES):
        _lib.check(L.bz_engines_step(hs, sts, P, 0, r.run_ahead))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    for e, st in zip(r.engines, r.streams):
        with torch.cuda.stream(st):
            assert e.status()[0] == r.batch   # every game was still running: PLIES searches per slot
    return dt


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


for key in PICK:
    what, channels, blocks, slots, sims, rows = SHAPES[key]
    rows = ROWS or rows
    torch.manual_seed(0)
    dnet = DeviceNet.from_module(PolicyValueNet(channels, blocks, 64).round_to_bf16_(), 2 * slots)
    ex = record(dnet, 2 * slots, rows)
    ex.kl = ex.q = None
    r = Reanalyser("reversi", sims, "net_bf16", dnet, batch=slots, pipelines=2)
    a, b = ex, type(ex)(**{**vars(ex), "pi": ex.pi.clone()})
    r.run(a), torch_refresh(r, b)                                     # the warm-up, and the check: the same bits
    assert torch.equal(a.pi.view(torch.int32), b.pi.view(torch.int32)), "the fused and the torch refresh differ"
    t = {"fused": [], "torch": []}
    for _ in range(REPS):                                              # interleaved
        t["fused"].append(wall(lambda: r.run(a)))
        t["torch"].append(wall(lambda: torch_refresh(r, b)))
    assert torch.equal(a.pi.view(torch.int32), b.pi.view(torch.int32))
    so = [search_only(r, ex) for _ in range(1 + REPS)][1:]
    sp = [self_play(r) for _ in range(1 + REPS)][1:]
    played = 2 * slots * PLIES
    rate = lambda xs: {"rows_per_s_median": round(rows / statistics.median(xs), 1),                                  # noqa: E731
                       "rows_per_s_min_max": [round(rows / max(xs), 1), round(rows / min(xs), 1)], "seconds": [round(x, 4) for x in xs]}
    per_round = min(2 * slots, rows)
    emit(dict(what="reanalysis, fused load / store against the torch gather / scatter", shape=what, net=f"{channels}x{blocks} bf16 untrained",
              sims=sims, slots_per_engine=slots, pipelines=2, rows=rows, reps=REPS, same_bits=True, fused=rate(t["fused"]), torch=rate(t["torch"]),
              fused_over_torch=round(statistics.median(t["torch"]) / statistics.median(t["fused"]), 4),
              self_play={"searches_per_s_median": round(played / statistics.median(sp), 1),
                         "searches_per_s_min_max": [round(played / max(sp), 1), round(played / min(sp), 1)],
                         "note": f"reset_games, then {PLIES} moves (search + play) of every slot by bz_engines_step: plies 0 .. {PLIES - 1} of the game"},
              searches_alone={"rows_per_s_median": round(per_round / statistics.median(so), 1),
                              "rows_per_s_min_max": [round(per_round / max(so), 1), round(per_round / min(so), 1)],
                              "note": "bz_engines_search on one round of loaded roots, no load and no store"}))
    del r, ex, a, b, dnet
    torch.cuda.empty_cache()

if OUT:
    with open(OUT, "w") as f:
        for row in lines:
            f.write(json.dumps(row) + "\n")
