#!/usr/bin/env python3
"""The cost of evaluating under a hashed board symmetry, on against off, interleaved in one process.

(a) Tower time per launch: the fused net kernel at 256 rows (latency geometry) and 4096 rows (throughput geometry) of the
    bench's 128x6 net, bf16 and fp8, plain forward against symmetry="hash"; every repeat times a run of back-to-back
    launches of each of the eight configurations in turn with device events, medians over the repeats.
(b) Self-play at tools/az_loop.py's defaults (Reversi 8x8, 2048 games, the 64x4 bf16 net, 64 simulations, two pipelines,
    temp_moves 10, openings on, Dirichlet noise 0.3 / 0.25; a staggered pool that restarts finished games), eval_symmetry
    off against on: games/s, medians over the repeats.
One JSON object per line on stdout; the ratios on / off are in the "on" lines.

    python tools/bench_symmetry.py [--quick] [--out profiles/symmetry_bench.jsonl]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from betazero_amd.engine import EvalSymmetry, PipelinedSelfPlay  # noqa: E402
from betazero_amd.net import DeviceNet, PolicyValueNet  # noqa: E402

QUICK = "--quick" in sys.argv
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
REPS, LAUNCHES = (3, 20) if QUICK else (9, 1000)
GAMES, SIMS, SP_REPS, PER, PIPES = (256, 16, 3, 2, 2) if QUICK else (2048, 64, 7, 8, 2)
ROWS = (256, 4096)
SEED = 12345
DEV = "cuda:0"
lines = []


def emit(row):
    lines.append(row)
    print(json.dumps(row), flush=True)


# ---------------------------------------------------------------- (a) the tower
torch.manual_seed(0)
net = DeviceNet.from_module(PolicyValueNet(128, 6, 64).round_to_bf16_(), max(ROWS))
rng = np.random.default_rng(0)
cells = rng.integers(0, 3, size=(max(ROWS), 64))  # random positions: every cell empty / own / opp
w = np.uint64(1) << np.arange(64, dtype=np.uint64)
own = torch.as_tensor(((cells == 1) * w).sum(1, dtype=np.uint64).view(np.int64)).to(DEV)
opp = torch.as_tensor(((cells == 2) * w).sum(1, dtype=np.uint64).view(np.int64)).to(DEV)
configs = [(kind, rows, on) for kind in ("bf16", "fp8") for rows in ROWS for on in (False, True)]


def launches(kind, rows, on, count):
    kw = dict(symmetry="hash", seed=SEED) if on else {}
    for _ in range(count):
        net.forward(own[:rows], opp[:rows], fp8=kind == "fp8", **kw)


for cfg in configs:  # warm every shape the timed window uses
    launches(*cfg, 5)
torch.cuda.synchronize()
us = {cfg: [] for cfg in configs}
for _ in range(REPS):
    for cfg in configs:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launches(*cfg, LAUNCHES)
        b.record()
        b.synchronize()
        us[cfg].append(a.elapsed_time(b) * 1e3 / LAUNCHES)
for kind, rows, on in configs:
    med = statistics.median(us[(kind, rows, on)])
    row = dict(what="tower under a hashed symmetry", net="128x6", kind=kind, rows=rows, symmetry="hash" if on else None,
               launches_per_repeat=LAUNCHES, repeats=REPS, us_per_launch_median=round(med, 2),
               us_per_launch_min=round(min(us[(kind, rows, on)]), 2), us_per_launch_all=[round(x, 2) for x in us[(kind, rows, on)]])
    if on:
        row["on_over_off_median"] = round(med / statistics.median(us[(kind, rows, False)]), 4)
    emit(row)
del net

# ---------------------------------------------------------------- (b) self-play at the az_loop defaults
torch.manual_seed(0)
spnet = DeviceNet.from_module(PolicyValueNet(64, 4, 64).round_to_bf16_(), GAMES)
sps = []
for on in (False, True):
    sp = PipelinedSelfPlay("reversi", GAMES, SIMS, "net_bf16", spnet, pipelines=PIPES, temp_moves=10, openings=1, rounds=8, stagger=60,
                           seed=1, dirichlet_alpha=0.3, dirichlet_eps=0.25, eval_symmetry=EvalSymmetry(SEED) if on else None)
    sp.reset_games()
    for _ in range(2):
        sp.step(True)
    sp.status()
    sps.append(sp)
rates = [[], []]
for _ in range(SP_REPS):
    for sp, acc in zip(sps, rates):
        f0 = sp.status()[1]
        t0 = time.perf_counter()
        for _ in range(PER):
            sp.step(True)
            sp.sync()
        f1 = sp.status()[1]
        acc.append((f1 - f0) / (time.perf_counter() - t0))
for on, acc in zip((False, True), rates):
    row = dict(what="self-play under a hashed symmetry", net="64x4", games=GAMES, sims=SIMS, pipelines=PIPES,
               eval_symmetry=SEED if on else None, steps_per_repeat=PER, games_per_s_median=round(statistics.median(acc), 2),
               games_per_s_all=[round(x, 2) for x in acc])
    if on:
        row["on_over_off_median"] = round(statistics.median(acc) / statistics.median(rates[0]), 4)
    emit(row)
if OUT:
    with open(OUT, "w") as f:
        for row in lines:
            f.write(json.dumps(row) + "\n")
