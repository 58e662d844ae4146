#!/usr/bin/env python3
"""Policy surprise weighting against the plain engine, surprise off and on interleaved in one process.  Fixed
(cfg 3's shape, the headline's): Reversi 8x8, 4096 games, the bench's 128x6 bf16 net, 800 simulations, evaluation cache on
(carry), two pipelines, temp_moves 8, openings on, a staggered pool that restarts finished games -- once without Dirichlet
noise (the headline) and once
with it (0.3, 0.25: tools/az_loop.py's self-play).  With surprise on a move costs three more one-lane-per-game launches (the
prior's copy, two around the play kernel) against 800 tree steps and 801 net launches.  Per configuration, medians
over the repeats: games/s.  Then surprise_resample at the sizes of a training window (rows of synthetic kl, exponentially
distributed): milliseconds per call, the wait for the size read-back included.  One JSON object per line on stdout.

    python tools/bench_surprise.py [--quick] [--out profiles/surprise_bench.jsonl]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from betazero_amd.engine import DeviceExamples, Examples, PipelinedSelfPlay  # noqa: E402
from betazero_amd.net import DeviceNet, PolicyValueNet  # noqa: E402
from betazero_amd.surprise import surprise_resample  # noqa: E402

QUICK = "--quick" in sys.argv
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
SIMS, B = (64, 512) if QUICK else (800, 4096)
NOISE = dict(dirichlet_alpha=0.3, dirichlet_eps=0.25)
CONFIGS = [(noise, on) for noise in (False, True) for on in (False, True)]
REPS, PER, PIPES = (3, 2, 2) if QUICK else (5, 4, 2)
WINDOWS = (1 << 14, 1 << 17) if QUICK else (237_000, 1 << 21, 1 << 23)  # one iteration's rows; an augmented window; a large one

torch.manual_seed(0)
net = DeviceNet.from_module(PolicyValueNet(128, 6, 64).round_to_bf16_(), B // PIPES)

sps = []
for noise, on in CONFIGS:
    sp = PipelinedSelfPlay("reversi", B, SIMS, "net_bf16", net, pipelines=PIPES, temp_moves=8, openings=1, rounds=8, stagger=60,
                           surprise=on, **(NOISE if noise else {}))
    sp.reset_games()
    for _ in range(2):
        sp.step(True)
    sp.status()
    sps.append(sp)

rates = [[] for _ in CONFIGS]
for r in range(REPS):
    for sp, acc in zip(sps, rates):
        f0 = sp.status()[1]
        t0 = time.perf_counter()
        for _ in range(PER):
            sp.step(True)
            sp.sync()
        f1 = sp.status()[1]
        acc.append((f1 - f0) / (time.perf_counter() - t0))
del sps

lines = []
for (noise, on), acc in zip(CONFIGS, rates):
    lines.append(dict(what="surprise, self-play", surprise=on, dirichlet=[NOISE["dirichlet_alpha"], NOISE["dirichlet_eps"]] if noise else None,
                      games=B, sims=SIMS, pipelines=PIPES, steps_per_repeat=PER, games_per_s_median=statistics.median(acc),
                      games_per_s_all=[round(x, 2) for x in acc]))
for noise in (False, True):
    off, on = (statistics.median(acc) for (nz, _), acc in zip(CONFIGS, rates) if nz == noise)
    lines.append(dict(what="surprise, self-play, on over off", dirichlet=noise, ratio=on / off))

rng = np.random.default_rng(0)
for n in WINDOWS:
    ex = DeviceExamples.from_host(Examples(rng.integers(0, 2 ** 62, n).astype(np.uint64), rng.integers(0, 2 ** 62, n).astype(np.uint64),
                                           np.zeros((n, 1), np.float32), np.zeros(n, np.int8), np.ones(n, np.int8), np.zeros(n, np.uint8),
                                           rng.integers(0, 1 << 20, n), rng.integers(0, 60, n).astype(np.int32), 8,
                                           rng.exponential(0.3, n).astype(np.float32)))
    res, counts = surprise_resample(ex, 0.5, seed=1, return_counts=True)  # (warm-up: the allocator's blocks)
    ms = []
    for _ in range(REPS + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        surprise_resample(ex, 0.5, seed=1)
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    lines.append(dict(what="surprise_resample", rows=n, uniform_frac=0.5, ms_median=statistics.median(ms), ms_all=[round(x, 3) for x in ms],
                      resampled_over_rows=len(res) / n, max_count=int(counts.max()), share_count_0=float((counts == 0).float().mean())))
    del ex, res, counts

for row in lines:
    print(json.dumps(row), flush=True)
if OUT:
    with open(OUT, "w") as f:
        for row in lines:
            f.write(json.dumps(row) + "\n")
