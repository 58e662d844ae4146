#!/usr/bin/env python3
"""Playout cap randomisation against the plain engine, the configurations interleaved in one process.
Fixed: Reversi 8x8, the bench's 128x6 bf16 net, 800 simulations, evaluation cache on (carry), two pipelines, temp_moves 8,
openings on, a staggered pool that restarts finished games (steady state, as bench.py measures).  Configurations: cap off at
4096 games (the reference point) and cap (100, 0.25) at 4096 / 8192 / 16384 games.  Per configuration, medians over the
repeats: games/s, recorded example rows/s, evaluator rows per net launch, and the select tree step's microseconds per launch
(k_tree_step / k_cap_step, the library's event timers, in a pass of its own).  One JSON object per configuration on stdout.

    python tools/bench_playout_cap.py [--quick] [--out profiles/playout_cap_bench.jsonl]"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from betazero_amd import _lib  # noqa: E402
from betazero_amd.engine import PipelinedSelfPlay, PlayoutCap  # noqa: E402
from betazero_amd.net import DeviceNet, PolicyValueNet  # noqa: E402

QUICK = "--quick" in sys.argv
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
SIMS, FAST, PROB = (64, 8, 0.25) if QUICK else (800, 100, 0.25)
CONFIGS = [("off", None, 4096), ("cap", PlayoutCap(FAST, PROB), 4096), ("cap", PlayoutCap(FAST, PROB), 8192),
           ("cap", PlayoutCap(FAST, PROB), 16384)]
if QUICK:
    CONFIGS = [(k, c, b // 8) for k, c, b in CONFIGS]
REPS, PER, PIPES = (3, 2, 2) if QUICK else (3, 4, 2)

torch.manual_seed(0)
net = DeviceNet.from_module(PolicyValueNet(128, 6, 64).round_to_bf16_(), max(b for _, _, b in CONFIGS) // PIPES)
L = _lib.lib()

sps = []
for kind, cap, B in CONFIGS:
    sp = PipelinedSelfPlay("reversi", B, SIMS, "net_bf16", net, pipelines=PIPES, temp_moves=8, openings=1, rounds=8, stagger=60,
                           playout_cap=cap)
    sp.reset_games()
    for _ in range(2):
        sp.step(True)
    sp.status()
    sps.append(sp)


rates = [{"games": [], "rows": [], "net_rows": []} for _ in CONFIGS]
for r in range(REPS):
    for (kind, cap, B), sp, acc in zip(CONFIGS, sps, rates):
        sp.reset_counters()
        f0 = sp.status()[1]
        rows = 0
        t0 = time.perf_counter()
        for _ in range(PER):
            sp.step(True)
            # example rows the move recorded: one per slot (every slot is in a game: finished ones restart at once), under
            # the cap one per full search -- the budgets are read before the next search overwrites them (the read waits
            # for the step; 4 bytes per game)
            if cap is None:
                sp.sync()  # (the same wait at the end of every step in every configuration)
                rows += sp.B
            else:
                rows += int((sp.budgets() == SIMS).sum())
        f1 = sp.status()[1]
        dt = time.perf_counter() - t0
        c = sp.counters()
        acc["games"].append((f1 - f0) / dt)
        acc["rows"].append(rows / dt)
        acc["net_rows"].append(c["n_net_leaves"] / (PER * (SIMS + 1) * PIPES))

lines = []
for (kind, cap, B), sp, acc in zip(CONFIGS, sps, rates):
    # the tree step per launch, timed by the library's events in a pass of its own (the timers serialise the streams)
    torch.cuda.synchronize()
    L.bz_profile_reset(); L.bz_profile_enable(1)
    sp.step(True)
    sp.sync()
    L.bz_profile_enable(0)
    prof = _lib.profile_read()
    n, t, ms = prof["select"]
    _, tt, tms = prof["tower"]
    row = dict(what="playout cap", mode=kind, games=B, sims=SIMS, fast_sims=cap.fast_sims if cap else None,
               full_prob=cap.full_prob if cap else None, pipelines=PIPES, steps_per_repeat=PER,
               games_per_s_median=statistics.median(acc["games"]), games_per_s_all=[round(x, 2) for x in acc["games"]],
               rows_per_s_median=statistics.median(acc["rows"]), rows_per_s_all=[round(x, 1) for x in acc["rows"]],
               net_rows_per_launch_median=statistics.median(acc["net_rows"]),
               tree_step_kernel="k_cap_step" if cap else "k_tree_step", tree_step_us_per_launch=ms / max(t, 1) * 1e3,
               tree_step_launches_timed=t, tower_us_per_launch=tms / max(tt, 1) * 1e3)
    lines.append(row)
    print(json.dumps(row), flush=True)
if OUT:
    with open(OUT, "w") as f:
        for row in lines:
            f.write(json.dumps(row) + "\n")
