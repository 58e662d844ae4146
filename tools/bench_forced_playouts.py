#!/usr/bin/env python3
"""Forced playouts and policy target pruning against the plain engine, the configurations interleaved in one
process.  Fixed (cfg 3's shape): Reversi 8x8, 4096 games, the bench's 128x6 bf16 net, 800 simulations, evaluation cache on
(carry), two pipelines, temp_moves 8, openings on, Dirichlet noise (0.3, 0.25) in EVERY configuration (so all of them run the
step kernels), a staggered pool that restarts finished games.  Configurations: forced off, forced on (k = 2, prune), forced on
under the playout cap (100, 0.25).  Per configuration, medians over the repeats: games/s, evaluator rows per net launch, and
the select tree step's microseconds per launch (the library's event timers, in a pass of its own).  Then, per forced
configuration, what the pruning does to the targets: 512 games played to the end twice with the same seed, prune on and prune
off -- the same games, since pruning changes pi alone -- and from the two pi of every row the share of root visits removed
(1 - sum N' / sum N = 1 - pi_raw[c*] / pi_pruned[c*], c* keeps its visits) and the share of rows in which a visited child
is pruned to 0.  One JSON object per configuration on stdout.

    python tools/bench_forced_playouts.py [--quick] [--out profiles/forced_playouts_bench.jsonl]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from betazero_amd import _lib  # noqa: E402
from betazero_amd.engine import ForcedPlayouts, PipelinedSelfPlay, PlayoutCap  # noqa: E402
from betazero_amd.net import DeviceNet, PolicyValueNet  # noqa: E402

QUICK = "--quick" in sys.argv
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
SIMS, FAST, PROB, B, BT = (64, 8, 0.25, 512, 64) if QUICK else (800, 100, 0.25, 4096, 512)
K = 2.0
NOISE = dict(dirichlet_alpha=0.3, dirichlet_eps=0.25)
CONFIGS = [("off", None, None), ("forced", ForcedPlayouts(K), None), ("forced+cap", ForcedPlayouts(K), PlayoutCap(FAST, PROB))]
REPS, PER, PIPES = (3, 2, 2) if QUICK else (5, 4, 2)
KERNEL = {"off": "k_tree_step", "forced": "k_forced_step", "forced+cap": "k_forced_cap_step"}

torch.manual_seed(0)
net = DeviceNet.from_module(PolicyValueNet(128, 6, 64).round_to_bf16_(), B // PIPES)
L = _lib.lib()

sps = []
for kind, fp, cap in CONFIGS:
    sp = PipelinedSelfPlay("reversi", B, SIMS, "net_bf16", net, pipelines=PIPES, temp_moves=8, openings=1, rounds=8, stagger=60,
                           playout_cap=cap, forced_playouts=fp, **NOISE)
    sp.reset_games()
    for _ in range(2):
        sp.step(True)
    sp.status()
    sps.append(sp)

rates = [{"games": [], "net_rows": []} for _ in CONFIGS]
for r in range(REPS):
    for sp, acc in zip(sps, rates):
        sp.reset_counters()
        f0 = sp.status()[1]
        t0 = time.perf_counter()
        for _ in range(PER):
            sp.step(True)
            sp.sync()
        f1 = sp.status()[1]
        dt = time.perf_counter() - t0
        c = sp.counters()
        acc["games"].append((f1 - f0) / dt)
        acc["net_rows"].append(c["n_net_leaves"] / (PER * (SIMS + 1) * PIPES))

timed = []
for sp in sps:  # the tree step per launch, timed by the library's events in a pass of its own (the timers serialise the streams)
    torch.cuda.synchronize()
    L.bz_profile_reset(); L.bz_profile_enable(1)
    sp.step(True)
    sp.sync()
    L.bz_profile_enable(0)
    timed.append(_lib.profile_read())
del sps


def targets(fp, cap):
    """(share of root visits removed, share of rows with a child pruned to 0, rows) over BT games, or None if the two runs did
    not play the same games"""
    ex = []
    for prune in (True, False):
        sp = PipelinedSelfPlay("reversi", BT, SIMS, "net_bf16", net, pipelines=PIPES, temp_moves=8, openings=1, seed=7, playout_cap=cap,
                               forced_playouts=ForcedPlayouts(fp.k, prune), **NOISE)
        sp.run_iteration()
        ex.append(sp.examples())
    a, b = ex
    if len(a) != len(b) or not (np.array_equal(a.act, b.act) and np.array_equal(a.game, b.game) and np.array_equal(a.own, b.own)):
        return None
    cs = b.pi.argmax(1)  # (the first maximum of N / sum N = c*)
    rows = np.arange(len(a))
    kept = b.pi[rows, cs] / a.pi[rows, cs]
    return float(1.0 - kept.mean()), float(((b.pi > 0) & (a.pi == 0)).any(1).mean()), len(a)


lines = []
for (kind, fp, cap), acc, prof in zip(CONFIGS, rates, timed):
    n, t, ms = prof["select"]
    _, tt, tms = prof["tower"]
    tg = targets(fp, cap) if fp else None
    row = dict(what="forced playouts", mode=kind, games=B, sims=SIMS, k=fp.k if fp else None, prune=fp.prune if fp else None,
               fast_sims=cap.fast_sims if cap else None, full_prob=cap.full_prob if cap else None, pipelines=PIPES,
               dirichlet=[NOISE["dirichlet_alpha"], NOISE["dirichlet_eps"]], steps_per_repeat=PER,
               games_per_s_median=statistics.median(acc["games"]), games_per_s_all=[round(x, 2) for x in acc["games"]],
               net_rows_per_launch_median=statistics.median(acc["net_rows"]),
               tree_step_kernel=KERNEL[kind], tree_step_us_per_launch=ms / max(t, 1) * 1e3, tree_step_launches_timed=t,
               tower_us_per_launch=tms / max(tt, 1) * 1e3,
               target_games=BT if tg else None, target_rows=tg[2] if tg else None,
               root_visits_pruned_share=tg[0] if tg else None, rows_with_a_child_pruned_to_0_share=tg[1] if tg else None)
    lines.append(row)
    print(json.dumps(row), flush=True)
if OUT:
    with open(OUT, "w") as f:
        for row in lines:
            f.write(json.dumps(row) + "\n")
