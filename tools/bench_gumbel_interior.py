#!/usr/bin/env python3
"""Gumbel interior selection against Gumbel root search with PUCT below the root, interior "puct" and "gumbel"
interleaved in one process, medians over the repeats, one JSON object per arm on stdout (and into --out).

  1. the tree step per launch: 4096 Reversi 8x8 games, 64 simulations, hash evaluator, a staggered pool of positions --
     k_gfull_step against k_gumbel_step in the same run (the library's event timers around the select launches).
  2. self-play games/s with the bench's 128x6 bf16 net in the loop, two pipelines, evaluation cache on, at 64 and at 800
     simulations; the mean walk length with it.
  3. with --match: play_match of the full rule (A) against root-only Gumbel (B) on that same, untrained net at 32 simulations --
     summary() as it is; a sanity check of the plumbing, not a strength claim.

    python tools/bench_gumbel_interior.py [--quick] [--match [--match-games N]] [--out profiles/gumbel_interior_bench.jsonl]"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from betazero_amd import _lib  # noqa: E402
from betazero_amd.engine import GumbelConfig, PipelinedSelfPlay, SelfPlayEngine  # noqa: E402
from betazero_amd.match import MatchPlayer, play_match  # noqa: E402
from betazero_amd.net import DeviceNet, PolicyValueNet  # noqa: E402


def _arg(name, default, conv=str):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


QUICK = "--quick" in sys.argv
OUT = _arg("--out", None)
B, REPS, PIPES = (512, 3, 2) if QUICK else (4096, 5, 2)
ARMS = [("puct", GumbelConfig(interior="puct")), ("gumbel", GumbelConfig(interior="gumbel"))]
KERNEL = {"puct": "k_gumbel_step", "gumbel": "k_gfull_step"}
L = _lib.lib()
lines = []


def emit(row):
    lines.append(row)
    print(json.dumps(row), flush=True)


# ---------------------------------------------------------------- 1. the tree step per launch
SIMS = 64
engs = []
for name, g in ARMS:
    e = SelfPlayEngine("reversi", B, SIMS, "hash", temp_moves=8, openings=1, rounds=64, stagger=60, gumbel=g)
    e.reset_games()
    e.search(); e.play(True)
    e.status()
    engs.append(e)
us, walk = [[] for _ in ARMS], [[] for _ in ARMS]
for r in range(REPS):
    for e, acc, wk in zip(engs, us, walk):
        e.reset_counters()
        torch.cuda.synchronize()
        L.bz_profile_reset(); L.bz_profile_enable(1)
        for _ in range(4):
            e.search(); e.play(True)
        torch.cuda.synchronize()
        L.bz_profile_enable(0)
        n, t, ms = _lib.profile_read()["select"]
        acc.append(ms / max(t, 1) * 1e3)
        c = e.counters()
        wk.append(c["n_path_nodes"] / max(1, c["n_sims"]))
        e.status()
for (name, g), acc, wk in zip(ARMS, us, walk):
    emit(dict(what="gumbel interior tree step", interior=name, kernel=KERNEL[name], games=B, sims=SIMS, evaluator="hash",
              us_per_launch_median=statistics.median(acc), us_per_launch_all=[round(x, 2) for x in acc],
              ratio_to_k_gumbel_step=statistics.median(acc) / statistics.median(us[0]), mean_walk_nodes_median=statistics.median(wk)))
del engs
torch.cuda.empty_cache()

# ---------------------------------------------------------------- 2. self-play with the net in the loop
torch.manual_seed(0)
net = DeviceNet.from_module(PolicyValueNet(128, 6, 64).round_to_bf16_(), B)
for sims, per in ((64, 2 if QUICK else 16), (800, 1 if QUICK else 2)):
    sps = []
    for name, g in ARMS:
        sp = PipelinedSelfPlay("reversi", B, sims, "net_bf16", net, pipelines=PIPES, temp_moves=8, openings=1, rounds=64, stagger=60, gumbel=g)
        sp.reset_games()
        sp.step(True)
        sp.status()
        sps.append(sp)
    rates = [{"games": [], "walk": []} for _ in sps]
    for r in range(REPS):
        for sp, acc in zip(sps, rates):
            sp.reset_counters()
            f0 = sp.status()[1]
            t0 = time.perf_counter()
            for _ in range(per):
                sp.step(True)
                sp.sync()
            f1 = sp.status()[1]
            dt = time.perf_counter() - t0
            c = sp.counters()
            acc["games"].append((f1 - f0) / dt)
            acc["walk"].append(c["n_path_nodes"] / max(1, c["n_sims"]))
    for (name, g), acc in zip(ARMS, rates):
        emit(dict(what="gumbel interior self-play", interior=name, games=B, sims=sims, net="128x6 bf16", pipelines=PIPES,
                  steps_per_repeat=per, games_per_s_median=statistics.median(acc["games"]),
                  games_per_s_all=[round(x, 2) for x in acc["games"]],
                  ratio_to_puct_interior=statistics.median(acc["games"]) / statistics.median(rates[0]["games"]),
                  mean_walk_nodes_median=statistics.median(acc["walk"])))
    del sps
    torch.cuda.empty_cache()

# ---------------------------------------------------------------- 3. full against root-only, same net
if "--match" in sys.argv:
    games, msims = _arg("--match-games", 128 if QUICK else 512, int), 32
    t0 = time.perf_counter()
    res = play_match("reversi", games, MatchPlayer(sims=msims, net=net, gumbel=ARMS[1][1]), MatchPlayer(sims=msims, net=net, gumbel=ARMS[0][1]),
                     opening_plies=4, seed=0)
    emit(dict(what="gumbel interior match, full (A) against root-only (B)", net="128x6 bf16, untrained (seed 0)", sims=msims, opening_plies=4,
              seconds=round(time.perf_counter() - t0, 1), **res.summary()))

if OUT:
    with open(OUT, "w") as f:
        for row in lines:
            f.write(json.dumps(row) + "\n")
