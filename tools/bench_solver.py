#!/usr/bin/env python3
"""Proven wins, losses and draws against the plain engine, the solver on and off interleaved in one process,
medians over the repeats, one JSON object per line on stdout (and into --out).

  1. self-play at the bench's shape: 4096 Reversi 8x8 games, 800 simulations, the 128x6 bf16 net in the loop, two pipelines,
     Dirichlet noise (both arms run the step kernels): games/s, net rows per search, tree-step us per launch (the library's
     event timers around the select launches).
  2. what the solver decides: 512 games played to the end with the solver on; per number of empty squares at the root the
     share of searches with a decided root, and the share of moves where the solver's move differs from argmax N.
  3. with --match: play_match of the solver on (A) against off (B) on the same (random, bf16) net, --match-games games at
     --match-sims simulations -- the score and its 95 % interval.  The net is untrained: a statement about the rule's
     effect on this evaluator, not about playing strength of a trained program.

    python tools/bench_solver.py [--quick] [--match] [--match-games N] [--match-sims S] [--out profiles/solver_bench.jsonl]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from betazero_amd import _lib  # noqa: E402
from betazero_amd.engine import PipelinedSelfPlay, SelfPlayEngine  # noqa: E402
from betazero_amd.match import MatchPlayer, play_match  # noqa: E402
from betazero_amd.net import DeviceNet, PolicyValueNet  # noqa: E402


def _arg(name, default, conv=str):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


QUICK = "--quick" in sys.argv
OUT = _arg("--out", None)
SIMS, B, REPS, PER, PIPES, B2 = (64, 512, 3, 2, 2, 64) if QUICK else (800, 4096, 5, 2, 2, 512)
NOISE = dict(dirichlet_alpha=0.3, dirichlet_eps=0.25)
L = _lib.lib()
lines = []


def emit(row):
    lines.append(row)
    print(json.dumps(row), flush=True)


torch.manual_seed(0)
module = PolicyValueNet(128, 6, 64).round_to_bf16_()

# ---------------------------------------------------------------- 1. self-play with the net in the loop, on and off interleaved
net = DeviceNet.from_module(module, B // PIPES)
sps = []
for solver in (False, True):
    sp = PipelinedSelfPlay("reversi", B, SIMS, "net_bf16", net, pipelines=PIPES, temp_moves=8, openings=1, rounds=8, stagger=60,
                           solver=solver, **NOISE)
    sp.reset_games()
    sp.step(True)
    sp.status()
    sps.append(sp)
acc = [{"games": [], "rows": [], "us": []} for _ in sps]
for r in range(REPS):
    for sp, a in zip(sps, acc):
        sp.reset_counters()
        f0 = sp.status()[1]
        torch.cuda.synchronize()
        L.bz_profile_reset(); L.bz_profile_enable(1)
        t0 = time.perf_counter()
        for _ in range(PER):
            sp.step(True)
            sp.sync()
        dt = time.perf_counter() - t0
        torch.cuda.synchronize()
        L.bz_profile_enable(0)
        n, t, ms = _lib.profile_read()["select"]
        f1 = sp.status()[1]
        c = sp.counters()
        a["games"].append((f1 - f0) / dt)
        a["rows"].append(c["n_net_leaves"] / (PER * B))
        a["us"].append(ms / max(t, 1) * 1e3)
for solver, a in zip((False, True), acc):
    emit(dict(what="solver self-play", solver=solver, games=B, sims=SIMS, net="128x6 bf16", pipelines=PIPES, steps_per_repeat=PER,
              games_per_s_median=statistics.median(a["games"]), games_per_s_all=[round(x, 2) for x in a["games"]],
              net_rows_per_search_median=statistics.median(a["rows"]), net_rows_per_search_all=[round(x, 1) for x in a["rows"]],
              tree_step_us_per_launch_median=statistics.median(a["us"]), tree_step_us_per_launch_all=[round(x, 2) for x in a["us"]]))
del sps, net

# ---------------------------------------------------------------- 2. what the solver decides, by empty squares
net = DeviceNet.from_module(module, B2)
eng = SelfPlayEngine("reversi", B2, SIMS, "net_bf16", net, temp_moves=8, openings=1, solver=True, **NOISE)
eng.reset_games()
searched, decided, moves, differ = {}, {}, 0, 0
while True:
    eng.search()
    own, opp, tm, st = eng.positions()
    N, _, _ = eng.root_stats()
    _, act = eng.root_policy()
    proven, _, _ = eng.proven()
    for g in np.nonzero(st == 0)[0]:
        k = 64 - bin(int(own[g]) | int(opp[g])).count("1")
        searched[k] = searched.get(k, 0) + 1
        decided[k] = decided.get(k, 0) + (proven[g] is not None)
    # argmax N is the tau = 0 move: the first temp_moves (8) moves of a game sample and are left out -- a root with at most
    # 64 - 4 - 8 empty squares has at least 8 moves behind it
    late = [g for g in np.nonzero(st == 0)[0] if 64 - bin(int(own[g]) | int(opp[g])).count("1") <= 64 - 4 - 8]
    for g in late:
        moves += 1
        differ += int(act[g]) != int(np.argmax(N[g]))
    eng.play(False)
    if eng.status()[0] == 0:
        break
emit(dict(what="solver decided roots", games=B2, sims=SIMS, net="128x6 bf16 (random weights)",
          decided_share_by_empty_squares={str(k): round(decided[k] / searched[k], 4) for k in sorted(searched)},
          searches_by_empty_squares={str(k): searched[k] for k in sorted(searched)},
          moves_compared=moves, share_of_moves_that_differ_from_argmax_n=round(differ / max(1, moves), 5)))
del eng, net

# ---------------------------------------------------------------- 3. solver against plain, same net
if "--match" in sys.argv:
    games, msims = _arg("--match-games", 1024, int), _arg("--match-sims", 200, int)
    dn = DeviceNet.from_module(module, games)
    t0 = time.perf_counter()
    res = play_match("reversi", games, MatchPlayer(sims=msims, net=dn, solver=True), MatchPlayer(sims=msims, net=dn), opening_plies=4, seed=0)
    emit(dict(what="solver match, on (A) against off (B)", net="128x6 bf16 (random weights)", sims=msims, opening_plies=4,
              seconds=round(time.perf_counter() - t0, 1), **res.summary()))

if OUT:
    with open(OUT, "w") as f:
        for row in lines:
            f.write(json.dumps(row) + "\n")
