#!/usr/bin/env python3
"""First-play urgency reduction against the plain engine, the arms interleaved in one process, medians over the
repeats, one JSON object per arm on stdout (and into --out).

  1. the tree step per launch: 4096 Reversi 8x8 games, 800 simulations, hash evaluator, a staggered pool of positions -- k_fpu_step
     against k_tree_step and k_gumbel_step in the same run (the library's event timers around the select launches).  The plain
     arm and the FPU arm draw Dirichlet noise (0.3, 0.25), which sends the plain arm through the step kernels instead of the
     fused search; Gumbel root search refuses the noise and always runs the step kernels.
  2. self-play games/s with the rule on and off: the bench's 128x6 bf16 net in the loop, two pipelines, evaluation cache on.
  3. with --net PATH (a PolicyValueNet state_dict; --channels / --blocks say its shape): play_match of the rule on against
     the rule off on that net at equal simulations -- the score and its 95 % interval.

    python tools/bench_fpu.py [--quick] [--net PATH --channels C --blocks NB --match-games N --match-sims S] [--out profiles/fpu_bench.jsonl]"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from betazero_amd import _lib  # noqa: E402
from betazero_amd.engine import Fpu, PipelinedSelfPlay, SelfPlayEngine  # noqa: E402
from betazero_amd.match import MatchPlayer, play_match  # noqa: E402
from betazero_amd.net import DeviceNet, PolicyValueNet  # noqa: E402


def _arg(name, default, conv=str):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


QUICK = "--quick" in sys.argv
OUT = _arg("--out", None)
NET = _arg("--net", None)
SIMS, B, REPS, PER, PIPES = (64, 512, 3, 2, 2) if QUICK else (800, 4096, 5, 2, 2)
FPU = Fpu()
NOISE = dict(dirichlet_alpha=0.3, dirichlet_eps=0.25)
L = _lib.lib()
lines = []


def emit(row):
    lines.append(row)
    print(json.dumps(row), flush=True)


# ---------------------------------------------------------------- 1. the tree step per launch
ARMS = [("k_tree_step", dict(**NOISE)), ("k_fpu_step", dict(fpu=FPU, **NOISE)), ("k_gumbel_step", dict(gumbel=True))]
engs = []
for name, kw in ARMS:
    e = SelfPlayEngine("reversi", B, SIMS, "hash", temp_moves=8, openings=1, rounds=8, stagger=60, **kw)
    e.reset_games()
    e.search(); e.play(True)
    e.status()
    engs.append(e)
us = [[] for _ in ARMS]
for r in range(REPS):
    for e, acc in zip(engs, us):
        torch.cuda.synchronize()
        L.bz_profile_reset(); L.bz_profile_enable(1)
        e.search(); e.play(True)
        torch.cuda.synchronize()
        L.bz_profile_enable(0)
        n, t, ms = _lib.profile_read()["select"]
        acc.append(ms / max(t, 1) * 1e3)
        e.status()
for (name, kw), acc in zip(ARMS, us):
    emit(dict(what="fpu tree step", kernel=name, games=B, sims=SIMS, evaluator="hash", dirichlet="dirichlet_eps" in kw,
              us_per_launch_median=statistics.median(acc), us_per_launch_all=[round(x, 2) for x in acc]))
del engs

# ---------------------------------------------------------------- 2. self-play with the net in the loop
torch.manual_seed(0)
net = DeviceNet.from_module(PolicyValueNet(128, 6, 64).round_to_bf16_(), B // PIPES)
sps = []
for fpu in (None, FPU):
    sp = PipelinedSelfPlay("reversi", B, SIMS, "net_bf16", net, pipelines=PIPES, temp_moves=8, openings=1, rounds=8, stagger=60, fpu=fpu, **NOISE)
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
        for _ in range(PER):
            sp.step(True)
            sp.sync()
        f1 = sp.status()[1]
        dt = time.perf_counter() - t0
        c = sp.counters()
        acc["games"].append((f1 - f0) / dt)
        acc["walk"].append(c["n_path_nodes"] / max(1, c["n_sims"]))
for fpu, acc in zip((None, FPU), rates):
    emit(dict(what="fpu self-play", fpu=[fpu.reduction, fpu.root_reduction] if fpu else None, games=B, sims=SIMS, net="128x6 bf16",
              pipelines=PIPES, steps_per_repeat=PER, games_per_s_median=statistics.median(acc["games"]),
              games_per_s_all=[round(x, 2) for x in acc["games"]], mean_walk_nodes_median=statistics.median(acc["walk"])))
del sps, net

# ---------------------------------------------------------------- 3. the rule on against the rule off, on a given net
if NET:
    ch, nb = _arg("--channels", 128, int), _arg("--blocks", 6, int)
    games, msims = _arg("--match-games", 512, int), _arg("--match-sims", 200, int)
    module = PolicyValueNet(ch, nb, 64)
    module.load_state_dict(torch.load(NET, map_location="cpu", weights_only=True))
    dn = DeviceNet.from_module(module.round_to_bf16_(), games)
    t0 = time.perf_counter()
    res = play_match("reversi", games, MatchPlayer(sims=msims, net=dn, fpu=FPU), MatchPlayer(sims=msims, net=dn), opening_plies=4, seed=0)
    s = res.summary()
    emit(dict(what="fpu match, on (A) against off (B)", net=os.path.basename(NET), channels=ch, blocks=nb, sims=msims, opening_plies=4,
              fpu=[FPU.reduction, FPU.root_reduction], seconds=round(time.perf_counter() - t0, 1), **s))

if OUT:
    with open(OUT, "w") as f:
        for row in lines:
            f.write(json.dumps(row) + "\n")
