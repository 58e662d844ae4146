#!/usr/bin/env python3
"""Evaluator rows per launch by simulation index within a move, for one pipeline of the benchmark's self-play (cfg 3:
800 simulations, evaluation cache with carry-over, steady-state pool): the step API with the packed-leaf count read
between select and the net.  The first moves after reset_games() have nothing to carry over, so they are skipped.
usage: python tools/rows_by_sim.py [games=2048] [moves=4] [skip=2] [out.txt]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from betazero_amd.engine import SelfPlayEngine  # noqa: E402
from betazero_amd.net import DeviceNet, PolicyValueNet  # noqa: E402

B = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
MOVES = int(sys.argv[2]) if len(sys.argv) > 2 else 4
SKIP = int(sys.argv[3]) if len(sys.argv) > 3 else 2
out = open(sys.argv[4], "w") if len(sys.argv) > 4 else sys.stdout
SIMS = 800
torch.manual_seed(0)
net = DeviceNet.from_module(PolicyValueNet(128, 6, 64).round_to_bf16_(), B)
eng = SelfPlayEngine("reversi", B, SIMS, "net_bf16", net=net, temp_moves=8, openings=1, seed=0, rounds=4, stagger=58)
eng.reset_games()
kind = eng.leaf_buffers()["kind"]
rows = np.zeros((MOVES, SIMS), dtype=np.int64)
for mv in range(SKIP + MOVES):
    eng.root_begin(); eng.evaluate(); eng.expand_backup(); eng.root_noise()
    for s in range(SIMS):
        eng.select(s)
        if mv >= SKIP:
            rows[mv - SKIP, s] = int((kind == 1).sum())
        eng.evaluate(); eng.expand_backup()
    eng.play(True)
eng.status()
c = eng.counters()
print(f"# {B} games, {SIMS} simulations, moves {SKIP}..{SKIP + MOVES - 1} after reset; rows counted {rows.sum()}; "
      f"counters over all {SKIP + MOVES} moves: n_net_leaves {c['n_net_leaves']} n_cache_hits {c['n_cache_hits']} "
      f"of which prev {c['n_cache_hits_prev']}", file=out)
print("# simulation index: mean / min / median / max rows per launch", file=out)
edges = [0, 1, 8, 16, 32, 48, 64, 80, 96, 112, 128, 160, 192, 256, 320, 384, 512, 640, 800]
for lo, hi in zip(edges[:-1], edges[1:]):
    d = rows[:, lo:hi]
    print(f"  [{lo:4d}, {hi:4d}): {d.mean():8.1f} {d.min():6d} {int(np.median(d)):6d} {d.max():6d}", file=out)
