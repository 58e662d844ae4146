#!/usr/bin/env python3
"""Leaf-parallel search: what K leaves per game per tree step buys, K values interleaved in one process.
  * MCTSPlayer.get_move along a Reversi game, 800 sims, 128x6 bf16 net, K in {1, 2, 4, 8, 16} (median ms per move);
  * the 64-game arena's search + move, same net and K values (median ms per move);
  * self-play games/s (PipelinedSelfPlay, two pipelines, bench-style stagger) at B in {512, 4096}, 800 sims, K in {1, 4, 8};
    K = 1 with the evaluation cache on and off (K > 1 runs without it).
Each row also gives the evaluator rows per launch and n_collisions / n_sims.  One JSON object per row on stdout.
python tools/bench_leaf_parallel.py [--quick]"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import betazero_amd as bz  # noqa: E402
from betazero_amd.engine import PipelinedSelfPlay, SelfPlayEngine  # noqa: E402
from betazero_amd.net import DeviceNet, PolicyValueNet  # noqa: E402

QUICK = "--quick" in sys.argv
SIMS = 800
KS_PLAYER = (1, 2, 4, 8, 16)
torch.manual_seed(0)
net = DeviceNet.from_module(PolicyValueNet(128, 6, 64).round_to_bf16_(), 4096 * 8)


def emit(**row):
    print(json.dumps(row), flush=True)


def steps_of(sims, K):
    return -(-sims // K)


# ---- MCTSPlayer.get_move along a game (the positions of one game, every K searches each of them)
positions, b, side = [], bz.ReversiBoard(), 1
for ply in range(12 if QUICK else 30):
    if b.is_game_over():
        break
    mv = b.generate_possible_moves(side)
    if not mv:
        side = -side
        continue
    positions.append((b, side))
    b = b.make_move(*mv[(7 * ply) % len(mv)], side)
    side = -side
players = {(K, s): bz.MCTSPlayer(s, sims=SIMS, net=net, leaves_per_step=K) for K in KS_PLAYER for s in (1, -1)}
for (K, s), pl in players.items():  # build every engine, warm every kernel
    pl.get_move(positions[0][0] if positions[0][1] == s else positions[1][0])
times = {K: [] for K in KS_PLAYER}
for bd, s in positions:
    for K in KS_PLAYER:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        players[(K, s)].get_move(bd)
        torch.cuda.synchronize()
        times[K].append(time.perf_counter() - t0)
for K in KS_PLAYER:
    c = {}
    for s in (1, -1):
        for k, v in players[(K, s)]._engine("reversi").counters().items():
            c[k] = c.get(k, 0) + v
    n_search = len(positions) + 2
    emit(what="MCTSPlayer.get_move", K=K, sims=SIMS, batch=1, moves=len(times[K]), ms_per_move_median=statistics.median(times[K]) * 1e3,
         ms_per_move_min=min(times[K]) * 1e3, evaluator_launches_per_move=steps_of(SIMS, K) + 1,
         rows_per_evaluator_launch=c["n_net_leaves"] / (n_search * (steps_of(SIMS, K) + 1)),
         collisions_per_sim=c.get("n_collisions", 0) / max(c["n_sims"], 1), cache_hits=c["n_cache_hits"])

# ---- the arena's shape: 64 games, search + move
moves = 4 if QUICK else 10
engs = {K: SelfPlayEngine("reversi", 64, SIMS, "net_bf16", net, temp_moves=8, openings=1, leaves_per_step=K) for K in KS_PLAYER}
for e in engs.values():
    e.reset_games(); e.search(); e.play(); e.reset_counters()
torch.cuda.synchronize()
times = {K: [] for K in KS_PLAYER}
for m in range(moves):
    for K, e in engs.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e.search(); e.play()
        torch.cuda.synchronize()
        times[K].append(time.perf_counter() - t0)
for K, e in engs.items():
    c = e.counters()
    emit(what="arena search + move", K=K, sims=SIMS, batch=64, moves=moves, ms_per_move_median=statistics.median(times[K]) * 1e3,
         ms_per_move_min=min(times[K]) * 1e3, rows_per_evaluator_launch=c["n_net_leaves"] / (moves * steps_of(SIMS, K)),
         collisions_per_sim=c.get("n_collisions", 0) / max(c["n_sims"], 1))
del engs

# ---- self-play games/s (two pipelines, staggered pool: completions spread as in bench.py's steady mode)
for B in (512, 4096):
    cfgs = [(1, True), (1, False), (4, False), (8, False)]
    sps = {}
    for K, cache in cfgs:
        sp = PipelinedSelfPlay("reversi", B, SIMS, "net_bf16", net, pipelines=2, leaves_per_step=K, temp_moves=8, openings=1,
                               rounds=16, stagger=60, eval_cache=cache)
        sp.reset_games()
        for _ in range(2):
            sp.step(True)
        sp.status()
        sp.reset_counters()
        sps[(K, cache)] = sp
    reps, per = (2, 3) if QUICK else (3, 6)
    rates = {k: [] for k in sps}
    moves_done = {k: 0 for k in sps}
    for r in range(reps):
        for k, sp in sps.items():
            f0 = sp.status()[1]
            t0 = time.perf_counter()
            for _ in range(per):
                sp.step(True)
            f1 = sp.status()[1]
            rates[k].append((f1 - f0) / (time.perf_counter() - t0))
            moves_done[k] += per
    for (K, cache), sp in sps.items():
        c = sp.counters()
        emit(what="self-play", K=K, eval_cache=cache, games=B, sims=SIMS, games_per_s_median=statistics.median(rates[(K, cache)]),
             games_per_s_all=[round(x, 2) for x in rates[(K, cache)]],
             rows_per_evaluator_launch=c["n_net_leaves"] / (2 * moves_done[(K, cache)] * steps_of(SIMS, K)),
             collisions_per_sim=c.get("n_collisions", 0) / max(c["n_sims"], 1), cache_hits_per_sim=c["n_cache_hits"] / max(c["n_sims"], 1))
    del sps
    torch.cuda.empty_cache()
