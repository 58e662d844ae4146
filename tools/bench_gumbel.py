#!/usr/bin/env python3
"""Gumbel root search against PUCT, the modes interleaved in one process:
  * self-play games/s (PipelinedSelfPlay, two pipelines, 4096 games, the bench's 128x6 bf16 net, bench-style stagger) for
    PUCT and Gumbel at sims in {16, 32, 64, 200}, plus PUCT at 800 (the headline's setting) as the reference point;
  * the select tree step's microseconds per launch in each mode (k_tree_step / k_gumbel_step, the library's event timers,
    one 4096-game engine, 64 sims);
  * MCTSPlayer.get_move ms per move along a Reversi game at 16 / 64 / 800 sims, same net;
  * tic-tac-toe arena (64 games, uniform evaluator) against the minimax player for both modes at low sims -- losses as a
    sanity check, not a strength claim.
One JSON object per row on stdout.  python tools/bench_gumbel.py [--quick]"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import betazero_amd as bz  # noqa: E402
from betazero_amd import _lib  # noqa: E402
from betazero_amd.arena import play_arena  # noqa: E402
from betazero_amd.engine import PipelinedSelfPlay, SelfPlayEngine  # noqa: E402
from betazero_amd.net import DeviceNet, PolicyValueNet  # noqa: E402

QUICK = "--quick" in sys.argv
MODES = (("puct", None), ("gumbel", True))
torch.manual_seed(0)
net = DeviceNet.from_module(PolicyValueNet(128, 6, 64).round_to_bf16_(), 4096)


def emit(**row):
    print(json.dumps(row), flush=True)


# ---- self-play games/s, 4096 games
B = 1024 if QUICK else 4096
for sims, modes in ((16, MODES), (32, MODES), (64, MODES), (200, MODES), (800, MODES[:1])):
    sps = {}
    for name, g in modes:
        sp = PipelinedSelfPlay("reversi", B, sims, "net_bf16", net, pipelines=2, temp_moves=8, openings=1, rounds=64,
                               stagger=60, gumbel=g)
        sp.reset_games()
        for _ in range(2):
            sp.step(True)
        sp.status()
        sp.reset_counters()
        sps[name] = sp
    reps, per = (2, 4) if QUICK else (3, 8 if sims >= 200 else 24)
    rates = {k: [] for k in sps}
    for r in range(reps):
        for k, sp in sps.items():
            f0 = sp.status()[1]
            t0 = time.perf_counter()
            for _ in range(per):
                sp.step(True)
            f1 = sp.status()[1]
            rates[k].append((f1 - f0) / (time.perf_counter() - t0))
    for k, sp in sps.items():
        c = sp.counters()
        emit(what="self-play", mode=k, games=B, sims=sims, games_per_s_median=statistics.median(rates[k]),
             games_per_s_all=[round(x, 2) for x in rates[k]], cache_hits_per_sim=c["n_cache_hits"] / max(c["n_sims"], 1))
    del sps
    torch.cuda.empty_cache()

# ---- tree step (select + expand/backup of the previous leaf) per launch, one engine
L = _lib.lib()
engs = {k: SelfPlayEngine("reversi", B, 64, "net_bf16", net, temp_moves=8, openings=1, gumbel=g) for k, g in MODES}
for e in engs.values():
    e.reset_games(); e.search(); e.play()
torch.cuda.synchronize()
for k, e in engs.items():
    L.bz_profile_reset(); L.bz_profile_enable(1)
    for _ in range(4):
        e.search(); e.play()
    torch.cuda.synchronize()
    L.bz_profile_enable(0)
    prof = _lib.profile_read()
    n, t, ms = prof["select"]
    _, tp, msp = prof["play"]
    emit(what="tree step", mode=k, games=B, sims=64, kernel="k_gumbel_step" if k == "gumbel" else "k_tree_step",
         us_per_launch=ms / max(t, 1) * 1e3, launches_timed=t, play_us_per_launch=msp / max(tp, 1) * 1e3)
del engs
torch.cuda.empty_cache()

# ---- MCTSPlayer.get_move along a game
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
for sims in (16, 64, 800):
    players = {(k, s): bz.MCTSPlayer(s, sims=sims, net=net, gumbel=g) for k, g in MODES for s in (1, -1)}
    for (k, s), pl in players.items():
        pl.get_move(positions[0][0] if positions[0][1] == s else positions[1][0])
    times = {k: [] for k, _ in MODES}
    for bd, s in positions:
        for k, _ in MODES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            players[(k, s)].get_move(bd)
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    for k, _ in MODES:
        emit(what="MCTSPlayer.get_move", mode=k, sims=sims, moves=len(times[k]), ms_per_move_median=statistics.median(times[k]) * 1e3,
             ms_per_move_min=min(times[k]) * 1e3)
    del players

# ---- tic-tac-toe arena against minimax (64 games, uniform evaluator, 2 random opening plies: many different games)
for sims in (16, 64, 200):
    for k, g in MODES:
        s = play_arena("ttt", 64, sims, evaluator="uniform", seed=1, opening_plies=2, gumbel=g).summary()
        emit(what="ttt arena vs minimax", mode=k, sims=sims, opening_plies=2, **s)
