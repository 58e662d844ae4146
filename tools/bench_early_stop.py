#!/usr/bin/env python3
"""What exact early stop saves, on and off interleaved in one process.
Fixed: Reversi 8x8, 4 opening plies, the bench's 128x6 bf16 net (untrained) and, with --net PATH, a trained one (a
PolicyValueNet state_dict, e.g. from `az_loop.py --save-net`; --channels / --blocks say its shape).

 1. play_match of a player against itself, early stop off and on, interleaved pairs, at 64 and 800 simulations: the games must
    be identical (asserted); wall time per match (medians), simulations and net rows per search, and the histogram of
    stop_at / sims over every search of the "on" match.
 2. MCTSPlayer.get_move ms per move along one game at 800 simulations: off, on with host exit, on without it.
 3. The empty-launch tail: tree steps issued for one search of the match's positions against the step in which the last slot
    stopped, for run_ahead 2, 16 and 64.

One JSON object per line on stdout.

    python tools/bench_early_stop.py [--quick] [--net PATH --channels C --blocks NB] [--out profiles/early_stop_bench.jsonl]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import betazero_amd as bz  # noqa: E402
from betazero_amd import _lib  # noqa: E402
from betazero_amd.engine import EarlyStop, SelfPlayEngine  # noqa: E402
from betazero_amd.match import MatchPlayer, play_match  # noqa: E402
from betazero_amd.net import DeviceNet, PolicyValueNet  # noqa: E402


def _arg(name, default, conv=str):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


QUICK = "--quick" in sys.argv
OUT = _arg("--out", None)
NET = _arg("--net", None)
GAMES, SIMS_LIST, REPS, MOVE_SIMS = (256, (64,), 2, 200) if QUICK else (1024, (64, 800), 3, 800)
L = _lib.lib()
lines = []


def emit(row):
    lines.append(row)
    print(json.dumps(row), flush=True)


def same(a, b):
    return (np.array_equal(a.actions, b.actions) and np.array_equal(a.movers, b.movers) and np.array_equal(a.winner, b.winner) and
            np.array_equal(a.plies, b.plies))


nets = []
torch.manual_seed(0)
nets.append(("untrained 128x6", DeviceNet.from_module(PolicyValueNet(128, 6, 64).round_to_bf16_(), GAMES)))
if NET:
    ch, nb = _arg("--channels", 64, int), _arg("--blocks", 4, int)
    sd = torch.load(NET, map_location="cpu", weights_only=True)
    module = PolicyValueNet(ch, nb, 64, fused_tower="tower_w" in sd)  # (az_loop trains the fused-tower form of the module)
    module.load_state_dict(sd)
    nets.append((f"trained {ch}x{nb} ({os.path.basename(NET)})", DeviceNet.from_module(module.round_to_bf16_(), GAMES)))


# ---------------------------------------------------------------- 1. a match against itself, off and on
def match(net, sims, es):
    """-> (result, seconds, {n_sims, n_net_leaves, searches} summed over both engines, histogram of stop_at / sims in tenths)"""
    seen, hist, searches = {}, np.zeros(11, np.int64), [0]

    def on_ply(engs, go):
        for i in go:
            seen[i] = engs[i]
            if es is not None:
                st = engs[i].stopped()
                st = st[st > 0]
                searches[0] += len(st)
                np.add.at(hist, (st.astype(np.int64) * 10) // sims, 1)
    p = MatchPlayer(sims=sims, net=net, early_stop=es)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = play_match("reversi", GAMES, p, p, size=8, opening_plies=4, seed=1, on_ply=on_ply)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    cnt = [e.counters() for e in seen.values()]
    tot = {k: sum(c[k] for c in cnt) for k in ("n_sims", "n_net_leaves")}
    return res, dt, tot, hist, searches[0]


for name, net in nets:
    for sims in SIMS_LIST:
        t = {"off": [], "on": []}
        ref = None
        for r in range(REPS):
            for arm, es in (("off", None), ("on", True)):
                res, dt, tot, hist, n_search = match(net, sims, es)
                if ref is None:
                    ref = res
                assert same(res, ref), f"early stop changed a game ({name}, {sims} sims, {arm})"
                t[arm].append(dt)
                if arm == "off":
                    off_tot = tot
                else:
                    on_tot, on_hist, on_search = tot, hist, n_search
        # (the hook's stopped() read is part of the "on" wall time: one small copy per searched engine per ply)
        emit(dict(what="early stop, match against itself", net=name, games=GAMES, sims=sims, opening_plies=4, identical_games=True,
                  searches=on_search, seconds_off_median=statistics.median(t["off"]), seconds_on_median=statistics.median(t["on"]),
                  seconds_off=[round(x, 3) for x in t["off"]], seconds_on=[round(x, 3) for x in t["on"]],
                  sims_per_search_off=off_tot["n_sims"] / on_search, sims_per_search_on=on_tot["n_sims"] / on_search,
                  net_rows_per_search_off=off_tot["n_net_leaves"] / on_search, net_rows_per_search_on=on_tot["n_net_leaves"] / on_search,
                  simulations_saved=1.0 - on_tot["n_sims"] / off_tot["n_sims"], net_rows_saved=1.0 - on_tot["n_net_leaves"] / off_tot["n_net_leaves"],
                  stopped_early=int(on_hist[:10].sum()), stop_at_over_sims_tenths=[int(x) for x in on_hist]))

# ---------------------------------------------------------------- 2. MCTSPlayer.get_move along a game
name, net = nets[-1]
arms = [("off", None), ("on, host exit", EarlyStop(True)), ("on, no host exit", EarlyStop(False))]
players = {a: {s: bz.MCTSPlayer(s, sims=MOVE_SIMS, net=net, early_stop=es) for s in (1, -1)} for a, es in arms}
ms = {a: [] for a, _ in arms}
sims_run = []
b, p = bz.ReversiBoard(size=8), 1
while not b.is_game_over():
    if not b.generate_possible_moves(p):
        p = -p
        continue
    moves = {}
    for a, _ in arms:
        pl = players[a][p]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        moves[a] = pl.get_move(b)
        ms[a].append((time.perf_counter() - t0) * 1e3)
    assert len(set(moves.values())) == 1, "early stop changed a move"
    sims_run.append(players["on, host exit"][p].last_sims)
    b = b.make_move(*moves["off"], p)
    p = -p
for a, _ in arms:
    emit(dict(what="early stop, MCTSPlayer.get_move along one game", net=name, sims=MOVE_SIMS, arm=a, moves=len(ms[a]),
              ms_per_move_mean=statistics.mean(ms[a][1:]), ms_per_move_median=statistics.median(ms[a][1:]),
              **({"sims_per_move_mean": statistics.mean(sims_run)} if a != "off" else {})))

# ---------------------------------------------------------------- 3. the empty-launch tail
sims = SIMS_LIST[-1]
eng = SelfPlayEngine("reversi", GAMES, sims, "net_bf16", net=net, early_stop=True, openings=1, stagger=40, seed=1)  # (slots at different plies)
for ra in (2, 16, 64):
    eng.reset_games()
    torch.cuda.synchronize()
    L.bz_profile_reset(); L.bz_profile_enable(1)
    with torch.cuda.device(eng.device):
        _lib.check(L.bz_engines_search((C.c_void_p * 1)(eng.h), (C.c_void_p * 1)(eng._stream()), 1, ra))
    torch.cuda.synchronize()
    L.bz_profile_enable(0)
    launched = _lib.profile_read()["select"][0]
    L.bz_profile_reset()
    last = int(eng.stopped().max())  # the step of index `last` is the first in which nobody walks
    emit(dict(what="early stop, empty-launch tail", net=name, games=GAMES, sims=sims, run_ahead=ra, tree_steps_issued=int(launched),
              tree_steps_needed=min(last + 1, sims), tail=int(launched) - min(last + 1, sims)))

if OUT:
    with open(OUT, "w") as f:
        for row in lines:
            f.write(json.dumps(row) + "\n")
