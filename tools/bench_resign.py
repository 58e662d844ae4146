#!/usr/bin/env python3
"""Resignation in self-play on the benchmark net: calibrate a threshold on played-out games, then measure what
it saves, resignation off and on interleaved in one process.
Fixed: Reversi 8x8, the bench's 128x6 bf16 net (untrained), 800 simulations, evaluation cache on (carry), two pipelines,
temp_moves 8, openings on.

 1. Calibration: every game played out (playout_frac = 1) with the root value of every search recorded (search_value); the
    rule is then replayed on the host over those q's for every threshold of a sweep -- the engine's own records at the
    threshold it ran with are compared with that replay -- giving, per threshold, the games that would have resigned, how
    many plies early, and the false-positive rate against the real outcomes.
 2. The loosest (highest) threshold of the sweep whose false-positive rate is <= 0.05 with at least one game resigning.
 3. Two games per slot played from the start to the last game's end, finished slots restarting at once, resignation off and
    on (that threshold, playout_frac 0.1): games/s over the whole run (its tail, where the last games drain, included),
    searches per game and net rows per game -- exact, over whole games -- medians over the repeats.

One JSON object per line on stdout: the sweep, the choice, then one per mode.

    python tools/bench_resign.py [--quick] [--out profiles/resign_bench.jsonl]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from betazero_amd.engine import PipelinedSelfPlay, Resign  # noqa: E402
from betazero_amd.net import DeviceNet, PolicyValueNet  # noqa: E402

QUICK = "--quick" in sys.argv
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
SIMS, B, CAL_B = (64, 512, 256) if QUICK else (800, 4096, 4096)
REPS, PIPES, ROUNDS = 3, 2, 2
CONSECUTIVE, FP_TARGET, PLAYOUT_FRAC, T0 = 2, 0.05, 0.1, -0.9
SWEEP = [round(-0.95 + 0.05 * i, 2) for i in range(19)]  # -0.95 .. -0.05

torch.manual_seed(0)
net = DeviceNet.from_module(PolicyValueNet(128, 6, 64).round_to_bf16_(), max(B, CAL_B) // PIPES)
KW = dict(pipelines=PIPES, temp_moves=8, openings=1)
lines = []


def emit(row):
    lines.append(row)
    print(json.dumps(row), flush=True)


def replay(q, mover, game, winner_of, threshold, consecutive):
    """the rule on the host over every game's recorded searches (no cap: every search is full and has a row): per game id
    (side, row index) of the first fire or None"""
    thr, out = np.float32(threshold), {}
    order = np.argsort(game, kind="stable")  # rows of a game are in ply order already
    g_sorted, starts = np.unique(game[order], return_index=True)
    ends = list(starts[1:]) + [len(order)]
    for gid, a, b in zip(g_sorted, starts, ends):
        streak, first = {1: 0, -1: 0}, None
        for k, i in enumerate(order[a:b]):
            p = int(mover[i])
            streak[p] = min(streak[p] + 1, 255) if q[i] < thr else 0
            if streak[p] >= consecutive:
                first = (p, k)
                break
        out[int(gid)] = first
    return out


# ---- 1. calibration
cal = PipelinedSelfPlay("reversi", CAL_B, SIMS, "net_bf16", net, resign=Resign(T0, CONSECUTIVE, 1.0), search_value=True, **KW)
t0 = time.perf_counter()
plies = cal.run_iteration()
ex = cal.examples()
winners, lens = cal.winners()
side, move, rq, played_out = cal.resign_rows()
cal_s = time.perf_counter() - t0
assert played_out.all() and (lens >= 0).all()
winner_of = {g: int(winners[0, g]) for g in range(CAL_B)}
rows_of = {g: int(lens[0, g]) for g in range(CAL_B)}
mine = replay(ex.q, ex.mover, ex.game, winner_of, T0, CONSECUTIVE)
agree = all((mine[g] is None) == (side[0, g] == 0) and (mine[g] is None or mine[g][0] == side[0, g]) for g in range(CAL_B))
sweep = []
for t in SWEEP:
    first = replay(ex.q, ex.mover, ex.game, winner_of, t, CONSECUTIVE)
    would = [g for g in first if first[g] is not None]
    fp = sum(winner_of[g] != -first[g][0] for g in would)
    saved = [rows_of[g] - first[g][1] for g in would]  # searches the game would not have run (the firing one is run)
    sweep.append({"threshold": t, "n_would_resign": len(would), "share": len(would) / CAL_B, "n_false_positive": fp,
                  "false_positive_rate": fp / len(would) if would else None,
                  "mean_searches_saved_per_resigned_game": float(np.mean(saved)) - 1 if would else None})
emit(dict(what="resign calibration", games=CAL_B, sims=SIMS, consecutive=CONSECUTIVE, plies=plies, seconds=round(cal_s, 1),
          mean_rows_per_game=float(lens.mean()), q_quantiles={str(p): float(np.quantile(ex.q, p)) for p in (0.001, 0.01, 0.1, 0.5, 0.9, 0.99, 0.999)},
          engine_records_at=T0, engine_records=int((side != 0).sum()), host_replay_agrees_with_the_engine=bool(agree), sweep=sweep))
del cal

# ---- 2. the loosest threshold within the target
ok = [s for s in sweep if s["n_would_resign"] > 0 and s["false_positive_rate"] <= FP_TARGET]
chosen = max(ok, key=lambda s: s["threshold"]) if ok else None
emit(dict(what="resign threshold", fp_target=FP_TARGET, chosen=chosen,
          note=None if chosen else "no threshold of the sweep resigns a game within the target: the on mode below runs at T0 and resigns nothing"))
threshold = chosen["threshold"] if chosen else T0

# ---- 3. off against on, interleaved: whole games only.  A window over a restarting pool counts the games that happen to end
# inside it, and with resignation on they end a few plies apart from where the pool's stagger put them: such a window measures
# the stagger.  So every repeat plays ROUNDS games per slot from the start to the last game's end, restarting finished slots.
MODES = [("off", None), ("on", Resign(threshold, CONSECUTIVE, PLAYOUT_FRAC))]
pools = [PipelinedSelfPlay("reversi", B, SIMS, "net_bf16", net, rounds=ROUNDS, resign=rs, **KW) for _, rs in MODES]
acc = [{"games": [], "searches": [], "net_rows": [], "steps": []} for _ in MODES]
for r in range(REPS):
    for (name, rs), sp, a in zip(MODES, pools, acc):
        sp.reset_counters()
        sp.reset_games()
        sp.sync()
        searches, steps, active = 0, 0, B
        t0 = time.perf_counter()
        while active:
            searches += active  # the slots in a game: each of them is searched once by the step
            sp.step(True)
            steps += 1
            active, finished = sp.status()
        dt = time.perf_counter() - t0
        assert finished == ROUNDS * B
        c = sp.counters()
        a["games"].append(finished / dt)
        a["searches"].append(searches / finished)
        a["net_rows"].append(c["n_net_leaves"] / finished)
        a["steps"].append(steps)
for (name, rs), sp, a in zip(MODES, pools, acc):
    st = sp.resign_stats() if rs is not None else {}
    emit(dict(what="resign", mode=name, games=B, rounds=ROUNDS, sims=SIMS, pipelines=PIPES, threshold=threshold if rs else None,
              consecutive=CONSECUTIVE if rs else None, playout_frac=PLAYOUT_FRAC if rs else None,
              games_per_s_median=statistics.median(a["games"]), games_per_s_all=[round(x, 2) for x in a["games"]],
              searches_per_game_median=statistics.median(a["searches"]), searches_per_game_all=[round(x, 3) for x in a["searches"]],
              net_rows_per_game_median=statistics.median(a["net_rows"]), net_rows_per_game_all=[round(x, 1) for x in a["net_rows"]],
              steps_all=a["steps"], **({"stats_of_the_last_repeat": st, "resigned_share": st["n_resigned"] / max(1, st["n_finished"])} if rs else {})))
if OUT:
    with open(OUT, "w") as f:
        for row in lines:
            f.write(json.dumps(row) + "\n")
