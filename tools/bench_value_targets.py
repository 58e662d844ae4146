#!/usr/bin/env python3
"""Search-value targets against the plain path, off and on alternating in one process, three repetitions each
after a warm-up.  Numbers, not gates: every on-minus-off difference is stated next to the run-to-run spread of the off runs.

(a) self-play rate at cfg 3's shape (the headline's): Reversi 8x8, 4096 games, 800 simulations, the bench's 128x6 bf16 net,
    evaluation cache on (carry), two pipelines, temp_moves 8, openings on, a staggered pool that restarts finished games; a
    fixed number of plies per repetition.  With search_value on a move costs one more one-lane-per-game launch (k_root_q)
    against 800 tree steps and 801 net launches.
(b) value_targets() on the rows that pool has finished by then: rows and microseconds per call (two launches and the one
    read-back of the status word).
(c) the graphed training step at (128 channels, 6 blocks, batch 1024): milliseconds per step with z (k_train_heads) and with vt
    (k_train_heads_vt), on synthetic rows.

    python tools/bench_value_targets.py [--quick] [--out profiles/value_targets_bench.json]"""
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from betazero_amd.engine import DeviceExamples, PipelinedSelfPlay  # noqa: E402
from betazero_amd.net import DeviceNet, PolicyValueNet  # noqa: E402
from betazero_amd.train import GraphedTrainStep  # noqa: E402
from betazero_amd.value_targets import value_targets  # noqa: E402

QUICK = "--quick" in sys.argv
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "value_targets_bench.json")
SIMS, B = (64, 512) if QUICK else (800, 4096)
REPS, PER, PIPES = 3, (2 if QUICK else 4), 2
TRAIN_STEPS, TRAIN_ROWS = (20, 1 << 14) if QUICK else (100, 1 << 17)
DEV = "cuda:0"


def spread(xs):
    return max(xs) - min(xs)


def on_minus_off(off, on, unit):
    d = statistics.median(on) - statistics.median(off)
    return {"unit": unit, "off_all": [round(x, 4) for x in off], "on_all": [round(x, 4) for x in on], "off_median": statistics.median(off),
            "on_median": statistics.median(on), "on_minus_off": d, "spread_of_the_off_runs": spread(off),
            "difference_above_the_spread": bool(abs(d) > spread(off))}


torch.manual_seed(0)
result = {"what": "search-value targets, off / on alternating", "quick": QUICK}

# ---- (a) self-play
net = DeviceNet.from_module(PolicyValueNet(128, 6, 64).round_to_bf16_(), B // PIPES)
sps = {}
for on in (False, True):
    sp = PipelinedSelfPlay("reversi", B, SIMS, "net_bf16", net, pipelines=PIPES, temp_moves=8, openings=1, rounds=8, stagger=60,
                           search_value=on)
    sp.reset_games()
    for _ in range(2):
        sp.step(True)
    sp.status()
    sps[on] = sp
rates = {False: [], True: []}
for r in range(REPS):
    for on in (False, True):
        sp = sps[on]
        f0 = sp.status()[1]
        t0 = time.perf_counter()
        for _ in range(PER):
            sp.step(True)
            sp.sync()
        f1 = sp.status()[1]
        rates[on].append((f1 - f0) / (time.perf_counter() - t0))
result["self_play"] = dict(games=B, sims=SIMS, pipelines=PIPES, plies_per_repetition=PER, **on_minus_off(rates[False], rates[True], "games/s"))

# ---- (b) value_targets on the finished games' rows of that pool
ex = sps[True].device_examples()
del sps
if len(ex):
    value_targets(ex, 0.8, 0.25)  # (warm-up: the allocator's blocks)
    us = []
    for _ in range(REPS + 4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        value_targets(ex, 0.8, 0.25)
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6)
    result["value_targets"] = dict(rows=len(ex), games=int(torch.unique(ex.game).numel()), lam=0.8, q_mix=0.25, us_per_call_median=statistics.median(us),
                                   us_per_call_all=[round(x, 1) for x in us], includes="two launches and the status word's read-back")
else:
    result["value_targets"] = dict(rows=0, note="no game had finished")
del ex, net

# ---- (c) the training step
g = torch.Generator(device=DEV).manual_seed(0)
n = TRAIN_ROWS
pi = torch.rand((n, 65), device=DEV, generator=g)
pi /= pi.sum(1, keepdim=True)
z = torch.randint(-1, 2, (n,), device=DEV, generator=g).to(torch.int8)
zero = lambda dt: torch.zeros(n, dtype=dt, device=DEV)  # noqa: E731
own = torch.randint(0, 2 ** 62, (n,), device=DEV, generator=g)
opp = torch.randint(0, 2 ** 62, (n,), device=DEV, generator=g) & ~own
data = DeviceExamples(own, opp, pi.contiguous(), z, torch.ones(n, dtype=torch.int8, device=DEV), zero(torch.uint8), zero(torch.int64),
                      zero(torch.int32), 8, vt=(torch.rand(n, device=DEV, generator=g) * 2 - 1).contiguous())
steps = {on: GraphedTrainStep(PolicyValueNet(128, 6, 64, fused_tower=True), lr=1e-4, batch=1024, value_targets=on) for on in (False, True)}
idx = torch.randint(0, n, (1024,), device=DEV, generator=g)
for st in steps.values():
    for _ in range(5):
        st(data, idx)
torch.cuda.synchronize()
ms = {False: [], True: []}
for r in range(REPS):
    for on in (False, True):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(TRAIN_STEPS):
            steps[on](data, idx)
        torch.cuda.synchronize()
        ms[on].append((time.perf_counter() - t0) * 1e3 / TRAIN_STEPS)
for st in steps.values():
    st.check()
result["train_step"] = dict(channels=128, blocks=6, batch=1024, steps_per_repetition=TRAIN_STEPS, **on_minus_off(ms[False], ms[True], "ms/step"))

print(json.dumps(result), flush=True)
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
