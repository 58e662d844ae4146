#!/usr/bin/env python3
"""Ownership targets against the plain path, off and on alternating in one process, three repetitions
each after a warm-up, medians.  Numbers, not gates: every on-minus-off difference is stated next to the run-to-run spread of the
off runs.

(a) self-play rate at bench.py's shape: Reversi 8x8, 4096 games, 800 simulations, the bench's 128x6 bf16 net, evaluation cache on
    (carry), two pipelines, temp_moves 8, openings on, a staggered pool that restarts finished games; a fixed number of plies per
    repetition.  With ownership on a move costs two more one-lane-per-game launches (k_root_policy, k_own_final) against 800 tree
    steps and 801 net launches.
(b) the graphed training step at (128 channels, 6 blocks, batch 1024): milliseconds per step without the head (ten launches) and
    with it (k_train_heads_own in place of k_train_heads, and k_train_own_finish as an eleventh), on synthetic rows.
(c) with --parent-tree DIR (a built checkout of the parent commit): the step without the head in this tree against the parent's
    step, in child processes that alternate (one library per process), the same script in both.

    python tools/bench_ownership.py [--quick] [--parent-tree DIR] [--out profiles/ownership_bench.json]"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = "--quick" in sys.argv
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "ownership_bench.json")
PARENT = sys.argv[sys.argv.index("--parent-tree") + 1] if "--parent-tree" in sys.argv else None
SIMS, B = (64, 512) if QUICK else (800, 4096)
REPS, PER, PIPES = 3, (2 if QUICK else 4), 2
TRAIN_STEPS, TRAIN_ROWS = (20, 1 << 14) if QUICK else (100, 1 << 17)
DEV = "cuda:0"

# the plain step alone, as a script both trees can run: prints the milliseconds per step of REPS repetitions
CHILD = r"""
import json, sys, time, torch
sys.path.insert(0, sys.argv[1])
from betazero_amd.engine import DeviceExamples
from betazero_amd.net import PolicyValueNet
from betazero_amd.train import GraphedTrainStep
steps, n, reps = int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
torch.manual_seed(0)
g = torch.Generator(device="cuda:0").manual_seed(0)
pi = torch.rand((n, 65), device="cuda:0", generator=g); pi /= pi.sum(1, keepdim=True)
z = torch.randint(-1, 2, (n,), device="cuda:0", generator=g).to(torch.int8)
zero = lambda dt: torch.zeros(n, dtype=dt, device="cuda:0")
own = torch.randint(0, 2 ** 62, (n,), device="cuda:0", generator=g)
opp = torch.randint(0, 2 ** 62, (n,), device="cuda:0", generator=g) & ~own
data = DeviceExamples(own, opp, pi.contiguous(), z, torch.ones(n, dtype=torch.int8, device="cuda:0"), zero(torch.uint8), zero(torch.int64), zero(torch.int32), 8)
st = GraphedTrainStep(PolicyValueNet(128, 6, 64, fused_tower=True), lr=1e-4, batch=1024)
idx = torch.randint(0, n, (1024,), device="cuda:0", generator=g)
for _ in range(5):
    st(data, idx)
ms = []
for r in range(reps):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(steps):
        st(data, idx)
    torch.cuda.synchronize(); ms.append((time.perf_counter() - t0) * 1e3 / steps)
st.check()
print(json.dumps(ms))
"""


def spread(xs):
    return max(xs) - min(xs)


def on_minus_off(off, on, unit, names=("off", "on")):
    a, b = names
    d = statistics.median(on) - statistics.median(off)
    return {"unit": unit, a + "_all": [round(x, 4) for x in off], b + "_all": [round(x, 4) for x in on], a + "_median": statistics.median(off),
            b + "_median": statistics.median(on), b + "_minus_" + a: d, "spread_of_the_" + a + "_runs": spread(off),
            "difference_above_the_spread": bool(abs(d) > spread(off))}


def child(tree):
    out = subprocess.run([sys.executable, "-c", CHILD, tree, str(TRAIN_STEPS), str(TRAIN_ROWS), "1"], capture_output=True, text=True,
                         timeout=600, cwd=tree)
    if out.returncode != 0:
        raise RuntimeError(out.stderr[-2000:])
    return json.loads(out.stdout.strip().splitlines()[-1])


result = {"what": "ownership targets, off / on alternating", "quick": QUICK}

# ---- (c) first, before this process opens the device for long: this tree's plain step against the parent's, alternating children
if PARENT:
    ms = {"parent": [], "this": []}
    for tree in (PARENT, ROOT):   # (a warm-up child each: code object caches)
        child(tree)
    for r in range(REPS):
        ms["parent"] += child(PARENT)
        ms["this"] += child(ROOT)
    result["train_step_off_against_the_parent"] = dict(channels=128, blocks=6, batch=1024, steps_per_repetition=TRAIN_STEPS,
                                                       **on_minus_off(ms["parent"], ms["this"], "ms/step", ("parent", "this")))

import torch  # noqa: E402

sys.path.insert(0, ROOT)
from betazero_amd.engine import DeviceExamples, PipelinedSelfPlay  # noqa: E402
from betazero_amd.net import DeviceNet, OwnershipHead, PolicyValueNet  # noqa: E402
from betazero_amd.train import GraphedTrainStep  # noqa: E402

torch.manual_seed(0)

# ---- (a) self-play
net = DeviceNet.from_module(PolicyValueNet(128, 6, 64).round_to_bf16_(), B // PIPES)
sps = {}
for on in (False, True):
    sp = PipelinedSelfPlay("reversi", B, SIMS, "net_bf16", net, pipelines=PIPES, temp_moves=8, openings=1, rounds=8, stagger=60, ownership=on)
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
del sps, net

# ---- (b) the training step
g = torch.Generator(device=DEV).manual_seed(0)
n = TRAIN_ROWS
pi = torch.rand((n, 65), device=DEV, generator=g)
pi /= pi.sum(1, keepdim=True)
z = torch.randint(-1, 2, (n,), device=DEV, generator=g).to(torch.int8)
zero = lambda dt: torch.zeros(n, dtype=dt, device=DEV)  # noqa: E731
own = torch.randint(0, 2 ** 62, (n,), device=DEV, generator=g)
opp = torch.randint(0, 2 ** 62, (n,), device=DEV, generator=g) & ~own
fown = torch.randint(0, 2 ** 62, (n,), device=DEV, generator=g)
fopp = torch.randint(0, 2 ** 62, (n,), device=DEV, generator=g) & ~fown
data = DeviceExamples(own, opp, pi.contiguous(), z, torch.ones(n, dtype=torch.int8, device=DEV), zero(torch.uint8), zero(torch.int64),
                      zero(torch.int32), 8, fown=fown, fopp=fopp)
steps = {on: GraphedTrainStep(PolicyValueNet(128, 6, 64, fused_tower=True), lr=1e-4, batch=1024, ownership=OwnershipHead(128) if on else None)
         for on in (False, True)}
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
