#!/usr/bin/env python3
"""fp8 quantisation-aware training, measured.  Numbers, not gates; every record is one JSON line appended to
--out (profiles/fp8_qat_bench.jsonl).

(a) step time: the graphed training step at (128 channels, 6 blocks, batch 1024) without and with fp8_qat, alternating in one
    process, three repetitions each after a warm-up; with --parent-tree DIR (a built checkout of the parent commit) also this
    tree's plain step against the parent's, in child processes that alternate (one library per process, the same script).
(b) fidelity: the same 128x4 net from the same seed trained on the same fixed example set (self-play rows of the uniform
    evaluator) for the same number of steps, once plainly and once with fp8_qat.  For each, over a held-out set: the total-variation
    distance between the policies and the mean |difference of the values| of DeviceNet.forward(fp8=True) and forward(bf16=True) of
    the SAME weights -- what post-training quantisation costs that net -- and the share of the step's stored activations at the
    saturation value 28 (the plain step: at or above it).
(c) --match A.pt B.pt: one recorded match (play_match) of net A against net B, both searched on net_fp8 (state_dicts written by
    az_loop.py --save-net, 128 channels, --blocks as given).

    python tools/bench_fp8_qat.py [--quick] [--parent-tree DIR] [--out profiles/fp8_qat_bench.jsonl]
    python tools/bench_fp8_qat.py --match qat.pt plain.pt [--blocks 4] [--games 512] [--sims 64]"""
import argparse
import copy
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--quick", action="store_true")
ap.add_argument("--parent-tree", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8_qat_bench.jsonl"))
ap.add_argument("--match", nargs=2, default=None, metavar=("A", "B"))
ap.add_argument("--blocks", type=int, default=4)
ap.add_argument("--games", type=int, default=512)
ap.add_argument("--sims", type=int, default=64)
ap.add_argument("--fidelity-steps", type=int, default=600)
args = ap.parse_args()
REPS = 3
TRAIN_STEPS, TRAIN_ROWS = (20, 1 << 14) if args.quick else (100, 1 << 17)
DEV = "cuda:0"

# the plain step alone, as a script both trees can run: prints the milliseconds per step of one repetition
CHILD = r"""
import json, sys, time, torch
sys.path.insert(0, sys.argv[1])
from betazero_amd.engine import DeviceExamples
from betazero_amd.net import PolicyValueNet
from betazero_amd.train import GraphedTrainStep
steps, n = int(sys.argv[2]), int(sys.argv[3])
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
torch.cuda.synchronize(); t0 = time.perf_counter()
for _ in range(steps):
    st(data, idx)
torch.cuda.synchronize()
print(json.dumps([(time.perf_counter() - t0) * 1e3 / steps]))
st.check()
"""


def emit(rec):
    print(json.dumps(rec), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(rec) + "\n")


def a_b(a, b, unit, names):
    na, nb = names
    ma, mb = statistics.median(a), statistics.median(b)
    return {"unit": unit, na + "_all": [round(x, 4) for x in a], nb + "_all": [round(x, 4) for x in b], na + "_median": round(ma, 4),
            nb + "_median": round(mb, 4), nb + "_over_" + na: round(mb / ma, 4), "spread_of_the_" + na + "_runs": round(max(a) - min(a), 4)}


def child(tree):
    out = subprocess.run([sys.executable, "-c", CHILD, tree, str(TRAIN_STEPS), str(TRAIN_ROWS)], capture_output=True, text=True,
                         timeout=300, cwd=tree)
    if out.returncode != 0:
        raise RuntimeError(out.stderr[-2000:])
    return json.loads(out.stdout.strip().splitlines()[-1])


if args.parent_tree and not args.match:   # before this process opens the device: alternating children, one library each
    ms = {"parent": [], "this": []}
    for tree in (args.parent_tree, ROOT):
        child(tree)
    for r in range(REPS):
        ms["parent"] += child(args.parent_tree)
        ms["this"] += child(ROOT)
    emit({"what": "plain training step, this tree against the parent, alternating child processes", "channels": 128, "blocks": 6,
          "batch": 1024, "steps_per_repetition": TRAIN_STEPS, **a_b(ms["parent"], ms["this"], "ms/step", ("parent", "this"))})

import torch  # noqa: E402

sys.path.insert(0, ROOT)
from betazero_amd.engine import DeviceExamples, SelfPlayEngine  # noqa: E402
from betazero_amd.net import DeviceNet, PolicyValueNet  # noqa: E402
from betazero_amd.train import GraphedTrainStep, refresh_device_net, select_rows  # noqa: E402

if args.match:
    from betazero_amd.match import MatchPlayer, play_match
    nets = []
    for path in args.match:
        mod = PolicyValueNet(128, args.blocks, 64, fused_tower=True)
        mod.load_state_dict(torch.load(path, map_location="cpu"))
        nets.append(DeviceNet.from_module(mod.round_to_bf16_(), args.games))
    t0 = time.time()
    res = play_match("reversi", args.games, MatchPlayer(sims=args.sims, net=nets[0], evaluator="net_fp8"),
                     MatchPlayer(sims=args.sims, net=nets[1], evaluator="net_fp8"), opening_plies=4, seed=1)
    emit({"what": "match on net_fp8: A against B", "A": os.path.basename(args.match[0]), "B": os.path.basename(args.match[1]),
          "sims": args.sims, "opening_plies": 4, **res.summary(), "seconds": round(time.time() - t0, 1)})
    sys.exit(0)

torch.manual_seed(0)
g = torch.Generator(device=DEV).manual_seed(0)

# ---- (a) the step, fp8_qat off / on alternating
n = TRAIN_ROWS
pi = torch.rand((n, 65), device=DEV, generator=g)
pi /= pi.sum(1, keepdim=True)
z = torch.randint(-1, 2, (n,), device=DEV, generator=g).to(torch.int8)
zero = lambda dt: torch.zeros(n, dtype=dt, device=DEV)  # noqa: E731
own = torch.randint(0, 2 ** 62, (n,), device=DEV, generator=g)
opp = torch.randint(0, 2 ** 62, (n,), device=DEV, generator=g) & ~own
data = DeviceExamples(own, opp, pi.contiguous(), z, torch.ones(n, dtype=torch.int8, device=DEV), zero(torch.uint8), zero(torch.int64),
                      zero(torch.int32), 8)
steps = {on: GraphedTrainStep(PolicyValueNet(128, 6, 64, fused_tower=True), lr=1e-4, batch=1024, fp8_qat=on) for on in (False, True)}
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
emit({"what": "training step, fp8_qat off / on alternating", "channels": 128, "blocks": 6, "batch": 1024, "steps_per_repetition": TRAIN_STEPS,
      **a_b(ms[False], ms[True], "ms/step", ("off", "on"))})
del steps, data

# ---- (b) fidelity of the fp8 engine to the bf16 engine, after plain and after quantisation-aware training
G, S = (256, 16) if args.quick else (1024, 32)
eng = SelfPlayEngine("reversi", G, S, "uniform", temp_moves=10, seed=1)
eng.run_iteration()
ex = eng.device_examples()
perm = torch.randperm(len(ex), device=DEV, generator=g)
n_val = min(4096, len(ex) // 5)
val, train = select_rows(ex, perm[:n_val]), select_rows(ex, perm[n_val:])
del eng
torch.manual_seed(1)
seed_net = PolicyValueNet(128, args.blocks, 64, fused_tower=True)
n_steps = 60 if args.quick else args.fidelity_steps
batches = [torch.randint(0, len(train), (1024,), device=DEV, generator=g) for _ in range(n_steps)]
for qat in (False, True):
    module = copy.deepcopy(seed_net)
    step = GraphedTrainStep(module, lr=2e-3, batch=1024, lr_warmup_steps=100, fp8_qat=qat)
    losses = [step(train, b) for b in batches]
    step.check()
    sp = step.step_plan
    acts = sp.acts.float()
    sat = float((acts >= 28.0).float().mean())
    dn = DeviceNet.from_module(copy.deepcopy(module).cpu().round_to_bf16_(), n_val)
    refresh_device_net(dn, module)
    l8, v8 = dn.forward(val.own, val.opp, fp8=True)
    l16, v16 = dn.forward(val.own, val.opp, bf16=True)
    tv = 0.5 * (torch.softmax(l8, 1) - torch.softmax(l16, 1)).abs().sum(1)
    ce = lambda lg: float(-(val.pi * torch.log_softmax(lg, 1)).sum(1).mean())  # noqa: E731
    emit({"what": "fidelity of forward(fp8=True) to forward(bf16=True) of the same trained weights, held-out rows", "fp8_qat": qat,
          "blocks": args.blocks, "steps": n_steps, "train_rows": len(train), "held_out_rows": n_val,
          "loss_last_tenth": [round(float(x), 4) for x in torch.stack(losses[-max(1, n_steps // 10):]).mean(0)],
          "policy_tv_mean": round(float(tv.mean()), 5), "policy_tv_max": round(float(tv.max()), 5),
          "value_abs_diff_mean": round(float((v8 - v16).abs().mean()), 5), "top1_agreement": round(float((l8.argmax(1) == l16.argmax(1)).float().mean()), 4),
          "held_out_policy_ce_fp8": round(ce(l8), 4), "held_out_policy_ce_bf16": round(ce(l16), 4),
          "held_out_value_mse_fp8": round(float(((v8 - val.z.float()) ** 2).mean()), 4),
          "held_out_value_mse_bf16": round(float(((v16 - val.z.float()) ** 2).mean()), 4),
          "share_of_stored_activations_at_or_above_28": round(sat, 6), "largest_stored_activation": round(float(acts.max()), 3)})
