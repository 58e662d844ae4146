#!/usr/bin/env python3
"""A board symmetry per row inside the training step against the eightfold copy, alternating runs, three
repetitions each after a warm-up, medians.  Numbers, not gates: every difference is stated next to the run-to-run spread.

(a) the graphed training step at (128 channels, 6 blocks, batch 1024) on synthetic rows: milliseconds per step with symmetry off
    (ten launches) and on (k_train_sym_batch in front: eleven), alternating in one process.
(b) with --parent-tree DIR (a built checkout of the parent commit): the step with symmetry off in this tree against the parent's
    step, in child processes that alternate (one library per process), the same script in both.
(c) the loop's cost at az_loop's defaults (2048 games, 64x4 net, batch 1024, window 3) and at bench.py's shape (4096 games, 128x6):
    synthetic training rows of one iteration (games x 60 plies x 0.8 after the hold-out split), augment_examples(dedupe=True) of
    them in seconds, the device bytes of a three-slot window with the eightfold copy and with the rows as played, and one
    iteration's training in seconds -- an epoch of graphed steps over the window, timed, with the flag off and on.
(d) with --parent-tree and --bench: plain `bench.py --gpus 1 --steps 8 --warmup 2`, parent against this tree, three interleaved
    pairs.

Whether a fresh symmetry per epoch trains better than a fixed eightfold copy is NOT measured here.

    python tools/bench_train_symmetry.py [--quick] [--parent-tree DIR [--bench]] [--out profiles/train_symmetry_bench.json]"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = "--quick" in sys.argv
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "train_symmetry_bench.json")
PARENT = sys.argv[sys.argv.index("--parent-tree") + 1] if "--parent-tree" in sys.argv else None
REPS = 3
TRAIN_STEPS, TRAIN_ROWS = (20, 1 << 14) if QUICK else (100, 1 << 17)
DEV = "cuda:0"
SHAPES = [("az_loop defaults", 2048, 64, 4)] + ([] if QUICK else [("bench.py shape", 4096, 128, 6)])
PLIES, TRAIN_SHARE, WINDOW, BATCH = 60, 0.8, 3, 1024


# the plain step alone, as a script both trees can run: prints the milliseconds per step of its repetitions
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


def note(msg):
    print(f"[bench_train_symmetry] {msg}", file=sys.stderr, flush=True)


result = {"what": "a board symmetry per row inside the training step, off / on alternating", "quick": QUICK}

# ---- (b) first, before this process opens the device: this tree's plain step against the parent's, alternating children
if PARENT:
    def child(tree):
        out = subprocess.run([sys.executable, "-c", CHILD, tree, str(TRAIN_STEPS), str(TRAIN_ROWS), "1"], capture_output=True, text=True,
                             timeout=600, cwd=tree)
        if out.returncode != 0:
            raise RuntimeError(out.stderr[-2000:])
        return json.loads(out.stdout.strip().splitlines()[-1])
    ms = {"parent": [], "this": []}
    for tree in (PARENT, ROOT):
        child(tree)
    for r in range(REPS):
        ms["parent"] += child(PARENT)
        ms["this"] += child(ROOT)
        note(f"parent / this pair {r + 1} of {REPS}: {ms['parent'][-1]:.4f} / {ms['this'][-1]:.4f} ms per step")
    result["train_step_off_against_the_parent"] = dict(channels=128, blocks=6, batch=1024, steps_per_repetition=TRAIN_STEPS,
                                                       **on_minus_off(ms["parent"], ms["this"], "ms/step", ("parent", "this")))
    if "--bench" in sys.argv:
        runs = []
        for pair in range(3):
            for arm, tree in (("parent", PARENT), ("new", ROOT)):
                out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "8", "--warmup", "2"], cwd=tree,
                                     capture_output=True, text=True, timeout=600)
                if out.returncode != 0:
                    raise RuntimeError(f"bench.py failed in {tree}: {out.stderr[-1500:]}")
                note(f"bench.py pair {pair + 1}, {arm}")
                runs.append((arm, json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])["value"]))
        val = {arm: [v for a, v in runs if a == arm] for arm in ("parent", "new")}
        result["bench_py"] = dict(what="bench.py --gpus 1 --steps 8 --warmup 2, parent commit against this tree, three interleaved pairs",
                                  unit="games/s", run_order=[[a, round(v, 2)] for a, v in runs], parent_median=statistics.median(val["parent"]),
                                  new_median=statistics.median(val["new"]),
                                  new_over_parent=round(statistics.median(val["new"]) / statistics.median(val["parent"]), 5))

import torch  # noqa: E402

sys.path.insert(0, ROOT)
from betazero_amd.augment import augment_examples  # noqa: E402
from betazero_amd.engine import DeviceExamples, concat_device_examples  # noqa: E402
from betazero_amd.examples import columns  # noqa: E402
from betazero_amd.net import PolicyValueNet  # noqa: E402
from betazero_amd.train import GraphedTrainStep  # noqa: E402

torch.manual_seed(0)
g = torch.Generator(device=DEV).manual_seed(0)


def rows(n):
    """synthetic training rows: random disjoint boards, a normalised pi"""
    pi = torch.rand((n, 65), device=DEV, generator=g)
    pi /= pi.sum(1, keepdim=True)
    zero = lambda dt: torch.zeros(n, dtype=dt, device=DEV)  # noqa: E731
    own = torch.randint(0, 2 ** 62, (n,), device=DEV, generator=g)
    opp = torch.randint(0, 2 ** 62, (n,), device=DEV, generator=g) & ~own
    return DeviceExamples(own, opp, pi.contiguous(), torch.randint(-1, 2, (n,), device=DEV, generator=g).to(torch.int8),
                          torch.ones(n, dtype=torch.int8, device=DEV), zero(torch.uint8), zero(torch.int64), zero(torch.int32), 8)


def timed_steps(steps, data, n_steps):
    """ms per step of n_steps graphed steps per arm, REPS repetitions, the arms alternating; idx (and sym) drawn per step as
    az_loop draws them"""
    ms = {k: [] for k in steps}
    for r in range(REPS + 1):   # (the first repetition is the warm-up)
        for on, st in steps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n_steps):
                idx = torch.randint(0, len(data[on]), (BATCH,), device=DEV, generator=g)
                if on:
                    st(data[on], idx, torch.randint(0, 8, (BATCH,), dtype=torch.uint8, device=DEV, generator=g))
                else:
                    st(data[on], idx)
            torch.cuda.synchronize()
            if r:
                ms[on].append((time.perf_counter() - t0) * 1e3 / n_steps)
    for st in steps.values():
        st.check()
    return ms


# ---- (a) the step alone
data = rows(TRAIN_ROWS)
steps = {on: GraphedTrainStep(PolicyValueNet(128, 6, 64, fused_tower=True), lr=1e-4, batch=BATCH, symmetry=on) for on in (False, True)}
ms = timed_steps(steps, {False: data, True: data}, TRAIN_STEPS)
result["train_step"] = dict(channels=128, blocks=6, batch=BATCH, steps_per_repetition=TRAIN_STEPS, **on_minus_off(ms[False], ms[True], "ms/step"))
note(f"step off / on: {ms[False]} / {ms[True]} ms")
del steps, data

# ---- (c) the loop's cost
result["loop"] = []
for name, games, C, NB in SHAPES:
    per_iter = int(games * PLIES * TRAIN_SHARE) // (8 if QUICK else 1)
    slots = [rows(per_iter) for _ in range(WINDOW)]
    aug_s = []
    for r in range(REPS + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        aug = augment_examples(slots[r % WINDOW], dedupe=True)
        torch.cuda.synchronize()
        if r:
            aug_s.append(time.perf_counter() - t0)
    window = {False: concat_device_examples([augment_examples(s, dedupe=True) for s in slots]), True: concat_device_examples(slots)}
    nbytes = {on: sum(t.numel() * t.element_size() for t in columns(w).values()) for on, w in window.items()}
    steps = {on: GraphedTrainStep(PolicyValueNet(C, NB, 64, fused_tower=True), lr=1e-4, batch=BATCH, symmetry=on) for on in (False, True)}
    n_steps = max(1, len(window[False]) // BATCH) // (8 if QUICK else 1)   # an epoch over the augmented window; the flag's epoch is 8 x rows
    ms = timed_steps(steps, window, n_steps)
    result["loop"].append(dict(shape=name, games=games, channels=C, blocks=NB, training_rows_per_iteration=per_iter, window_slots=WINDOW,
                               augment_examples_s_per_iteration=dict(all=[round(x, 4) for x in aug_s], median=statistics.median(aug_s)),
                               window_rows=dict(augmented=len(window[False]), as_played=len(window[True])),
                               window_device_bytes=dict(augmented=nbytes[False], as_played=nbytes[True]),
                               steps_per_epoch=n_steps,
                               training_s_per_iteration=on_minus_off([x * n_steps / 1e3 for x in ms[False]], [x * n_steps / 1e3 for x in ms[True]], "s")))
    note(f"{name}: done")
    del steps, window, slots, aug
    torch.cuda.empty_cache()

print(json.dumps(result), flush=True)
os.makedirs(os.path.dirname(OUT), exist_ok=True)
with open(OUT, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
