#!/usr/bin/env python3
"""What a checkpoint costs, measured.  Numbers, not gates: they say what --checkpoint-every should default to.
The record goes to --out (profiles/checkpoint_bench.json).

Two shapes: tools/az_loop.py's defaults (64 channels x 4 blocks, 2048 games, 64 simulations, window 3: ~60 recorded rows a game)
and a window of bench.py's shape (128 x 6, 4096 games: ~237,000 rows an iteration, window 3).  For each, in this process, on
synthetic rows of that count (a checkpoint's cost depends on the rows' number, not on their content -- apart from the zip
being stored, not compressed):

    write_s            save_checkpoint of the loop's state: the step's state_dict (device -> host), the rows, the file
    write_no_window_s  the same without the window
    resume_s           load_checkpoint, the step's load_state_dict, the rows back onto the device and augment_examples(dedupe=True)
    bytes, bytes_no_window

and, with --parent-tree DIR (a built checkout of the parent commit), seconds per iteration of `az_loop.py --iters K
--checkpoint-every 1` in this tree against the parent's loop without checkpoints, child processes that alternate, --pairs times.

    python tools/bench_checkpoint.py [--quick] [--parent-tree DIR] [--out profiles/checkpoint_bench.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
ap = argparse.ArgumentParser()
ap.add_argument("--quick", action="store_true", help="a tenth of the rows, one pair, two iterations")
ap.add_argument("--parent-tree", default=None)
ap.add_argument("--pairs", type=int, default=3)
ap.add_argument("--iters", type=int, default=3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "checkpoint_bench.json"))
args = ap.parse_args()

import torch  # noqa: E402

from az_loop import rows_to_device, to_host, window_rows  # noqa: E402
from betazero_amd.augment import augment_examples  # noqa: E402
from betazero_amd.checkpoint import load_checkpoint, save_checkpoint  # noqa: E402
from betazero_amd.engine import DeviceExamples  # noqa: E402
from betazero_amd.net import PolicyValueNet  # noqa: E402
from betazero_amd.train import GraphedTrainStep  # noqa: E402

DEV = "cuda:0"
SHAPES = {"az_loop_defaults": dict(channels=64, blocks=4, batch=1024, rows=2048 * 60, window=3, loop=[]),
          "bench_window": dict(channels=128, blocks=6, batch=1024, rows=237000, window=3,
                               loop=["--channels", "128", "--blocks", "6", "--games", "4096"])}


def synthetic_rows(n, gen):
    """n distinct-looking rows before augmentation, with the columns a default run records"""
    own = torch.randint(0, 2 ** 62, (n,), device=DEV, generator=gen)
    opp = torch.randint(0, 2 ** 62, (n,), device=DEV, generator=gen) & ~own
    pi = torch.rand((n, 65), device=DEV, generator=gen)
    pi /= pi.sum(1, keepdim=True)
    zero = lambda dt: torch.zeros(n, dtype=dt, device=DEV)  # noqa: E731
    return DeviceExamples(own, opp, pi.contiguous(), torch.randint(-1, 2, (n,), device=DEV, generator=gen).to(torch.int8),
                          torch.ones(n, dtype=torch.int8, device=DEV), zero(torch.uint8), torch.arange(n, device=DEV) // 60, zero(torch.int32), 8)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def in_process(name, shape):
    gen = torch.Generator(device=DEV).manual_seed(0)
    torch.manual_seed(0)
    rows = shape["rows"] // (10 if args.quick else 1)
    step = GraphedTrainStep(PolicyValueNet(shape["channels"], shape["blocks"], 64, fused_tower=True), lr=2e-3, batch=shape["batch"])
    slots = []
    for _ in range(shape["window"]):
        ex = synthetic_rows(rows, gen)
        cut = int(0.8 * rows)
        idx = torch.arange(rows, device=DEV)
        from betazero_amd.train import select_rows
        slots.append((select_rows(ex, idx[:cut]), select_rows(ex, idx[cut:])))

    def state(window):
        return to_host({"iter": 1, "args": {}, "lines": [], "step": step.state_dict(), "generator": gen.get_state(),
                        "window": [{"train": window_rows(a), "val": window_rows(b)} for a, b in slots] if window else None})

    def resume(path):
        ck = load_checkpoint(path)
        step.load_state_dict(ck["step"])
        return [(augment_examples(rows_to_device(w["train"]), dedupe=True), rows_to_device(w["val"])) for w in ck["window"]]

    rec = {"shape": name, "rows_per_iteration": rows, "window": shape["window"], "channels": shape["channels"], "blocks": shape["blocks"]}
    with tempfile.TemporaryDirectory() as d:
        full, small = os.path.join(d, "full.ckpt"), os.path.join(d, "small.ckpt")
        for _ in range(2):   # the second repetition is the record (the first pays the allocator and the page cache)
            rec["write_s"] = round(timed(lambda: save_checkpoint(full, state(True)))[0], 3)
            rec["write_no_window_s"] = round(timed(lambda: save_checkpoint(small, state(False)))[0], 3)
            t, win = timed(lambda: resume(full))
            rec["resume_s"] = round(t, 3)
        rec["augmented_rows"] = int(sum(len(a) for a, _ in win))
        rec["bytes"], rec["bytes_no_window"] = os.path.getsize(full), os.path.getsize(small)
    return rec


def loop_seconds(tree, flags, iters, checkpoint):
    """wall seconds per iteration of one az_loop child process in `tree` (its two opening arenas included in both arms)"""
    with tempfile.TemporaryDirectory() as d:
        extra = ["--checkpoint", os.path.join(d, "run.ckpt"), "--checkpoint-every", "1"] if checkpoint else []
        t0 = time.perf_counter()
        out = subprocess.run([sys.executable, os.path.join(tree, "tools", "az_loop.py"), *flags, "--iters", str(iters), "--arena-games", "16",
                              "--final-depths", "", *extra], capture_output=True, text=True, timeout=1500)
        if out.returncode != 0:
            raise RuntimeError(out.stderr[-2000:])
        return (time.perf_counter() - t0) / iters


record = {"in_process": [in_process(k, v) for k, v in SHAPES.items()], "per_iteration": "not measured (needs --parent-tree)"}
if args.parent_tree:
    record["per_iteration"] = []
    iters, pairs = (2, 1) if args.quick else (args.iters, args.pairs)
    for name, shape in SHAPES.items():
        ours, parent = [], []
        for _ in range(pairs):   # interleaved: parent, this tree, parent, ...
            parent.append(loop_seconds(args.parent_tree, shape["loop"], iters, False))
            ours.append(loop_seconds(ROOT, shape["loop"], iters, True))
        record["per_iteration"].append({"shape": name, "iters": iters, "parent_s": [round(x, 2) for x in parent],
                                        "checkpoint_every_1_s": [round(x, 2) for x in ours],
                                        "ratio_of_medians": round(statistics.median(ours) / statistics.median(parent), 4)})
print(json.dumps(record, indent=1))
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    json.dump(record, f, indent=1)
