#!/usr/bin/env python3
"""Position averaging on one MI355X: how much of a real training window is repeated positions, and what the
merge costs.

 1. The repeated share of real augmented windows: self-play with an untrained net, az_loop's data path (80 / 20 hold-out split,
    8-fold augmentation + exact dedupe of the training part, a window of 3 iterations) at az_loop's defaults (2048 games, 64
    simulations, 64x4 net) and at bench.py's shape (4096 games, 800 simulations, 128x6 net): rows before and after the merge,
    the largest group, the share of rows standing in groups larger than 1 -- in total and by ply.
 2. The merge's time at those row counts -- merge_positions as az_loop calls it, grouping and the one wait included, and its
    three kernels alone -- against a torch restatement of the same integer rule written here (the same grouping, index_add_ on
    int64, integer floor division): the torch time is the yardstick.  The two results must be the same bits (asserted).
 3. With --parent-tree DIR (a built checkout of the parent commit): plain `bench.py --gpus 1 --steps 8 --warmup 2` there and
    here, three interleaved pairs -- self-play must be untouched.

One JSON object per line on stdout.

    python tools/bench_merge.py [--quick] [--out profiles/merge_bench.jsonl]
    python tools/bench_merge.py --ab-only --parent-tree DIR [--out profiles/merge_bench.jsonl]   # part 3 alone, appended: this
                                                                                                 # process then opens no GPU"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from betazero_amd import _lib  # noqa: E402
from betazero_amd import merge as M  # noqa: E402
from betazero_amd.augment import augment_examples  # noqa: E402
from betazero_amd.engine import PipelinedSelfPlay, concat_device_examples  # noqa: E402
from betazero_amd.net import DeviceNet, PolicyValueNet  # noqa: E402
from betazero_amd.train import holdout_split, select_rows  # noqa: E402


def _arg(name, default, conv=str):
    return conv(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


QUICK = "--quick" in sys.argv
AB_ONLY = "--ab-only" in sys.argv
OUT = _arg("--out", None)
PARENT = _arg("--parent-tree", None)
DEV = "cuda:0"
REPS = 2 if QUICK else 5
# (name, games, sims, channels, blocks)
SHAPES = [("az_loop defaults", 256 if QUICK else 2048, 16 if QUICK else 64, 64, 4)] + \
         ([] if QUICK else [("bench.py shape", 4096, 800, 128, 6)])
if AB_ONLY:
    SHAPES = []
lines = []


def emit(row):
    lines.append(row)
    print(json.dumps(row), flush=True)


def window(games, sims, channels, blocks, iters=3):
    """az_loop's training window from an untrained net: (augmented rows of `iters` iterations, rows self-play recorded)"""
    torch.manual_seed(0)
    gen = torch.Generator(device=DEV).manual_seed(0)
    dnet = DeviceNet.from_module(PolicyValueNet(channels, blocks, 64).round_to_bf16_(), games)
    parts, recorded = [], 0
    for it in range(1, iters + 1):
        sp = PipelinedSelfPlay("reversi", games, sims, "net_bf16", dnet, pipelines=2, temp_moves=10, openings=1, seed=it,
                               dirichlet_alpha=0.3, dirichlet_eps=0.25)
        sp.run_iteration()
        ex = sp.device_examples()
        recorded += len(ex)
        tr_idx, _ = holdout_split(len(ex), 0.2, gen, ex.own.device)
        parts.append(augment_examples(select_rows(ex, tr_idx), dedupe=True))
        del sp
    return concat_device_examples(parts), recorded


def group_sizes(data):
    """per input row: the rows of its group"""
    order, start, dst, head, count, n_groups = M._grouping(data.own.contiguous(), data.opp.contiguous())
    per_sorted = count[dst.to(torch.int64)]
    return torch.empty_like(per_sorted).scatter_(0, order, per_sorted)


def torch_merge(data):
    """the rule of DESIGN.md 3.26 restated in torch: (pi, vt, counts) of the merged rows"""
    n, na = data.pi.shape
    order, start, dst, head, count, n_groups = M._grouping(data.own.contiguous(), data.opp.contiguous())
    groups = int(n_groups)
    row_group = torch.empty(n, dtype=torch.int64, device=DEV).scatter_(0, order, dst.to(torch.int64))
    cnt = count[:groups].to(torch.int64)
    val = data.z.to(torch.float32) if data.vt is None else data.vt

    def mean(x):
        fixed = (x * 4294967296.0).to(torch.int64)  # truncates
        S = torch.zeros((groups,) + x.shape[1:], dtype=torch.int64, device=DEV).index_add_(0, row_group, fixed)
        c = cnt.view(-1, *([1] * (x.dim() - 1)))
        m = torch.div(2 * S + c, 2 * c, rounding_mode="floor")
        return torch.where(c == 1, x[head[:groups]], (m.to(torch.float64) * 2.0 ** -32).to(torch.float32))
    return mean(data.pi), mean(val), count[:groups]


def kernels_only(data):
    """a closure that launches bz_merge_positions' three kernels on prepared index lists, and nothing else"""
    n, na = data.pi.shape
    own, opp, pi = data.own.contiguous(), data.opp.contiguous(), data.pi.contiguous()
    order, start, dst, head, count, n_groups = M._grouping(own, opp)
    new = lambda t, *s: torch.empty((n, *s), dtype=t.dtype, device=DEV)  # noqa: E731
    o = dict(own=new(own), opp=new(opp), pi=new(pi, na), z=torch.empty(n, dtype=torch.int8, device=DEV),
             mover=torch.empty(n, dtype=torch.int8, device=DEV), act=torch.empty(n, dtype=torch.uint8, device=DEV), game=new(own),
             ply=torch.empty(n, dtype=torch.int32, device=DEV), vt=new(pi), q=None, kl=None)
    keep = [own, opp, pi, order, start, dst, head, count, n_groups, o]
    L = _lib.lib()
    wbytes = L.bz_merge_workspace_bytes(n, na)
    ws = torch.empty(wbytes + 256, dtype=torch.uint8, device=DEV)
    ws = ws[(-ws.data_ptr()) & 255:][:wbytes]
    status = torch.zeros(1, dtype=torch.int64, device=DEV)
    z, mover, act = data.z.to(torch.int8).contiguous(), data.mover.to(torch.int8).contiguous(), data.act.to(torch.uint8).contiguous()
    game, ply = data.game.to(torch.int64).contiguous(), data.ply.to(torch.int32).contiguous()
    keep += [z, mover, act, game, ply]
    rin = M._rows(own, opp, pi, z, mover, act, game, ply, data.vt, None, None)
    rout = M._rows(**o)
    st = torch.cuda.current_stream().cuda_stream

    def run():
        _lib.check(L.bz_merge_positions(C.byref(rin), n, na, order.data_ptr(), start.data_ptr(), dst.data_ptr(), head.data_ptr(),
                                        count.data_ptr(), n_groups.data_ptr(), ws.data_ptr(), wbytes, C.byref(rout), status.data_ptr(), st))
    run.keep = keep
    return run


def timed(fn):
    """median and all wall times in ms of REPS calls after one warm-up, the device drained before and after each"""
    fn()
    out = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), [round(x, 3) for x in out]


for name, games, sims, channels, blocks in SHAPES:
    data, recorded = window(games, sims, channels, blocks)
    n = len(data)
    merged, counts = M.merge_positions(data, return_counts=True)
    size = group_sizes(data)
    ply = data.ply.to(torch.int64)
    rows_by_ply = torch.bincount(ply, minlength=61)
    rep_by_ply = torch.bincount(ply, weights=(size > 1).to(torch.float64), minlength=61)
    by_ply = {int(p): round(float(rep_by_ply[p] / rows_by_ply[p]), 4) for p in range(len(rows_by_ply)) if int(rows_by_ply[p]) and
              (p < 12 or p % 10 == 0)}
    emit(dict(what="merge, repeated share of an augmented training window", shape=name, games=games, sims=sims, net=f"{channels}x{blocks} untrained",
              iterations=3, val_split=0.2, rows_recorded=recorded, rows_before=n, rows_after=len(merged), largest_group=int(counts.max()),
              share_rows_in_groups=round(float((size > 1).double().mean()), 4), share_by_ply=by_ply,
              last_ply_with_a_repeat=int(ply[size > 1].max()) if bool((size > 1).any()) else None))
    # the two restatements agree to the bit before either is timed
    t_pi, t_vt, t_cnt = torch_merge(data)
    assert torch.equal(t_pi.view(torch.int32), merged.pi.view(torch.int32)) and torch.equal(t_vt.view(torch.int32), merged.vt.view(torch.int32))
    assert torch.equal(t_cnt, counts)
    run = kernels_only(data)
    grouping_ms = timed(lambda: M._grouping(data.own, data.opp))
    merge_ms, torch_ms, kernels_ms = timed(lambda: M.merge_positions(data)), timed(lambda: torch_merge(data)), timed(run)
    emit(dict(what="merge, time", shape=name, rows=n, groups=len(merged), reps=REPS,
              merge_positions_ms_median=round(merge_ms[0], 3), merge_positions_ms=merge_ms[1],
              torch_restatement_ms_median=round(torch_ms[0], 3), torch_restatement_ms=torch_ms[1],
              grouping_ms_median=round(grouping_ms[0], 3), grouping_ms=grouping_ms[1],
              kernels_ms_median=round(kernels_ms[0], 3), kernels_ms=kernels_ms[1], same_bits=True,
              note="merge_positions and the torch restatement both include the grouping (two stable sorts and the index lists: "
                   "grouping_ms) and one wait; kernels_ms is k_merge_zero + k_merge_reduce + k_merge_finish alone; the torch restatement "
                   "merges pi and the value only, merge_positions every column"))
    del data, merged, run
    torch.cuda.empty_cache()

if PARENT:
    if SHAPES:  # the processes below own the GPU one at a time; this one keeps its context but runs nothing meanwhile
        torch.cuda.synchronize()
    runs = []
    for pair in range(3):
        for arm, tree in (("parent", PARENT), ("new", ROOT)):
            out = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "8", "--warmup", "2"], cwd=tree,
                                 capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise RuntimeError(f"bench.py failed in {tree}: {out.stderr[-1500:]}")
            res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
            runs.append((arm, res["value"]))
    val = {arm: [v for a, v in runs if a == arm] for arm in ("parent", "new")}
    emit(dict(what="bench.py --gpus 1 --steps 8 --warmup 2, parent commit against this tree, three interleaved pairs", unit="games/s",
              run_order=[[a, round(v, 2)] for a, v in runs], parent_median=round(statistics.median(val["parent"]), 2),
              new_median=round(statistics.median(val["new"]), 2),
              new_over_parent=round(statistics.median(val["new"]) / statistics.median(val["parent"]), 5)))

if OUT:
    with open(OUT, "a" if AB_ONLY else "w") as f:
        for row in lines:
            f.write(json.dumps(row) + "\n")
