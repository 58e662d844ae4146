#!/usr/bin/env python3
"""Time the benchmark net's tower shapes against the device-side row count: the sweep the adaptive-shape threshold
(kAdaptT1, csrc/bz_net.hip) is read from.  Buffers of max_n = 2048 rows, a count on the device, every shape forced in turn
(DeviceNet.set_adaptive_shape: 2 = latency, 0 = throughput, 1 = the adaptive pair, which adds the empty launch), in two
configurations: `alone`, and `two_streams` = the same launch running on a second stream at the same time, which is what
the head of a move looks like with two pipelines.  us = wall time of `reps` back-to-back launches per stream / reps.
--rows / --max-n / --modes time other counts, buffers and shapes (e.g. the engine's 1300 and 4096 rows on the throughput
shape alone); --tile-map 0|1 picks the throughput shape's kernel (DeviceNet.set_tile_map: board-row tiles / edge-aware).
usage: python tools/bench_tower_shapes.py [out.jsonl] [--reps N] [--rows A,B,..] [--max-n N] [--modes latency,throughput,adaptive]
       [--tile-map 0|1]"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from betazero_amd.net import DeviceNet, PolicyValueNet  # noqa: E402

ROWS = (16, 32, 64, 128, 192, 256, 384, 512, 768, 1024, 1536, 2048)
MAX_N = 2048
MODES = (("latency", 2), ("throughput", 0), ("adaptive", 1))


def main():
    args = sys.argv[1:]
    opt = lambda k, d: args[args.index(k) + 1] if k in args else d  # noqa: E731
    reps = int(opt("--reps", 200))
    ROWS = tuple(int(v) for v in opt("--rows", ",".join(map(str, globals()["ROWS"]))).split(","))
    MAX_N = int(opt("--max-n", max(globals()["MAX_N"], max(ROWS))))
    MODES = tuple(m for m in globals()["MODES"] if m[0] in opt("--modes", "latency,throughput,adaptive").split(","))
    tile_map = opt("--tile-map", None)
    out = open(args[0], "w") if args and not args[0].startswith("--") else None
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    net = DeviceNet.from_module(PolicyValueNet(128, 6, 64).round_to_bf16_(), MAX_N, dev)
    if tile_map is not None:
        net.set_tile_map(int(tile_map))
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "reversi_random_games.npz"))["rows"]
    d = d[d[:, 1] == 8]
    idx = np.arange(MAX_N) % len(d)
    own = torch.from_numpy(d[idx, 2].astype(np.uint64).view(np.int64)).to(dev)
    opp = torch.from_numpy(d[idx, 3].astype(np.uint64).view(np.int64)).to(dev)
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    bufs = [(own.clone(), opp.clone(), torch.zeros(1, dtype=torch.int32, device=dev),
             torch.empty((MAX_N, 65), dtype=torch.float32, device=dev), torch.empty(MAX_N, dtype=torch.float32, device=dev))
            for _ in streams]

    def run(n_streams, k):
        for st, (o, p, c, lg, v) in list(zip(streams, bufs))[:n_streams]:
            with torch.cuda.stream(st):
                for _ in range(k):
                    net.forward_counted(o, p, c, lg, v)

    for rows in ROWS:
        for b in bufs:
            b[2].fill_(rows)
        for name, mode in MODES:
            net.set_adaptive_shape(mode)
            rec = {"shape": name, "rows": rows, "max_n": MAX_N, "reps": reps}
            if tile_map is not None:
                rec["tile_map"] = int(tile_map)
            for cfg, ns in (("alone", 1), ("two_streams", 2)):
                run(ns, 10)
                torch.cuda.synchronize(dev)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                cur = torch.cuda.current_stream(dev)
                e0.record(cur)
                for st in streams[:ns]:
                    st.wait_stream(cur)
                run(ns, reps)
                for st in streams[:ns]:
                    cur.wait_stream(st)
                e1.record(cur)
                torch.cuda.synchronize(dev)
                rec[cfg + "_us"] = round(e0.elapsed_time(e1) * 1e3 / reps, 2)
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
    net.set_adaptive_shape(1)
    net.shape_tally()


if __name__ == "__main__":
    main()
