#!/usr/bin/env python3
"""Tower and tree-step duration by simulation index within a move, from a rocprofv3 --kernel-trace result database
(rocpd SQLite) of a self-play bench run.  Per stream (queue), a k_root_begin dispatch starts a move; the n-th tower
dispatch after it is the root evaluation (n = 0) or simulation n - 1, and so is the n-th k_tree_step (k_pace_step).  The head of a
move is where the evaluation cache serves nearly every leaf, so the tower launches there carry few rows.
An empty (self-gated) tower launch is listed apart from the one that did the work: of the launches of one evaluation the
longest is the worker.
usage: python tools/tower_trace.py <results.db> [out.txt]"""
import sqlite3
import sys

import numpy as np

db = sys.argv[1]
out = open(sys.argv[2], "w") if len(sys.argv) > 2 else sys.stdout
c = sqlite3.connect(db)
cols = [r[1] for r in c.execute("pragma table_info(kernels)").fetchall()]
key = next((k for k in ("stream_id", "queue_id", "queue", "stream", "tid") if k in cols), None)
rows = c.execute(f"select name, start, duration, {key or '0'} from kernels order by start").fetchall()
print(f"# {len(rows)} dispatches; pipelines told apart by column {key!r}", file=out)

TOWER = ("k_tower_bf16", "k_edge_bf16", "k_sym_bf16", "k_tower_fp8", "k_sym_fp8")
state = {}  # stream -> [tower evaluations seen this move, tree steps seen this move, evaluation open?]
tower, gate, tree, names = [], [], [], {}
for name, start, dur, q in rows:
    st = state.setdefault(q, [0, 0, None])
    if "k_root_begin" in name:
        st[0] = st[1] = 0
        st[2] = None
    elif any(t in name for t in TOWER):
        names[name] = names.get(name, 0) + 1
        if st[2] is None:
            st[2] = [st[0], dur]          # first launch of this evaluation
            st[0] += 1
        else:                             # a second launch of the same evaluation: the shorter one only looked at the count
            gate.append((st[2][0], min(st[2][1], dur)))
            st[2][1] = max(st[2][1], dur)
    elif "k_tree_step" in name or "k_pace_step" in name:  # (the paced step of a replay-seeded search)
        if st[2] is not None:
            tower.append(tuple(st[2]))
            st[2] = None
        tree.append((st[1], dur))
        st[1] += 1
for n, k in sorted(names.items(), key=lambda kv: -kv[1]):
    print(f"# {k:7d} x {n[:110]}", file=out)


def table(title, seq):
    if not seq:
        return
    a = np.array(seq, dtype=np.int64)
    print(f"{title}: {len(a)} dispatches, mean {a[:, 1].mean() / 1e3:.1f} us, total {a[:, 1].sum() / 1e6:.1f} ms", file=out)
    print("  index within the move: mean / min / median / max (us), n", file=out)
    edges = [0, 1, 2, 8, 16, 32, 48, 64, 80, 96, 112, 128, 160, 192, 256, 320, 384, 512, 640, 10**9]
    for lo, hi in zip(edges[:-1], edges[1:]):
        m = (a[:, 0] >= lo) & (a[:, 0] < hi)
        if m.any():
            d = a[m, 1] / 1e3
            print(f"  [{lo:4d}, {min(hi, int(a[:, 0].max()) + 1):4d}): {d.mean():8.1f} {d.min():8.1f} {np.median(d):8.1f} {d.max():8.1f}   n={m.sum()}",
                  file=out)


table("tower (index 0 = the root evaluation, n = simulation n - 1)", tower)
table("empty tower launch of a gated pair", gate)
table("k_tree_step / k_pace_step", tree)
