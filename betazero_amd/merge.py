"""Position averaging (AlphaZero.jl's use_position_averaging): the rows of a training window that share a
position -- exactly equal (own, opp), the side-to-move canonical boards -- become one row carrying the mean pi, the mean value
target and a count.  The rule is integer arithmetic on fixed-point values (csrc/bz_merge.h), so the result does not depend on
the order of the rows or on how the device splits the sums:

    fix_k(x) = (int64)(x * 2^k)                       k = 32 for pi, the value input and q; 24 for kl
    M = floor((2 S + n) / (2 n))                      S = the group's sum of fix_k, n = its rows: round half up
    mean = (float)((double)M * 2^-k)

A row's value input is vt when the examples carry it, otherwise (float)z.  A group of one row comes back bit for bit (with vt =
its value input), so a window without a repeated position is unchanged.  Merged rows are meant for
GraphedTrainStep(value_targets=True): vt is always set, and z = the sign of the value sum only keeps the int8 column meaningful.
Grouping is torch plumbing (two stable sorts, a neighbour compare); the sums and the means are bz_merge_positions' kernels."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .examples import COLUMN, DeviceExamples, Examples, columns

MAX_ROWS = 1 << 26  # bz_merge_positions' limit (include/bz_abi.h): no sum leaves int64
POLICIES = ("constant", "log")


def _check(ex, return_counts):
    if not isinstance(ex, (Examples, DeviceExamples)):
        raise ValueError(f"merge_positions: Examples or DeviceExamples expected (got {type(ex).__name__})")
    if not isinstance(return_counts, bool):
        raise ValueError(f"merge_positions: return_counts must be a bool (got {return_counts!r})")
    if ex.fown is not None or ex.fopp is not None:
        raise ValueError("merge_positions: the rows carry ownership targets (fown / fopp): those are bitboards of the games' final "
                         "positions and have no mean -- position averaging does not combine with ownership")
    if len(ex) > MAX_ROWS:
        raise ValueError(f"merge_positions: at most 2^26 rows (got {len(ex)})")
    na = ex.pi.shape[1] if ex.pi.ndim == 2 else None
    if na not in (9, 65):
        raise ValueError(f"merge_positions: pi must be [n, 9] (tic-tac-toe) or [n, 65] (Reversi), got {tuple(ex.pi.shape)}")
    return na


def _grouping(own, opp):
    """the index lists bz_merge_positions takes (include/bz_abi.h), without a wait: nothing here reads a size back"""
    n, dev = own.numel(), own.device
    by_opp = torch.sort(opp, stable=True).indices
    order = by_opp[torch.sort(own[by_opp], stable=True).indices]  # equal (own, opp) adjacent, in input order inside a run
    so, sp = own[order], opp[order]
    newrun = torch.ones(n, dtype=torch.bool, device=dev)
    newrun[1:] = (so[1:] != so[:-1]) | (sp[1:] != sp[:-1])
    pos = torch.arange(n, dtype=torch.int64, device=dev)
    start = torch.cummax(torch.where(newrun, pos, torch.zeros_like(pos)), 0).values  # the sorted position of the run's head
    first = torch.zeros(n, dtype=torch.bool, device=dev).scatter_(0, order, newrun)  # per input row: a first occurrence?
    rank = torch.cumsum(first, 0) - 1                                                # ... and the output row it opens
    n_groups = (rank[-1:] + 1).contiguous()
    dst = rank[order[start]]
    count = torch.zeros(n, dtype=torch.int32, device=dev).scatter_add_(0, dst, torch.ones(n, dtype=torch.int32, device=dev))
    head = torch.empty(n + 1, dtype=torch.int64, device=dev).scatter_(0, torch.where(first, rank, torch.full_like(rank, n)), pos)
    return order.contiguous(), start.to(torch.int32), dst.to(torch.int32), head, count, n_groups


_MERGED = tuple(name for name, _ in _lib.MergeRows._fields_)  # the columns bz_merge_positions reads and writes, in the struct's order


def _rows(cols):
    return _lib.MergeRows(*(cols[k].data_ptr() if k in cols else None for k in _MERGED))


def merge_positions(ex, return_counts=False):
    """Examples / DeviceExamples (n rows) -> the same type: one row per distinct (own, opp), in the order of the positions' first
    occurrence, with pi, the value target (`vt`, always set) and -- when present -- q and kl averaged by the rule above, z = the
    sign of the value sum and mover, act, game, ply of the first occurrence.  return_counts: also the int32 rows per merged row
    (a device tensor; numpy for host Examples).  Bit for bit the same on every run and for every order of the rows.
    Raises ValueError -- before any device call -- for rows that carry ownership targets (bitboards have no mean), for more
    than 2^26 rows and for rows that are on no GPU; RuntimeError, at the one place the function waits for the device, when rows
    held a value that is not finite or outside its range (pi in [0, 1], vt and q in [-1, 1], kl in [0, 128]): such rows were
    left out of the sums."""
    na = _check(ex, return_counts)
    host_in = isinstance(ex, Examples)
    n = len(ex)
    if n == 0:  # nothing to launch
        if host_in:
            out, cnt = Examples(**{**vars(ex), "vt": np.zeros(0, np.float32)}), np.zeros(0, np.int32)
        else:
            out = DeviceExamples(**{**vars(ex), "vt": torch.zeros(0, dtype=torch.float32, device=ex.own.device)})
            cnt = torch.zeros(0, dtype=torch.int32, device=ex.own.device)
        return (out, cnt) if return_counts else out
    if host_in:
        _lib.require_gpu()
        ex = DeviceExamples.from_host(ex)
    dev = ex.own.device
    if dev.type != "cuda":
        raise ValueError("merge_positions: the examples must live on the GPU (DeviceExamples)")
    cin = {k: t.to(COLUMN[k].device).contiguous() for k, t in columns(ex).items() if k in _MERGED}
    o = {k: torch.empty_like(t) for k, t in cin.items()}
    o.setdefault("vt", torch.empty(n, dtype=torch.float32, device=dev))  # always set: a row's value input is vt or (float)z
    L = _lib.lib()
    wbytes = L.bz_merge_workspace_bytes(n, na)
    if wbytes < 0:
        raise RuntimeError(_lib.last_error())
    ws = torch.empty(wbytes + 256, dtype=torch.uint8, device=dev)
    ws = ws[(-ws.data_ptr()) & 255:][:wbytes]
    status = torch.empty(1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        order, start, dst, head, count, n_groups = _grouping(cin["own"], cin["opp"])
        rin, rout = _rows(cin), _rows(o)
        _lib.check(L.bz_merge_positions(C.byref(rin), n, na, order.data_ptr(), start.data_ptr(), dst.data_ptr(), head.data_ptr(),
                                        count.data_ptr(), n_groups.data_ptr(), ws.data_ptr(), wbytes, C.byref(rout),
                                        status.data_ptr(), torch.cuda.current_stream().cuda_stream))
        bad, groups = (int(x) for x in torch.cat([status, n_groups]).cpu())  # the one wait
    if bad:
        raise RuntimeError(f"merge_positions: {bad} row(s) held a value that is not finite or outside its range (pi in [0, 1], vt and "
                           "q in [-1, 1], kl in [0, 128]); they were left out of the sums")
    cut = lambda t: None if t is None else (t[:groups].clone() if groups < n else t)  # noqa: E731  (lets the n-row buffers go)
    out = DeviceExamples(size=ex.size, **{k: cut(v) for k, v in o.items()})
    cnt = cut(count)
    if host_in:
        out, cnt = out.cpu(), cnt.cpu().numpy()
    return (out, cnt) if return_counts else out


def merged_repeats(count, policy="constant"):
    """The merged rows' counts -> an int64 index list (on the counts' device) to sample training rows through: a merged row
    stands once ("constant") or 1 + floor(log2 n) times ("log") -- AlphaZero.jl's two weightings that keep the merge.  A
    weighting linear in n is not offered: it undoes the merge.  Integer arithmetic only."""
    if policy not in POLICIES:
        raise ValueError(f"merged_repeats: policy must be one of {POLICIES} (got {policy!r}); a linear weighting would undo the merge")
    if isinstance(count, np.ndarray):
        count = torch.as_tensor(count)
    if not torch.is_tensor(count) or count.dim() != 1 or count.dtype not in (torch.int32, torch.int64):
        raise ValueError("merged_repeats: count must be the one-dimensional int32 / int64 tensor merge_positions returns")
    rows = torch.arange(count.numel(), dtype=torch.int64, device=count.device)
    if policy == "constant":
        return rows
    powers = 2 ** torch.arange(1, 32, dtype=torch.int64, device=count.device)
    ilog2 = (count.to(torch.int64)[:, None] >= powers).sum(1)  # floor(log2 n) for n >= 1; 0 for anything below
    return torch.repeat_interleave(rows, 1 + ilog2)
