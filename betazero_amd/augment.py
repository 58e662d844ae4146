"""8-fold symmetry augmentation + dedupe of (s, pi, z) examples on the GPU.
Reference: TicTacToeDataset.expand_with_transforms, src/tic_tac_toe/SL/train.py:24-52
(the 8 transforms in its order, then keep the first occurrence of every distinct
(state, action) pair in insertion order).

Device in, device out: DeviceExamples (what gather_examples_device / SelfPlayEngine.device_examples hand over)
stay on the GPU through the transforms, the dedupe and into train_step; host Examples are accepted too and come
back as host Examples."""
import torch

from . import _lib
from .examples import DeviceExamples, Examples, columns


def _first_by_key(key8, own8, opp8, pi8):
    """indices (ascending = insertion order) of the first of every set of exactly equal (own, opp, pi) rows AMONG THE
    ROWS THAT SHARE A KEY.  Rows are grouped by key (stable sort: insertion order inside a group) and every row is
    compared with the HEAD of its group on the full content: the head is kept, rows equal to it are duplicates and
    dropped, rows that differ (another content sharing the key) go into the next pass among themselves -- a collision
    can neither drop a distinct row nor keep a duplicate.  With honest keys that is one pass plus one emptiness check.
    pi8 holds the BIT PATTERNS (int32: a row holding a NaN equals itself -- with float comparison a group head
    containing a NaN differed from itself and was handed to the next pass for ever), and a pass never hands its own
    heads on, so every pass removes at least one row: the loop ends."""
    kept = []
    cur = torch.arange(key8.numel(), device=key8.device)
    while cur.numel():
        sk, o = torch.sort(key8[cur], stable=True)
        order = cur[o]
        newrun = torch.ones_like(sk, dtype=torch.bool)
        newrun[1:] = sk[1:] != sk[:-1]
        heads = newrun.nonzero(as_tuple=True)[0]                 # sorted positions of the group heads
        head_row = order[heads[torch.cumsum(newrun, 0) - 1]]     # for every sorted position: the row id of its group's head
        same = (own8[order] == own8[head_row]) & (opp8[order] == opp8[head_row]) & (pi8[order] == pi8[head_row]).all(1)
        kept.append(order[newrun])
        cur = torch.sort(order[~same & ~newrun]).values          # ascending again: the stable sort keeps insertion order
    return torch.sort(torch.cat(kept)).values if kept else cur


def _first_occurrences(key8, own8, opp8, pi8):
    """indices (ascending = insertion order) of the rows to keep: the first of every set of EXACTLY equal
    (own, opp, pi) rows -- SL/train.py:45-50 keeps the first of every exactly-equal pair -- whatever the keys do.
    _first_by_key under the kernel's 64-bit content key does the work; it is exact when equal rows carry equal keys
    (the kernel's key is a function of the content).  Keys that are NOT a function of the content would leave a copy
    standing in every key group it occurs in, so the survivors go through _first_by_key once more under a key computed
    here from the content alone (boards and the sum of pi's bit patterns: weak, and exact all the same).  After honest
    keys the second round finds nothing: one more sort over the kept rows."""
    pi8 = pi8.view(torch.int32)
    keep = _first_by_key(key8, own8, opp8, pi8)
    own, opp, pi = own8[keep], opp8[keep], pi8[keep]
    content = own * -0x61C8864680B583EB + opp * -0x3D4D51C2D82B14B1 + pi.sum(1, dtype=torch.int64)  # (int64 wraps)
    return keep[_first_by_key(content, own, opp, pi)]


def augment_examples(ex, dedupe=True, device="cuda:0"):
    """Examples / DeviceExamples (n rows) -> the same type (<= 8n rows, row 8*i+t = transform t of row i before dedupe).
    z, mover, game and ply and -- when present -- kl, q, vt and count are the source row's: the eight copies share them, and the
    dedupe keeps the first occurrence's; `act` is permuted with the board.
    `fown` / `fopp` (the ownership target) are boards: they go through the same kernel, so every copy's target is
    transformed by the symmetry of its position; the dedupe key does not see them and keeps the first occurrence's."""
    _lib.require_gpu()
    host_in = isinstance(ex, Examples)
    if host_in:
        ex = DeviceExamples.from_host(ex, device)
    dev = ex.own.device
    n, na, size = len(ex), ex.pi.shape[1], ex.size
    own, opp, pi = ex.own.contiguous(), ex.opp.contiguous(), ex.pi.contiguous()
    own8 = torch.empty(8 * n, dtype=torch.int64, device=dev)
    opp8 = torch.empty(8 * n, dtype=torch.int64, device=dev)
    pi8 = torch.empty((8 * n, na), dtype=torch.float32, device=dev)
    key8 = torch.empty(8 * n, dtype=torch.int64, device=dev)
    # the move played, as a one-hot "policy", goes through the same kernel to permute `act`
    act1 = torch.zeros((n, na), dtype=torch.float32, device=dev)
    act1[torch.arange(n, device=dev), ex.act.to(torch.int64)] = 1.0
    act8 = torch.empty((8 * n, na), dtype=torch.float32, device=dev)
    scr_a = torch.empty(8 * n, dtype=torch.int64, device=dev)  # two distinct buffers: the kernel's outputs
    scr_b = torch.empty(8 * n, dtype=torch.int64, device=dev)  # are __restrict__
    has_own = ex.fown is not None and ex.fopp is not None
    if (ex.fown is None) != (ex.fopp is None):
        raise ValueError("augment_examples: the examples must carry both fown and fopp (ownership target), or neither")
    with torch.cuda.device(dev):
        st = torch.cuda.current_stream().cuda_stream
        L = _lib.lib()
        if has_own:  # (its policy output lands in pi8, which the next call overwrites: the stream orders them)
            fown, fopp = ex.fown.contiguous(), ex.fopp.contiguous()
            fown8 = torch.empty(8 * n, dtype=torch.int64, device=dev)
            fopp8 = torch.empty(8 * n, dtype=torch.int64, device=dev)
            _lib.check(L.bz_augment_d4_batch(fown.data_ptr(), fopp.data_ptr(), pi.data_ptr(), n, size, na, fown8.data_ptr(),
                                             fopp8.data_ptr(), pi8.data_ptr(), None, st))
        _lib.check(L.bz_augment_d4_batch(own.data_ptr(), opp.data_ptr(), pi.data_ptr(), n, size, na, own8.data_ptr(),
                                         opp8.data_ptr(), pi8.data_ptr(), key8.data_ptr(), st))
        _lib.check(L.bz_augment_d4_batch(own.data_ptr(), opp.data_ptr(), act1.data_ptr(), n, size, na,
                                         scr_a.data_ptr(), scr_b.data_ptr(), act8.data_ptr(), None, st))
    keep = _first_occurrences(key8, own8, opp8, pi8) if dedupe else torch.arange(8 * n, device=dev)
    # the columns that went through the kernel; every other column the rows carry is the source row's
    moved = dict(own=own8[keep], opp=opp8[keep], pi=pi8[keep], act=act8[keep].argmax(1).to(torch.uint8))
    if has_own:
        moved.update(fown=fown8[keep], fopp=fopp8[keep])
    src = keep // 8
    out = DeviceExamples(size=size, **{k: moved[k] if k in moved else t[src] for k, t in columns(ex).items()})
    return out.cpu() if host_in else out
