"""The yard-stick of the tic-tac-toe self-play loop (tools/ttt_az.py): a net with a value head against full-depth
minimax (bz_ttt_minimax, the host build of the arena kernel's code) on a set of positions -- the mean squared error of its value
and the share of positions whose best legal logit is a minimax-optimal move."""
import ctypes as C

import numpy as np

from . import _lib


def minimax_targets(own, opp):
    """own / opp: side-to-move bitboards (cell i = bit i) of non-terminal positions [n] -> (value [n] float32 in {-1, 0, +1}
    for the side to move, optimal [n, 9] bool: the legal moves that keep that value)"""
    L = _lib.lib()
    memo = {}

    def score(a, b):  # the value of (a to move, b) for a
        if (a, b) not in memo:
            mv, sc = C.c_int32(), C.c_int32()
            _lib.check(L.bz_ttt_minimax(a, b, 1, C.byref(mv), C.byref(sc)))
            memo[(a, b)] = sc.value
        return memo[(a, b)]
    own = np.asarray(own, dtype=np.uint64).astype(np.int64)
    opp = np.asarray(opp, dtype=np.uint64).astype(np.int64)
    value = np.zeros(own.size, np.float32)
    optimal = np.zeros((own.size, 9), bool)
    for i, (a, b) in enumerate(zip(own.tolist(), opp.tolist())):
        moves = [c for c in range(9) if not (a | b) >> c & 1]
        if not moves:
            raise ValueError("minimax_targets: a full board has no move")
        child = np.array([-score(b, a | 1 << c) for c in moves])   # after the move the opponent is to move
        value[i] = child.max()
        optimal[i, np.array(moves)[child == child.max()]] = True
    return value, optimal


def yardstick(net, own, opp, targets=None, bf16=False):
    """net: a DeviceMLP with a value head.  -> {"value_mse", "optimal_top1", "positions"} over the positions (own, opp);
    targets: minimax_targets(own, opp), when the caller has them already"""
    value, optimal = targets if targets is not None else minimax_targets(own, opp)
    own = np.asarray(own, dtype=np.uint64)
    opp = np.asarray(opp, dtype=np.uint64)
    lg, v = [], []
    for i in range(0, own.size, net.max_batch):
        a, b = net.forward(own[i:i + net.max_batch], opp[i:i + net.max_batch], bf16=bf16, value=True)
        lg.append(a.cpu().numpy()); v.append(b.cpu().numpy())
    lg, v = np.concatenate(lg), np.concatenate(v)
    cells = np.arange(9, dtype=np.uint64)
    legal = (((own | opp)[:, None] >> cells) & np.uint64(1)) == 0
    best = np.where(legal, lg, -np.inf).argmax(1)
    return {"value_mse": float(np.mean((v.astype(np.float64) - value) ** 2)),
            "optimal_top1": float(optimal[np.arange(own.size), best].mean()), "positions": int(own.size)}
