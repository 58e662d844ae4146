"""Search-value targets, the training side: from the root value q every recorded row carries (self-play with
search_value=True) and the games' outcomes z to a float value target per row,

    G_t  = (1 - lam) * q_{t+1} + lam * G_{t+1},  G_{T-1} = z            (TD(lambda), Sutton 1988; in one frame of reference)
    vt_t = (1 - q_mix) * G_t + q_mix * q_t

computed by bz_value_targets on the device, one game's rows at a time in ply order.  lam = 1, q_mix = 0 is the plain outcome
(vt == z); q_mix = 0.5 at lam = 1 is the average of z and the root value.  The training step reads vt through
GraphedTrainStep(value_targets=True)."""
import dataclasses

import torch

from . import _lib

MAX_ROWS = 1 << 26  # bz_value_targets' limit (include/bz_abi.h)


def _unit(name, x):
    if isinstance(x, bool) or not isinstance(x, (int, float)) or not 0.0 <= x <= 1.0:  # (NaN fails)
        raise ValueError(f"value_targets: {name} must be a number in [0, 1] (got {x!r})")
    return float(x)


def value_targets(ex, lam=1.0, q_mix=0.0):
    """DeviceExamples with q -> the same rows with `vt` set (fp32 [n], in [-1, 1], for the mover like z).  Call it on an
    iteration's packed rows BEFORE the hold-out split and the augmentation, while every game's rows stand together in ply
    order: a game is told from its neighbours by the game id changing or the ply not rising.  Bit for bit the same on every run.
    Raises ValueError when the examples carry no q, a parameter is not a number in [0, 1] or the rows are not on the GPU, and
    RuntimeError -- at the one place the function waits for the device -- when a game had more than 1024 rows (such games keep
    vt = z; the engine's have at most 256)."""
    if getattr(ex, "q", None) is None:
        raise ValueError("value_targets: the examples carry no q (self-play with search_value=True records it)")
    lam, q_mix = _unit("lam", lam), _unit("q_mix", q_mix)
    n = len(ex)
    if n > MAX_ROWS:
        raise ValueError(f"value_targets: at most 2^26 rows (got {n})")
    if not torch.is_tensor(ex.q) or ex.q.device.type != "cuda":
        raise ValueError("value_targets: the examples must live on the GPU (DeviceExamples)")
    dev = ex.q.device
    q = ex.q.to(torch.float32).contiguous()
    z, mover = ex.z.to(torch.int8).contiguous(), ex.mover.to(torch.int8).contiguous()
    game, ply = ex.game.to(torch.int64).contiguous(), ex.ply.to(torch.int32).contiguous()
    vt = torch.empty(n, dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().bz_value_targets(q.data_ptr(), z.data_ptr(), mover.data_ptr(), game.data_ptr(), ply.data_ptr(), n, lam,
                                               q_mix, vt.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream))
    long_segments = int(status.item())  # the one wait
    if long_segments:
        raise RuntimeError(f"value_targets: {long_segments} game(s) had more than 1024 rows in a row; their rows kept vt = z "
                           "(are the rows still in the packed block's order?)")
    return dataclasses.replace(ex, vt=vt)
