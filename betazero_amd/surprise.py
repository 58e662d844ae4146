"""Policy surprise weighting, the training side (KataGo, Wu 2019, section 3.3): rows whose search policy
disagrees with the net's prior are trained on more often, in proportion to KL(pi || P).  The rows are not reweighted in the
loss; they are repeated in the data: surprise_resample() turns the rows' kl into an index list in which row i stands count_i
times, and the training step gathers by index as it always has (bz_train_batch.idx)."""
import torch

from . import _lib

MAX_ROWS = 1 << 26  # bz_surprise_resample's limit (include/bz_abi.h)


def _check(ex, uniform_frac):
    if getattr(ex, "kl", None) is None:
        raise ValueError("surprise_resample: the examples carry no kl (self-play with surprise=True records it)")
    u = uniform_frac
    if isinstance(u, bool) or not isinstance(u, (int, float)) or not 0.0 <= u <= 1.0:  # (NaN fails)
        raise ValueError(f"surprise_resample: uniform_frac must be a number in [0, 1] (got {uniform_frac!r})")
    if len(ex) > MAX_ROWS:
        raise ValueError(f"surprise_resample: at most 2^26 rows (got {len(ex)})")
    return float(u)


def surprise_resample(ex, uniform_frac=0.5, seed=0, capacity=None, return_counts=False):
    """DeviceExamples with kl -> a device int64 index tensor holding row i count_i times, ascending, with
    w_i = uniform_frac + (1 - uniform_frac) kl_i / mean(kl) and count_i = floor(w_i) + [a 24-bit draw < frac(w_i) 2^24]: about
    len(ex) entries in all.  The draw is keyed by (seed, game, ply, own, opp) -- the row's content, not its position -- so the
    result does not depend on where a row stands in the window and the D4 copies of a row draw independently.  Bit for bit the
    same on every run.  capacity: entries the result may hold (default 2 n + 1024); more raises RuntimeError at the one place
    the function waits for the device, to size its result.  return_counts: also the int32 [n] counts."""
    u = _check(ex, uniform_frac)
    n = len(ex)
    dev = ex.kl.device
    if dev.type != "cuda":
        raise ValueError("surprise_resample: the examples must live on the GPU (DeviceExamples)")
    cap = int(2 * n + 1024 if capacity is None else capacity)
    if cap < 0:
        raise ValueError(f"surprise_resample: capacity must be >= 0 (got {capacity!r})")
    L = _lib.lib()
    wbytes = L.bz_surprise_resample_workspace_bytes(n)
    if wbytes < 0:
        raise RuntimeError(_lib.last_error())
    ws = torch.empty(wbytes + 256, dtype=torch.uint8, device=dev)
    pad = (-ws.data_ptr()) & 255
    ws = ws[pad:pad + wbytes]
    count = torch.empty(n, dtype=torch.int32, device=dev)
    idx = torch.empty(cap, dtype=torch.int64, device=dev)
    n_out = torch.empty(1, dtype=torch.int64, device=dev)
    kl = ex.kl.to(torch.float32).contiguous()
    game, ply = ex.game.to(torch.int64).contiguous(), ex.ply.to(torch.int32).contiguous()
    own, opp = ex.own.contiguous(), ex.opp.contiguous()
    with torch.cuda.device(dev):
        _lib.check(L.bz_surprise_resample(kl.data_ptr(), game.data_ptr(), ply.data_ptr(), own.data_ptr(), opp.data_ptr(), n, u,
                                          int(seed) & (2**64 - 1), ws.data_ptr(), wbytes, count.data_ptr(), idx.data_ptr(), cap,
                                          n_out.data_ptr(), torch.cuda.current_stream().cuda_stream))
    head = ws[:24].view(torch.int64).cpu()  # (integer kl sum, sum of the counts, dropped entries): the one wait
    if int(head[2]):
        raise RuntimeError(f"surprise_resample: {int(head[2])} of {int(head[1])} entries did not fit into capacity = {cap}")
    res = idx[:int(head[1])]
    return (res, count) if return_counts else res
