"""Reanalysis (MuZero Reanalyse, Schrittwieser et al. 2021): stored example rows are searched again with the
current net and their policy target -- and, where the rows carry them, the policy surprise and the search value -- are
overwritten in place, on the device: k_reanalyse_load takes a chunk of rows in as fresh roots, bz_engines_search searches
the chunks of the pipelines side by side, k_reanalyse_store puts the targets back."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .engine import SelfPlayEngine, pipeline_streams
from .examples import _GAMES, _SIZES, COLUMN, DeviceExamples, Examples, columns

_GAME_OF_SIZE = {3: "ttt", 8: "reversi", 6: "reversi6", 4: "reversi4"}


def reanalyse_rows(n, frac, seed, key):
    """the rows of an n-row window slot one reanalysis refreshes: round(frac n) distinct indices in 0 .. n - 1, sorted, as an
    int64 CPU tensor.  Drawn from a CPU torch.Generator seeded from (seed, key) -- key an int or a tuple of ints, e.g.
    (iteration, slot age) -- so the draw is a function of its arguments alone, whatever the device.  frac outside [0, 1]
    (or not a number) is refused."""
    if not (isinstance(frac, (int, float, np.integer, np.floating)) and not isinstance(frac, (bool, np.bool_)) and 0.0 <= frac <= 1.0):
        raise ValueError(f"reanalyse_rows: frac must be in [0, 1] (got {frac!r})")
    n = int(n)
    if n < 0:
        raise ValueError(f"reanalyse_rows: n must be >= 0 (got {n})")
    k = min(n, int(round(float(frac) * n)))
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    for v in (key if isinstance(key, (tuple, list)) else (key,)):  # splitmix64 over the words: every word moves every bit
        s = (s + 0x9E3779B97F4A7C15 + (int(v) & 0xFFFFFFFFFFFFFFFF)) & 0xFFFFFFFFFFFFFFFF
        s = ((s ^ (s >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        s = ((s ^ (s >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        s ^= s >> 31
    g = torch.Generator(device="cpu").manual_seed(s & 0x7FFFFFFFFFFFFFFF)
    return torch.sort(torch.randperm(n, generator=g, dtype=torch.int64)[:k]).values


def check_reanalyse(ex, rows, update_q, size):
    """what Reanalyser.run refuses (ValueError), on host Examples or DeviceExamples alike, before anything is written and
    before any engine exists: rows of another game, merged rows, value targets that would go stale, a `rows` that is not an
    int64 tensor where the examples live, an index outside 0 .. n - 1 (one min / max read)"""
    if ex.size != size:
        raise ValueError(f"reanalyse: the examples are of board size {ex.size}, the search is of size {size}")
    if ex.count is not None:
        raise ValueError("reanalyse: the examples carry count (merged positions, DESIGN.md 3.26): a merged row has no single search")
    if ex.vt is not None and update_q:
        raise ValueError("reanalyse: the examples carry vt (value targets) and update_q is set: vt would go stale against the "
                         "new q -- pass update_q=False, or compute the value targets afterwards")
    n = len(ex)
    if rows is None:
        return n
    where = ex.own.device if torch.is_tensor(ex.own) else torch.device("cpu")
    if not torch.is_tensor(rows) or rows.dtype != torch.int64 or rows.dim() != 1:
        raise ValueError("reanalyse: rows must be a one-dimensional int64 tensor (or None = every row)")
    if rows.device != where:
        raise ValueError(f"reanalyse: rows live on {rows.device}, the examples on {where}")
    if rows.numel():
        lo, hi = (int(v) for v in torch.stack([rows.min(), rows.max()]).cpu())
        if lo < 0 or hi >= n:
            raise ValueError(f"reanalyse: row index {lo if lo < 0 else hi} outside 0 .. {n - 1}")
    return int(rows.numel())


class Reanalyser:
    """`pipelines` search engines of `batch` slots each, on streams of their own, sharing one net; built once and used again
    every iteration (weights pushed into the shared net between two runs are seen by the next run).

    The engines search with temp_moves = 0, openings = 0 and no Dirichlet noise, and take no playout cap, resignation,
    ownership, early stop, subtree reuse or root store; the search options that shape a search or its pi -- gumbel, fpu,
    forced_playouts, solver, eval_symmetry, leaves_per_step -- are SelfPlayEngine's, through its constructor, so the table of
    refused pairs (SEARCH_OPTION_CONFLICTS) applies as it is.  A reanalysed row is therefore a pure function of (position,
    weights, sims, search options, evaluation-symmetry seed): it does not depend on the slot that searched it, on batch and
    pipelines (the chunking), on the order of `rows`, or on what else `rows` names."""

    def __init__(self, game, sims, evaluator="uniform", net=None, batch=1024, pipelines=2, c_puct=1.5, gumbel=None, fpu=None,
                 forced_playouts=None, solver=False, eval_symmetry=None, leaves_per_step=1, seed=0, device="cuda:0", run_ahead=16):
        if game not in _GAMES:
            raise ValueError(f"Reanalyser: unknown game {game!r}")
        if not (isinstance(batch, (int, np.integer)) and batch >= 1 and isinstance(pipelines, (int, np.integer)) and 1 <= pipelines <= 16):
            raise ValueError(f"Reanalyser: batch must be >= 1 and pipelines in 1 .. 16 (got {batch!r}, {pipelines!r})")
        self.size = _SIZES[_GAMES[game]]
        self.device = torch.device(device)
        self.batch, self.pipelines, self.run_ahead = int(batch), int(pipelines), int(run_ahead)
        # the evaluation cache within a search only: consecutive chunks hold unrelated positions, nothing is worth carrying
        self.engines = [SelfPlayEngine(game, self.batch, sims, evaluator, net, c_puct, temp_moves=0, openings=0, seed=seed,
                                       device=device, eval_cache="search", root_store=False, replay_seed=False,
                                       leaves_per_step=leaves_per_step, gumbel=gumbel, forced_playouts=forced_playouts, fpu=fpu,
                                       solver=solver, eval_symmetry=eval_symmetry)
                        for _ in range(self.pipelines)]
        self.streams = pipeline_streams(self.device, self.pipelines)
        for e, st in zip(self.engines, self.streams):
            e.track_stream(st)
        self.na = self.engines[0].na

    def run(self, ex, rows=None, update_q=True):
        """search the rows `rows` (int64 device tensor of indices into ex; None = every row; duplicates are harmless) of the
        DeviceExamples `ex` again and overwrite, in place: pi; kl where ex carries it; q where ex carries it and update_q is
        set.  Every other column and every row not named stays as it is.  A `rows` that is a strided view (idx[::2], an
        expanded scalar) is read as the indices it shows: the kernels get a contiguous copy.  Chunk i of `batch` rows runs on engine i mod
        pipelines: load, bz_engines_search, store; the host waits only where bz_engines_search does and in one status() per
        engine at the end, which raises what any chunk raised (a terminal root among the rows: its row is left alone, the
        others are written).  ValueError, before anything is written: check_reanalyse's refusals.
        -> {"rows", "chunks", "counters": the engines' work counters, summed}"""
        if not isinstance(ex, DeviceExamples):
            raise ValueError("Reanalyser.run takes DeviceExamples (reanalyse() takes host Examples too)")
        total = check_reanalyse(ex, rows, update_q, self.size)
        n = len(ex)
        if ex.own.device != self.device:
            raise ValueError(f"reanalyse: the examples live on {ex.own.device}, the engines on {self.device}")
        q = ex.q if update_q else None
        touched = ("own", "opp", "mover", "pi", "kl") + (("q",) if update_q else ())  # what the kernels read or write, when carried
        for k, t in columns(ex).items():
            dt = COLUMN[k].device
            if k in touched and (t.dtype != dt or not t.is_contiguous() or t.shape[0] != n):
                raise ValueError(f"reanalyse: column {k} must be a contiguous {dt} tensor of {n} rows")
        if tuple(ex.pi.shape) != (n, self.na):
            raise ValueError(f"reanalyse: pi must be [{n}, {self.na}] (got {tuple(ex.pi.shape)})")
        if rows is not None:
            rows = rows.contiguous()   # the kernels read rows[first + g] at unit stride; (a copy lives until the status() below)
        B, P = self.batch, self.pipelines
        chunks = (total + B - 1) // B
        if chunks == 0:
            return {"rows": 0, "chunks": 0, "counters": {}}
        L = _lib.lib()
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        used = min(P, chunks)
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            for i in range(used):
                self.streams[i].wait_stream(cur)  # behind the caller's work: rows just written, weights just pushed
                _lib.check(L.bz_engine_reset_counters(self.engines[i].h, self.streams[i].cuda_stream))
            sts = (C.c_void_p * P)(*[st.cuda_stream for st in self.streams])
            for c0 in range(0, chunks, P):
                live = [(i, (c0 + i) * B, min(B, total - (c0 + i) * B)) for i in range(P) if c0 + i < chunks]
                for i, first, count in live:
                    _lib.check(L.bz_engine_reanalyse_load(self.engines[i].h, ptr(ex.own), ptr(ex.opp), ptr(ex.mover), n, ptr(rows), first,
                                                          count, int(c0 == 0), self.streams[i].cuda_stream))
                on = {i for i, _, _ in live}
                _lib.check(L.bz_engines_search((C.c_void_p * P)(*[self.engines[i].h if i in on else None for i in range(P)]), sts, P,
                                               self.run_ahead))
                for i, first, count in live:
                    _lib.check(L.bz_engine_reanalyse_store(self.engines[i].h, ptr(ex.pi), ptr(q), ptr(ex.kl), n, ptr(rows), first, count,
                                                           self.streams[i].cuda_stream))
            err, cnt = None, {}
            for i in range(used):
                with torch.cuda.stream(self.streams[i]):
                    try:
                        self.engines[i].status()  # (synchronises the engine's stream: ex and rows were kept alive until here)
                    except RuntimeError as x:
                        err = err or x
                    for k, v in self.engines[i].counters().items():
                        cnt[k] = cnt.get(k, 0) + v
                cur.wait_stream(self.streams[i])
        if err is not None:
            raise err
        return {"rows": total, "chunks": chunks, "counters": cnt}


def reanalyse(ex, rows=None, *, sims, game=None, update_q=True, device="cuda:0", **reanalyser_kwargs):
    """one-shot Reanalyser(game, sims, **reanalyser_kwargs).run(ex, rows, update_q).  game: by default the game of ex.size.
    DeviceExamples are updated in place and returned; host Examples (rows: an int64 CPU tensor or None) go through
    DeviceExamples.from_host and come back as new host Examples.  The refusals of run come before any engine is built."""
    if game is None:
        if ex.size not in _GAME_OF_SIZE:
            raise ValueError(f"reanalyse: no game of board size {ex.size}")
        game = _GAME_OF_SIZE[ex.size]
    if game not in _GAMES:
        raise ValueError(f"reanalyse: unknown game {game!r}")
    host = isinstance(ex, Examples)
    if not host and not isinstance(ex, DeviceExamples):
        raise ValueError("reanalyse takes Examples or DeviceExamples")
    check_reanalyse(ex, rows, update_q, _SIZES[_GAMES[game]])
    dev = torch.device(device) if host else ex.own.device
    r = Reanalyser(game, sims, device=str(dev), **reanalyser_kwargs)
    dex = DeviceExamples.from_host(ex, dev) if host else ex
    r.run(dex, None if rows is None else rows.to(dev), update_q)
    return dex.cpu() if host else dex
