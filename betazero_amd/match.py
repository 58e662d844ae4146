"""Batched head-to-head matches between two search players: B concurrent games, each side with its own
net, simulations and search mode, colours swapped inside every pair of games, on the GPU.

Reference anchors: the turn loop with its pass rule is ReversiTerminal.play (reversi_terminal.py:16-38) resp.
TicTacToeHeadless.play (tic_tac_toe.py:13-34) with a search player on both sides.  A match is two SelfPlayEngines over the
same B slots; everything between two searches -- move of the side to move, opening moves, rules, pass rule, winners, the
move log, the next roots of both engines -- is ONE kernel per ply (csrc/bz_match.hip) and the host reads 32 bytes per ply.
Neither side draws noise (temp_moves 0, no Dirichlet): a match is a pure function of (players, game, n_games,
opening_plies, seed)."""
import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _lib
from .engine import (check_early_stop, check_eval_cache, check_fpu, check_gumbel, check_leaves_per_step, check_sims,
                     check_solver)


@dataclass
class MatchPlayer:
    """One side of a match; the fields are MCTSPlayer's.  evaluator: "uniform" | "hash" | "net_f32" | "net_bf16" | "net_fp8"
    (a betazero_amd.net.DeviceNet as `net`, Reversi) | "mlp_f32" | "mlp_bf16" (a betazero_amd.mlp.DeviceMLP, tic-tac-toe);
    default: "net_bf16" / "mlp_f32" with a net, else "uniform".  leaves_per_step: DESIGN.md 3.12; gumbel (True or an
    engine.GumbelConfig): DESIGN.md 3.13, the side plays the Gumbel move without Gumbel noise; eval_cache: SelfPlayEngine's;
    eval_symmetry (True or a symmetry.EvalSymmetry): DESIGN.md 3.19, the side evaluates every leaf under a hashed board
    symmetry (True: seed 0) -- a match stays a pure function of its arguments.  fpu (True or an engine.Fpu): DESIGN.md 3.20,
    the side searches with first-play urgency reduction (not with gumbel or leaves_per_step > 1).  Each side has its own
    GumbelConfig.interior ("puct" or "gumbel").  solver=True: DESIGN.md 3.23, the side books proven wins, losses and
    draws and plays the solver's move (not with gumbel, fpu or leaves_per_step > 1).  early_stop (True or an engine.EarlyStop):
    DESIGN.md 3.25, the side's searches stop once the simulations left cannot change the move -- the games are the games without
    it (not with gumbel, solver or leaves_per_step > 1)."""
    sims: int = 800
    net: object = None
    evaluator: str = None
    c_puct: float = 1.5
    leaves_per_step: int = 1
    gumbel: object = None
    eval_cache: object = True
    eval_symmetry: object = None
    fpu: object = None
    solver: bool = False
    early_stop: object = None

    def checked(self, game, n_games, side):
        """-> (evaluator name, GumbelConfig or None); ValueError for anything a match cannot play, before any device is touched"""
        check_sims(self.sims)
        k = check_leaves_per_step(self.leaves_per_step)
        gumbel = check_gumbel(self.gumbel, leaves_per_step=k)
        check_eval_cache(self.eval_cache)
        fpu = check_fpu(self.fpu, leaves_per_step=k, gumbel=gumbel)
        solver = check_solver(self.solver, leaves_per_step=k, gumbel=gumbel, fpu=fpu)
        check_early_stop(self.early_stop, leaves_per_step=k, gumbel=gumbel, solver=solver)
        is_mlp = type(self.net).__name__ == "DeviceMLP"
        ev = self.evaluator or (("mlp_f32" if is_mlp else "net_bf16") if self.net is not None else "uniform")
        if not isinstance(ev, str) or ev not in ("uniform", "hash", "net_f32", "net_bf16", "net_fp8", "mlp_f32", "mlp_bf16"):
            raise ValueError(f"play_match: player {side}: evaluator must be 'uniform', 'hash', 'net_f32', 'net_bf16', 'net_fp8', "
                             f"'mlp_f32' or 'mlp_bf16' (got {self.evaluator!r})")
        if game == "ttt" and ev.startswith("net"):
            raise ValueError("the conv net evaluators serve the Reversi boards; use evaluator='uniform' or 'hash' for tic-tac-toe")
        if game != "ttt" and (is_mlp or ev.startswith("mlp")):
            raise ValueError("the MLP (DeviceMLP, evaluators 'mlp_f32' / 'mlp_bf16') serves tic-tac-toe, not Reversi")
        if ev.startswith(("net", "mlp")):
            if self.net is None:
                raise ValueError(f"play_match: player {side}: evaluator {ev!r} needs a net")
            if self.net.max_batch < k * n_games:
                raise ValueError(f"play_match: player {side}: the net's max_batch {self.net.max_batch} < n_games {n_games}" +
                                 (f" x leaves_per_step {k}" if k > 1 else "") + " (both engines hold all the match's slots)")
        from .symmetry import check_eval_symmetry
        check_eval_symmetry(self.eval_symmetry, 0, game, ev)
        return ev, gumbel


def elo_of_score(score):
    """-400 log10(1 / score - 1); -inf at score 0, +inf at score 1"""
    if score <= 0.0:
        return -math.inf
    if score >= 1.0:
        return math.inf
    return -400.0 * math.log10(1.0 / score - 1.0)


@dataclass
class MatchResult:
    winner: np.ndarray      # int8 [B] absolute winner per game: +1 / -1 / 0
    a_colour: np.ndarray    # int8 [B] the colour player A had: +1 in game 2k, -1 in game 2k + 1
    plies: np.ndarray       # int32 [B] moves played (a pass is no move)
    actions: np.ndarray     # uint8 [T][B] the move of every game at every ply, 255 = none (game over)
    movers: np.ndarray      # int8 [T][B] the colour that moved, 0 = none

    @property
    def score(self):
        """outcome for A per game: +1 win, 0 draw, -1 loss"""
        return (self.winner.astype(np.int32) * self.a_colour).astype(np.int8)

    @property
    def pair_score(self):
        """outcome for A per opening pair (games 2k, 2k + 1: the same opening, colours swapped), in -2 .. +2"""
        s = self.score.astype(np.int32)
        return s[0::2] + s[1::2]

    def summary(self):
        """games, wins / draws / losses for A (also split by A's colour), score = (W + D / 2) / n, elo = -400 log10(1 / score
        - 1) (+-inf at score 1 / 0), and elo_ci95: with paired openings the PAIR is the independent unit, so the interval is
        score +- 1.96 sqrt(var(m) / P) over the P pairs' mean points m_k = (pair_score_k + 2) / 4 (sample variance, P - 1),
        clipped to [0, 1] and mapped through the same logistic; one pair has no variance: (-inf, +inf)."""
        s = self.score
        split = lambda m: {"wins": int((s[m] > 0).sum()), "draws": int((s[m] == 0).sum()), "losses": int((s[m] < 0).sum())}  # noqa: E731
        n = int(len(s))
        out = {"games": n, **split(slice(None)), "as_x": split(self.a_colour > 0), "as_o": split(self.a_colour < 0)}
        score = (out["wins"] + 0.5 * out["draws"]) / n
        m = (self.pair_score.astype(np.float64) + 2.0) / 4.0
        P = len(m)
        if P >= 2:
            half = 1.96 * math.sqrt(float(m.var(ddof=1)) / P)
            ci = [elo_of_score(max(0.0, score - half)), elo_of_score(min(1.0, score + half))]
        else:
            ci = [-math.inf, math.inf]
        out.update(score=score, elo=elo_of_score(score), elo_ci95=ci)
        return out


_ENGINE_ERRS = ((1, "edge arena overflow"), (2, "terminal root"), (4, "example buffer overflow"),
                (8, "walk deeper than the path buffer"), (16, "the evaluator returned a non-finite logit or value"))


class Match:
    """The device side of a match: the bz_match workspace (torch-owned) and its ABI (include/bz_abi.h)."""

    def __init__(self, game, n_games, device="cuda:0", max_plies=0):
        import torch
        from .engine import _GAMES
        _lib.require_gpu()
        L = _lib.lib()
        self.device = torch.device(device)
        self.game = _GAMES[game]
        nbytes = L.bz_match_workspace_bytes(self.game, n_games, max_plies)
        if nbytes < 0:
            raise ValueError(_lib.last_error())
        self.ws = torch.zeros(nbytes + 256, dtype=torch.uint8, device=self.device)
        self._pad = (-self.ws.data_ptr()) & 255
        self.base = self.ws.data_ptr() + self._pad
        h = C.c_void_p()
        _lib.check(L.bz_match_create(self.game, n_games, max_plies, self.base, nbytes, C.byref(h)))
        self.h = h
        self.lay = _lib.MatchLayout()
        _lib.check(L.bz_match_get_layout(self.h, C.byref(self.lay)))
        self.B, self.T = self.lay.n_games, self.lay.max_plies

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self.device).cuda_stream

    def view(self, off, dtype, shape):
        import torch
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        return self.ws[self._pad + off:self._pad + off + n].view(dtype).view(*shape)

    def begin(self, seed, opening_plies):
        _lib.check(_lib.lib().bz_match_begin(self.h, int(seed) & (2**64 - 1), int(opening_plies), self._stream()))

    def ply(self, act_a, act_b, eng_a=None, eng_b=None):
        """act_a / act_b: int32 CUDA tensors [B] (bz_engine_root_policy's actions); eng_a / eng_b: SelfPlayEngines or None"""
        _lib.check(_lib.lib().bz_match_ply(self.h, act_a.data_ptr(), act_b.data_ptr(), eng_a.h if eng_a is not None else None,
                                           eng_b.h if eng_b is not None else None, self._stream()))

    def header(self):
        """the one synchronising read of a ply -> _lib.MatchHdr"""
        hdr = _lib.MatchHdr()
        _lib.check(_lib.lib().bz_match_header(self.h, self._stream(), C.byref(hdr)))
        return hdr

    def state(self):
        """the per-slot state as numpy arrays (own, opp as uint64)"""
        import torch
        L, B = self.lay, self.B
        n = lambda off, dt: self.view(off, dt, (B,)).cpu().numpy()  # noqa: E731
        return {"own": n(L.own, torch.int64).view(np.uint64), "opp": n(L.opp, torch.int64).view(np.uint64),
                "to_move": n(L.to_move, torch.int8), "active": n(L.active, torch.uint8), "winner": n(L.winner, torch.int8),
                "plies": n(L.plies, torch.int32), "a_colour": n(L.a_colour, torch.int8),
                "to_move_a": n(L.to_move_a, torch.int8), "to_move_b": n(L.to_move_b, torch.int8)}

    def log(self):
        import torch
        return (self.view(self.lay.log_action, torch.uint8, (self.T, self.B)).cpu().numpy(),
                self.view(self.lay.log_mover, torch.int8, (self.T, self.B)).cpu().numpy())

    def __del__(self):
        try:
            import torch
            torch.cuda.synchronize(self.device)
            _lib.lib().bz_match_destroy(self.h)
        except Exception:
            pass


def check_match(game, n_games, a, b, size, opening_plies):
    """validate a match's arguments (ValueError) without touching a device -> (engine game name, (ev_a, gumbel_a), (ev_b, gumbel_b))"""
    if game not in ("ttt", "tic_tac_toe", "reversi"):
        raise ValueError(f"play_match: game must be 'ttt' or 'reversi' (got {game!r})")
    ttt = game != "reversi"
    if not ttt and size not in (8, 6, 4):
        raise ValueError(f"play_match: the search engine plays Reversi on 8x8, 6x6 and 4x4 boards, not {size}x{size}")
    n = n_games
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 2 or n % 2:
        raise ValueError(f"play_match: n_games must be an even int >= 2 (got {n!r}): games 2k and 2k + 1 share an opening with "
                         "the colours swapped")
    if n > 1 << 24:
        raise ValueError(f"play_match: n_games must be <= {1 << 24} (got {n})")
    op = opening_plies
    if isinstance(op, bool) or not isinstance(op, (int, np.integer)) or op < 0:
        raise ValueError(f"play_match: opening_plies must be an int >= 0 (got {op!r})")
    for side, p in (("a", a), ("b", b)):
        if not isinstance(p, MatchPlayer):
            raise ValueError(f"play_match: player {side} must be a MatchPlayer (got {type(p).__name__})")
    g = "ttt" if ttt else "reversi"
    ename = "ttt" if ttt else {8: "reversi", 6: "reversi6", 4: "reversi4"}[size]
    return ename, a.checked(g, int(n), "a"), b.checked(g, int(n), "b")


def play_match(game, n_games, a, b, size=8, opening_plies=0, seed=0, device="cuda:0", run_ahead=16, on_ply=None):
    """n_games concurrent games between the MatchPlayers a and b -> MatchResult.  game: "ttt" | "reversi" (size 8, 6 or 4).
    Games 2k and 2k + 1 are a pair: the same `opening_plies` seeded random opening moves (by neither player), a plays X
    (moves first) in game 2k and O in game 2k + 1.  Past the opening every move is the mover's search: the first maximum
    of the visit counts (PUCT) or the Gumbel move.  Per ply: the roots of both engines, the two searches on two streams
    (interleaved step by step by bz_engines_search, at most `run_ahead` simulations ahead of the streams), their moves, one
    k_match_ply launch, one 32-byte read.  Both engines hold all n_games slots (about half are searched per ply).
    on_ply(engines, searched): a measuring hook, called after every ply's searches and before its moves are applied, with the
    two SelfPlayEngines and the indices of those that searched; it may read them (root_stats(), stopped(), counters())."""
    ename, (ev_a, gum_a), (ev_b, gum_b) = check_match(game, n_games, a, b, size, opening_plies)
    import torch
    from .engine import SelfPlayEngine, pipeline_streams
    _lib.require_gpu()
    L = _lib.lib()
    dev = torch.device(device)
    B = int(n_games)
    engs = [SelfPlayEngine(ename, B, p.sims, ev, p.net, p.c_puct, device=device, eval_cache=p.eval_cache,
                           leaves_per_step=p.leaves_per_step, gumbel=gum, eval_symmetry=p.eval_symmetry, fpu=p.fpu, solver=bool(p.solver),
                           early_stop=p.early_stop)
            for p, ev, gum in ((a, ev_a, gum_a), (b, ev_b, gum_b))]
    m = Match(ename, B, device)
    streams = pipeline_streams(dev, 2)
    for e, st in zip(engs, streams):
        e.track_stream(st)
    lay = m.lay
    tms = (m.base + lay.to_move_a, m.base + lay.to_move_b)
    acts = [torch.full((B,), -1, dtype=torch.int32, device=dev) for _ in engs]
    pis = [torch.empty((B, e.na), dtype=torch.float32, device=dev) for e in engs]
    with torch.cuda.device(dev):
        m.begin(seed, opening_plies)
        hdr = m.header()
        while hdr.n_active > 0:
            cur = torch.cuda.current_stream(dev)
            go = [i for i, n in enumerate((hdr.n_to_move_a, hdr.n_to_move_b)) if n > 0]  # a side with no slot to move is not searched
            for i in go:
                streams[i].wait_stream(cur)
                _lib.check(L.bz_engine_set_roots(engs[i].h, m.base + lay.own, m.base + lay.opp, tms[i], streams[i].cuda_stream))
            _lib.check(L.bz_engines_search((C.c_void_p * 2)(*[engs[i].h if i in go else None for i in range(2)]),
                                           (C.c_void_p * 2)(*[st.cuda_stream for st in streams]), 2, int(run_ahead)))
            if on_ply is not None:
                on_ply(engs, go)
            for i in go:
                _lib.check(L.bz_engine_root_policy(engs[i].h, pis[i].data_ptr(), acts[i].data_ptr(), streams[i].cuda_stream))
                cur.wait_stream(streams[i])
            m.ply(acts[0], acts[1], engs[0], engs[1])
            hdr = m.header()
            if hdr.error or hdr.engine_err_a or hdr.engine_err_b:
                break
        _raise_on_error(m, hdr)
        st = m.state()
        actions, movers = m.log()
    T = int(st["plies"].max())
    return MatchResult(st["winner"], st["a_colour"], st["plies"], actions[:T].copy(), movers[:T].copy())


def _raise_on_error(m, hdr):
    for side, e in (("a", hdr.engine_err_a), ("b", hdr.engine_err_b)):
        if e:
            raise RuntimeError(f"play_match: player {side}'s engine raised error flags 0x{e:x}: " +
                               ", ".join(n for bit, n in _ENGINE_ERRS if e & bit))
    if hdr.error:
        g = hdr.error & _lib.MATCH_ERR_SLOT_MASK
        st = m.state()
        what = "no action" if (hdr.error & ~_lib.MATCH_ERR_SLOT_MASK) == _lib.MATCH_ERR_NO_ACTION else "an illegal move"
        who = "a" if st["to_move"][g] == st["a_colour"][g] else "b"
        raise RuntimeError(f"play_match: player {who} produced {what}: game {g}, ply {int(st['plies'][g])}, own "
                           f"{int(st['own'][g]):#018x} opp {int(st['opp'][g]):#018x}")
    if hdr.n_active:
        raise RuntimeError("play_match: games still running after the last ply")
