#!/usr/bin/env python3
"""play_match (one k_match_ply launch and one 32-byte read per ply) against the same match driven by the
public pieces the package had before it -- the arena's loop (betazero_amd/arena.py) with a second engine in the minimax
player's place: set_roots / search / root_policy_dev or root_stats / torch glue / bz_*_step_batch, everything on the
current stream, a handful of host synchronisations per ply.  Both drivers run interleaved in one process, mirror matches
(the same player on both sides), 4 random opening plies per pair, at B in {256, 4096}, sims in {16, 64, 800}, with the
uniform evaluator and the bench's 128x6 bf16 net.

One JSON object per configuration on stdout (and appended to --out): medians of --repeats whole matches per driver, every
repeat's time, ms per ply and games/s.

    python tools/bench_match.py [--repeats 5] [--only uniform|net_bf16] [--games 256,4096] [--sims 16,64,800] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from betazero_amd import _lib  # noqa: E402
from betazero_amd.match import MatchPlayer, MatchResult, check_match, play_match  # noqa: E402


def parent_pieces_match(game, n_games, a, b, size=8, opening_plies=0, seed=0, device="cuda:0", max_plies=200):
    """The match through the pieces play_arena is made of: two SelfPlayEngines searched one after the other on the current
    stream, the mover's action picked with torch, one batched env step, torch.where for the pass rule.  Pairing as in
    play_match (A is X in game 2k, O in 2k + 1).  opening_plies > 0 draws the openings from a torch generator per pair (the
    arena's way): the same amount of work as play_match's openings, not the same moves -- with opening_plies == 0 the result
    equals play_match's game for game."""
    from betazero_amd.engine import SelfPlayEngine
    ename, (ev_a, gum_a), (ev_b, gum_b) = check_match(game, n_games, a, b, size, opening_plies)
    _lib.require_gpu()
    L = _lib.lib()
    dev = torch.device(device)
    ttt = ename == "ttt"
    B = int(n_games)
    engs = [SelfPlayEngine(ename, B, p.sims, ev, p.net, p.c_puct, device=device, eval_cache=p.eval_cache,
                           leaves_per_step=p.leaves_per_step, gumbel=g) for p, ev, g in ((a, ev_a, gum_a), (b, ev_b, gum_b))]
    st = lambda: torch.cuda.current_stream(dev).cuda_stream  # noqa: E731
    if ttt:
        own = torch.zeros(B, dtype=torch.int16, device=dev)
        opp = torch.zeros(B, dtype=torch.int16, device=dev)
    else:
        p = size // 2 - 1
        x0 = (1 << (8 * p + p)) | (1 << (8 * (p + 1) + p + 1))
        o0 = (1 << (8 * p + p + 1)) | (1 << (8 * (p + 1) + p))
        own = torch.full((B,), x0, dtype=torch.int64, device=dev)
        opp = torch.full((B,), o0, dtype=torch.int64, device=dev)
    to_move = torch.ones(B, dtype=torch.int8, device=dev)
    a_colour = torch.as_tensor(np.where(np.arange(B) % 2 == 0, 1, -1).astype(np.int8)).to(dev)
    active = torch.ones(B, dtype=torch.bool, device=dev)
    winner = torch.zeros(B, dtype=torch.int8, device=dev)
    plies = torch.zeros(B, dtype=torch.int32, device=dev)
    wdt = torch.int16 if ttt else torch.int64
    own_n, opp_n, legal_n = (torch.empty(B, dtype=wdt, device=dev) for _ in range(3))
    status = torch.empty(B, dtype=torch.uint8, device=dev)
    win_n = torch.empty(B, dtype=torch.int8, device=dev)
    log = []
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    valid = (1 << 9) - 1 if ttt else sum(((1 << size) - 1) << (8 * r) for r in range(size))
    valid_t = torch.tensor(valid - (1 << 64) if valid >= 1 << 63 else valid, dtype=torch.int64, device=dev)
    shifts = torch.arange(64, dtype=torch.int64, device=dev)
    for ply in range(max_plies):
        if not bool(active.any()):
            break
        turns = [active & (to_move == a_colour), active & (to_move != a_colour)]
        action = torch.full((B,), 255, dtype=torch.uint8, device=dev)
        if ply < opening_plies:  # a random legal move for every pair, by neither player
            if ttt:
                legal = ~(own | opp).to(torch.int64) & valid_t
            else:
                legal = torch.empty(B, dtype=torch.int64, device=dev)
                with torch.cuda.device(dev):
                    _lib.check(L.bz_reversi_legal_batch(own.data_ptr(), opp.data_ptr(), B, legal.data_ptr(), st()))
                legal = legal & valid_t
            bits = ((legal.unsqueeze(1) >> shifts) & 1).bool()
            draw = torch.rand((B // 2, 64), generator=gen, device=dev).repeat_interleave(2, 0)
            pick = torch.where(bits, draw, torch.full_like(draw, -1.0)).argmax(1).to(torch.uint8)
            action = torch.where(active, pick, action)
            turns = [torch.zeros_like(active)] * 2
        for eng, turn in zip(engs, turns):
            if not bool(turn.any()):
                continue
            roots_tm = torch.where(turn, to_move, torch.zeros_like(to_move))
            o64 = own.to(torch.int64) if ttt else own
            p64 = opp.to(torch.int64) if ttt else opp
            with torch.cuda.device(dev):
                _lib.check(L.bz_engine_set_roots(eng.h, o64.data_ptr(), p64.data_ptr(), roots_tm.data_ptr(), st()))
            eng.search()
            if eng.gumbel is not None:
                pick = eng.root_policy_dev()[1].to(torch.uint8)
            else:
                eng._call(L.bz_engine_root_stats)
                pick = eng._view(eng.lay.root_N, torch.int32, (B, eng.na)).argmax(1).to(torch.uint8)  # first maximum of N
            eng.status()
            action = torch.where(turn, pick, action)
        log.append((action.cpu().numpy(), torch.where(active, to_move, torch.zeros_like(to_move)).cpu().numpy()))
        safe = torch.where(active, action, torch.zeros_like(action))
        with torch.cuda.device(dev):
            if ttt:
                _lib.check(L.bz_ttt_step_batch(own.data_ptr(), opp.data_ptr(), safe.data_ptr(), to_move.data_ptr(), B,
                                               own_n.data_ptr(), opp_n.data_ptr(), legal_n.data_ptr(), status.data_ptr(),
                                               win_n.data_ptr(), st()))
            else:
                _lib.check(L.bz_reversi_step_batch_sized(own.data_ptr(), opp.data_ptr(), safe.data_ptr(), B, size,
                                                         own_n.data_ptr(), opp_n.data_ptr(), legal_n.data_ptr(),
                                                         status.data_ptr(), win_n.data_ptr(), st()))
        if bool((active & (status == _lib.ST_ILLEGAL)).any()):
            raise RuntimeError(f"parent_pieces_match: an illegal move at ply {ply}")
        term = active & (status == _lib.ST_TERMINAL)
        winner = torch.where(term, win_n if ttt else (win_n * to_move).to(torch.int8), winner)
        plies = plies + active.to(torch.int32)
        must_pass = active & (status == _lib.ST_MUST_PASS)
        run = active & (status == _lib.ST_RUNNING)
        own, opp = (torch.where(run, own_n, torch.where(must_pass, opp_n, own)),
                    torch.where(run, opp_n, torch.where(must_pass, own_n, opp)))
        to_move = torch.where(run, -to_move, to_move)
        active = active & ~term
    if bool(active.any()):
        raise RuntimeError("parent_pieces_match: games still running after max_plies")
    T = len(log)
    return MatchResult(winner.cpu().numpy(), a_colour.cpu().numpy(), plies.cpu().numpy(),
                       np.stack([x[0] for x in log]) if T else np.zeros((0, B), np.uint8),
                       np.stack([x[1] for x in log]) if T else np.zeros((0, B), np.int8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, choices=("uniform", "net_bf16"))
    ap.add_argument("--games", default="256,4096")
    ap.add_argument("--sims", default="16,64,800")
    ap.add_argument("--opening-plies", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from betazero_amd.net import DeviceNet, PolicyValueNet
    torch.manual_seed(0)
    games = [int(x) for x in args.games.split(",")]
    net = None
    for ev in ("uniform", "net_bf16"):
        if args.only and ev != args.only:
            continue
        if ev == "net_bf16" and net is None:
            net = DeviceNet.from_module(PolicyValueNet(128, 6, 64).round_to_bf16_(), max(games))
        for B in games:
            for sims in (int(x) for x in args.sims.split(",")):
                pl = MatchPlayer(sims=sims, net=net if ev == "net_bf16" else None, evaluator=ev)
                kw = dict(size=8, opening_plies=args.opening_plies, seed=1)
                drivers = {"play_match": lambda: play_match("reversi", B, pl, pl, **kw),
                           "parent_pieces": lambda: parent_pieces_match("reversi", B, pl, pl, **kw)}
                times, plies = {k: [] for k in drivers}, {}
                for k, fn in drivers.items():  # warm-up: allocations, the stream pair
                    plies[k] = int(fn().plies.max())
                for _ in range(args.repeats):
                    for k, fn in drivers.items():
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        fn()
                        torch.cuda.synchronize()
                        times[k].append(time.perf_counter() - t0)
                row = {"what": "match", "game": "reversi", "evaluator": ev, "games": B, "sims": sims,
                       "opening_plies": args.opening_plies, "repeats": args.repeats}
                for k in drivers:
                    med = statistics.median(times[k])
                    row[k] = {"seconds_median": round(med, 4), "seconds_all": [round(t, 4) for t in times[k]], "plies": plies[k],
                              "ms_per_ply": round(med / plies[k] * 1e3, 3), "games_per_s": round(B / med, 1)}
                row["speedup_median"] = round(row["parent_pieces"]["seconds_median"] / row["play_match"]["seconds_median"], 3)
                line = json.dumps(row)
                print(line, flush=True)
                if args.out:
                    with open(args.out, "a") as f:
                        f.write(line + "\n")


if __name__ == "__main__":
    main()
