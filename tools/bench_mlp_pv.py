"""What the value head of the tic-tac-toe MLP costs, on one GPU.  The variants of each comparison are
interleaved round by round in one process and the median over the rounds is reported; prints one JSON line per section:
  - forward: us per launch, PV (logits and value) against policy-only (logits), f32 and bf16, at n = 1, 128, 4520, 65536;
  - train: us per step, bz_mlp_train_step_pv against bz_mlp_train_step, at batch 128 and at PVTrainer's default batch;
  - self_play: tic-tac-toe games/s with the mlp_bf16 evaluator, a PV handle against a policy-only one.
    python tools/bench_mlp_pv.py [--hidden 256] [--games 1024] [--sims 50] [--reps 50] [--rounds 7] [--out FILE.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.record()
    for _ in range(reps):
        fn()
    en.record()
    en.synchronize()
    return st.elapsed_time(en) * 1e3 / reps  # us


def interleaved(variants, reps, rounds):
    """variants: {name: fn} -> {name: {"median_us", "min_us", "max_us"}}; one warm-up pass, then `rounds` rounds in which every
    variant is timed once, in turn"""
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    got = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            got[k].append(timed(fn, reps))
    return {k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)} for k, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from betazero_amd import _lib
    from betazero_amd.engine import self_play
    from betazero_amd.mlp import DeviceMLP, MLPTrainer, PVTrainer, TicTacToePVNet
    torch.manual_seed(0)
    H = a.hidden
    pv_mod = TicTacToePVNet(H).eval()
    pol_mod = pv_mod.policy_net()
    pv, pol = DeviceMLP.from_module(pv_mod), DeviceMLP.from_module(pol_mod)
    L = _lib.lib()
    lines = []

    def emit(rec):
        rec = {"hidden": H, **rec}
        print(json.dumps(rec)); lines.append(rec)
    g = torch.Generator().manual_seed(1)
    for n in (1, 128, 4520, 65536):
        own = torch.randint(0, 512, (n,), generator=g).cuda()
        opp = (torch.randint(0, 512, (n,), generator=g).cuda() & ~own)
        lg, v = torch.empty((n, 9), device="cuda"), torch.empty(n, device="cuda")
        st = torch.cuda.current_stream().cuda_stream
        # the C entry points on preallocated outputs: the launch alone, not torch.empty
        res = interleaved({
            "policy_f32": lambda: L.bz_mlp_forward_f32(pol.h, own.data_ptr(), opp.data_ptr(), n, lg.data_ptr(), st),
            "pv_f32": lambda: L.bz_mlp_forward_pv_f32(pv.h, own.data_ptr(), opp.data_ptr(), n, lg.data_ptr(), v.data_ptr(), st),
            "policy_bf16": lambda: L.bz_mlp_forward_bf16(pol.h, own.data_ptr(), opp.data_ptr(), n, lg.data_ptr(), st),
            "pv_bf16": lambda: L.bz_mlp_forward_pv_bf16(pv.h, own.data_ptr(), opp.data_ptr(), n, lg.data_ptr(), v.data_ptr(), st),
        }, a.reps, a.rounds)
        emit({"section": "forward", "n": n, "reps": a.reps, "rounds": a.rounds, **res})
    for batch in (128, 1024):
        x = torch.randint(-1, 2, (batch, 9), generator=g).float().cuda()
        t = torch.randint(0, 9, (batch,), generator=g).to(torch.int32).cuda()
        pi = torch.rand((batch, 9), generator=g).cuda()
        pi = pi / pi.sum(1, keepdim=True)
        vt = (torch.randint(-1, 2, (batch,), generator=g)).float().cuda()
        sl, az = MLPTrainer(pol_mod, max_batch=batch), PVTrainer(pv_mod, max_batch=batch)
        res = interleaved({"supervised": lambda: sl.step(x, t), "pv": lambda: az.step(x, pi, vt)}, a.reps, a.rounds)
        assert sl.error() == 0 and az.error() == 0
        emit({"section": "train", "batch": batch, "reps": a.reps, "rounds": a.rounds, **res})

    def games_per_s(net):
        t0 = time.perf_counter()
        self_play("ttt", a.games, a.sims, net=net, evaluator="mlp_bf16", temp_moves=4)
        torch.cuda.synchronize()
        return a.games / (time.perf_counter() - t0)
    for net in (pol, pv):
        games_per_s(net)
    got = {"policy": [], "pv": []}
    for _ in range(a.rounds):
        got["policy"].append(games_per_s(pol)); got["pv"].append(games_per_s(pv))
    emit({"section": "self_play", "games": a.games, "sims": a.sims, "rounds": a.rounds,
          **{k: {"median_games_per_s": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
             for k, v in got.items()}})
    if a.out:
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
