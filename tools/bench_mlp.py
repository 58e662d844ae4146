"""Benchmark of the tic-tac-toe MLP (betazero_amd.mlp) on one GPU; prints ONE JSON line:
  - forward: us per launch at n = 1, 128, 4520, 65536 for f32 and bf16, with the achieved TFLOP/s as a fraction of the
    dense peak of that precision (MI355X: 157.3 TFLOP/s fp32 vector, 2516.6 TFLOP/s bf16 MFMA);
  - train: us per training step at batch 128 (bz_mlp_train_step: 2 launches) against torch eager fp32 + Adam;
  - self_play: tic-tac-toe games/s with the mlp_bf16 evaluator, with uniform, and with an external torch MLP at the same
    games and sims.
    python tools/bench_mlp.py [--hidden 256] [--games 1024] [--sims 50] [--reps 50]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = {"f32": 157.3e12, "bf16": 2516.6e12}


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st.record()
    for _ in range(reps):
        fn()
    en.record()
    en.synchronize()
    return st.elapsed_time(en) * 1e3 / reps  # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    from betazero_amd.engine import SelfPlayEngine, self_play
    from betazero_amd.mlp import DeviceMLP, MLPTrainer, TicTacToeNet
    torch.manual_seed(0)
    H = a.hidden
    m = TicTacToeNet(9, H, 9).eval()
    net = DeviceMLP.from_module(m, max_batch=65536)
    flops_row = 2 * (9 * H + 2 * H * H + 9 * H)
    out = {"hidden": H, "forward": {}, "train": {}, "self_play": {}}
    g = torch.Generator().manual_seed(1)
    for n in (1, 128, 4520, 65536):
        own = torch.randint(0, 512, (n,), generator=g).cuda()
        opp = (torch.randint(0, 512, (n,), generator=g).cuda() & ~own)
        for prec in ("f32", "bf16"):
            us = timed(lambda: net.forward(own, opp, bf16=prec == "bf16"), a.reps)
            tf = flops_row * n / (us * 1e-6)
            out["forward"][f"{prec}_n{n}"] = {"us": round(us, 2), "tflops": round(tf / 1e12, 3),
                                              "frac_peak": round(tf / PEAK[prec], 5)}
    # training step, batch 128
    x = torch.randint(-1, 2, (128, 9), generator=g).float().cuda()
    t = torch.randint(0, 9, (128,), generator=g).cuda()
    tr = MLPTrainer(m)
    out["train"]["bz_us"] = round(timed(lambda: tr.step(x, t), a.reps), 2)
    tm = TicTacToeNet(9, H, 9).cuda()
    opt = torch.optim.Adam(tm.parameters(), lr=1e-4)
    crit = torch.nn.CrossEntropyLoss()

    def torch_step():
        opt.zero_grad()
        crit(tm(x), t).backward()
        opt.step()
    out["train"]["torch_eager_us"] = round(timed(torch_step, a.reps), 2)
    # self-play games/s at the same games and sims
    def games_per_s(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = fn()
        torch.cuda.synchronize()
        return round(n / (time.perf_counter() - t0), 1)

    def sp(evaluator):
        def run():
            self_play("ttt", a.games, a.sims, net=net if evaluator.startswith("mlp") else None, evaluator=evaluator, temp_moves=4)
            return a.games
        return run

    def external():
        e = SelfPlayEngine("ttt", a.games, a.sims, "external", temp_moves=4)
        tmf = m.cuda()

        def fn(own, opp, kind):
            cells = torch.arange(9, device=own.device)
            xx = (((own[:, None] >> cells) & 1) - ((opp[:, None] >> cells) & 1)).float()
            with torch.no_grad():
                return tmf(xx), torch.zeros(own.numel(), device=own.device)
        e.reset_games()
        for _ in range(12):
            e.search_external(fn)
            e.play(False)
            if e.status()[0] == 0:
                break
        return a.games
    out["self_play"] = {"games": a.games, "sims": a.sims, "mlp_bf16": games_per_s(sp("mlp_bf16")),
                        "mlp_f32": games_per_s(sp("mlp_f32")), "uniform": games_per_s(sp("uniform")),
                        "external_torch": games_per_s(external)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
