"""The AlphaZero loop on tic-tac-toe with the MLP that has a value head (TicTacToePVNet).  Per iteration:
self-play with the current net in the search (PipelinedSelfPlay, evaluator mlp_bf16, Dirichlet noise, --temp-moves) ->
device_examples -> [value_targets] -> augment_examples -> a window of --window iterations [-> merge_positions] ->
PVTrainer.fit_examples; the engines search with the updated handle.  Every --arena-every iterations the net plays minimax
(play_arena, full depth) as X and as O, and the yard-stick is taken: value MSE and the share of minimax-optimal top legal
logits over the 4,520 non-terminal reachable positions (tests/golden/ttt_mlp.npz).  One JSON line per iteration; --out
collects them.
    python tools/ttt_az.py [--hidden 64] [--games 1024] [--sims 50] [--iters 20] [--window 4] [--epochs 2] [--batch 1024]
                           [--lr 1e-3] [--value-weight 1.0] [--temp-moves 4] [--arena-every 5] [--arena-games 64]
                           [--merge-positions] [--value-lambda 1.0] [--value-q-mix 0.0] [--init-net FILE] [--save-net FILE]
                           [--out JSON] [--seed 0]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def load_net(path, hidden):
    """--init-net: a TicTacToeNet or TicTacToePVNet state_dict, or one of the reference's checkpoints (whole module or
    state_dict: load_reference_model); nothing: a fresh TicTacToePVNet"""
    from betazero_amd.mlp import TicTacToePVNet, load_reference_model
    if not path:
        return TicTacToePVNet(hidden)
    try:
        sd = torch.load(path, map_location="cpu", weights_only=True)
    except Exception:
        sd = None
    if isinstance(sd, dict) and "fc4.weight" in sd and sd["fc4.weight"].shape[0] == 10:
        m = TicTacToePVNet(int(sd["fc1.weight"].shape[0]))
        m.load_state_dict({k: v.to(torch.float32) for k, v in sd.items()})
        return m
    return TicTacToePVNet.from_policy_net(load_reference_model(path))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--games", type=int, default=1024)
    ap.add_argument("--sims", type=int, default=50)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--window", type=int, default=4)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--value-weight", type=float, default=1.0)
    ap.add_argument("--temp-moves", type=int, default=4)
    ap.add_argument("--dirichlet-eps", type=float, default=0.25)
    ap.add_argument("--dirichlet-alpha", type=float, default=1.0)
    ap.add_argument("--arena-every", type=int, default=5)
    ap.add_argument("--arena-games", type=int, default=64)
    ap.add_argument("--arena-sims", type=int, default=100)
    ap.add_argument("--merge-positions", action="store_true")
    ap.add_argument("--value-lambda", type=float, default=1.0)
    ap.add_argument("--value-q-mix", type=float, default=0.0)
    ap.add_argument("--init-net", default=None)
    ap.add_argument("--save-net", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    from betazero_amd.arena import play_arena
    from betazero_amd.augment import augment_examples
    from betazero_amd.engine import PipelinedSelfPlay
    from betazero_amd.examples import concat
    from betazero_amd.merge import merge_positions
    from betazero_amd.mlp import PVTrainer
    from betazero_amd.ttt_yardstick import minimax_targets, yardstick
    from betazero_amd.value_targets import value_targets
    torch.manual_seed(a.seed)
    z = np.load(os.path.join(ROOT, "tests", "golden", "ttt_mlp.npz"))
    own = np.where(z["to_move"] == 1, z["x_bits"], z["o_bits"]).astype(np.uint64)
    opp = np.where(z["to_move"] == 1, z["o_bits"], z["x_bits"]).astype(np.uint64)
    targets = minimax_targets(own, opp)
    tr = PVTrainer(load_net(a.init_net, a.hidden), lr=a.lr, value_weight=a.value_weight, max_batch=a.batch)
    search_value = a.value_lambda < 1.0 or a.value_q_mix > 0.0
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(a.seed)
    lines, window = [], []

    def measure(rec):
        rec["yardstick"] = yardstick(tr.device_mlp, own, opp, targets)
        rec["arena"] = {}
        for name, ev in (("mlp_bf16", "mlp_bf16"),):
            res = play_arena("ttt", a.arena_games, a.arena_sims, opponent_depth=9, evaluator=ev, net=tr.device_mlp, seed=a.seed)
            s = res.score
            side = np.where(np.arange(len(s)) % 2 == 0, "X", "O")   # play_arena: the search plays X in the even games
            rec["arena"][name] = {c: {"wins": int((s[side == c] > 0).sum()), "draws": int((s[side == c] == 0).sum()),
                                      "losses": int((s[side == c] < 0).sum())} for c in ("X", "O")}

    rec0 = {"iter": 0, "hidden": tr.H, "args": vars(a)}
    measure(rec0)
    print(json.dumps(rec0)); lines.append(rec0)
    t0 = time.perf_counter()
    for it in range(1, a.iters + 1):
        t1 = time.perf_counter()
        sp = PipelinedSelfPlay("ttt", a.games, a.sims, "mlp_bf16", net=tr.device_mlp, temp_moves=a.temp_moves,
                               dirichlet_eps=a.dirichlet_eps, dirichlet_alpha=a.dirichlet_alpha, seed=a.seed * 100003 + it,
                               search_value=search_value)
        sp.run_iteration()
        ex = sp.device_examples()
        z_mean = float(ex.z.float().mean())
        if search_value:
            ex = value_targets(ex, a.value_lambda, a.value_q_mix)
        ex = augment_examples(ex)
        window = (window + [ex])[-a.window:]
        rows = concat(window)
        if a.merge_positions:
            rows = merge_positions(rows)
        t2 = time.perf_counter()
        hist = tr.fit_examples(rows, a.epochs, a.batch, gen)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        rec = {"iter": it, "games": a.games, "rows": len(ex), "train_rows": len(rows), "z_mean": round(z_mean, 4),
               "loss": round(hist[-1]["loss"], 5), "steps": tr.steps, "self_play_s": round(t2 - t1, 3), "train_s": round(t3 - t2, 3),
               **{k: round(v, 5) for k, v in tr.evaluate(ex).items() if k != "rows"}}
        if it % a.arena_every == 0 or it == a.iters:
            measure(rec)
        print(json.dumps(rec)); lines.append(rec)
    print(f"wall time {time.perf_counter() - t0:.1f} s", file=sys.stderr)
    if a.save_net:
        torch.save(tr.to_module().state_dict(), a.save_net)
        torch.save(tr.to_module().policy_net().state_dict(), a.save_net + ".policy")   # what the reference's AIPlayer loads
    if a.out:
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
