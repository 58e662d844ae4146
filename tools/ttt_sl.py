"""The reference's supervised tic-tac-toe pipeline (SL/generate_training_games.py -> SL/train.py -> AIPlayer) on the
device: minimax games (OptimalPlayer x 2) -> D4 augmentation with dedupe -> MLPTrainer.fit -> AIPlayer and
MCTSPlayer(net=...) against OptimalPlayer as X and as O.  Prints losses, accuracies, results and wall time.
    python tools/ttt_sl.py [--games 100] [--epochs 500] [--hidden 256] [--matches 50] [--sims 100] [--seed 0]"""
import argparse
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=100)
    ap.add_argument("--epochs", type=int, default=500)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--matches", type=int, default=50)
    ap.add_argument("--sims", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import betazero_amd as bz
    from betazero_amd.augment import augment_examples
    from betazero_amd.engine import Examples
    from betazero_amd.examples_io import collect_game_data
    random.seed(a.seed)
    torch.manual_seed(a.seed)
    t0 = time.perf_counter()
    states, actions = collect_game_data(a.games, bz.OptimalPlayer(1), bz.OptimalPlayer(-1))
    n = len(states)
    w = (1 << np.arange(9)).astype(np.int64)
    s = states.reshape(n, 9)
    ex = Examples(own=((s == 1) * w).sum(1).astype(np.uint64), opp=((s == -1) * w).sum(1).astype(np.uint64),
                  pi=actions.reshape(n, 9).astype(np.float32), z=np.zeros(n, np.int8), mover=np.ones(n, np.int8),
                  act=actions.reshape(n, 9).argmax(1).astype(np.uint8), game=np.zeros(n, np.int64),
                  ply=np.zeros(n, np.uint8), size=3)
    aug = augment_examples(ex)
    cells = np.arange(9, dtype=np.uint64)
    x = (((aug.own[:, None] >> cells) & np.uint64(1)).astype(np.float32)
         - ((aug.opp[:, None] >> cells) & np.uint64(1)).astype(np.float32))
    t1 = time.perf_counter()
    print(f"data: {a.games} games -> {n} rows -> {len(x)} augmented rows ({t1 - t0:.1f} s)")
    tr = bz.MLPTrainer(bz.TicTacToeNet(9, a.hidden, 9))
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(a.seed)
    hist = tr.fit(x, aug.pi, a.epochs, generator=gen,
                  log=lambda r: print(f"epoch {r['epoch']:4d}: train loss {r['train_loss']:.4f} acc {r['train_acc']:.4f}  "
                                      f"val loss {r['val_loss']:.4f} acc {r['val_acc']:.4f}")
                  if r["epoch"] == 1 or r["epoch"] % 50 == 0 else None)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(f"training: {a.epochs} epochs, {tr.steps} steps in {t2 - t1:.1f} s ({(t2 - t1) / max(tr.steps, 1) * 1e3:.2f} ms/step "
          f"incl. validation); final val acc {hist[-1]['val_acc']:.4f}")
    net = bz.DeviceMLP.from_module(tr.to_module(), max_batch=16)
    for name, make in (("AIPlayer", lambda sym: bz.AIPlayer(net, sym)),
                       (f"MCTSPlayer(mlp_f32, {a.sims} sims)", lambda sym: bz.MCTSPlayer(sym, sims=a.sims, net=net))):
        for sym in (1, -1):
            res = {"won": 0, "drawn": 0, "lost": 0}
            for _ in range(a.matches):
                p1, p2 = (make(1), bz.OptimalPlayer(-1)) if sym == 1 else (bz.OptimalPlayer(1), make(-1))
                _, winner = bz.TicTacToeHeadless(p1, p2).play()
                res["drawn" if not winner else ("won" if winner == sym else "lost")] += 1
            print(f"{name} as {'X' if sym == 1 else 'O'} vs OptimalPlayer: {res}")
    print(f"wall time {time.perf_counter() - t0:.1f} s")


if __name__ == "__main__":
    main()
