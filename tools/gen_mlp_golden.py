"""Write tests/golden/ttt_mlp.npz from the reference's own TicTacToeNet and AIPlayer (run where the reference is checked
out; nothing of it enters the repository but these arrays):

    python tools/gen_mlp_golden.py /path/to/BetaZero [checkpoint]

checkpoint defaults to the reference's src/tic_tac_toe/SL/models/tic_tac_toe_model_2023-12-23_13-26-47.pth.  It is read
with torch.load(weights_only=True) and an allowlist (the reference's class under __main__.TicTacToeNet, nn.Linear,
nn.ReLU): no pickle code runs.  The fixture holds
  - the eight parameter tensors (fp32, torch layouts): fc1_w fc1_b ... fc4_w fc4_b;
  - every non-terminal position of ttt_exhaustive.npz: x_bits / o_bits (cell i = bit i) and to_move (+1 X, -1 O);
  - states [n, 9] f32 = to_move * board, the reference's input;
  - logits [n, 9] f32 = the reference module's fp32 forward of states (torch CPU);
  - move [n] i32 = 3 * row + col of the reference AIPlayer.get_move (its debug prints captured and dropped)."""
import contextlib
import io
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ref = os.path.abspath(sys.argv[1])
    ckpt = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ref, "src", "tic_tac_toe", "SL", "models",
                                                              "tic_tac_toe_model_2023-12-23_13-26-47.pth")
    sys.path.insert(0, os.path.join(ref, "src", "tic_tac_toe", "SL"))
    sys.path.insert(0, os.path.join(ref, "src", "tic_tac_toe"))
    sys.path.insert(0, os.path.join(ref, "src"))
    from neural_networks import TicTacToeNet as RefNet  # the reference's module
    import players as ref_players                       # the reference's AIPlayer
    from tic_tac_toe_board import TicTacToeBoard as RefBoard

    with torch.serialization.safe_globals([(RefNet, "__main__.TicTacToeNet"), nn.Linear, nn.ReLU]):
        obj = torch.load(ckpt, map_location="cpu", weights_only=True)
    sd = obj.state_dict() if isinstance(obj, nn.Module) else obj
    H = sd["fc1.weight"].shape[0]
    model = RefNet(9, H, 9)
    model.load_state_dict(sd)
    model.eval()

    pos = np.load(os.path.join(ROOT, "tests", "golden", "ttt_exhaustive.npz"))["pos"]
    live = pos[pos[:, 4] == 0]  # columns: x bits, o bits, mover (1 = X, 3 = O), legal, over, winner + 1
    xb, ob = live[:, 0].astype(np.int64), live[:, 1].astype(np.int64)
    to_move = np.where(live[:, 2] == 1, 1, -1).astype(np.int8)
    cells = np.arange(9)
    board = ((xb[:, None] >> cells) & 1) - ((ob[:, None] >> cells) & 1)        # +1 X, -1 O, row-major
    states = (to_move[:, None] * board).astype(np.float32)
    with torch.no_grad():
        logits = model(torch.from_numpy(states)).numpy().astype(np.float32)

    player = ref_players.AIPlayer.__new__(ref_players.AIPlayer)  # its __init__ would torch.load without weights_only
    player.model = model
    moves = np.empty(len(live), np.int32)
    for i in range(len(live)):
        player.symbol = int(to_move[i])
        b = RefBoard()
        b.board = board[i].reshape(3, 3).astype(int)
        with contextlib.redirect_stdout(io.StringIO()), torch.no_grad():
            r, c = player.get_move(b)
        moves[i] = 3 * r + c

    out = {}
    for l in (1, 2, 3, 4):
        out[f"fc{l}_w"] = sd[f"fc{l}.weight"].to(torch.float32).numpy()
        out[f"fc{l}_b"] = sd[f"fc{l}.bias"].to(torch.float32).numpy()
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "ttt_mlp.npz"), x_bits=xb, o_bits=ob, to_move=to_move,
                        states=states, logits=logits, move=moves, **out)
    print(f"ttt_mlp.npz: H={H}, {len(live)} positions")


if __name__ == "__main__":
    main()
