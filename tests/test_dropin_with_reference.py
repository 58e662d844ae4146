"""Drop-in demonstration against fixture F13 (tests/golden/dropin.json, oracle/gen_golden.py gen_f13): what the
REFERENCE's own game loops and players printed and played over its own boards under fixed `random` seeds.  The
package's loops, players and board classes, under the same seeds, must reproduce it exactly."""
import json
import os
import random

import numpy as np
import pytest

import betazero_amd as bz


@pytest.fixture(scope="module")
def f13(golden_dir):
    with open(os.path.join(golden_dir, "dropin.json")) as f:
        return json.load(f)


def _board(arr, size):
    b = bz.ReversiBoard(size=size)
    b.board = np.asarray(arr)
    return b


@pytest.mark.parametrize("size", [4, 6, 8])
def test_reference_reversi_terminal_loop_over_our_board(size, f13, capsys):
    """ReversiTerminal.play (reversi_terminal.py:16-38) printed the board before every turn, a line for every pass, the
    final board and get_score(print_result=True).  bz.ReversiHeadless is that loop without the prints: its record
    (the position before every move and who moved) rebuilds the same transcript, character for character."""
    ref = f13["reversi_terminal"][str(size)]
    random.seed(ref["seed"])
    game = bz.ReversiHeadless(bz.ReversiRandomPlayer(1), bz.ReversiRandomPlayer(-1), size=size)
    positions, _ = game.play()
    movers = game.movers
    capsys.readouterr()
    for i, m in enumerate(movers):
        print(_board(positions[i], size), "\n")
        if i + 1 < len(movers) and movers[i + 1] == m:  # the other side could not move in between
            print(_board(positions[i + 1], size), "\n")
            print(f"Player {'X' if m == -1 else 'O'} cannot move.")
    print(game.board, "\n")
    game.board.get_score(print_result=True)
    got = capsys.readouterr().out
    assert got == ref["stdout"] and ("wins!" in got or "tie" in got)       # every printed board, pass line and score


def test_reference_ttt_minimax_player_over_our_board(f13):
    """the reference's OptimalPlayer (players.py:30-70) vs itself: bz.OptimalPlayer over OUR TicTacToeBoard, same moves"""
    for ref in f13["ttt_optimal_games"]:
        random.seed(ref["seed"])
        b, cur, moves = bz.TicTacToeBoard(), 1, []
        p = {1: bz.OptimalPlayer(1), -1: bz.OptimalPlayer(-1)}
        while not b.is_game_over()[0]:
            mv = p[cur].get_move(b)
            moves.append([int(v) for v in mv])
            b = b.make_move(*mv, cur)
            cur = -cur
        over, w = b.is_game_over()
        assert moves == ref["moves"] and [bool(over), int(w)] == ref["game_over"] == [True, 0]
        assert np.asarray(b.board).tolist() == ref["board"]


def test_reference_reversi_minimax_player_over_our_board(f13):
    """the reference's depth-limited OptimalPlayer (reversi_players.py:35-77) against its RandomPlayer on 6x6:
    bz.ReversiOptimalPlayer / bz.ReversiRandomPlayer over OUR ReversiBoard, same moves and board"""
    ref = f13["reversi_optimal_vs_random"]
    random.seed(ref["seed"])
    b, cur, moves = bz.ReversiBoard(size=ref["size"]), 1, []
    pl = {1: bz.ReversiOptimalPlayer(1, max_depth=2), -1: bz.ReversiRandomPlayer(-1)}
    for _ in range(ref["turns"]):
        if b.generate_possible_moves(cur):
            mv = pl[cur].get_move(b)
            moves.append([int(v) for v in mv])
            b = b.make_move(*mv, cur)
        cur = -cur
    assert moves == ref["moves"] and np.asarray(b.board).tolist() == ref["board"]


def test_collect_game_data_reproduces_the_reference_generator(f13, tmp_path):
    """SL/generate_training_games.py end to end: the states and actions of the reference's collect_game_data loop with
    its OptimalPlayer over its board against betazero_amd.examples_io.collect_game_data with OUR OptimalPlayer, same
    `random` seed: identical states and actions, and an identical CSV, in the format of the reference's
    tic_tac_toe_data.csv."""
    from betazero_amd.examples_io import collect_game_data, save_to_csv
    ref = f13["ttt_collect_game_data"]
    rs, ra = np.array(ref["states"], dtype=np.int64), np.array(ref["actions"], dtype=np.int64)
    random.seed(ref["seed"])
    s, a = collect_game_data(ref["games"], bz.OptimalPlayer(1), bz.OptimalPlayer(-1))
    assert np.array_equal(s, rs) and np.array_equal(a, ra) and len(s) == ref["games"] * 9
    f1, f2 = tmp_path / "ours.csv", tmp_path / "ref.csv"
    save_to_csv(s, a, str(f1)); save_to_csv(rs, ra, str(f2))
    assert f1.read_bytes() == f2.read_bytes() and f1.read_text().startswith("State,Action\n")
