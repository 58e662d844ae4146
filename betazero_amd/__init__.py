"""betazero_amd -- MI355X-native self-play data generation behind BetaZero's
Python Game / Player API (reference: whaiproject/BetaZero).

Single-board rule calls go through the scalar entry points of libbz_hip.so;
everything batched (env step, MCTS, net, self-play) runs as gfx950 HIP kernels
and raises when no HIP device is present -- there is no CPU fallback."""
from .reversi import ReversiBoard, ReversiHeadless  # noqa: F401
from .tic_tac_toe import TicTacToeBoard, TicTacToeHeadless, process_game_positions  # noqa: F401
from .players import (Player, ReversiPlayer, RandomPlayer, ReversiRandomPlayer, MCTSPlayer,  # noqa: F401
                      OptimalPlayer, ReversiOptimalPlayer, NetPlayer, AIPlayer)

__all__ = ["ReversiBoard", "ReversiHeadless", "TicTacToeBoard", "TicTacToeHeadless", "process_game_positions",
           "Player", "ReversiPlayer", "RandomPlayer", "ReversiRandomPlayer", "MCTSPlayer",
           "OptimalPlayer", "ReversiOptimalPlayer", "NetPlayer", "AIPlayer",
           "TicTacToeNet", "TicTacToePVNet", "DeviceMLP", "MLPTrainer", "PVTrainer", "load_reference_model",
           "MatchPlayer", "MatchResult", "play_match", "Resign", "check_resign", "EarlyStop",
           "check_early_stop", "merge_positions", "merged_repeats", "save_checkpoint", "load_checkpoint",
           "Reanalyser", "reanalyse", "reanalyse_rows", "transform_rows"]


def __getattr__(name):  # the MLP names load torch: only when asked for
    if name in ("TicTacToeNet", "TicTacToePVNet", "DeviceMLP", "MLPTrainer", "PVTrainer", "load_reference_model"):
        from . import mlp
        return getattr(mlp, name)
    if name in ("MatchPlayer", "MatchResult", "play_match"):  # head-to-head matches
        from . import match
        return getattr(match, name)
    if name in ("Resign", "check_resign"):  # resignation in self-play
        from . import engine
        return getattr(engine, name)
    if name in ("EarlyStop", "check_early_stop"):  # exact early stop of a decided search
        from . import engine
        return getattr(engine, name)
    if name in ("merge_positions", "merged_repeats"):  # position averaging of the training window
        from . import merge
        return getattr(merge, name)
    if name in ("save_checkpoint", "load_checkpoint"):  # one file that carries a training run across processes
        from . import checkpoint
        return getattr(checkpoint, name)
    if name in ("Reanalyser", "reanalyse", "reanalyse_rows"):  # re-search stored rows with the current net
        import importlib
        mod = importlib.import_module(".reanalyse", __name__)   # (`reanalyse` is the MODULE; its one-shot function is betazero_amd.reanalyse.reanalyse)
        return mod if name == "reanalyse" else getattr(mod, name)
    if name == "transform_rows":  # a board symmetry per row of a training batch
        from . import train_symmetry
        return train_symmetry.transform_rows
    raise AttributeError(f"module 'betazero_amd' has no attribute {name!r}")
