"""Player plug-in point (reference: src/tic_tac_toe/players.py:6-9,
src/reversi/players/reversi_players.py:5-8) and the MCTS player that fills it."""
import random
from abc import ABC, abstractmethod

import numpy as np


class Player(ABC):
    @abstractmethod
    def get_move(self, board):
        pass


class ReversiPlayer(ABC):
    @abstractmethod
    def get_move(self, board):
        pass


class RandomPlayer(Player):  # players.py:25-27
    def get_move(self, board):
        return random.choice(board.generate_possible_moves())


class ReversiRandomPlayer(ReversiPlayer):  # reversi_players.py:26-32
    def __init__(self, symbol):
        self.symbol = symbol

    def get_move(self, board):
        moves = board.generate_possible_moves(self.symbol)
        return random.choice(moves) if moves else (None, None)


class OptimalPlayer(Player):
    """The reference's tic-tac-toe OptimalPlayer (src/tic_tac_toe/players.py:30-70) on the library's
    minimax (bz_ttt_minimax: the host build of the code the arena kernel runs): random opening move on an
    empty board, otherwise the first move with the best full-depth minimax score."""

    def __init__(self, symbol):
        self.symbol = symbol

    def minimax(self, board, is_maximizing=True):
        """(score, move) for `symbol` to move -- the reference's minimax(board, True)"""
        import ctypes as C
        from . import _lib
        assert is_maximizing, "only the root call minimax(board, True) is mirrored"
        own, opp = board.bits(self.symbol)
        mv, sc = C.c_int32(), C.c_int32()
        _lib.check(_lib.lib().bz_ttt_minimax(own, opp, self.symbol, C.byref(mv), C.byref(sc)))
        return sc.value, (None if mv.value < 0 else (mv.value // 3, mv.value % 3))

    def get_move(self, board):
        moves = board.generate_possible_moves()
        if len(moves) == 9:
            return random.choice(moves)
        return self.minimax(board, True)[1]


class ReversiOptimalPlayer(ReversiPlayer):
    """The reference's Reversi OptimalPlayer (src/reversi/players/reversi_players.py:35-77): depth-limited
    minimax on the stone difference, no pass rule inside the search, random.choice when no move scores above
    -inf -- on bz_reversi_minimax.  Any max_depth >= 0, like the reference's recursion (the scalar entry point keeps a
    stack of 60 frames -- no line of play is longer; only the BATCHED kernel of the arena is limited to depth 8)."""

    def __init__(self, symbol, max_depth=4):
        if int(max_depth) < 0:
            raise ValueError(f"ReversiOptimalPlayer: max_depth must be >= 0 (got {max_depth})")
        self.symbol, self.max_depth = symbol, int(max_depth)

    def minimax(self, board, is_maximizing=True, depth=0):
        import ctypes as C
        from . import _lib
        assert is_maximizing and depth == 0, "only the root call minimax(board, True, 0) is mirrored"
        own, opp = board.bits(self.symbol)
        mv, sc = C.c_int32(), C.c_int32()
        _lib.check(_lib.lib().bz_reversi_minimax(own, opp, board.size, self.max_depth, C.byref(mv), C.byref(sc)))
        score = float("inf") if sc.value >= 1000 else (float("-inf") if sc.value <= -1000 else sc.value)
        return score, (None if mv.value < 0 else (mv.value // 8, mv.value % 8))

    def get_move(self, board):
        _, best_move = self.minimax(board, True, 0)
        if best_move is None:
            return random.choice(board.generate_possible_moves(self.symbol))
        return best_move


class NetPlayer(ReversiPlayer):
    """The net-only player: AIPlayer.get_move (src/tic_tac_toe/players.py:84-98) for Reversi (8x8, or the reference's
    6x6 / 4x4 boards in the top-left corner of the 8x8 planes) and the conv
    policy/value net -- canonicalise the position for the side to move (:85), one forward (:86), play the best LEGAL
    move in descending-logit order (:92-98; ties -> lowest action, where torch.sort leaves them unspecified)."""

    def __init__(self, symbol, net, precision="bf16"):
        self.symbol, self.net, self.precision = symbol, net, precision
        self.last_logits = None

    def get_move(self, board):
        import torch
        own, opp = board.bits(self.symbol)
        o = torch.as_tensor(np.array([own], dtype=np.uint64).view(np.int64)).to(self.net.device)
        p = torch.as_tensor(np.array([opp], dtype=np.uint64).view(np.int64)).to(self.net.device)
        lg, _ = self.net.forward(o, p, bf16=self.precision != "f32", fp8=self.precision == "fp8")
        lg = lg[0, :64].cpu().numpy()
        self.last_logits = lg
        moves = board.generate_possible_moves(self.symbol)
        if not moves:
            return (None, None)
        idx = np.array([8 * r + c for r, c in moves])
        best = idx[np.argmax(lg[idx])]  # generate_possible_moves is row-major: the first maximum is the lowest action
        return int(best) // 8, int(best) % 8


class AIPlayer(Player):
    """The reference's AIPlayer (src/tic_tac_toe/players.py:76-104) on the device MLP: AIPlayer(path_to_model, symbol)
    loads the reference's checkpoint (mlp.load_reference_model: weights_only=True, never a pickle's code); path_to_model
    may also be a TicTacToeNet, a TicTacToePVNet (its logits alone are used) or a DeviceMLP.  get_move runs one forward of symbol * board and plays the best LEGAL move
    in descending-logit order; ties go to the lowest cell (torch.sort leaves their order unspecified).  Unlike the
    reference it prints nothing (its three debug print lines, :100-102); the logits of the last call are in last_logits.
    precision: "f32" (parity) or "bf16" (MFMA)."""

    def __init__(self, path_to_model, symbol, precision="f32", device="cuda:0"):
        import torch.nn as nn
        from .mlp import DeviceMLP, load_reference_model
        if precision not in ("f32", "bf16"):
            raise ValueError("AIPlayer: precision is 'f32' or 'bf16'")
        if isinstance(path_to_model, DeviceMLP):
            self.net = path_to_model
        else:
            mod = path_to_model if isinstance(path_to_model, nn.Module) else load_reference_model(path_to_model)
            self.net = DeviceMLP.from_module(mod, max_batch=16, device=device)
        self.symbol, self.precision = symbol, precision
        self.last_logits = None

    def get_move(self, board):
        x = self.symbol * np.asarray(board.board, dtype=np.float32).reshape(1, 9)
        lg = self.net.forward_states(x, bf16=self.precision == "bf16")[0].cpu().numpy()
        self.last_logits = lg
        moves = board.generate_possible_moves()
        idx = np.array([3 * r + c for r, c in moves])
        best = int(idx[np.argmax(lg[idx])])  # moves are row-major: the first maximum is the lowest cell
        return best // 3, best % 3


class MCTSPlayer(Player):
    """get_move(board) -> (row, col) by one GPU search (PUCT, `sims` simulations)
    from `board` with `symbol` to move; plays argmax visit count (ties -> lowest
    action).  Works for TicTacToeBoard and 8x8 ReversiBoard; evaluator "net_bf16"
    / "net_f32" need a betazero_amd.net.DeviceNet (Reversi, any of the reference's board sizes); "mlp_f32" (the default
    with a betazero_amd.mlp.DeviceMLP) / "mlp_bf16" the reference's tic-tac-toe MLP (policy only: leaf value 0; a
    DeviceMLP of a TicTacToePVNet gives the leaves its own value).
    gumbel (True or an engine.GumbelConfig): Gumbel root search -- the move is the one the Gumbel search
    plays (SelfPlayEngine.root_policy) and last_policy its improved policy; the player draws no Gumbel noise (temp_moves 0),
    so it is deterministic.  eval_symmetry (True or a symmetry.EvalSymmetry): every leaf is evaluated under a hashed board
    symmetry (True: seed 0); net evaluators on Reversi only.  fpu (True or an engine.Fpu): first-play urgency
    reduction in the select rule; not with gumbel or leaves_per_step > 1.  GumbelConfig(interior="gumbel"):
    the Gumbel interior rule below the root instead of PUCT.  solver=True: the search books proven wins,
    losses and draws and the move is the solver's (SelfPlayEngine.root_policy): the lowest proven win, never
    a proven loss while another move is left; last_proven is then the root's proven value for the mover or None; not with
    gumbel, fpu or leaves_per_step > 1.  early_stop (True or an engine.EarlyStop): the search stops once the simulations left
    cannot change the move -- the move is the full search's; last_sims is then the number of simulations the
    last search ran and last_visits the visits of the shortened tree; not with gumbel, solver or leaves_per_step > 1."""

    def __init__(self, symbol, sims=800, net=None, evaluator=None, c_puct=1.5, device="cuda:0", leaves_per_step=1,
                 gumbel=None, eval_symmetry=None, fpu=None, solver=False, early_stop=None):
        from .engine import check_early_stop, check_fpu, check_gumbel, check_leaves_per_step, check_sims, check_solver
        check_sims(sims)  # a ValueError naming the limit here, not a RuntimeError at the first get_move
        self.leaves_per_step = check_leaves_per_step(leaves_per_step)  # K walks per tree step
        self.gumbel = check_gumbel(gumbel, leaves_per_step=self.leaves_per_step)
        self.fpu = check_fpu(fpu, leaves_per_step=self.leaves_per_step, gumbel=self.gumbel)
        self.solver = check_solver(solver, leaves_per_step=self.leaves_per_step, gumbel=self.gumbel, fpu=self.fpu)
        self.last_proven = None  # solver mode: the root's proven value of the last search (-1, 0, +1) or None
        self.early_stop = check_early_stop(early_stop, leaves_per_step=self.leaves_per_step, gumbel=self.gumbel, solver=self.solver)
        self.last_sims = None  # early stop: the simulations the last search ran (<= sims)
        self.symbol, self.sims, self.net, self.c_puct, self.device = symbol, sims, net, c_puct, device
        # evaluator: "uniform" | "hash" | "net_bf16" | "net_f32" | "net_fp8", or a callable (own, opp, kind) -> (logits, value)
        # on CUDA tensors (SelfPlayEngine.search_external): any torch module, e.g. an MLP for tic-tac-toe
        self.eval_fn = evaluator if callable(evaluator) else None
        if self.eval_fn is not None:
            evaluator = "external"
        from .mlp import DeviceMLP
        self._mlp = isinstance(net, DeviceMLP)
        self.evaluator = evaluator or (("mlp_f32" if self._mlp else "net_bf16") if net is not None else "uniform")
        from .symmetry import check_eval_symmetry
        self.eval_symmetry = check_eval_symmetry(eval_symmetry, 0, None, self.evaluator)
        self._eng = {}
        self.last_visits = None
        self.last_policy = None  # Gumbel mode: the improved policy of the last search, float32 [NA]

    def _engine(self, game):
        from .engine import SelfPlayEngine
        if game not in self._eng:
            self._eng[game] = SelfPlayEngine(game, 1, self.sims, self.evaluator, self.net, self.c_puct,
                                             device=self.device, leaves_per_step=self.leaves_per_step, gumbel=self.gumbel,
                                             eval_symmetry=self.eval_symmetry, fpu=self.fpu, solver=self.solver,
                                             early_stop=self.early_stop)
        return self._eng[game]

    def get_move(self, board):
        if hasattr(board, "size") and board.size not in (8, 6, 4):
            raise ValueError(f"the search engine plays Reversi on 8x8, 6x6 and 4x4 boards, not {board.size}x{board.size} "
                             "(the rule calls of ReversiBoard cover every size)")
        game = {8: "reversi", 6: "reversi6", 4: "reversi4"}[board.size] if hasattr(board, "size") else "ttt"
        if game == "ttt" and self.evaluator.startswith("net"):
            raise ValueError("the conv net evaluators serve the Reversi boards; use evaluator='uniform' or 'hash' for tic-tac-toe")
        if game != "ttt" and (self._mlp or self.evaluator.startswith("mlp")):
            raise ValueError("the MLP (DeviceMLP, evaluators 'mlp_f32' / 'mlp_bf16') serves tic-tac-toe, not Reversi")
        own, opp = board.bits(self.symbol)
        eng = self._engine(game)
        eng.set_roots([own], [opp], [self.symbol])
        if self.eval_fn is not None:
            eng.search_external(self.eval_fn)
        else:
            eng.search()
        N, _, _ = eng.root_stats()
        eng.status()  # raises on engine error flags (e.g. terminal root)
        self.last_visits = N[0]
        if self.solver:
            self.last_proven = eng.proven()[0][0]
        if self.early_stop is not None:
            self.last_sims = int(eng.stopped()[0])
        if self.gumbel is not None or self.solver:
            pi, act = eng.root_policy()
            self.last_policy = pi[0]
            a = int(act[0])
            if a < 0 or a == 64:
                return (None, None)  # mover has no move (reversi_players.py:32)
            n = 3 if game == "ttt" else 8
            return a // n, a % n
        a = int(np.argmax(N[0]))  # first maximum = lowest action
        if N[0][a] == 0 or a == 64:
            return (None, None)  # mover has no move (reversi_players.py:32)
        n = 3 if game == "ttt" else 8
        return a // n, a % n
