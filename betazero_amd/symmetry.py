"""Evaluation under a hashed board symmetry: the option type, its checks, and the host view of the
symmetry tables the net kernels use (bz_sym_index / bz_sym_board / bz_sym_action_map).

AlphaGo Zero and KataGo evaluate every search leaf under a randomly chosen dihedral symmetry, because a conv net is
not equivariant and its orientation bias would otherwise go straight into every prior and value of the tree.  Here the
symmetry of a position is a hash of (position, seed): the evaluator stays a function of the position alone, so the
evaluation cache, its carry-over and every bit-for-bit statement of the engine keep holding."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib

SYM_FIXED, SYM_HASHED, SYM_MEAN = 0, 1, 2  # BZ_SYM_* (include/bz_abi.h)
N_SYM = 8
# 0..6 = bz_augment_d4_batch's transforms 0..6; 7 = the anti-transpose, which the reference's list lacks
SYM_NAMES = ("id", "flip_rows", "flip_cols", "rot90", "rot180", "rot270", "transpose", "anti_transpose")
SYM_INVERSE = (0, 1, 2, 5, 4, 3, 6, 7)
_NET_EVALUATORS = ("net_f32", "net_bf16", "net_fp8")
_SIZES = {"reversi": 8, "reversi8": 8, "reversi6": 6, "reversi4": 4, _lib.GAME_REVERSI: 8, _lib.GAME_REVERSI6: 6,
          _lib.GAME_REVERSI4: 4}


@dataclass(frozen=True)
class EvalSymmetry:
    """Evaluate every search leaf under the symmetry bz_sym_index(seed, own, opp) of its own position.  seed: an int in
    0 .. 2^64 - 1; another seed is another assignment of orientations to positions."""
    seed: int = 0


def check_eval_symmetry(eval_symmetry, seed=0, game=None, evaluator=None):
    """None / False: off (None returned); True: EvalSymmetry(seed = the engine's seed); or an EvalSymmetry -- validated,
    and refused on tic-tac-toe and with the synthetic, external and MLP evaluators (ValueError, before any device is
    touched).  game / evaluator None: not checked (the caller has neither yet)."""
    if eval_symmetry is None or eval_symmetry is False:
        return None
    es = EvalSymmetry(seed) if eval_symmetry is True else eval_symmetry
    if not isinstance(es, EvalSymmetry):
        raise ValueError(f"eval_symmetry must be None, False, True or an EvalSymmetry (got {eval_symmetry!r})")
    s = es.seed
    if isinstance(s, bool) or not isinstance(s, (int, np.integer)) or not 0 <= int(s) < 2 ** 64:
        raise ValueError(f"eval_symmetry: seed must be an int in 0 .. 2^64 - 1 (got {s!r})")
    if game is not None and game not in _SIZES:
        raise ValueError(f"eval_symmetry: the evaluation symmetry serves the Reversi boards (got game {game!r})")
    if evaluator is not None and evaluator not in _NET_EVALUATORS:
        raise ValueError(f"eval_symmetry: the evaluation symmetry serves the net_f32 / net_bf16 / net_fp8 evaluators "
                         f"(got evaluator {evaluator!r})")
    return EvalSymmetry(int(s))


def check_forward_symmetry(symmetry, size=8, seed=0):
    """DeviceNet.forward's `symmetry`: None (plain), an int 0..7 (FIXED), "hash" (HASHED with `seed`) or "mean" ->
    None or (mode, arg); ValueError for anything else, before any device is touched"""
    if size not in (8, 6, 4):
        raise ValueError(f"size must be 8, 6 or 4 (got {size!r})")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) < 2 ** 64:
        raise ValueError(f"seed must be an int in 0 .. 2^64 - 1 (got {seed!r})")
    if symmetry is None:
        return None
    if isinstance(symmetry, str):
        if symmetry == "hash":
            return SYM_HASHED, int(seed)
        if symmetry == "mean":
            return SYM_MEAN, 0
    elif not isinstance(symmetry, bool) and isinstance(symmetry, (int, np.integer)) and 0 <= int(symmetry) < N_SYM:
        return SYM_FIXED, int(symmetry)
    raise ValueError(f'symmetry must be None, an int in 0..7, "hash" or "mean" (got {symmetry!r})')


def sym_index(seed, own, opp):
    """the symmetry 0..7 a position is evaluated under for `seed` (host, per item; needs no GPU)"""
    return int(_lib.lib().bz_sym_index(int(seed), int(own), int(opp)))


def sym_board(b, size, s):
    """T_s(b): the bitboard with its size x size corner transformed (host, per item; needs no GPU)"""
    out = C.c_uint64()
    _lib.check(_lib.lib().bz_sym_board(int(b), int(size), int(s), C.byref(out)))
    return int(out.value)


def sym_action_map(size, s):
    """tau_s as uint8 [65]: a stone on cell j moves to map[j]; cells outside the corner and the pass action stay"""
    m = np.zeros(65, np.uint8)
    _lib.check(_lib.lib().bz_sym_action_map(int(size), int(s), m.ctypes.data))
    return m
