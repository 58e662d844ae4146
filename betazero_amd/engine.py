"""SelfPlayEngine: torch-owned workspace + the bz_engine C ABI (batched MCTS
self-play on one GPU), and self_play(), the batched counterpart of the
reference's data-generation loop (SL/generate_training_games.py:25-38)."""
import ctypes as C
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from .symmetry import EvalSymmetry, check_eval_symmetry  # noqa: F401  (EvalSymmetry: re-exported next to the other options)
from ._lib import (EVAL_EXTERNAL, EVAL_HASH, EVAL_NET_BF16, EVAL_NET_F32, EVAL_NET_FP8, EVAL_UNIFORM, GAME_REVERSI,  # noqa: F401
                   GAME_REVERSI4, GAME_REVERSI6, GAME_TTT, EngineCfg, EngineLayout)
# the row types and the block code live in betazero_amd.examples; their names stay importable from here
from .examples import (_EX_FIELDS, _GAMES, _PK_FIELDS, _SIZES, COLUMN, EX_MAGIC, PACKED_MAGIC, DeviceExamples, Examples,  # noqa: F401
                       _packed_views, _u64, alloc_packed_block, build_example_block, build_packed_block, concat_device_examples,
                       concat_examples, example_block_views, packed_block_header, packed_layout, unpack_example_block,
                       unpack_example_block_device, unpack_packed_block, unpack_packed_block_device)

_EVALS = {"uniform": EVAL_UNIFORM, "hash": EVAL_HASH, "net_f32": EVAL_NET_F32, "net_bf16": EVAL_NET_BF16,
          "external": EVAL_EXTERNAL, "net_fp8": EVAL_NET_FP8,
          # the reference's tic-tac-toe MLP (betazero_amd.mlp.DeviceMLP as `net`): policy logits; value 0, or the net's own with a value head
          "mlp_f32": _lib.EVAL_MLP_F32, "mlp_bf16": _lib.EVAL_MLP_BF16}


_EVAL_NAMES = {v: k for k, v in _EVALS.items()}

MAX_SIMS, MAX_SIMS_REUSE = 8189, 2045  # BZ_ENGINE_MAX_SIMS / BZ_ENGINE_MAX_SIMS_REUSE (include/bz_abi.h)


def check_sims(sims, reuse_subtree=False):
    """the packed edge record holds node ids in 13 bits: refuse larger searches where they are asked for"""
    lim = MAX_SIMS_REUSE if reuse_subtree else MAX_SIMS
    if not 1 <= int(sims) <= lim:
        raise ValueError(f"sims must be in 1..{lim}" + (" with subtree reuse" if reuse_subtree else "") +
                         f" (got {sims}): the tree's packed edge record holds at most 8191 nodes per game "
                         "(BZ_ENGINE_MAX_SIMS / BZ_ENGINE_MAX_SIMS_REUSE in include/bz_abi.h)")


MAX_LEAVES_PER_STEP = 32  # the 5-bit BZ_ENGINE_LEAVES_* field of cfg.flags (include/bz_abi.h)


def check_leaves_per_step(leaves_per_step):
    """leaf-parallel search: K walks per game per tree step, an int in 1..32 (bool refused)"""
    k = leaves_per_step
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= MAX_LEAVES_PER_STEP:
        raise ValueError(f"leaves_per_step must be an int in 1..{MAX_LEAVES_PER_STEP} (got {k!r})")
    return int(k)


EVAL_CACHE_MODES = (True, "carry", "search", False, None)


def check_eval_cache(eval_cache):
    """True / "carry": the evaluation cache with carry-over; "search": within a search only; False / None: off.  Anything
    else (a misspelt mode such as "off" is truthy) is refused with ValueError, before any device is touched."""
    if not any(eval_cache is m or (isinstance(m, str) and isinstance(eval_cache, str) and eval_cache == m)
               for m in EVAL_CACHE_MODES):
        raise ValueError(f"eval_cache must be one of True, 'carry', 'search', False, None (got {eval_cache!r})")
    return eval_cache


ROOT_STORE_DEFAULT = (256, 3)  # (entries, plies) of the root store an engine with the carry-over cache gets


def check_root_store(root_store, eval_cache=True):
    """None: ROOT_STORE_DEFAULT with eval_cache True / "carry", else off; False: off; (entries, plies): 1 <= entries <= 65536,
    1 <= plies <= 64.  Returns the pair or None; anything else is refused with ValueError, before any device is touched."""
    carry = eval_cache is True or (isinstance(eval_cache, str) and eval_cache == "carry")
    if root_store is None:
        return ROOT_STORE_DEFAULT if carry else None
    if root_store is False:
        return None
    ok = (isinstance(root_store, (tuple, list)) and len(root_store) == 2 and
          all(isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) for v in root_store) and
          1 <= root_store[0] <= 65536 and 1 <= root_store[1] <= 64)
    if not ok:
        raise ValueError(f"root_store must be None, False or (entries in 1..65536, plies in 1..64) (got {root_store!r})")
    return (int(root_store[0]), int(root_store[1])) if carry else None


MAX_CONSIDERED = 64  # BZ_GUMBEL_MAX_CONSIDERED (include/bz_abi.h)

# ---- The search options and THE table of the pairs that do not run together ("The search mode"), under
# SelfPlayEngine's keyword names: the rows of BZ_OPT_* / kOptions and the pairs of kConflicts (csrc/bz_options.h), in their
# order -- kept here as well because these messages name keywords, not setters, and because the checks run before the library
# or a device is touched (argument parsers call them).  tests/test_option_conflicts_cpu.py holds the two tables equal.
SEARCH_OPTIONS = {  # keyword: the phrase the messages use
    "reuse_subtree": "subtree reuse", "leaves_per_step": "leaves_per_step > 1", "dirichlet_eps": "Dirichlet noise",
    "gumbel": "Gumbel root search", "gumbel_interior": "the Gumbel interior rule",  # (GumbelConfig.interior == "gumbel")
    "playout_cap": "playout cap randomisation", "forced_playouts": "forced playouts", "fpu": "first-play urgency reduction",
    "solver": "the solver", "early_stop": "early stop", "root_store": "the root store", "surprise": "policy surprise weighting",
    "search_value": "search-value targets", "ownership": "ownership targets", "resign": "resignation"}
SEARCH_OPTION_CONFLICTS = (  # (keyword, keyword, reason or None): each pair once, in either order
    *(("reuse_subtree", o, None) for o in ("gumbel", "playout_cap", "forced_playouts", "fpu", "solver", "early_stop")),
    *(("leaves_per_step", o, None) for o in ("gumbel", "playout_cap", "forced_playouts", "fpu")),
    ("leaves_per_step", "solver", "concurrent walks race on proofs"), ("leaves_per_step", "early_stop", None),
    ("dirichlet_eps", "gumbel", None),
    *(("gumbel", o, None) for o in ("playout_cap", "forced_playouts", "fpu", "solver")),
    ("gumbel", "early_stop", "sequential halving is its own schedule"),
    ("solver", "forced_playouts", "both score +inf"), ("solver", "fpu", None), ("solver", "early_stop", None),
    ("early_stop", "playout_cap", None), ("early_stop", "forced_playouts", None),
    ("early_stop", "root_store", "a shortened tree must not seed a later search"),
    *(("early_stop", o, "its targets come from complete searches") for o in ("surprise", "search_value", "ownership")),
    ("early_stop", "resign", "its records come from complete searches"),
    ("ownership", "resign", "a resigned game has no final board"))


def _option_on(name, value):
    if name == "leaves_per_step":
        return value != 1
    if name == "dirichlet_eps":
        return value > 0
    return bool(value) if name == "reuse_subtree" else value is not None and value is not False


def refuse_option_conflict(name, others):
    """ValueError for the first pair of SEARCH_OPTION_CONFLICTS that option `name` makes with an option that is on in `others`,
    {keyword: value} (an option it does not name is off); before any device is touched"""
    for a, b, reason in SEARCH_OPTION_CONFLICTS:
        other = b if a == name else a if b == name else None
        if other in others and _option_on(other, others[other]):
            p = SEARCH_OPTIONS[name]
            raise ValueError(f"{name}: {p} {'do' if p.endswith('s') else 'does'} not combine with {SEARCH_OPTIONS[other]} ({other})" +
                             (f": {reason}" if reason else ""))


def check_replay_seed(replay_seed):
    """None (by the engine's size), True or False; anything else is refused (ValueError, before any device is touched)"""
    if replay_seed is None:
        return None
    if not isinstance(replay_seed, (bool, np.bool_)):
        raise ValueError(f"replay_seed must be None, True or False (got {replay_seed!r})")
    return bool(replay_seed)


@dataclass(frozen=True)
class GumbelConfig:
    """Gumbel root search (Danihelka et al., ICLR 2022).  The defaults are those of mctx's
    gumbel_muzero_policy: max_considered root actions (1..64) for the sequential halving, the Gumbel noise scale (0: no
    noise), and sigma's maxvisit_init / value_scale.  interior: the select rule below the root -- "puct" (the default: PUCT
    with c_puct, an unvisited child worth 0) or "gumbel" (the paper's interior rule, the action whose visit
    share lags the node's improved policy softmax(log P + sigma(completed Q)) the most; no c_puct, no noise)."""
    max_considered: int = 16
    scale: float = 1.0
    maxvisit_init: float = 50.0
    value_scale: float = 0.1
    interior: str = "puct"


GUMBEL_INTERIORS = ("puct", "gumbel")


def check_gumbel(gumbel, reuse_subtree=False, leaves_per_step=1, dirichlet_eps=0.0):
    """None / False: off (None returned); True: GumbelConfig(); or a GumbelConfig -- validated, and refused against the other
    options named (SEARCH_OPTION_CONFLICTS; ValueError, before any device is touched)"""
    if gumbel is None or gumbel is False:
        return None
    cfg = GumbelConfig() if gumbel is True else gumbel
    if not isinstance(cfg, GumbelConfig):
        raise ValueError(f"gumbel must be None, False, True or a GumbelConfig (got {gumbel!r})")
    m = cfg.max_considered
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or not 1 <= int(m) <= MAX_CONSIDERED:
        raise ValueError(f"gumbel: max_considered must be an int in 1..{MAX_CONSIDERED} (got {m!r})")
    for name in ("scale", "maxvisit_init", "value_scale"):
        x = getattr(cfg, name)
        if isinstance(x, bool) or not isinstance(x, (int, float, np.integer, np.floating)) or not np.isfinite(x) or x < 0:
            raise ValueError(f"gumbel: {name} must be a finite number >= 0 (got {x!r})")
    if not isinstance(cfg.interior, str) or cfg.interior not in GUMBEL_INTERIORS:
        raise ValueError(f"gumbel: interior must be 'puct' or 'gumbel' (got {cfg.interior!r})")
    refuse_option_conflict("gumbel", dict(reuse_subtree=reuse_subtree, leaves_per_step=leaves_per_step, dirichlet_eps=dirichlet_eps))
    return GumbelConfig(int(m), float(cfg.scale), float(cfg.maxvisit_init), float(cfg.value_scale), str(cfg.interior))


@dataclass(frozen=True)
class PlayoutCap:
    """Playout cap randomisation (KataGo, Wu 2019, section 3.1): before every move a game draws a full
    search (`sims` simulations, probability full_prob, records its example row) or a fast one (`fast_sims` simulations,
    only plays its move).  1 <= fast_sims < sims; full_prob in [0, 1], applied in units of 2^-16."""
    fast_sims: int
    full_prob: float = 0.25

    @property
    def full_q(self):
        """the probability of a full search in units of 2^-16 (what the engine compares 16 random bits with)"""
        return int(round(float(self.full_prob) * 65536))


def check_playout_cap(playout_cap, sims=None, reuse_subtree=False, leaves_per_step=1, gumbel=None):
    """None / False: off (None returned); or a PlayoutCap -- validated, and refused against the other options named
    (SEARCH_OPTION_CONFLICTS; ValueError, before any device is touched)"""
    if playout_cap is None or playout_cap is False:
        return None
    cap = playout_cap
    if not isinstance(cap, PlayoutCap):
        raise ValueError(f"playout_cap must be None, False or a PlayoutCap (got {playout_cap!r})")
    n = cap.fast_sims
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1 or (sims is not None and n >= int(sims)):
        raise ValueError(f"playout_cap: fast_sims must be an int in 1..sims - 1 (got {n!r}" +
                         (f", sims = {sims})" if sims is not None else ")"))
    p = cap.full_prob
    if isinstance(p, bool) or not isinstance(p, (int, float, np.integer, np.floating)) or not 0.0 <= p <= 1.0:  # (NaN fails)
        raise ValueError(f"playout_cap: full_prob must be a number in [0, 1] (got {p!r})")
    refuse_option_conflict("playout_cap", dict(reuse_subtree=reuse_subtree, leaves_per_step=leaves_per_step, gumbel=gumbel))
    return PlayoutCap(int(n), float(p))


@dataclass(frozen=True)
class Resign:
    """Resignation in self-play (AlphaGo Zero): a side whose root value q = sum W / sum N stayed below
    `threshold` (strict, float32) for `consecutive` full searches in a row (1..255) resigns -- the game ends there, the other
    side wins, the firing search records no row.  A seeded share `playout_frac` of the games (applied in units of 2^-16,
    drawn per global game id) never resigns and only records where it would have: their real outcomes give the
    false-positive rate (SelfPlayEngine.resign_stats)."""
    threshold: float = -0.9
    consecutive: int = 2
    playout_frac: float = 0.1

    @property
    def playout_q(self):
        """the share of played-out games in units of 2^-16 (what the engine compares 16 random bits with)"""
        return int(round(float(self.playout_frac) * 65536))


def check_resign(resign, ownership=False):
    """None / False: off (None returned); True: Resign(); or a Resign -- validated in float32, and refused against the other
    option named (SEARCH_OPTION_CONFLICTS; ValueError, before any device is touched)"""
    if resign is None or resign is False:
        return None
    cfg = Resign() if resign is True else resign
    if not isinstance(cfg, Resign):
        raise ValueError(f"resign must be None, False, True or a Resign (got {resign!r})")
    t = cfg.threshold
    with np.errstate(over="ignore", under="ignore"):
        ok = not isinstance(t, (bool, np.bool_)) and isinstance(t, (int, float, np.integer, np.floating))
        t32 = float(np.float32(t)) if ok else 2.0
    if not -1.0 <= t32 <= 1.0:  # (NaN fails)
        raise ValueError(f"resign: threshold must be a finite number in [-1, 1] in float32 (got {t!r})")
    n = cfg.consecutive
    if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) <= 255:
        raise ValueError(f"resign: consecutive must be an int in 1..255 (got {n!r})")
    f = cfg.playout_frac
    if isinstance(f, (bool, np.bool_)) or not isinstance(f, (int, float, np.integer, np.floating)) or not 0.0 <= f <= 1.0:  # (NaN fails)
        raise ValueError(f"resign: playout_frac must be a number in [0, 1] (got {f!r})")
    refuse_option_conflict("resign", dict(ownership=ownership))
    return Resign(t32, int(n), float(f))


def resign_stats(side, played_out, winner, length):
    """the calibration figures of DESIGN.md 3.24 from resign_rows() and winners(): arrays of one shape, one element per game
    (length < 0: the game is not finished).  A false positive is a finished played-out game with a record whose recorded
    side did not lose -- it won or drew."""
    side, out, winner = np.asarray(side), np.asarray(played_out).astype(bool), np.asarray(winner)
    fin = np.asarray(length) >= 0
    would = fin & out & (side != 0)
    fp = would & (winner.astype(np.int64) != -side.astype(np.int64))
    n_would, n_fp = int(would.sum()), int(fp.sum())
    return {"n_finished": int(fin.sum()), "n_resigned": int((fin & ~out & (side != 0)).sum()), "n_played_out": int((fin & out).sum()),
            "n_would_resign": n_would, "n_false_positive": n_fp, "false_positive_rate": n_fp / n_would if n_would else None}


def _sum_resign_stats(parts):
    tot = {k: sum(p[k] for p in parts) for k in ("n_finished", "n_resigned", "n_played_out", "n_would_resign", "n_false_positive")}
    tot["false_positive_rate"] = tot["n_false_positive"] / tot["n_would_resign"] if tot["n_would_resign"] else None
    return tot


@dataclass(frozen=True)
class ForcedPlayouts:
    """Forced playouts and policy target pruning (KataGo, Wu 2019, section 3.2): every visited root child
    is searched until it has sqrt(k P sum N) visits (P the prior after the Dirichlet noise); the recorded pi then drops
    the visits PUCT would not have made on its own (prune=True) or stays N / sum N (prune=False).  k > 0, finite."""
    k: float = 2.0
    prune: bool = True


def check_forced_playouts(forced_playouts, reuse_subtree=False, leaves_per_step=1, gumbel=None):
    """None / False: off (None returned); True: ForcedPlayouts(); or a ForcedPlayouts -- validated, and refused against the other
    options named (SEARCH_OPTION_CONFLICTS; ValueError, before any device is touched)"""
    if forced_playouts is None or forced_playouts is False:
        return None
    fp = ForcedPlayouts() if forced_playouts is True else forced_playouts
    if not isinstance(fp, ForcedPlayouts):
        raise ValueError(f"forced_playouts must be None, False, True or a ForcedPlayouts (got {forced_playouts!r})")
    k = fp.k
    with np.errstate(over="ignore", under="ignore"):
        k32 = float(np.float32(k)) if not isinstance(k, bool) and isinstance(k, (int, float, np.integer, np.floating)) else 0.0
    if not 0.0 < k32 < np.inf:
        raise ValueError(f"forced_playouts: k must be a finite number > 0 in float32 (got {k!r})")  # (NaN fails)
    if not isinstance(fp.prune, (bool, np.bool_)):
        raise ValueError(f"forced_playouts: prune must be a bool (got {fp.prune!r})")
    refuse_option_conflict("forced_playouts", dict(reuse_subtree=reuse_subtree, leaves_per_step=leaves_per_step, gumbel=gumbel))
    return ForcedPlayouts(float(k), bool(fp.prune))


@dataclass(frozen=True)
class Fpu:
    """First-play urgency reduction (Leela Zero, LC0, KataGo): the select rule scores a child that was never
    visited with its parent's value minus reduction * sqrt(prior mass of the visited children) instead of with 0;
    root_reduction is the reduction at the root.  Both finite and >= 0 (KataGo's fpuReductionMax / rootFpuReductionMax)."""
    reduction: float = 0.2
    root_reduction: float = 0.1


def check_fpu(fpu, reuse_subtree=False, leaves_per_step=1, gumbel=None):
    """None / False: off (None returned); True: Fpu(); or an Fpu -- validated, and refused against the other options named
    (SEARCH_OPTION_CONFLICTS; ValueError, before any device is touched)"""
    if fpu is None or fpu is False:
        return None
    cfg = Fpu() if fpu is True else fpu
    if not isinstance(cfg, Fpu):
        raise ValueError(f"fpu must be None, False, True or an Fpu (got {fpu!r})")
    out = []
    for name in ("reduction", "root_reduction"):
        x = getattr(cfg, name)
        with np.errstate(over="ignore", under="ignore"):
            ok = not isinstance(x, (bool, np.bool_)) and isinstance(x, (int, float, np.integer, np.floating))
            x32 = float(np.float32(x)) if ok else -1.0
        if not 0.0 <= x32 < np.inf:  # (NaN fails)
            raise ValueError(f"fpu: {name} must be a finite number >= 0 in float32 (got {x!r})")
        out.append(x32)
    refuse_option_conflict("fpu", dict(reuse_subtree=reuse_subtree, leaves_per_step=leaves_per_step, gumbel=gumbel))
    return Fpu(*out)


def check_solver(solver, reuse_subtree=False, leaves_per_step=1, gumbel=None, forced_playouts=None, fpu=None):
    """proven wins, losses and draws: a bool; True is refused against the other options named
    (SEARCH_OPTION_CONFLICTS; ValueError, before any device is touched)"""
    if solver is None:
        return False
    if not isinstance(solver, (bool, np.bool_)):
        raise ValueError(f"solver must be a bool (got {solver!r})")
    if not solver:
        return False
    refuse_option_conflict("solver", dict(reuse_subtree=reuse_subtree, leaves_per_step=leaves_per_step, gumbel=gumbel,
                                          forced_playouts=forced_playouts, fpu=fpu))
    return True


@dataclass(frozen=True)
class EarlyStop:
    """Exact early stop (Huang, Coulom and Lin 2010; Baier and Winands 2012; LC0's "smart pruning" without its
    slack): a search whose move is the first maximum of the root's visits stops at the first simulation index at which the
    simulations left can no longer change that move.  The move is the full search's, always.  host_exit: the host also stops
    issuing the tree steps of an engine once none of its slots walks any more (same results, fewer empty launches)."""
    host_exit: bool = True


def check_early_stop(early_stop, reuse_subtree=False, leaves_per_step=1, gumbel=None, playout_cap=None, forced_playouts=None,
                     solver=False, root_store=None, surprise=False, search_value=False, ownership=False, resign=None):
    """None / False: off (None returned); True: EarlyStop(); or an EarlyStop -- validated, and refused against the other options
    named (SEARCH_OPTION_CONFLICTS; root_store: the checked value, a pair or None; ValueError, before any device is touched)"""
    if early_stop is None or early_stop is False:
        return None
    cfg = EarlyStop() if early_stop is True else early_stop
    if not isinstance(cfg, EarlyStop):
        raise ValueError(f"early_stop must be None, False, True or an EarlyStop (got {early_stop!r})")
    if not isinstance(cfg.host_exit, (bool, np.bool_)):
        raise ValueError(f"early_stop: host_exit must be a bool (got {cfg.host_exit!r})")
    refuse_option_conflict("early_stop", dict(
        reuse_subtree=reuse_subtree, leaves_per_step=leaves_per_step, gumbel=gumbel, playout_cap=playout_cap,
        forced_playouts=forced_playouts, solver=solver, root_store=root_store, surprise=surprise, search_value=search_value,
        ownership=ownership, resign=resign))
    return EarlyStop(bool(cfg.host_exit))


def check_search_value(search_value):
    """search-value targets: a bool, anything else is refused (ValueError, before any device is touched)"""
    if not isinstance(search_value, (bool, np.bool_)):
        raise ValueError(f"search_value must be a bool (got {search_value!r})")
    return bool(search_value)


def check_ownership(ownership):
    """ownership targets: a bool, anything else is refused (ValueError, before any device is touched)"""
    if not isinstance(ownership, (bool, np.bool_)):
        raise ValueError(f"ownership must be a bool (got {ownership!r})")
    return bool(ownership)


# ---- THE table of the columns an engine records beside its example block, per engine option: (columns, device dtype, pack entry
# point).  SelfPlayEngine._pack_extra / _pack_with_extras and _attach_extras are written against it ("Adding a
# per-row column").
ENGINE_EXTRAS = {"surprise": (("kl",), torch.float32, "bz_engine_pack_surprise"),
                 "search_value": (("q",), torch.float32, "bz_engine_pack_search_value"),
                 "ownership": (("fown", "fopp"), torch.int64, "bz_engine_pack_ownership")}


def _attach_extras(ex, extras):
    """_pack_with_extras' {column: [cap_rows] device tensor} cut to ex's rows and set on ex (host Examples: copied out, in the
    column's host dtype); -> ex"""
    for k, t in extras.items():
        t = t[:len(ex)]
        setattr(ex, k, t if isinstance(ex, DeviceExamples) else t.cpu().numpy().view(COLUMN[k].host))
    return ex


class SelfPlayEngine:
    def __init__(self, game, n_games, sims, evaluator="uniform", net=None, c_puct=1.5, temp_moves=0, openings=0,
                 seed=0, rounds=1, game_id_base=0, game_id_stride=None, device="cuda:0", stagger=0,
                 dirichlet_alpha=0.0, dirichlet_eps=0.0, reuse_subtree=False, ttt_lanes=0, eval_cache=True,
                 leaves_per_step=1, gumbel=None, playout_cap=None, forced_playouts=None, surprise=False, search_value=False,
                 eval_symmetry=None, fpu=None, ownership=False, root_store=None, solver=False, resign=None, early_stop=None,
                 replay_seed=None):
        """eval_cache (BZ_ENGINE_EVAL_CACHE, bz_abi.h): with a net evaluator, a leaf whose position was evaluated earlier in
        the same search shares that evaluation instead of running the net again; True / "carry" (the default) also takes
        evaluations from the slot's PREVIOUS search (BZ_ENGINE_EVAL_CACHE_CARRY: after a move, the played child's old subtree
        is re-created node for node by the new search), "search" only from the same search, False / None none; any other
        value is refused (ValueError, before any device is touched).  Every result is bit
        for bit what it is without the cache (the net is a function of the position); counters()["n_cache_hits"] (of which
        "n_cache_hits_prev" from the previous search) says how often it fired.  Ignored for the synthetic / external
        evaluators, with reuse_subtree and with leaves_per_step > 1.

        leaves_per_step = K (BZ_ENGINE_LEAVES_*): every tree step runs K PUCT walks per game with virtual
        loss, and the evaluator takes up to K x n_games rows per launch; 1 (the default) is the one-walk engine, unchanged.
        counters()["n_collisions"] (K > 1 only) counts the walks that stopped at a node another walk of the same step created.

        gumbel: None / False = PUCT at every node (the default, unchanged); True or a GumbelConfig = Gumbel
        root search: Gumbel-top-k plus sequential halving at the root (PUCT below it), the move is the halving's survivor and
        the example rows' pi is the improved policy.  Gumbel noise is drawn while moves made < temp_moves (and scale > 0).
        GumbelConfig(interior="gumbel") replaces PUCT below the root by the paper's interior rule;
        set_gumbel_interior() changes it between searches.

        playout_cap: None / False = every search has `sims` simulations (the default, unchanged); a
        PlayoutCap(fast_sims, full_prob) = every move draws a full search (sims, records its example row) or a fast one
        (fast_sims, records nothing; Dirichlet noise is drawn on full searches only).  budgets() reads the last search's
        draws.

        forced_playouts: None / False = off (the default, unchanged); True or a ForcedPlayouts(k, prune) =
        forced playouts at the root and, with prune, the pruned policy target in the example rows and in root_policy().  The
        move choice and root_stats() keep the raw visits.  Under playout_cap only the full searches force.

        surprise: False = off (the default, unchanged); True = policy surprise weighting: every recorded
        row also gets kl = KL(pi || the root's raw prior), which examples() / device_examples() then carry as `kl` and
        betazero_amd.surprise.surprise_resample turns into repeat counts.  Searches, moves and rows are what they are
        without it.  surprise_rows() is the unpacked per-row view.

        search_value: False = off (the default, unchanged); True = every recorded row also gets q = the root's
        sum W / sum N of its search (the mover's expected outcome, from the raw visit statistics), which examples() /
        device_examples() then carry as `q` and betazero_amd.value_targets.value_targets turns into value targets.  Searches,
        moves and rows are what they are without it.  search_value_rows() is the unpacked per-row view.

        eval_symmetry: None / False = off (the default, unchanged); True or an EvalSymmetry(seed) = every
        leaf is evaluated under a board symmetry chosen by a hash of (its position, the seed) -- True takes the engine's
        `seed` -- inside the fused net kernels; priors and values come back in the position's own orientation.  The
        evaluator stays a function of the position, so it combines with every search option and the cache stays
        exact; set_eval_symmetry() changes it between searches.  Refused on tic-tac-toe and with the synthetic, external
        and MLP evaluators.

        fpu: None / False = an unvisited child is scored with q = 0 (the default, unchanged); True or an
        Fpu(reduction, root_reduction) = first-play urgency reduction at every level of every walk.  root_stats(), pi, the
        move choice and the rows follow the usual rules on the tree this search builds.  set_fpu() changes it between searches.

        ownership: False = off (the default, unchanged); True = the final board of every finished game is kept
        (ownership_rows()), and examples() / device_examples() carry every row's ownership target `fown`, `fopp`: that board in
        the row's side-to-move frame.  Searches, moves and rows are what they are without it.

        root_store: None = the default for the cache mode -- ROOT_STORE_DEFAULT = (entries, plies) with
        eval_cache True / "carry", off otherwise; False = off; (entries, plies) = a store of that size.  Finished searches of
        roots fewer than `plies` moves behind a game's start are kept, and a slot whose next root is on file starts from that
        tree's evaluations.  Results are unchanged; root_store_counters() says how often it fired.  Ignored where the engine
        does not run the carry-over cache.

        solver: False = off (the default, unchanged); True = the search books proven wins, losses and draws:
        an edge whose child is decided is marked, the mark travels up the path with the backup, the select rule never
        walks through a decided edge, and play() / root_policy() play the lowest winning move and avoid lost ones.  pi stays
        N / sum N.  proven() reads the proof state; set_solver() changes it between searches.

        resign: None / False = every game is played to the end (the default, unchanged); True or a
        Resign(threshold, consecutive, playout_frac) = a side whose root value stayed below the threshold for `consecutive`
        full searches in a row resigns; a seeded share of the games is played out and only records where it would have
        resigned.  resign_rows() reads the records, resign_stats() the false-positive rate; set_resign() changes the rule
        between searches.  Searches, and the rows of games that do not resign, are what they are without it.

        early_stop: None / False = every search runs its whole budget (the default, unchanged); True or an
        EarlyStop(host_exit) = a slot whose move is the first maximum of the visits (moves made >= temp_moves) stops searching
        at the first simulation index at which the simulations left cannot change that move.  The move is the full search's;
        root_stats() and pi are those of the shortened tree (pi = N / stop_at), stopped() reads stop_at, set_early_stop()
        changes it between searches.  Meant for matches and players, not for training games.  With it on, root_store=None
        means no root store.

        replay_seed: True = where the carry-over cache is on and the search is otherwise plain (no other search
        option, no noise, no reuse_subtree, no eval_symmetry), a slot's search starts from a copy of the played child's old
        subtree -- what its first N_e - 1 simulations would rebuild -- and spreads its remaining walks evenly over the move's tree
        steps; False = every search is stepped simulation by simulation; None (the default) = True for an engine of more than
        1024 games, where level launches pay, else False.  No result and no counter depends on it; everywhere else it is
        ignored.  set_replay_seed() changes it between searches.

        Which of these options run together: every pair but those of SEARCH_OPTION_CONFLICTS (the matrix of DESIGN.md 5, "The
        search mode"), in __init__ and in every set_*(); a refused pair is a ValueError that names both keywords, before any
        device is touched.  Every evaluator and eval_cache mode serves every option."""
        self.replay_seed = check_replay_seed(replay_seed)
        if early_stop is not None and early_stop is not False and root_store is None:
            root_store = False  # (a shortened tree is not worth an entry and must not seed a later search)
        # every option is validated, then refused against what is on so far (_switch): the later of a refused pair names it
        self._reuse, self._dirichlet_eps, self.K = bool(reuse_subtree), dirichlet_eps, check_leaves_per_step(leaves_per_step)
        self.root_store = check_root_store(root_store, eval_cache)
        self.ownership = check_ownership(ownership)
        self.resign = self._switch("resign", check_resign(resign))
        self.eval_symmetry = check_eval_symmetry(eval_symmetry, seed, game, evaluator)
        if not isinstance(surprise, (bool, np.bool_)):
            raise ValueError(f"surprise must be a bool (got {surprise!r})")
        self.surprise = bool(surprise)
        self.search_value = check_search_value(search_value)
        check_sims(sims, reuse_subtree)
        check_eval_cache(eval_cache)
        self.gumbel = self._switch("gumbel", check_gumbel(gumbel))
        self.playout_cap = self._switch("playout_cap", check_playout_cap(playout_cap, sims))
        self.forced_playouts = self._switch("forced_playouts", check_forced_playouts(forced_playouts))
        self.fpu = self._switch("fpu", check_fpu(fpu))
        self.solver = self._switch("solver", check_solver(solver))
        self.early_stop = self._switch("early_stop", check_early_stop(early_stop))
        if evaluator.startswith("mlp_") and _GAMES[game] != GAME_TTT:
            raise ValueError(f"evaluator {evaluator!r}: the MLP evaluators serve tic-tac-toe only")
        _lib.require_gpu()
        L = _lib.lib()
        self.game = _GAMES[game]
        self.device = torch.device(device)
        self._streams = {}  # every stream this engine's kernels were launched on (drained before the workspace dies)
        self._buffers = {}  # the caller-owned option buffers (_option_buffer), kept like the workspace until __del__ has drained
        t_max = 9 if self.game == GAME_TTT else 64
        self.cfg = EngineCfg(self.game, n_games, sims, _EVALS[evaluator], c_puct, temp_moves, openings, rounds, t_max,
                             stagger, seed, game_id_base, n_games if game_id_stride is None else game_id_stride,
                             (_lib.ENGINE_REUSE_SUBTREE if reuse_subtree else 0) | (_lib.ENGINE_EVAL_CACHE if eval_cache else 0) |
                             (_lib.ENGINE_EVAL_CACHE_CARRY if eval_cache in (True, "carry") else 0) |
                             ((self.K - 1) << _lib.ENGINE_LEAVES_SHIFT),
                             dirichlet_alpha, dirichlet_eps, ttt_lanes)
        nbytes = L.bz_engine_workspace_bytes(C.byref(self.cfg))
        if nbytes < 0:
            raise RuntimeError(_lib.last_error())
        self.ws = torch.zeros(nbytes + 256, dtype=torch.uint8, device=self.device)
        self._pad = (-self.ws.data_ptr()) & 255
        h = C.c_void_p()
        _lib.check(L.bz_engine_create(C.byref(self.cfg), self.ws.data_ptr() + self._pad, nbytes, C.byref(h)))
        self.h = h
        self.lay = EngineLayout()
        _lib.check(L.bz_engine_get_layout(self.h, C.byref(self.lay)))
        self.B, self.sims, self.rounds, self.na, self.t_max = n_games, sims, rounds, self.lay.na, t_max
        self.size = _SIZES[self.game]
        self.net = net
        if net is not None:
            from .mlp import DeviceMLP
            if isinstance(net, DeviceMLP):
                if net.max_batch < n_games * self.K:
                    raise ValueError(f"DeviceMLP max_batch {net.max_batch} < n_games {n_games}" +
                                     (f" x leaves_per_step {self.K}" if self.K > 1 else ""))
                _lib.check(L.bz_engine_set_mlp(self.h, net.h))
            else:
                _lib.check(L.bz_engine_set_net(self.h, net.h))
        if self.replay_seed is not None:
            _lib.check(L.bz_engine_set_replay_seed(self.h, int(self.replay_seed)))
        if self.gumbel is not None:
            gc = self.gumbel
            self._call(L.bz_engine_set_gumbel, gc.max_considered, gc.scale, gc.maxvisit_init, gc.value_scale,
                       *self._option_buffer("gumbel", L.bz_engine_gumbel_bytes, gc.max_considered))
            if gc.interior == "gumbel":
                self._set_gumbel_interior(True)
        if self.playout_cap is not None:
            self._call(L.bz_engine_set_playout_cap, self.playout_cap.fast_sims, self.playout_cap.full_q,
                       *self._option_buffer("playout_cap", L.bz_engine_playout_cap_bytes))
        if self.forced_playouts is not None:
            self._call(L.bz_engine_set_forced_playouts, self.forced_playouts.k, int(self.forced_playouts.prune))
        if self.fpu is not None:
            self._set_fpu(self.fpu)
        if self.solver:
            self._set_solver(True)
        if self.surprise:
            self._call(L.bz_engine_set_surprise, *self._option_buffer("surprise", L.bz_engine_surprise_bytes))
        if self.eval_symmetry is not None:
            _lib.check(L.bz_engine_set_eval_symmetry(self.h, 1, self.eval_symmetry.seed))
        if self.search_value:
            self._call(L.bz_engine_set_search_value, *self._option_buffer("search_value", L.bz_engine_search_value_bytes))
        if self.root_store is not None:
            # (empty, not zeros: the setter clears the index, and nothing reads an entry the index does not name)
            ptr, rbytes = self._option_buffer("root_store", L.bz_engine_root_store_bytes, *self.root_store, zero=False)
            if rbytes == 0:  # no carry-over cache in this engine (synthetic evaluator, reuse_subtree, leaves_per_step > 1)
                self.root_store = None
            else:
                self._call(L.bz_engine_set_root_store, ptr, rbytes, *self.root_store)
        if self.ownership:
            self._call(L.bz_engine_set_ownership, *self._option_buffer("ownership", L.bz_engine_ownership_bytes))
        if self.resign is not None:
            self._set_resign(self.resign)
        if self.early_stop is not None:
            self._set_early_stop(self.early_stop)

    # ---- the search options
    def _options(self):
        """the value every search option (SEARCH_OPTIONS) has now, by keyword; one that __init__ has not reached yet is off"""
        on = {k: vars(self).get(k) for k in SEARCH_OPTIONS}
        on.update(reuse_subtree=self._reuse, leaves_per_step=self.K, dirichlet_eps=self._dirichlet_eps,
                  gumbel_interior=on["gumbel"] is not None and on["gumbel"].interior == "gumbel")
        return on

    def _switch(self, name, value):
        """`value`, the checked new value of option `name`, unless it is on and makes a refused pair with what is on"""
        if _option_on(name, value):
            refuse_option_conflict(name, self._options())
        return value

    def _option_buffer(self, key, bytes_fn, *args, zero=True):
        """(pointer, bytes) of the caller-owned device buffer of option `key`, 256-byte aligned: allocated at its first use --
        bytes_fn(cfg, *args) of the library says how large -- and used again when the option is switched off and on;
        (0, 0) where the library says the engine has no such buffer"""
        if key not in self._buffers:
            n = bytes_fn(C.byref(self.cfg), *args)
            if n < 0:
                raise RuntimeError(_lib.last_error())
            if n == 0:
                return 0, 0
            t = (torch.zeros if zero else torch.empty)(n + 256, dtype=torch.uint8, device=self.device)
            pad = (-t.data_ptr()) & 255
            self._buffers[key] = t[pad:pad + n]
        return self._buffers[key].data_ptr(), self._buffers[key].numel()

    # ---- views into the workspace
    def _view(self, off, dtype, shape):
        n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        o = self._pad + off
        return self.ws[o:o + n].view(dtype).view(*shape)

    def _stream(self):
        st = torch.cuda.current_stream(self.device)
        self._streams[st.cuda_stream] = st
        return st.cuda_stream

    def track_stream(self, stream):
        """a torch stream on which the caller launches this engine's kernels through the ABI itself (play_match, Reanalyser): kept, and
        drained with the others before the workspace dies"""
        self._streams[stream.cuda_stream] = stream

    def _call(self, fn, *args):
        with torch.cuda.device(self.device):
            _lib.check(fn(self.h, *args, self._stream()))

    # ---- ABI passthroughs
    def reset_games(self):
        self._call(_lib.lib().bz_engine_reset_games)

    def set_roots(self, own, opp, to_move):
        own = torch.as_tensor(np.asarray(own, dtype=np.uint64).view(np.int64)).to(self.device)
        opp = torch.as_tensor(np.asarray(opp, dtype=np.uint64).view(np.int64)).to(self.device)
        tm = torch.as_tensor(np.asarray(to_move, dtype=np.int8)).to(self.device)
        assert own.numel() == self.B
        self._call(_lib.lib().bz_engine_set_roots, own.data_ptr(), opp.data_ptr(), tm.data_ptr())
        torch.cuda.current_stream(self.device).synchronize()  # keep own/opp/tm alive until consumed

    def set_eval_symmetry(self, eval_symmetry):
        """switch the hashed evaluation symmetry on, off or to another seed, between searches: None /
        False, True (the engine's seed) or an EvalSymmetry.  Like a change of weights it is a change of evaluator: the
        evaluation cache carries nothing over it."""
        es = check_eval_symmetry(eval_symmetry, int(self.cfg.seed), self.game, _EVAL_NAMES[self.cfg.eval_kind])
        self.drain()
        _lib.check(_lib.lib().bz_engine_set_eval_symmetry(self.h, int(es is not None), es.seed if es is not None else 0))
        self.eval_symmetry = es

    def _set_gumbel_interior(self, on):
        L = _lib.lib()
        if not on:
            self._call(L.bz_engine_set_gumbel_interior, 0, None, 0)
            return
        self._call(L.bz_engine_set_gumbel_interior, 1, *self._option_buffer("gumbel_interior", L.bz_engine_gumbel_interior_bytes))

    def set_gumbel_interior(self, interior):
        """switch the select rule below the root of a Gumbel search between "puct" and "gumbel" (DESIGN.md 3.21), between
        searches; ValueError without Gumbel root search"""
        if self.gumbel is None:
            raise ValueError("gumbel: the interior rule needs Gumbel root search (gumbel=)")
        from dataclasses import replace
        gc = check_gumbel(replace(self.gumbel, interior=interior))
        self._switch("gumbel_interior", gc.interior == "gumbel")
        self.drain()
        self._set_gumbel_interior(gc.interior == "gumbel")
        self.gumbel = gc

    def _set_fpu(self, fp):
        L = _lib.lib()
        if fp is None:
            self._call(L.bz_engine_set_fpu, 0, 0.0, 0.0, None, 0)
            return
        self._call(L.bz_engine_set_fpu, 1, fp.reduction, fp.root_reduction, *self._option_buffer("fpu", L.bz_engine_fpu_bytes))

    def set_fpu(self, fpu):
        """switch first-play urgency reduction on, off or to other reductions, between searches: None /
        False, True (the defaults) or an Fpu"""
        fp = self._switch("fpu", check_fpu(fpu))
        self.drain()
        self._set_fpu(fp)
        self.fpu = fp

    def _set_solver(self, on):
        L = _lib.lib()
        if not on:
            self._call(L.bz_engine_set_solver, 0, None, 0)
            return
        self._call(L.bz_engine_set_solver, 1, *self._option_buffer("solver", L.bz_engine_solver_bytes))

    def set_solver(self, solver):
        """switch the solver on or off, between searches"""
        on = self._switch("solver", check_solver(solver))
        self.drain()
        self._set_solver(on)
        self.solver = on

    def _set_early_stop(self, es):
        L = _lib.lib()
        if es is None:
            self._call(L.bz_engine_set_early_stop, 0, 0, None, 0)
            return
        self._call(L.bz_engine_set_early_stop, 1, int(es.host_exit), *self._option_buffer("early_stop", L.bz_engine_early_stop_bytes))

    def set_early_stop(self, early_stop):
        """switch exact early stop on, off or to another host_exit, between searches: None / False, True or an
        EarlyStop"""
        es = self._switch("early_stop", check_early_stop(early_stop))
        self.drain()
        self._set_early_stop(es)
        self.early_stop = es

    def stopped(self):
        """after a search with early stop on: stop_at, numpy uint32 [B] -- the simulations every slot's search
        ran: sims when it ran its whole budget, 0 for a slot that sat the search out"""
        if self.early_stop is None:
            raise RuntimeError("stopped(): early stop is off (early_stop=)")
        out = torch.empty(self.B, dtype=torch.int32, device=self.device)
        self._call(_lib.lib().bz_engine_stopped, out.data_ptr())
        return out.cpu().numpy().view(np.uint32)

    def _set_resign(self, rs):
        L = _lib.lib()
        if rs is None:
            self._call(L.bz_engine_set_resign, 0.0, 0, 0, None, 0)
            return
        # (the same buffer every time: while resignation stays on the setter keeps its streaks and records)
        self._call(L.bz_engine_set_resign, rs.threshold, rs.consecutive, rs.playout_q, *self._option_buffer("resign", L.bz_engine_resign_bytes))

    def set_resign(self, resign):
        """switch resignation on, off or to another rule, between searches: None / False, True (the defaults)
        or a Resign.  While it stays on, streaks and records are kept; switching it off and on again clears them."""
        rs = self._switch("resign", check_resign(resign))
        self.drain()
        self._set_resign(rs)
        self.resign = rs

    def resign_rows(self):
        """resignation: every game's record, numpy [rounds, B] each -- side int8 (the side that fired first,
        +1 / -1; 0 = none), move int32 (moves made at that search), q float32 (its root value) and played_out bool (the game
        never resigns; known once the game has had a play)"""
        if self.resign is None:
            raise RuntimeError("resign_rows(): resignation is off (resign=)")
        n = self.rounds * self.B
        side = torch.empty(n, dtype=torch.int8, device=self.device)
        move = torch.empty(n, dtype=torch.int32, device=self.device)
        q = torch.empty(n, dtype=torch.float32, device=self.device)
        out = torch.empty(n, dtype=torch.uint8, device=self.device)
        self._call(_lib.lib().bz_engine_resign_rows, side.data_ptr(), move.data_ptr(), q.data_ptr(), out.data_ptr())
        shp = (self.rounds, self.B)
        return (side.cpu().numpy().reshape(shp), move.cpu().numpy().reshape(shp), q.cpu().numpy().reshape(shp),
                out.cpu().numpy().astype(bool).reshape(shp))

    def resign_stats(self):
        """the calibration figures over the games finished so far: n_finished, n_resigned, n_played_out
        (finished and played out), n_would_resign (of those, with a record), n_false_positive (of those, the recorded side won
        or drew) and false_positive_rate (None when n_would_resign == 0)"""
        side, _, _, out = self.resign_rows()
        winner, length = self.winners()
        return resign_stats(side, out, winner, length)

    def proven(self):
        """after a search with the solver on: (root, edges, counts) -- root: per slot the root's proven value
        for its mover (-1, 0, +1) or None; edges: int8 [B, NA], the decided value of the root edge of every action for the
        mover AFTER it (-1: the move wins), 2 where undecided or no such edge; counts: {"n_decided": nodes newly decided in
        the last search, "n_proven_stops": walks that ended at a decided edge that is not terminal}"""
        if not self.solver:
            raise RuntimeError("proven(): the solver is off")
        edge = torch.empty((self.B, self.na), dtype=torch.int8, device=self.device)
        root = torch.empty(self.B, dtype=torch.int8, device=self.device)
        cnt = torch.empty(2, dtype=torch.int32, device=self.device)
        self._call(_lib.lib().bz_engine_root_proven, edge.data_ptr(), root.data_ptr(), cnt.data_ptr())
        r, c = root.cpu().numpy(), cnt.cpu().numpy().view(np.uint32)
        return ([None if v == 2 else int(v) for v in r], edge.cpu().numpy(),
                {"n_decided": int(c[0]), "n_proven_stops": int(c[1])})

    def search(self):
        if self.early_stop is not None and self.early_stop.host_exit and self.cfg.eval_kind != EVAL_EXTERNAL:
            #  host exit lives in the interleaving loop: one engine, play_match's run-ahead
            with torch.cuda.device(self.device):
                _lib.check(_lib.lib().bz_engines_search((C.c_void_p * 1)(self.h), (C.c_void_p * 1)(self._stream()), 1, 16))
            return
        self._call(_lib.lib().bz_engine_search)

    def search_external(self, eval_fn):
        """One full search with a caller-supplied evaluator (engine built with evaluator="external"): eval_fn(own, opp,
        kind) gets the leaf positions as int64 CUDA tensors [K*B] (uint64 bit patterns, side-to-move canonical -- the input
        convention of the reference's AIPlayer, players.py:85) and kind (uint8 [K*B], 1 = needs evaluation; row g*K + j =
        walk j of game g, K = leaves_per_step) and returns (logits [K*B, NA] float32, value [K*B] float32) CUDA tensors;
        legality masking and the softmax happen in the expansion.
        Any torch module can sit here -- e.g. an MLP over the 9 tic-tac-toe cells like the reference's TicTacToeNet."""
        lb = self.leaf_buffers()

        def fill():
            lg, v = eval_fn(lb["own"], lb["opp"], lb["kind"])
            lb["logits"].copy_(lg.to(torch.float32).reshape(lb["logits"].shape))
            lb["value"].copy_(v.to(torch.float32).reshape(lb["value"].shape))
        self.root_begin(); fill(); self.expand_backup()
        self.root_noise()  # (no-op unless dirichlet_eps > 0) same place as in bz_engine_search
        for s in range(0, self.sims, self.K):  # one step = min(K, sims - s) walks per game
            self.select(s); fill(); self.expand_backup()

    def root_begin(self):
        self._call(_lib.lib().bz_engine_root_begin)

    def root_noise(self):
        """Dirichlet noise on the expanded roots' priors (no-op when dirichlet_eps == 0); step-API callers run it
        after the expand_backup() that follows root_begin() and before select(0)"""
        self._call(_lib.lib().bz_engine_root_noise)

    def select(self, sim_index):
        self._call(_lib.lib().bz_engine_select, sim_index)

    def evaluate(self):
        self._call(_lib.lib().bz_engine_evaluate)

    def expand_backup(self):
        self._call(_lib.lib().bz_engine_expand_backup)

    def play(self, restart=False):
        self._call(_lib.lib().bz_engine_play, int(restart))

    def reset_counters(self):
        self._call(_lib.lib().bz_engine_reset_counters)

    def status(self):
        a, f, e = C.c_int32(), C.c_int64(), C.c_int32()
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().bz_engine_status(self.h, self._stream(), C.byref(a), C.byref(f), C.byref(e)))
        if e.value:
            names = [n for bit, n in ((1, "edge arena overflow"), (2, "terminal root"), (4, "example buffer overflow"),
                                      (8, "walk deeper than the path buffer"),
                                      (16, "the evaluator returned a non-finite logit or value"),
                                      (32, "reanalyse row index out of range")) if e.value & bit]
            raise RuntimeError(f"bz_engine error flags 0x{e.value:x}: " + ", ".join(names))
        return a.value, f.value

    def root_stats(self):
        self._call(_lib.lib().bz_engine_root_stats)
        shp = (self.B, self.na)
        N = self._view(self.lay.root_N, torch.int32, shp).cpu().numpy().view(np.uint32)
        W = self._view(self.lay.root_W, torch.float32, shp).cpu().numpy()
        P = self._view(self.lay.root_P, torch.float32, shp).cpu().numpy()
        return N, W, P

    def root_policy_dev(self):
        """root_policy() as CUDA tensors (pi float32 [B, NA], action int32 [B]) on the current stream, nothing copied"""
        pi = torch.empty((self.B, self.na), dtype=torch.float32, device=self.device)
        act = torch.empty(self.B, dtype=torch.int32, device=self.device)
        self._call(_lib.lib().bz_engine_root_policy, pi.data_ptr(), act.data_ptr())
        return pi, act

    def root_policy(self):
        """after a search: the pi and the action play() would write and play, per slot (pi float32 [B, NA], action int32
        [B]; idle or finished slots: zeros and -1).  PUCT: N / sum N and the visit-count move (tau = 1 sampling while moves
        made < temp_moves); Gumbel: the improved policy and the Gumbel move"""
        pi, act = self.root_policy_dev()
        return pi.cpu().numpy(), act.cpu().numpy()

    def budgets(self):
        """playout cap randomisation: the simulation budget every slot drew for the last search, uint32 [B]
        read from the device -- sims (full) or fast_sims; 0 for a slot that took no part (finished / idle, or no search yet)"""
        if self.playout_cap is None:
            raise RuntimeError("budgets(): the engine was built without playout_cap")
        self.drain()
        torch.cuda.current_stream(self.device).synchronize()
        return self._buffers["playout_cap"][:4 * self.B].view(torch.int32).cpu().numpy().view(np.uint32)

    def counters(self):
        """the work counters by name (_lib.COUNTER_NAMES); "n_collisions" only for leaves_per_step > 1"""
        self._call(_lib.lib().bz_engine_sum_counters)
        c = self._view(self.lay.counters, torch.int64, (24,)).cpu().numpy()
        # n_collisions (counters[10]) only for a leaf-parallel engine: at K = 1 it is 0 by definition, and the dict stays
        # what it was before leaves_per_step existed
        names = _lib.COUNTER_NAMES if self.K > 1 else _lib.COUNTER_NAMES[:_lib.COUNTER_NAMES.index("n_collisions")]
        return dict(zip(names, (int(v) for v in c[:len(names)])))

    def set_replay_seed(self, on=None):
        """the replay seed on (True), off (False) or by the engine's size (None) from the next search on; results
        and counters do not depend on it"""
        self.replay_seed = check_replay_seed(on)
        _lib.check(_lib.lib().bz_engine_set_replay_seed(self.h, 2 if self.replay_seed is None else int(self.replay_seed)))

    def replay_seed_counters(self):
        """the replay seed's counters: n_replay_seeds -- searches of a slot that began from the played child's old
        subtree --, n_replay_sims -- the simulations those subtrees stood for, each one a tree step the slot then sat out"""
        self._call(_lib.lib().bz_engine_sum_counters)
        c = self._view(self.lay.counters, torch.int64, (24,)).cpu().numpy()
        return {"n_replay_seeds": int(c[14]), "n_replay_sims": int(c[15])}

    def root_store_counters(self):
        """the root store's counters: n_seeded_evals -- evaluations taken from a seeded tree (part of
        counters()["n_cache_hits_prev"]) --, n_seeded_searches and n_root_saves (trees filed; at most `entries` per evaluator)"""
        self._call(_lib.lib().bz_engine_sum_counters)
        c = self._view(self.lay.counters, torch.int64, (24,)).cpu().numpy()
        return {"n_seeded_evals": int(c[11]), "n_seeded_searches": int(c[12]), "n_root_saves": int(c[13])}

    # leaf buffers for BZ_EVAL_EXTERNAL callers (torch tensors aliasing the workspace): K*B rows, row g*K + j = walk j of game g
    def leaf_buffers(self):
        R = self.B * self.K
        return {"own": self._view(self.lay.leaf_own, torch.int64, (R,)),
                "opp": self._view(self.lay.leaf_opp, torch.int64, (R,)),
                "kind": self._view(self.lay.leaf_kind, torch.uint8, (R,)),
                "logits": self._view(self.lay.logits, torch.float32, (R, self.na)),
                "value": self._view(self.lay.value, torch.float32, (R,))}

    def positions(self):
        return (_u64(self._view(self.lay.g_own, torch.int64, (self.B,))),
                _u64(self._view(self.lay.g_opp, torch.int64, (self.B,))),
                self._view(self.lay.g_to_move, torch.int8, (self.B,)).cpu().numpy(),
                self._view(self.lay.g_state, torch.uint8, (self.B,)).cpu().numpy())

    # ---- example buffers
    def example_tensors(self):
        """fixed-capacity device tensors [rounds, B, t_max, ...] (what the all-gather ships)"""
        R, B, T = self.rounds, self.B, self.t_max
        return {"own": self._view(self.lay.ex_own, torch.int64, (R, B, T)),
                "opp": self._view(self.lay.ex_opp, torch.int64, (R, B, T)),
                "pi": self._view(self.lay.ex_pi, torch.float32, (R, B, T, self.na)),
                "z": self._view(self.lay.ex_z, torch.int8, (R, B, T)),
                "mover": self._view(self.lay.ex_mover, torch.int8, (R, B, T)),
                "act": self._view(self.lay.ex_act, torch.uint8, (R, B, T)),
                "len": self._view(self.lay.ex_len, torch.int32, (R, B)),
                "winner": self._view(self.lay.ex_winner, torch.int8, (R, B))}

    def example_block(self):
        """the ONE contiguous, self-describing byte range [ex_own .. ex_winner | 256-B header] of the
        workspace (uint8 view, no copy) -- what the iteration-end all-gather ships"""
        o = self._pad + self.lay.ex_begin
        return self.ws[o:o + self.lay.ex_bytes]

    def surprise_rows(self):
        """policy surprise weighting: the engine's ex_kl, a float32 [rounds, B, t_max] view of the surprise
        buffer indexed like example_tensors()["pi"] (rows past a game's ex_len hold whatever an earlier game left)"""
        if not self.surprise:
            raise RuntimeError("surprise_rows(): the engine was built without surprise=True")
        n = self.rounds * self.B * self.t_max * 4
        buf = self._buffers["surprise"]
        o = buf.numel() - ((n + 255) & ~255)  # ex_kl is the buffer's last array
        return buf[o:o + n].view(torch.float32).view(self.rounds, self.B, self.t_max)

    def pack_surprise(self, out=None, cap_rows=None, append=False):
        """_pack_extra("surprise"): the finished games' kl, float32 [cap_rows] on the device"""
        return self._pack_extra("surprise", out if out is None else (out,), cap_rows, append)[0]

    def search_value_rows(self):
        """search-value targets: the engine's ex_q, a float32 [rounds, B, t_max] view of the search-value
        buffer indexed like example_tensors()["pi"] (rows past a game's ex_len hold whatever an earlier game left)"""
        if not self.search_value:
            raise RuntimeError("search_value_rows(): the engine was built without search_value=True")
        n = self.rounds * self.B * self.t_max * 4
        return self._buffers["search_value"][:n].view(torch.float32).view(self.rounds, self.B, self.t_max)

    def pack_search_value(self, out=None, cap_rows=None, append=False):
        """_pack_extra("search_value"): the finished games' q, float32 [cap_rows] on the device"""
        return self._pack_extra("search_value", out if out is None else (out,), cap_rows, append)[0]

    def ownership_rows(self):
        """ownership targets: the finished games' final boards in absolute colours, (fin_x, fin_o), int64
        [rounds, B] views of the ownership buffer holding the uint64 bit patterns, indexed like example_tensors()["len"] (valid
        where len >= 0, 0 elsewhere)"""
        if not self.ownership:
            raise RuntimeError("ownership_rows(): the engine was built without ownership=True")
        n = self.rounds * self.B * 8
        step = (n + 255) & ~255  # fin_x and fin_o are the buffer's first two arrays
        return tuple(self._buffers["ownership"][k * step:k * step + n].view(torch.int64).view(self.rounds, self.B) for k in (0, 1))

    def pack_ownership(self, out=None, cap_rows=None, append=False):
        """_pack_extra("ownership"): the finished games' rows' ownership targets, (fown, fopp), int64 [cap_rows] on the device"""
        return self._pack_extra("ownership", out, cap_rows, append)

    def _pack_extra(self, option, out=None, cap_rows=None, append=False):
        """the finished games' columns of `option` (ENGINE_EXTRAS) in the row order of the packed block the preceding
        pack_examples() (same cap_rows, same stream) filled: one [cap_rows] device tensor per column, rows [0, n_rows) valid"""
        cols, dtype, entry = ENGINE_EXTRAS[option]
        cap = int(cap_rows or self.rounds * self.B * self.t_max)
        if out is None:
            assert not append
            out = tuple(torch.zeros(cap, dtype=dtype, device=self.device) for _ in cols)
        self._call(getattr(_lib.lib(), entry), *(t.data_ptr() for t in out), cap, int(append))
        return out

    def _pack_with_extras(self, out=None, cap_rows=None, append=False, extras=None):
        """pack_examples() and, right behind it, while the row offsets it left are current, the columns of the options that are on:
        (block, {column: [cap_rows] device tensor in the block's row order}).  `extras`: the dict to fill (append=True: behind
        the rows of the engines before this one)"""
        cap = int(cap_rows or self.rounds * self.B * self.t_max)
        out = self.pack_examples(out, cap, append)
        on = {o: cols for o, (cols, _, _) in ENGINE_EXTRAS.items() if getattr(self, o)}
        if extras is None:
            assert not append
            extras = {k: torch.zeros(cap, dtype=ENGINE_EXTRAS[o][1], device=self.device) for o, cols in on.items() for k in cols}
        for o, cols in on.items():
            self._pack_extra(o, tuple(extras[k] for k in cols), cap, append)
        return out, extras

    def _extras(self):
        """the columns of the options that are on, in (round, slot, ply) order -- the order of examples() and device_examples() --
        behind ONE pack_examples(); an engine without such an option packs nothing"""
        return self._pack_with_extras()[1] if any(getattr(self, o) for o in ENGINE_EXTRAS) else {}

    def examples(self):
        """finished games' rows, compacted on the device; only the valid rows cross PCIe"""
        return _attach_extras(unpack_example_block(self.example_block()), self._extras())

    def block_geometry(self):
        """host-side description of this engine's example block (what its 256-byte header says), so that a block of the
        same geometry -- this engine's, or a peer rank's copy of it after the all-gather -- can be unpacked on the
        device without reading the header back"""
        L = self.lay
        offs = [o - L.ex_begin for o in (L.ex_own, L.ex_opp, L.ex_pi, L.ex_z, L.ex_mover, L.ex_act, L.ex_len, L.ex_winner)]
        return {"B": self.B, "rounds": self.rounds, "t_max": self.t_max, "na": self.na, "game": self.game,
                "size": self.size, "offs": offs, "ex_bytes": int(L.ex_bytes)}

    def device_examples(self):
        """finished games' rows as DeviceExamples: nothing leaves the GPU"""
        return _attach_extras(unpack_example_block_device(self.example_block(), self.block_geometry()), self._extras())

    def winners(self):
        t = self.example_tensors()
        return t["winner"].cpu().numpy(), t["len"].cpu().numpy()

    def run_iteration(self, max_plies=None):
        """play every slot's game to termination (one self-play iteration)"""
        self.reset_games()
        plies = 0
        limit = max_plies or (12 if self.game == GAME_TTT else 140)
        while True:
            self.search()
            self.play(False)
            plies += 1
            active, _ = self.status()
            if active == 0 or plies >= limit:
                return plies

    def pack_examples(self, out=None, cap_rows=None, append=False):
        """finished games' rows -> a packed example block (bz_abi.h "Packed examples": header + compacted rows in
        (round, slot, ply) order), by two kernels on the current stream; nothing is copied to the host.  `out`: a block
        from alloc_packed_block() (append=True: add this engine's rows behind those already in it)."""
        cap = int(cap_rows or self.rounds * self.B * self.t_max)
        if out is None:
            assert not append
            out = alloc_packed_block(self.na, cap, self.device)
        self._call(_lib.lib().bz_engine_pack_examples, out.data_ptr(), out.numel(), cap, int(append))
        return out

    def drain(self):
        """wait for every stream this engine's kernels were launched on"""
        for st in self._streams.values():
            st.synchronize()

    def __del__(self):
        try:
            self.drain()  # the caching allocator only knows the stream the workspace was allocated on
            _lib.lib().bz_engine_destroy(self.h)
        except Exception:
            pass


# ---------------------------------------------------------------- pipelined self-play
_PIPE_STREAMS, _PIPE_INFO, _PIPE_REJECTED = {}, {}, []


def stream_overlap_ratio(a, b, spin_us=300, reps=2):
    """bz_stream_overlap_probe on two torch streams: ~1.0 = they run side by side, ~2.0 = one waits for the other"""
    r = C.c_float()
    with torch.cuda.device(a.device):
        _lib.check(_lib.lib().bz_stream_overlap_probe(a.cuda_stream, b.cuda_stream, spin_us, reps, C.byref(r)))
    return float(r.value)


def pipeline_streams(device="cuda:0", n=2, max_tries=4):
    """the n HIP streams the pipelines of this process run on: created ONCE per (device, n) and reused by every
    PipelinedSelfPlay.  torch hands streams out round-robin from a pool and not every pair runs side by side on this
    stack (profiles/r03_torch_stream_pool_pairs.txt: the third and fourth stream of a process serialise -- 12 % of the
    headline), so a candidate set is accepted only when bz_stream_overlap_probe sees every two of its streams overlap
    (two 0.3-ms single-wave kernels behind a common event finish in ~0.3 ms, not ~0.6); otherwise the next set is
    tried and the best one seen is kept."""
    dev = torch.device(device)
    key = (str(dev), n)
    if key not in _PIPE_STREAMS:
        tried = []
        for _ in range(max_tries if n > 1 else 1):
            st = [torch.cuda.Stream(device=dev) for _ in range(n)]
            worst = max([stream_overlap_ratio(st[i], st[j]) for i in range(n) for j in range(i + 1, n)], default=1.0)
            tried.append((worst, st))
            if worst < 1.5:
                break
        best = min(range(len(tried)), key=lambda i: tried[i][0])
        _PIPE_REJECTED.extend(t[1] for i, t in enumerate(tried) if i != best)  # kept alive: torch would hand them out again
        _PIPE_STREAMS[key] = tried[best][1]
        _PIPE_INFO[key] = {"overlap_ratio_of_candidates": [round(t[0], 3) for t in tried], "picked": best}
    return _PIPE_STREAMS[key]


def pipeline_stream_info(device="cuda:0", n=2):
    """what the probe saw when pipeline_streams() chose its streams (None before the first call)"""
    return _PIPE_INFO.get((str(torch.device(device)), n))


def _check_search_options(sims, reuse_subtree, leaves_per_step, dirichlet_eps, gumbel, playout_cap, forced_playouts, fpu, solver):
    """the search options self_play and its pipelines pass on to their engines, each validated before it is another's "other
    option" (ValueError, before any device is touched)"""
    cfg = dict(reuse_subtree=reuse_subtree, leaves_per_step=check_leaves_per_step(leaves_per_step))
    gumbel = check_gumbel(gumbel, dirichlet_eps=dirichlet_eps, **cfg)
    check_playout_cap(playout_cap, sims, gumbel=gumbel, **cfg)
    forced_playouts = check_forced_playouts(forced_playouts, gumbel=gumbel, **cfg)
    fpu = check_fpu(fpu, gumbel=gumbel, **cfg)
    check_solver(solver, gumbel=gumbel, forced_playouts=forced_playouts, fpu=fpu, **cfg)


class PipelinedSelfPlay:
    """The batched self-play of `n_games` concurrent games on one GPU as `pipelines` independent SelfPlayEngines of
    n_games / pipelines slots, each on its own HIP stream, sharing one net: the tree step of one pipeline overlaps the
    net launch of the other and their net launches fill each other's tail (the shape the headline is
    measured on).  Games keep their global ids (slot s of pipeline i = id base + offset_i + s), so the examples are
    the same rows whatever the number of pipelines.  Batched counterpart of collect_game_data,
    src/tic_tac_toe/SL/generate_training_games.py:25-38.

    Stream contract: work is issued behind whatever the caller's current stream holds at that moment (weights just
    updated there are seen); join() makes the caller's current stream wait for the pipelines without blocking the
    host, and everything that hands data out (status, counters, pack_examples, examples ...) joins first."""

    def __init__(self, game, n_games, sims, evaluator="uniform", net=None, pipelines=2, streams=None, game_id_base=0,
                 game_id_stride=None, device="cuda:0", run_ahead=16, leaves_per_step=1, gumbel=None, playout_cap=None,
                 forced_playouts=None, surprise=False, search_value=False, eval_symmetry=None, fpu=None, ownership=False,
                 solver=False, resign=None, **engine_kwargs):
        assert 1 <= pipelines <= n_games
        if "early_stop" in engine_kwargs:  #  a shortened search changes pi: not for training games
            raise ValueError("PipelinedSelfPlay: early_stop is for matches and players, not for self-play pipelines")
        check_ownership(ownership)
        check_resign(resign, ownership=ownership)
        # every pipeline gets the same seed, so the same position has the same orientation in all of them
        eval_symmetry = check_eval_symmetry(eval_symmetry, engine_kwargs.get("seed", 0), game, evaluator)
        check_search_value(search_value)
        _check_search_options(sims, engine_kwargs.get("reuse_subtree", False), leaves_per_step, engine_kwargs.get("dirichlet_eps", 0.0),
                              gumbel, playout_cap, forced_playouts, fpu, solver)
        check_eval_cache(engine_kwargs.get("eval_cache", True))
        check_root_store(engine_kwargs.get("root_store"), engine_kwargs.get("eval_cache", True))
        # simulations the host thread may queue ahead of the GPU (0 = unbounded: it then spins on the runtime's full queue,
        # 2 cores per rank against 0.18 -- profiles/r04_host_run_ahead.txt)
        self.run_ahead = run_ahead
        self.device = torch.device(device)
        self.sizes = [n_games // pipelines + (1 if i < n_games % pipelines else 0) for i in range(pipelines)]
        self.streams = list(streams) if streams is not None else pipeline_streams(self.device, pipelines)
        assert len(self.streams) == pipelines
        stride = n_games if game_id_stride is None else game_id_stride
        self.engines = [SelfPlayEngine(game, self.sizes[i], sims, evaluator, net, game_id_base=game_id_base + sum(self.sizes[:i]),
                                       game_id_stride=stride, device=device, leaves_per_step=leaves_per_step, gumbel=gumbel,
                                       playout_cap=playout_cap, forced_playouts=forced_playouts, surprise=surprise,
                                       search_value=search_value, eval_symmetry=eval_symmetry, fpu=fpu, ownership=ownership, solver=solver,
                                       resign=resign, **engine_kwargs)
                        for i in range(pipelines)]
        self.surprise, self.search_value, self.ownership = bool(surprise), bool(search_value), bool(ownership)
        e0 = self.engines[0]
        self.B, self.sims, self.na, self.t_max, self.rounds, self.size, self.game = n_games, sims, e0.na, e0.t_max, e0.rounds, e0.size, e0.game

    # ---- stream plumbing
    def _fork(self):
        cur = torch.cuda.current_stream(self.device)
        for st in self.streams:
            st.wait_stream(cur)

    def join(self):
        """the caller's current stream waits for everything issued on the pipelines so far (no host block)"""
        cur = torch.cuda.current_stream(self.device)
        for st in self.streams:
            cur.wait_stream(st)

    def sync(self):
        for st in self.streams:
            st.synchronize()

    def _each(self, fn):
        out = []
        for e, st in zip(self.engines, self.streams):
            with torch.cuda.stream(st):
                out.append(fn(e))
        return out

    # ---- the loop
    def reset_games(self):
        self._fork()
        self._each(lambda e: e.reset_games())

    def step(self, restart=False):
        """one move for every active slot of every pipeline: search (root expansion + sims simulations) + play, issued
        by bz_engines_step: ONE host thread, the pipelines interleaved simulation by simulation, at most `run_ahead`
        simulations ahead of the streams (it sleeps on blocking events instead of spinning on a full queue).  Returns
        with the tail of the move still queued."""
        self._fork()
        n = len(self.engines)
        for e, st in zip(self.engines, self.streams):
            e._streams[st.cuda_stream] = st
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().bz_engines_step((C.c_void_p * n)(*[e.h for e in self.engines]),
                                                  (C.c_void_p * n)(*[st.cuda_stream for st in self.streams]), n,
                                                  int(restart), int(self.run_ahead)))

    def status(self):
        """(active slots, finished games) over all pipelines; waits for them; raises on engine error flags"""
        r = self._each(lambda e: e.status())
        return sum(a for a, _ in r), sum(f for _, f in r)

    def run_iteration(self, max_plies=None):
        """play every slot's game to termination (one self-play iteration); returns the number of moves"""
        self.reset_games()
        plies, limit = 0, max_plies or (12 if self.game == GAME_TTT else 140)
        while True:
            self.step(False)
            plies += 1
            if self.status()[0] == 0 or plies >= limit:
                return plies

    def reset_counters(self):
        self._each(lambda e: e.reset_counters())

    def budgets(self):
        """the last search's budgets of all pipelines, in slot order (SelfPlayEngine.budgets)"""
        self.sync()
        return np.concatenate([e.budgets() for e in self.engines])

    def replay_seed_counters(self):
        tot = {}
        for c in self._each(lambda e: e.replay_seed_counters()):
            for k, v in c.items():
                tot[k] = tot.get(k, 0) + v
        return tot

    def root_store_counters(self):
        tot = {}
        for c in self._each(lambda e: e.root_store_counters()):
            for k, v in c.items():
                tot[k] = tot.get(k, 0) + v
        return tot

    def counters(self):
        tot = {}
        for c in self._each(lambda e: e.counters()):
            for k, v in c.items():
                tot[k] = tot.get(k, 0) + v
        return tot

    # ---- examples
    def example_blocks(self):
        """the engines' raw fixed-capacity example blocks (views into their workspaces)"""
        self.join()
        return [e.example_block() for e in self.engines]

    def packed_capacity(self, games=None):
        """rows a packed block needs for `games` finished games (default: every slot of every round)"""
        return int((games if games is not None else self.rounds * self.B) * self.t_max)

    def pack_examples(self, out=None, cap_rows=None):
        """ONE packed example block with the finished games of all pipelines (pipeline order, then round, slot, ply),
        written by the pack kernels on the caller's current stream behind the pipelines' work; no host visit."""
        cap = int(cap_rows or self.packed_capacity())
        if out is None:
            out = alloc_packed_block(self.na, cap, self.device)
        self.join()
        for i, e in enumerate(self.engines):
            e.pack_examples(out, cap, append=i > 0)
        return out

    def _pack_with_extras(self, out=None, cap_rows=None):
        """pack_examples() plus the per-row columns the engines record next to the block (ENGINE_EXTRAS): (block, {column:
        [cap_rows] device tensor in the block's row order}).  Each engine's arrays are packed right behind its rows, while the
        row offsets its pack left are current."""
        cap = int(cap_rows or self.packed_capacity())
        if out is None:
            out = alloc_packed_block(self.na, cap, self.device)
        extras = None
        self.join()
        for i, e in enumerate(self.engines):
            out, extras = e._pack_with_extras(out, cap, append=i > 0, extras=extras)
        return out, extras

    def pack_examples_with_ownership(self, out=None, cap_rows=None):
        """pack_examples() plus the rows' ownership targets (ownership=True): (block, fown, fopp), int64 [cap_rows] device
        tensors in the block's row order"""
        if not self.ownership:
            raise RuntimeError("pack_examples_with_ownership(): built without ownership=True")
        blk, x = self._pack_with_extras(out, cap_rows)
        return blk, x["fown"], x["fopp"]

    def pack_examples_with_surprise(self, out=None, cap_rows=None):
        """pack_examples() plus the rows' kl (surprise=True): (block, float32 [cap_rows] device tensor in the block's row
        order)"""
        if not self.surprise:
            raise RuntimeError("pack_examples_with_surprise(): built without surprise=True")
        blk, x = self._pack_with_extras(out, cap_rows)
        return blk, x["kl"]

    def pack_examples_with_search_value(self, out=None, cap_rows=None):
        """pack_examples() plus the rows' q (search_value=True): (block, float32 [cap_rows] device tensor in the block's row
        order)"""
        if not self.search_value:
            raise RuntimeError("pack_examples_with_search_value(): built without search_value=True")
        blk, x = self._pack_with_extras(out, cap_rows)
        return blk, x["q"]

    def device_examples(self):
        blk, extras = self._pack_with_extras()
        return _attach_extras(unpack_packed_block_device(blk), extras)

    def examples(self):
        blk, extras = self._pack_with_extras()
        return _attach_extras(unpack_packed_block(blk), extras)

    def ownership_rows(self):
        """the final boards of all pipelines, slots in pipeline order: (fin_x, fin_o), int64 [rounds, B] device tensors
        (SelfPlayEngine.ownership_rows)"""
        if not self.ownership:
            raise RuntimeError("ownership_rows(): built without ownership=True")
        self.join()
        r = [e.ownership_rows() for e in self.engines]
        return torch.cat([a for a, _ in r], dim=1), torch.cat([b for _, b in r], dim=1)

    def set_resign(self, resign):
        """SelfPlayEngine.set_resign on every pipeline, between searches"""
        rs = check_resign(resign, ownership=self.ownership)
        self.sync()
        self._each(lambda e: e.set_resign(rs))

    def resign_rows(self):
        """the resignation records of all pipelines in global game order: (side, move, q, played_out), numpy [rounds, B]
        (SelfPlayEngine.resign_rows)"""
        self.join()
        r = self._each(lambda e: e.resign_rows())
        return tuple(np.concatenate([p[k] for p in r], axis=1) for k in range(4))

    def resign_stats(self):
        """SelfPlayEngine.resign_stats summed over the pipelines"""
        self.join()
        return _sum_resign_stats(self._each(lambda e: e.resign_stats()))

    def winners(self):
        self.join()
        w = [e.winners() for e in self.engines]
        return np.concatenate([a for a, _ in w], axis=1), np.concatenate([b for _, b in w], axis=1)

    def __del__(self):
        try:
            self.sync()
        except Exception:
            pass


def self_play(game, n_games, sims, net=None, seed=0, evaluator=None, temp_moves=0, openings=0, c_puct=1.5,
              device="cuda:0", game_id_base=0, game_id_stride=None, dirichlet_alpha=0.0, dirichlet_eps=0.0,
              reuse_subtree=False, pipelines=None, leaves_per_step=1, gumbel=None, playout_cap=None, forced_playouts=None,
              surprise=False, search_value=False, eval_symmetry=None, fpu=None, ownership=False, solver=False, resign=None):
    """Play n_games concurrent self-play games to the end on one GPU and return
    (s, pi, z): canonical states int8 [n, size, size], visit-count policies
    f32 [n, NA], outcomes for the mover int8 [n] -- plus the Examples object.
    With a net evaluator the games run as two pipelines on two HIP streams (PipelinedSelfPlay: the shape bench.py
    measures); `pipelines` overrides.  The rows do not depend on it.  leaves_per_step: SelfPlayEngine;
    gumbel: SelfPlayEngine -- pi is then the improved policy.  playout_cap: SelfPlayEngine
    -- only the moves searched with the full budget yield rows.  forced_playouts: SelfPlayEngine -- pi is
    then the pruned policy target.  surprise: SelfPlayEngine -- the Examples then carry `kl`.
    search_value: SelfPlayEngine -- the Examples then carry `q`.  eval_symmetry: SelfPlayEngine (DESIGN.md
    3.19) -- every leaf is evaluated under a hashed board symmetry (True: seeded by `seed`).  fpu: SelfPlayEngine (DESIGN.md
    3.20) -- first-play urgency reduction in the select rule.  ownership: SelfPlayEngine -- the Examples then
    carry `fown`, `fopp`.  resign: SelfPlayEngine -- decided games end early; a resigned game's rows are the
    first rows of the game it would have been."""
    check_ownership(ownership)
    check_resign(resign, ownership=ownership)
    check_search_value(search_value)
    _check_search_options(sims, reuse_subtree, leaves_per_step, dirichlet_eps, gumbel, playout_cap, forced_playouts, fpu, solver)
    if evaluator is None:
        from .mlp import DeviceMLP
        evaluator = ("mlp_bf16" if isinstance(net, DeviceMLP) else "net_bf16") if net is not None else "uniform"
    eval_symmetry = check_eval_symmetry(eval_symmetry, seed, game, evaluator)
    if pipelines is None:
        pipelines = 2 if (evaluator.startswith(("net_", "mlp_")) and n_games >= 2) else 1
    sp = PipelinedSelfPlay(game, n_games, sims, evaluator, net, pipelines, game_id_base=game_id_base,
                           game_id_stride=game_id_stride, device=device, c_puct=c_puct, temp_moves=temp_moves,
                           openings=openings, seed=seed, rounds=1, dirichlet_alpha=dirichlet_alpha,
                           dirichlet_eps=dirichlet_eps, reuse_subtree=reuse_subtree, leaves_per_step=leaves_per_step,
                           gumbel=gumbel, playout_cap=playout_cap, forced_playouts=forced_playouts, surprise=surprise,
                           search_value=search_value, eval_symmetry=eval_symmetry, fpu=fpu, ownership=ownership, solver=solver,
                           resign=resign)
    sp.run_iteration()
    ex = sp.examples()
    return ex.states(), ex.pi, ex.z, ex
