"""The search options' conflict table ("The search mode"): csrc/bz_options.h and engine.SEARCH_OPTION_CONFLICTS are
the same pairs, every check_* refuses exactly them, and the config entry points answer what they answered before the table.
No GPU."""
import ctypes as C
import inspect
import itertools

import pytest

from betazero_amd import _lib, engine
from betazero_amd.engine import SEARCH_OPTION_CONFLICTS, SEARCH_OPTIONS

KEYS = list(SEARCH_OPTIONS)  # in BZ_OPT_* order
PAIRS = {frozenset(p[:2]) for p in SEARCH_OPTION_CONFLICTS}
# a value that switches each option on, as a check_* takes it ("other option" arguments take the same values)
ON = {"reuse_subtree": True, "leaves_per_step": 2, "dirichlet_eps": 0.25, "gumbel": engine.GumbelConfig(),
      "playout_cap": engine.PlayoutCap(4, 0.25), "forced_playouts": engine.ForcedPlayouts(), "fpu": engine.Fpu(), "solver": True,
      "early_stop": engine.EarlyStop(), "root_store": (16, 2), "surprise": True, "search_value": True, "ownership": True,
      "resign": engine.Resign()}
CHECKS = {"gumbel": engine.check_gumbel, "playout_cap": engine.check_playout_cap, "forced_playouts": engine.check_forced_playouts,
          "fpu": engine.check_fpu, "solver": engine.check_solver, "early_stop": engine.check_early_stop, "resign": engine.check_resign}


def test_the_python_table_names_every_option_and_every_pair_once():
    assert len(KEYS) == 15 and len(SEARCH_OPTION_CONFLICTS) == len(PAIRS) == 29
    for a, b, reason in SEARCH_OPTION_CONFLICTS:
        assert a in SEARCH_OPTIONS and b in SEARCH_OPTIONS and a != b and (reason is None or isinstance(reason, str))


def test_the_c_table_is_the_python_table():
    L = _lib.lib()
    n = 0
    while L.bz_option_name(n) is not None:
        n += 1
    assert n == len(KEYS)  # the two option lists have the same length ...
    for i, key in enumerate(KEYS):  # ... and the same phrases in the same order
        assert L.bz_option_name(i).decode() == SEARCH_OPTIONS[key]
    for i, j in itertools.product(range(n), repeat=2):
        want = int(frozenset((KEYS[i], KEYS[j])) in PAIRS)
        assert L.bz_option_conflict(i, j) == L.bz_option_conflict(j, i) == want, (KEYS[i], KEYS[j])
    for bad in (-1, n, n + 1, 1 << 20, -(1 << 31)):
        assert L.bz_option_name(bad) is None
        assert L.bz_option_conflict(bad, 0) == L.bz_option_conflict(0, bad) == L.bz_option_conflict(bad, bad) == -1


def _others(name):
    """the "other option" keywords check_<name> takes"""
    return [p for p in inspect.signature(CHECKS[name]).parameters if p in SEARCH_OPTIONS and p != name]


def _call(name, other):
    args = (ON[name], 16) if name == "playout_cap" else (ON[name],)  # (check_playout_cap also takes sims)
    return CHECKS[name](*args, **{other: ON[other]})


def test_every_direction_some_check_can_express_is_covered():
    expressed = {frozenset((name, other)) for name in CHECKS for other in _others(name)}
    # every pair has at least one direction, but for the interior rule (no pair) nothing is missing
    assert PAIRS <= expressed, PAIRS - expressed


@pytest.mark.parametrize("name", list(CHECKS))
def test_each_check_refuses_exactly_the_pairs_of_the_table(name):
    others = _others(name)
    assert others
    for other in others:
        if frozenset((name, other)) in PAIRS:
            with pytest.raises(ValueError) as ei:
                _call(name, other)
            msg = str(ei.value)
            assert msg.startswith(f"{name}: {SEARCH_OPTIONS[name]} ") and "not combine with" in msg, msg
            assert f"{SEARCH_OPTIONS[other]} ({other})" in msg, msg
        else:
            assert _call(name, other) is not None
    # off: nothing is refused, whatever else is on
    assert not CHECKS[name](*((None, 16) if name == "playout_cap" else (None,)), **{o: ON[o] for o in others})


def test_no_pair_outside_the_table_is_refused_by_the_one_refusal():
    for a, b in itertools.permutations(KEYS, 2):
        if frozenset((a, b)) in PAIRS:
            with pytest.raises(ValueError, match=rf"\({b}\)"):
                engine.refuse_option_conflict(a, {b: ON.get(b, True)})
        else:
            engine.refuse_option_conflict(a, {b: ON.get(b, True)})
    engine.refuse_option_conflict("early_stop", {"gumbel": None, "solver": False, "leaves_per_step": 1, "dirichlet_eps": 0.0,
                                                 "reuse_subtree": False, "root_store": None})


def test_a_refusal_gives_the_reason_of_the_table():
    with pytest.raises(ValueError, match="both score \\+inf$"):
        engine.check_solver(True, forced_playouts=True)
    with pytest.raises(ValueError, match=r"^ownership: ownership targets do not combine with resignation \(resign\): a resigned game"):
        engine.refuse_option_conflict("ownership", {"resign": True})
    with pytest.raises(ValueError, match=r"^fpu: first-play urgency reduction does not combine with the solver \(solver\)$"):
        engine.refuse_option_conflict("fpu", {"solver": True})


# ---- the config entry points: what the build before the table answered (recorded by running it), for a Reversi config of 4 games
# and 16 simulations with the net_bf16 evaluator and the carry-over cache -- plain, with subtree reuse, with leaves_per_step = 2
# and with dirichlet_eps = 0.25
def _cfg(flags=0, eps=0.0):
    return _lib.EngineCfg(1, 4, 16, _lib.EVAL_NET_BF16, 1.5, 0, 0, 1, 64, 0, 0, 0, 4,
                          flags | _lib.ENGINE_EVAL_CACHE | _lib.ENGINE_EVAL_CACHE_CARRY, 0.3 if eps else 0.0, eps, 0)


CFGS = {"plain": _cfg(), "reuse": _cfg(_lib.ENGINE_REUSE_SUBTREE), "leaves2": _cfg(1 << _lib.ENGINE_LEAVES_SHIFT), "dirichlet": _cfg(eps=0.25)}
RECORDED = {
    "bz_engine_gumbel_bytes": ((16,), {"plain": 1536, "reuse": -1, "leaves2": -1, "dirichlet": -1}),
    "bz_engine_gumbel_interior_bytes": ((), {"plain": 512, "reuse": -1, "leaves2": -1, "dirichlet": -1}),
    "bz_engine_playout_cap_bytes": ((), {"plain": 256, "reuse": -1, "leaves2": -1, "dirichlet": 256}),
    "bz_engine_forced_playouts_check": ((C.c_float(2.0),), {"plain": 0, "reuse": 1, "leaves2": 1, "dirichlet": 0}),
    "bz_engine_fpu_bytes": ((), {"plain": 256, "reuse": -1, "leaves2": -1, "dirichlet": 256}),
    "bz_engine_fpu_check": ((C.c_float(0.2), C.c_float(0.1)), {"plain": 0, "reuse": 1, "leaves2": 1, "dirichlet": 0}),
    "bz_engine_solver_bytes": ((), {"plain": 512, "reuse": -1, "leaves2": -1, "dirichlet": 512}),
    "bz_engine_solver_check": ((), {"plain": 0, "reuse": 1, "leaves2": 1, "dirichlet": 0}),
    "bz_engine_early_stop_bytes": ((), {"plain": 512, "reuse": -1, "leaves2": -1, "dirichlet": 512}),
    "bz_engine_early_stop_check": ((), {"plain": 0, "reuse": 1, "leaves2": 1, "dirichlet": 0}),
    "bz_engine_surprise_bytes": ((), {"plain": 2048, "reuse": 2048, "leaves2": 2048, "dirichlet": 2048}),
    "bz_engine_search_value_bytes": ((), {"plain": 1024, "reuse": 1024, "leaves2": 1024, "dirichlet": 1024}),
    "bz_engine_ownership_bytes": ((), {"plain": 2048, "reuse": 2048, "leaves2": 2048, "dirichlet": 2048}),
    "bz_engine_resign_bytes": ((), {"plain": 1280, "reuse": 1280, "leaves2": 1280, "dirichlet": 1280}),
    "bz_engine_root_store_bytes": ((16, 2), {"plain": 201728, "reuse": 0, "leaves2": 0, "dirichlet": 201728}),
}
HOW = {"reuse": b"subtree reuse (BZ_ENGINE_REUSE_SUBTREE)", "leaves2": b"leaves_per_step > 1 (BZ_ENGINE_LEAVES_*)",
       "dirichlet": b"Dirichlet noise (dirichlet_eps > 0)"}


def test_every_config_entry_point_has_a_recorded_answer():
    """(every exported *_bytes / *_check that takes an engine config and belongs to an option)"""
    have = {n for n in _lib.ABI_SYMBOLS if n.startswith("bz_engine_") and n.endswith(("_bytes", "_check")) and n != "bz_engine_workspace_bytes"}
    assert have == set(RECORDED), have ^ set(RECORDED)


@pytest.mark.parametrize("fn", list(RECORDED))
def test_the_config_entry_points_answer_what_they_answered_before_the_table(fn):
    L = _lib.lib()
    args, want = RECORDED[fn]
    for key, cfg in CFGS.items():
        got = getattr(L, fn)(C.byref(cfg), *args)
        assert got == want[key], (fn, key, got)
        if got not in (0, want["plain"]):  # a refusal: the message names the function and how the config carries the option
            err = L.bz_last_error()
            assert err.startswith(fn.encode() + b": ") and b"not combine with " + HOW[key] in err, err
    assert _lib.BZ_EINVAL == 1
