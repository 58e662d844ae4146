"""The setters on a live engine refuse exactly the pairs of the options' conflict table ("The search mode"), in both
orders: test_gpu_early_stop.py's test_the_setters_refuse_each_other_on_a_live_engine_in_both_orders over the whole table.  No
search is run: engines are created and setters called."""
import pytest
import torch

from betazero_amd import _lib
from betazero_amd.engine import (SEARCH_OPTION_CONFLICTS, SEARCH_OPTIONS, EarlyStop, ForcedPlayouts, Fpu, GumbelConfig, PlayoutCap,
                                 Resign, SelfPlayEngine)
from test_gpu_early_stop import _bf16_net

pytestmark = pytest.mark.gpu

# the keywords that switch option A on in an engine, and every option such an engine then has on
BUILD = {"reuse_subtree": dict(reuse_subtree=True), "leaves_per_step": dict(leaves_per_step=2),
         "dirichlet_eps": dict(dirichlet_alpha=0.3, dirichlet_eps=0.25), "gumbel": dict(gumbel=GumbelConfig()),
         "gumbel_interior": dict(gumbel=GumbelConfig(interior="gumbel")), "playout_cap": dict(playout_cap=PlayoutCap(4, 0.25)),
         "forced_playouts": dict(forced_playouts=ForcedPlayouts()), "fpu": dict(fpu=Fpu()), "solver": dict(solver=True),
         "early_stop": dict(early_stop=EarlyStop()), "root_store": dict(root_store=(16, 2)), "surprise": dict(surprise=True),
         "search_value": dict(search_value=True), "ownership": dict(ownership=True), "resign": dict(resign=Resign())}
ALSO_ON = {"gumbel_interior": ("gumbel",)}  # (the interior rule needs Gumbel root search)
PAIRS = {frozenset(p[:2]) for p in SEARCH_OPTION_CONFLICTS}


def _first_conflict(b, on):
    """the option of `on` the table refuses setter b with first (cfg-carried first, then table order), or None"""
    for x, y, _ in SEARCH_OPTION_CONFLICTS:
        other = y if x == b else x if y == b else None
        if other in on:
            return other
    return None


def test_every_setter_refuses_exactly_the_pairs_of_the_table_on_a_live_engine():
    L = _lib.lib()
    assert set(BUILD) == set(SEARCH_OPTIONS)
    st = torch.cuda.current_stream().cuda_stream
    buf = torch.zeros(1 << 22, dtype=torch.uint8, device="cuda:0")  # every setter's buffer: nothing searches, nothing reads it
    p, nb = buf.data_ptr() + ((-buf.data_ptr()) & 255), (1 << 22) - 256
    setters = {  # option B: (its raw setter switched on, the same switched off)
        "gumbel": (lambda h: L.bz_engine_set_gumbel(h, 16, 1.0, 50.0, 0.1, p, nb, st), lambda h: L.bz_engine_set_gumbel(h, 0, 0.0, 0.0, 0.0, None, 0, st)),
        "gumbel_interior": (lambda h: L.bz_engine_set_gumbel_interior(h, 1, p, nb, st), lambda h: L.bz_engine_set_gumbel_interior(h, 0, None, 0, st)),
        "playout_cap": (lambda h: L.bz_engine_set_playout_cap(h, 4, 16384, p, nb, st), lambda h: L.bz_engine_set_playout_cap(h, 0, 0, None, 0, st)),
        "forced_playouts": (lambda h: L.bz_engine_set_forced_playouts(h, 2.0, 1, st), lambda h: L.bz_engine_set_forced_playouts(h, 0.0, 0, st)),
        "fpu": (lambda h: L.bz_engine_set_fpu(h, 1, 0.2, 0.1, p, nb, st), lambda h: L.bz_engine_set_fpu(h, 0, 0.0, 0.0, None, 0, st)),
        "solver": (lambda h: L.bz_engine_set_solver(h, 1, p, nb, st), lambda h: L.bz_engine_set_solver(h, 0, None, 0, st)),
        "early_stop": (lambda h: L.bz_engine_set_early_stop(h, 1, 1, p, nb, st), lambda h: L.bz_engine_set_early_stop(h, 0, 0, None, 0, st)),
        "root_store": (lambda h: L.bz_engine_set_root_store(h, p, nb, 16, 2, st), lambda h: L.bz_engine_set_root_store(h, None, 0, 16, 2, st)),
        "surprise": (lambda h: L.bz_engine_set_surprise(h, p, nb, st), lambda h: L.bz_engine_set_surprise(h, None, 0, st)),
        "search_value": (lambda h: L.bz_engine_set_search_value(h, p, nb, st), lambda h: L.bz_engine_set_search_value(h, None, 0, st)),
        "ownership": (lambda h: L.bz_engine_set_ownership(h, p, nb, st), lambda h: L.bz_engine_set_ownership(h, None, 0, st)),
        "resign": (lambda h: L.bz_engine_set_resign(h, -0.9, 2, 6554, p, nb, st), lambda h: L.bz_engine_set_resign(h, 0.0, 0, 0, None, 0, st)),
    }
    assert set(setters) == set(SEARCH_OPTIONS) - {"reuse_subtree", "leaves_per_step", "dirichlet_eps"}  # (cfg-carried: the "A" side only)
    dn = _bf16_net()
    engines = {}

    def engine(a, net=False, **more):
        """Reversi, 4 games, 16 simulations, option `a` on; the hash evaluator unless the root store needs the carry-over cache"""
        key = (a, net, tuple(more))
        if key not in engines:
            kw = {**BUILD[a], **more}
            if net or "root_store" in kw:
                engines[key] = SelfPlayEngine("reversi", 4, 16, "net_bf16", net=dn, **{"root_store": False, **kw})
            else:
                engines[key] = SelfPlayEngine("reversi", 4, 16, "hash", **kw)
        return engines[key]

    n_refused = n_accepted = 0
    for a in SEARCH_OPTIONS:
        for b, (switch_on, switch_off) in setters.items():
            on = (a,) + ALSO_ON.get(a, ())
            if b in on:
                continue
            if b == "gumbel_interior":  # its requirement first: an engine with A and Gumbel root search, where there is one
                if frozenset((a, "gumbel")) in PAIRS:
                    continue
                eng, on = engine(a, gumbel=GumbelConfig()), on + ("gumbel",)
            else:
                eng = engine(a, net=b == "root_store")  # (without the carry-over cache bz_engine_set_root_store only switches off)
            other = _first_conflict(b, on)
            assert (other is not None) == any(frozenset((x, b)) in PAIRS for x in on)
            rc = switch_on(eng.h)
            if other is None:
                assert rc == _lib.BZ_OK, (a, b, L.bz_last_error())
                assert switch_off(eng.h) == _lib.BZ_OK, (a, b, L.bz_last_error())
                n_accepted += 1
            else:
                err = L.bz_last_error()
                assert rc == _lib.BZ_EINVAL, (a, b, rc)
                assert err.startswith(f"bz_engine_set_{b}: {SEARCH_OPTIONS[b]} ".encode()), (a, b, err)
                assert f"not combine with {SEARCH_OPTIONS[other]} (".encode() in err, (a, b, err)
                n_refused += 1
    torch.cuda.synchronize()
    # the 16 setter-setter pairs in both orders, the 13 cfg-setter pairs in one, and what the interior rule inherits from Gumbel root search
    assert n_refused >= 2 * 16 + 13 and n_accepted > n_refused, (n_refused, n_accepted)
