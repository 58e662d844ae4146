"""The replay seed and the paced tree step: a slot whose previous search is carried over starts its search from a
copy of the played child's old subtree and makes its remaining walks in the launches csrc/bz_pace.h gives it.  Nothing may
change: every test runs an engine with the seed beside one with replay_seed=False on the same games, in lockstep, and compares
after EVERY move the root N / W / P bits, every work counter and the boards, then every example tensor; and every case holds
that slots were in fact seeded (each seeded simulation is a tree step the slot sat out), so that none passes idle.  Small shapes:
net_f32 32 channels x 2 blocks and net_bf16 64 x 2 (the narrowest bf16 tower), 8 - 64 games, 64 - 200 simulations, staggered
pools; one case with 320 slots per pipeline, where both tower shapes serve paced launches; a few games against the oracle."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _module(C=32, NB=2, seed=3, bf16=False, sharp=1.0):
    """sharp: the policy head's logits scaled -- a random net's priors are near uniform, and 64 simulations then leave no root
    edge with a single visit"""
    from betazero_amd.net import PolicyValueNet
    torch.manual_seed(seed)
    m = PolicyValueNet(C, NB, 64)
    with torch.no_grad():
        m.polfc.weight.mul_(sharp); m.polfc.bias.mul_(sharp)
    return m.round_to_bf16_() if bf16 else m


def _dn(B, mode="f32", seed=3):
    from betazero_amd.net import DeviceNet
    return DeviceNet.from_module(_module(64, 2, seed, True) if mode == "bf16" else _module(32, 2, seed), B)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _pair(game, B, sims, mode, dn, **kw):
    from betazero_amd.engine import SelfPlayEngine
    return [SelfPlayEngine(game, B, sims, "net_" + mode, net=dn, replay_seed=on, **kw) for on in (True, False)]


def _stones(own, opp):
    return np.array([bin(int(a) | int(b)).count("1") for a, b in zip(own, opp)])


def _lockstep(on, off, moves, at=None):
    """`moves` moves (search, play with restart) on both engines; compared after every search: root N / W / P and every counter,
    after every play: the boards; at the end every example tensor.  at: {move: fn()} called before that move's search.  Returns
    what the run saw: the visits of every played edge, forced passes, finished games, the seed's counters after every move."""
    seen = {"Ne": [], "passes": 0, "seeds": []}
    for e in (on, off):
        e.reset_games(); e.reset_counters()
    for mv in range(moves):
        if at and mv in at:
            at[mv]()
        for e in (on, off):
            e.search()
        sa, sb = on.root_stats(), off.root_stats()
        for x, y, what in zip(sa, sb, "NWP"):
            assert np.array_equal(_bits(x), _bits(y)), ("root stats", what, mv)
        ca, cb = on.counters(), off.counters()
        assert ca == cb, ("counters", mv, {k: (ca[k], cb[k]) for k in ca if ca[k] != cb[k]})
        seen["seeds"].append(on.replay_seed_counters())
        own0, opp0, tm0, st0 = on.positions()
        _, act = on.root_policy()
        live = st0 == 0
        seen["Ne"] += [int(sa[0][g, act[g]]) for g in np.nonzero(live)[0]]
        for e in (on, off):
            e.play(True)
        pa, pb = on.positions(), off.positions()
        for x, y in zip(pa, pb):
            assert np.array_equal(x, y), ("boards", mv)
        # a forced pass: the same side moves again in a game that went on (one stone more on the board)
        seen["passes"] += int((live & (pa[3] == 0) & (pa[2] == tm0) & (_stones(pa[0], pa[1]) == _stones(own0, opp0) + 1)).sum())
    ta, tb = on.example_tensors(), off.example_tensors()
    for k in ta:
        assert np.array_equal(_bits(ta[k].cpu().numpy()), _bits(tb[k].cpu().numpy())), ("examples", k)
    seen["finished"] = on.status()[1]
    assert off.status()[1] == seen["finished"]
    assert off.replay_seed_counters() == {"n_replay_seeds": 0, "n_replay_sims": 0}
    return seen


def _busy(seen):
    s = seen["seeds"][-1]
    assert s["n_replay_seeds"] > 0 and s["n_replay_sims"] >= s["n_replay_seeds"], s  # seeded slots, tree steps they sat out
    assert seen["seeds"][0] == {"n_replay_seeds": 0, "n_replay_sims": 0}            # (the first search has nothing to copy)


# (game, mode, B, sims, stagger, moves, temp_moves)
SHAPES = {"8x8-f32": ("reversi", "f32", 32, 64, 12, 6, 64), "6x6-f32": ("reversi6", "f32", 16, 200, 30, 6, 2),
          "8x8-bf16": ("reversi", "bf16", 16, 128, 10, 4, 8), "6x6-bf16": ("reversi6", "bf16", 8, 96, 28, 5, 0),
          "4x4-f32": ("reversi4", "f32", 16, 64, 6, 12, 4)}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_seeded_engine_equals_an_unseeded_one_after_every_move(shape):
    game, mode, B, sims, stagger, moves, temp = SHAPES[shape]
    on, off = _pair(game, B, sims, mode, _dn(B, mode), temp_moves=temp, openings=1, seed=5, rounds=8, stagger=stagger)
    seen = _lockstep(on, off, moves)
    _busy(seen)
    print(shape, "N_e of the played edges:", sorted(seen["Ne"])[:6], "...", sorted(seen["Ne"])[-6:], seen["seeds"][-1])
    if shape == "4x4-f32":   # the small board: forced passes, edges with all the visits (one legal move), games that end (terminal
        # children in the copied subtrees) and restart beside carried slots, and restarted slots the root store seeds
        assert seen["passes"] > 0 and seen["finished"] > 0 and max(seen["Ne"]) >= sims - 2, (seen["passes"], seen["finished"])
        r = on.root_store_counters()
        assert r["n_seeded_searches"] > 0 and r == off.root_store_counters(), r


def test_roots_set_to_chosen_children_are_seeded_with_exactly_their_visits():
    """N_e = 1 and the largest N_e, made to happen: after one search every slot's root is SET (set_roots) to the child behind an
    edge picked from its root statistics -- even slots the least visited edge, odd slots the most visited one -- and searched again.
    The carry-over is the slot's, whatever moved the root, so the seed must fire for exactly the slots with N_e >= 2 (a child
    visited once was created and never walked: nothing to copy), with exactly N_e - 1 simulations each; a child behind a forced
    pass or a finished game is not a root the driver would search and is left out."""
    from betazero_amd.engine import SelfPlayEngine
    from betazero_amd.net import DeviceNet
    from oracle import oracle as orc
    B, sims = 64, 64
    dn = DeviceNet.from_module(_module(sharp=12.0), B)
    on, off = [SelfPlayEngine("reversi", B, sims, "net_f32", net=dn, replay_seed=r, openings=1, seed=5, stagger=14) for r in (True, False)]
    for e in (on, off):
        e.reset_games(); e.reset_counters(); e.search()
    N = on.root_stats()[0]
    own, opp, tm, st = on.positions()
    n_own, n_opp, n_tm = np.zeros(B, np.uint64), np.zeros(B, np.uint64), np.zeros(B, np.int8)
    picked = []
    for g in range(B):
        acts = [a for a in range(64) if N[g, a] > 0]
        if st[g] != 0 or not acts:
            continue
        a = min(acts, key=lambda a: (N[g, a], a)) if g % 2 == 0 else max(acts, key=lambda a: (N[g, a], -a))
        o2, p2, _ = orc.reversi_apply(int(own[g]), int(opp[g]), 8, a // 8, a % 8)
        if orc.reversi_game_over(p2, o2, 8) or orc.reversi_legal(p2, o2, 8) == 0:
            continue
        n_own[g], n_opp[g], n_tm[g] = p2, o2, -tm[g]   # (the child, seen by its mover; to_move 0 = the slot sits out)
        picked.append(int(N[g, a]))
    assert min(picked) == 1 and max(picked) >= sims // 2, sorted(picked)
    for e in (on, off):
        e.set_roots(n_own, n_opp, n_tm)
        e.search()
    for x, y, what in zip(on.root_stats(), off.root_stats(), "NWP"):
        assert np.array_equal(_bits(x), _bits(y)), ("root stats", what)
    assert on.counters() == off.counters()
    on.status(); off.status()
    s = on.replay_seed_counters()
    assert s == {"n_replay_seeds": sum(1 for n in picked if n >= 2), "n_replay_sims": sum(n - 1 for n in picked if n >= 2)}, (s, sorted(picked))


def test_nothing_is_seeded_across_a_weight_update():
    B, sims = 16, 64
    dn = _dn(B)
    on, off = _pair("reversi", B, sims, "f32", dn, temp_moves=8, openings=1, seed=6, stagger=10)
    seen = _lockstep(on, off, 5, at={3: lambda: dn.update(_module(seed=11).flat_params())})
    _busy(seen)
    s = seen["seeds"]
    assert s[2]["n_replay_seeds"] > s[1]["n_replay_seeds"]   # seeded before the update ...
    assert s[3] == s[2]                                      # ... nothing in the search behind it ...
    assert s[4]["n_replay_seeds"] > s[3]["n_replay_seeds"]   # ... and again from the next one on


def test_the_switch_and_the_other_ways_to_search_take_no_seed():
    """set_replay_seed(False) on a live engine, Dirichlet noise, eval_cache="search" and the step API: the counters stand still"""
    from betazero_amd.engine import SelfPlayEngine
    B, sims = 8, 64
    dn = _dn(B)
    kw = dict(temp_moves=4, openings=1, seed=7, stagger=8)
    e = SelfPlayEngine("reversi", B, sims, "net_f32", net=dn, replay_seed=True, **kw)
    e.reset_games(); e.reset_counters()
    for _ in range(2):
        e.search(); e.play(True)
    a = e.replay_seed_counters()
    assert a["n_replay_seeds"] > 0
    e.set_replay_seed(False)
    e.search(); e.play(True)
    assert e.replay_seed_counters() == a
    e.set_replay_seed(True)
    e.search(); e.play(True)      # (the search before was not a paced one: nothing to copy from)
    assert e.replay_seed_counters() == a
    e.search(); e.play(True)
    assert e.replay_seed_counters()["n_replay_seeds"] > a["n_replay_seeds"]
    for other in (dict(dirichlet_alpha=0.3, dirichlet_eps=0.25), dict(eval_cache="search"), dict(fpu=True), dict(replay_seed=None)):
        other = dict(dict(replay_seed=True), **other)  # (None: by the engine's size, and 8 games are few)
        o = SelfPlayEngine("reversi", B, sims, "net_f32", net=dn, **kw, **other)
        o.reset_games(); o.reset_counters()
        for _ in range(3):
            o.search(); o.play(True)
        assert o.replay_seed_counters() == {"n_replay_seeds": 0, "n_replay_sims": 0}, other
    with pytest.raises(ValueError, match="replay_seed"):
        SelfPlayEngine("reversi", B, sims, "net_f32", net=dn, replay_seed=1)
    big = SelfPlayEngine("reversi", 1025, 8, "net_f32", net=_dn(1025), **kw)  # the default: on from 1025 games up
    big.reset_games(); big.reset_counters()
    for _ in range(3):
        big.search(); big.play(True)
    assert big.replay_seed_counters()["n_replay_seeds"] > 0


@pytest.mark.parametrize("mode,B,sims,moves", [("f32", 16, 64, 5), ("bf16", 640, 64, 4)], ids=["2x8", "2x320-both-tower-shapes"])
def test_two_paced_pipelines_equal_two_unpaced(mode, B, sims, moves):
    from betazero_amd.engine import PipelinedSelfPlay
    dn = _dn(B // 2, mode)
    kw = dict(pipelines=2, temp_moves=8, openings=1, seed=9, stagger=14)
    on = PipelinedSelfPlay("reversi", B, sims, "net_" + mode, dn, replay_seed=True, **kw)
    off = PipelinedSelfPlay("reversi", B, sims, "net_" + mode, dn, replay_seed=False, **kw)
    for sp in (on, off):
        sp.reset_games(); sp.reset_counters()
    for mv in range(moves):
        for sp in (on, off):
            sp.step(True)
        ca, cb = on.counters(), off.counters()
        assert ca == cb, ("counters", mv, {k: (ca[k], cb[k]) for k in ca if ca[k] != cb[k]})
        for ea, eb in zip(on.engines, off.engines):
            for x, y in zip(ea.positions(), eb.positions()):
                assert np.array_equal(x, y), ("boards", mv)
            for x, y, what in zip(ea.root_stats(), eb.root_stats(), "NWP"):
                assert np.array_equal(_bits(x), _bits(y)), ("root stats", what, mv)
    for ea, eb in zip(on.engines, off.engines):
        ta, tb = ea.example_tensors(), eb.example_tensors()
        for k in ta:
            assert np.array_equal(_bits(ta[k].cpu().numpy()), _bits(tb[k].cpu().numpy())), ("examples", k)
    on.status(); off.status()
    s = on.replay_seed_counters()
    assert s["n_replay_seeds"] > B and s["n_replay_sims"] > s["n_replay_seeds"], s
    assert off.replay_seed_counters() == {"n_replay_seeds": 0, "n_replay_sims": 0}


def test_paced_selfplay_equals_the_oracle():
    """as tests/test_gpu_search_net.py: the games of a paced two-pipeline pool against orc.selfplay_game, row for row, and the
    work counters of the searched moves"""
    from betazero_amd.engine import PipelinedSelfPlay
    from test_gpu_search_net import ENGINE_EVAL, _dn as exact_dn, _games_equal_oracle, _net
    mode, B, sims, moves = "bf16", 8, 64, 5
    P, on = _net(mode, 64, 1)
    sp = PipelinedSelfPlay("reversi", B, sims, ENGINE_EVAL[mode], exact_dn(P, B // 2), pipelines=2, temp_moves=8, openings=1, seed=0,
                           replay_seed=True)
    sp.reset_games(); sp.reset_counters()
    for _ in range(moves):
        sp.step(False)
    sp.status()
    h = B // 2
    for i, e in enumerate(sp.engines):
        _games_equal_oracle(e, "reversi", mode, on, [i * h + s for s in range(h)], sims, slots=list(range(h)), max_moves=moves,
                            temp_moves=8, openings=1, seed=0)
    s = sp.replay_seed_counters()
    assert s["n_replay_seeds"] > 0 and s["n_replay_sims"] > 0, s
