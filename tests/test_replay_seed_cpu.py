"""The replay seed without a GPU.

The claim the seed rests on: after a search of `sims` simulations, the subtree behind a root edge with N_e visits IS the tree a
fresh search of N_e - 1 simulations from that child builds under the same evaluator -- node for node in the same creation order,
N, W and the priors bit for bit.  Checked here on the sequential twin (whose trees can be read) over every root edge of every
move of a few 4x4 / 6x6 / 8x8 games, and the fresh search's root statistics against the C oracle's.  The cases must include a
pass edge, a terminal child, N_e = 1 and an edge that took nearly all visits.

And the pacing rule (csrc/bz_pace.h through bz_pace_walk) against a Python-integer twin."""
import ctypes as C

import numpy as np
import pytest

from betazero_amd import _lib
from oracle import oracle as orc
from oracle.py_twin import Twin
from test_leaf_parallel_cpu import boards


class StampTwin(Twin):
    """the twin, every node stamped with its creation index within its search"""

    def new_node(self, b, p):
        n = super().new_node(b, p)
        n["id"] = self.made
        self.made += 1
        return n

    def search(self, b, p, sims):
        self.made = 0
        return super().search(b, p, sims)


def _nodes(root):
    """every node of the tree below root, in creation order"""
    out, stack = [], [root]
    while stack:
        n = stack.pop()
        out.append(n)
        for e in n["edges"] or []:
            if e["child"] is not None:
                stack.append(e["child"])
    return sorted(out, key=lambda n: n["id"])


def _bits(x):
    return np.float32(x).view(np.uint32)


def _same_tree(old, new):
    """old: a subtree of a longer search; new: a fresh search's tree.  Same structure in the same creation order, same N / W / P."""
    a, b = _nodes(old), _nodes(new)
    assert len(a) == len(b)
    rank = {id(n): k for k, n in enumerate(a)}
    for k, (x, y) in enumerate(zip(a, b)):
        assert y["id"] == k  # (a fresh search stamps 0, 1, 2, ...: the old subtree's nodes keep their relative order)
        assert x["term"] == y["term"] and x["tv"] == y["tv"] and x["p"] == y["p"]
        assert np.array_equal(x["b"].board, y["b"].board)
        assert (x["edges"] is None) == (y["edges"] is None)
        for ex, ey in zip(x["edges"] or [], y["edges"] or []):
            assert ex["a"] == ey["a"] and ex["N"] == ey["N"]
            assert _bits(ex["W"]) == _bits(ey["W"]) and _bits(ex["P"]) == _bits(ey["P"])
            assert (ex["child"] is None) == (ey["child"] is None)
            if ex["child"] is not None:
                assert rank[id(ex["child"])] == ey["child"]["id"]
        assert len(x["edges"] or []) == len(y["edges"] or [])


GAMES = {"reversi4": orc.GAME_REVERSI4, "reversi6": orc.GAME_REVERSI6, "reversi": orc.GAME_REVERSI}


def _check_move(tw, game, b, p, sims, seen):
    """search (b, p); compare the subtree behind EVERY root edge with a fresh search of its child; -> the root"""
    root = tw.search(b, p, sims)
    for e in root["edges"]:
        ch, Ne = e["child"], e["N"]
        if ch is None:
            continue
        if ch["term"]:
            seen.add("terminal child")
            continue
        if len(ch["edges"]) == 1 and ch["edges"][0]["a"] == 64:  # the driver skips the forced pass: the next root lies behind it
            seen.add("pass edge")
            pe = ch["edges"][0]
            ch, Ne = pe["child"], pe["N"]
            if ch is None or ch["term"]:
                continue
        if Ne == 1:
            seen.add("N_e = 1")
        if Ne >= sims - 2:
            seen.add("nearly all visits")
        keep = (ch, Ne)
        fresh = tw.search(ch["b"], ch["p"], Ne - 1)  # (restamps from 0; the old subtree keeps its stamps)
        _same_tree(keep[0], fresh)
        # ... and the C oracle's search of that child: the root statistics of the old subtree, bit for bit
        own, opp = tw.bits(ch["b"], ch["p"])
        N, W, P, _ = orc.mcts_search(GAMES[game], own, opp, ch["p"], Ne - 1, orc.EVAL_HASH) if Ne > 1 else (None,) * 4
        for oe in ch["edges"]:
            if Ne > 1:
                assert N[oe["a"]] == oe["N"] and _bits(W[oe["a"]]) == _bits(oe["W"]) and _bits(P[oe["a"]]) == _bits(oe["P"])
            else:
                assert oe["N"] == 0
    return root


@pytest.mark.parametrize("game,sims,plies", [("reversi4", 48, 12), ("reversi6", 40, 6), ("reversi", 32, 3)])
def test_a_played_childs_subtree_is_the_fresh_search_of_its_visits(game, sims, plies):
    tw = StampTwin(game, "hash", boards=boards())
    seen = set()
    for start in range(2 if game == "reversi4" else 1):
        b, p = tw.ReversiBoard(size=tw.size), 1
        for ply in range(plies):
            if tw.terminal(b)[0]:
                break
            if not tw.moves(b, p):
                p = -p
                continue
            root = _check_move(tw, game, b, p, sims, seen)
            # the move: the most visited edge, or (second game) the least visited one that was visited -- other lines, small N_e
            es = [e for e in root["edges"] if e["N"] > 0]
            pick = max(es, key=lambda e: e["N"]) if start == 0 else min(es, key=lambda e: e["N"])
            b, p = tw.play(b, p, pick["a"]), -p
    if game == "reversi4":  # the small board meets every case the issue names
        assert seen >= {"pass edge", "terminal child", "N_e = 1", "nearly all visits"}, seen


# ---------------------------------------------------------------- the pacing rule
def pace_twin(L, r, sims):
    """launch L of a slot with r walks left to make in `sims` launches: (walks?, walks made before this launch)"""
    return ((L + 1) * r) // sims > (L * r) // sims, (L * r) // sims


@pytest.mark.parametrize("sims", [1, 2, 7, 64, 800, 8189])
def test_pacing_rule_against_python_integers(sims):
    L = _lib.lib()
    walk = np.zeros(sims, np.uint8)
    done = np.zeros(sims, np.uint32)
    ls = np.arange(sims, dtype=np.int64)
    for r in range(sims + 1):
        assert L.bz_pace_walk(sims, r, walk.ctypes.data, done.ctypes.data) == _lib.BZ_OK
        # the twin over every launch (int64: no product comes near 2^63), and in Python integers at a few launches
        t_done = (ls * r) // sims
        t_walk = ((ls + 1) * r) // sims > t_done
        assert np.array_equal(walk, t_walk.astype(np.uint8)) and np.array_equal(done, t_done.astype(np.uint32))
        for l in {0, sims // 3, sims - 1}:
            assert (bool(walk[l]), int(done[l])) == pace_twin(l, r, sims)
        assert int(walk.sum()) == r                                   # exactly r walks
        assert np.all(np.diff(done.astype(np.int64)) >= 0)           # in order
        assert np.array_equal(done[walk == 1], np.arange(r))          # walk k is the slot's k-th, none twice
        if r:
            assert walk[sims - 1] == 1                                # the last walk is launch sims - 1's, none later
    assert L.bz_pace_walk(0, 0, walk.ctypes.data, done.ctypes.data) == _lib.BZ_EINVAL
    assert L.bz_pace_walk(sims, sims + 1, walk.ctypes.data, done.ctypes.data) == _lib.BZ_EINVAL
    assert L.bz_pace_walk(8190, 1, walk.ctypes.data, done.ctypes.data) == _lib.BZ_EINVAL
    assert L.bz_pace_walk(sims, 0, None, done.ctypes.data) == _lib.BZ_EINVAL
