"""Proven wins, losses and draws without a GPU: bz_solver_node / bz_solver_pick -- the functions the kernels run
-- against restatements, the solver twin (SolverTwin: CapTwin with the rule in simulate, the proof pass behind the backup and the
move rule), its soundness against a plain negamax over the twin's own play / terminal functions, its completeness on the
tic-tac-toe endgames, its invariants, and the ABI / Python validation.  tests/test_gpu_solver.py pins the engine to this twin."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import betazero_amd as bz
from betazero_amd import _lib
from oracle.py_twin import Twin, f32, rng_draw
from test_forced_playouts_cpu import _score
from test_ownership_cpu import OwnTwin, winner_of
from test_playout_cap_cpu import CapTwin, _cfg, boards, cap_budget
from test_surprise_cpu import _Surprise
from test_value_targets_cpu import _Value

UND = 2  # "undecided" at the ABI
TTT_GW = 4  # lanes per tic-tac-toe game in the tree kernels (csrc/bz_rules.h)
S_COMPLETE = 256  # the smallest power of two at which the twin decides every tic-tac-toe root with >= 5 stones (uniform evaluator)


# ---------------------------------------------------------------- the two rules, restated
def node_rule(vals):
    """vals: every edge's decided value for the child's mover (-1, 0, +1) or None -> the node's value for its mover or None"""
    if any(c == -1 for c in vals):
        return 1
    if not vals or any(c is None for c in vals):
        return None
    return max(-c for c in vals)


def pick_rule(N, vals, tau1, draw):
    """the index of the played root edge"""
    for i, c in enumerate(vals):
        if c == -1:
            return i
    keep = [i for i, c in enumerate(vals) if c != 1]
    if sum(N[i] for i in keep) == 0:
        keep = list(range(len(N)))
    tot = sum(N[i] for i in keep)
    if tau1:
        if tot == 0:
            return 0
        r, cum = draw % tot, 0
        for i in keep:
            cum += N[i]
            if cum > r:
                return i
    best, bn = 0, 0
    for i in keep:
        if N[i] > bn:
            best, bn = i, N[i]
    return best


class SolverTwin(CapTwin):
    """CapTwin with the solver.  An edge carries "c": its decided value for the mover at its child, or None.  cap = (fast_sims,
    full_q) or None (every search full).  Per search: root["proven"] (the recorded root value or None), n_decided, n_stops.  Over
    the twin's life: max_depth (the longest walk), n_pass_proofs (pass nodes decided), n_walks.  After selfplay(): log = one dict
    per search."""

    def __init__(self, game, eval_kind, cap=None, eval_fn=None, **kw):
        fast, full_q = cap if cap is not None else (0, 65536)
        super().__init__(game, eval_kind, fast, full_q, eval_fn=eval_fn, **kw)
        self.n_decided = self.n_stops = self.max_depth = self.n_pass_proofs = self.n_walks = 0
        self.log = []

    def search(self, b, p, sims):
        self.n_decided = self.n_stops = 0
        root = super().search(b, p, sims)
        root.setdefault("proven", None)
        root["n_decided"], root["n_stops"] = self.n_decided, self.n_stops  # this search's two counts
        return root

    def simulate(self, root):
        node, path = root, []
        while True:
            edges = node["edges"]
            sumN = sum(e["N"] for e in edges)
            sq = np.sqrt(f32(max(sumN, 1)))
            best, bests = None, None
            for e in edges:
                c = e.get("c")
                q = e["W"] / f32(e["N"]) if e["N"] > 0 else f32(0.0)
                if c == 0:
                    q = f32(0.0)
                s = _score(q, self.c, e["P"], sq, e["N"])
                if c == -1:
                    s = f32(np.inf)
                elif c == 1:
                    s = f32(-np.inf)
                if best is None or s > bests:  # (edge 0 stands in when every edge scores -inf)
                    best, bests = e, s
            path.append((node, best))
            if best["child"] is not None:
                if best.get("c") is not None:  # a decided edge ends the walk: no walk passes one
                    v = f32(best["c"])
                    proven = True
                    self.n_stops += not best["child"]["term"]
                    break
                node = best["child"]
                continue
            ch = self.new_node(self.play(node["b"], node["p"], best["a"]), -node["p"])
            best["child"] = ch
            proven = ch["term"]
            if ch["term"]:
                best["c"] = int(ch["tv"])
                v = f32(ch["tv"])
            else:
                v = self.expand(ch)
            break
        val = -v
        for _, e in reversed(path):
            e["N"] += 1
            e["W"] = f32(e["W"] + val)
            val = -val
        self.n_walks += 1
        self.max_depth = max(self.max_depth, len(path))
        if proven:  # the proof pass
            d = len(path) - 1
            while True:
                x = path[d][0]
                pv = node_rule([e.get("c") for e in x["edges"]])
                if pv is None:
                    break
                if d == 0:
                    if root.get("proven") is None:
                        root["proven"] = pv
                        self.n_decided += 1
                    break
                assert path[d - 1][1].get("c") is None
                path[d - 1][1]["c"] = pv
                self.n_decided += 1
                self.n_pass_proofs += len(x["edges"]) == 1 and x["edges"][0]["a"] == 64
                d -= 1

    def pick(self, root, tau1, draw):
        e = root["edges"]
        return e[pick_rule([x["N"] for x in e], [x.get("c") for x in e], tau1, draw)]

    def selfplay(self, gid, sims, temp_moves, openings, seed, slot=0, stagger=0):
        b, p, made = self.start(slot, gid, openings, seed, stagger)
        ex, passes = [], 0
        self.budgets, self.root_sums, self.log = [], [], []
        while True:
            budget = cap_budget(seed, gid, made, sims, self.fast_sims, self.full_q)
            full = budget == sims
            self.noise_key, self.noise_on = (seed, gid, made), full
            root = self.search(b, p, budget)
            edges = root["edges"]
            N = [e["N"] for e in edges]
            sumN = sum(N)
            self.budgets.append(budget)
            self.root_sums.append(sumN)
            pick = self.pick(root, made < temp_moves, rng_draw(seed, gid, made))
            pi = [f32(0.0)] * self.na
            for e in edges:
                pi[e["a"]] = f32(e["N"]) / f32(sumN)
            self.log.append({"budget": budget, "b": b, "p": p, "a": [e["a"] for e in edges], "N": N, "W": [e["W"] for e in edges],
                             "P": [e["P"] for e in edges], "c": [e.get("c") for e in edges], "proven": root["proven"], "pi": pi,
                             "act": pick["a"], "n_decided": self.n_decided, "n_stops": self.n_stops})
            if full:
                own, opp = self.bits(b, p)
                ex.append((own, opp, pi, p, pick["a"]))
            b = self.play(b, p, pick["a"])
            p, made = -p, made + 1
            over, w = self.terminal(b)
            if over:
                return ex, w, passes
            if not self.moves(b, p):
                p, passes = -p, passes + 1


# ---------------------------------------------------------------- the yardstick: plain negamax over the twin's own functions
def negamax(tw, b, p, memo):
    """the game-theoretic value of (b, p to move) for p; a mover without a move passes (the twin's pass edge)"""
    key = (tw.bits(b, 1), p)
    if key not in memo:
        over, w = tw.terminal(b)
        if over:
            memo[key] = w * p
        else:
            mv = tw.moves(b, p)
            memo[key] = -negamax(tw, b, -p, memo) if not mv else max(-negamax(tw, tw.play(b, p, a), -p, memo) for a in mv)
    return memo[key]


def check_sound(tw, root, memo):
    """every decided edge below `root` and the root's record equal negamax; returns the number of decided edges"""
    n, stack = 0, [root]
    if root.get("proven") is not None:
        assert root["proven"] == negamax(tw, root["b"], root["p"], memo), (root["b"], root["p"])
    while stack:
        x = stack.pop()
        for e in x["edges"] or []:
            ch = e["child"]
            if e.get("c") is not None:
                assert ch is not None and e["c"] == negamax(tw, ch["b"], ch["p"], memo), (x["b"], x["p"], e["a"])
                n += 1
            elif ch is not None:
                stack.append(ch)  # (nothing below a decided edge is ever walked again)
    return n


@functools.lru_cache(maxsize=None)
def ttt_positions(min_stones):
    """every non-terminal tic-tac-toe position reachable from the empty board with >= min_stones stones: [(board, mover)]"""
    tw = Twin("ttt", "uniform", boards=boards())
    seen, out, level = set(), [], [(bz.TicTacToeBoard(), 1)]
    while level:
        nxt = []
        for b, p in level:
            if tw.terminal(b)[0]:
                continue
            if int((b.board != 0).sum()) >= min_stones:
                out.append((b, p))
            for a in tw.moves(b, p):
                c = tw.play(b, p, a)
                k = c.board.tobytes()
                if k not in seen:
                    seen.add(k)
                    nxt.append((c, -p))
        level = nxt
    return tuple(out)


@functools.lru_cache(maxsize=None)
def rev4_positions(n=64, seed=20260):
    """n distinct non-terminal Reversi 4x4 positions with the mover able to move, from seeded random playouts, at ply >= 4"""
    tw = Twin("reversi4", "uniform", boards=boards())
    rng = np.random.default_rng(seed)
    out, seen = [], set()
    while len(out) < n:
        b, p, ply = bz.ReversiBoard(size=4), 1, 0
        while not tw.terminal(b)[0]:
            mv = tw.moves(b, p)
            if not mv:
                p = -p
                continue
            k = (tw.bits(b, 1), p)
            if ply >= 4 and k not in seen and len(out) < n and rng.random() < 0.5:
                seen.add(k)
                out.append((b, p))
            b, p, ply = tw.play(b, p, mv[int(rng.integers(len(mv)))]), -p, ply + 1
    return tuple(out)


# ---------------------------------------------------------------- the two functions
def _abi(vals):
    return np.array([UND if c is None else c for c in vals], np.int8)


def _c_node(vals):
    v = _abi(vals)
    r = int(_lib.lib().bz_solver_node(v.ctypes.data, len(v)))
    return None if r == UND else r


def _c_pick(N, vals, tau1, draw):
    n, v = np.asarray(N, np.uint32), _abi(vals)
    return int(_lib.lib().bz_solver_pick(n.ctypes.data, v.ctypes.data, len(n), int(tau1), C.c_uint64(draw)))


def test_node_rule_equals_the_restatement_on_every_assignment_up_to_five_edges_and_random_ones_up_to_34():
    for n in range(1, 6):
        for vals in itertools.product((None, -1, 0, 1), repeat=n):
            assert _c_node(vals) == node_rule(list(vals)), vals
    rng = np.random.default_rng(1)
    for _ in range(2000):
        n = int(rng.integers(1, 35))
        probs = rng.dirichlet(np.ones(4) * 0.3)
        vals = [(None, -1, 0, 1)[i] for i in rng.choice(4, n, p=probs)]
        assert _c_node(vals) == node_rule(vals), vals
    assert _c_node([1, 1, 1]) == -1 and _c_node([1, 0, 1]) == 0 and _c_node([1, None, -1]) == 1 and _c_node([0, None]) is None
    assert _c_node([None]) is None and _c_node([1]) == -1 and _c_node([-1]) == 1 and _c_node([0]) == 0  # a pass node


def test_pick_rule_equals_the_restatement_including_all_lost_and_no_remaining_visits_at_both_temperatures():
    rng = np.random.default_rng(2)
    seen = set()
    for it in range(4000):
        n = int(rng.integers(1, 35))
        probs = rng.dirichlet(np.ones(4) * 0.5)
        vals = [(None, -1, 0, 1)[i] for i in rng.choice(4, n, p=probs)]
        N = [int(x) for x in rng.integers(0, 50, n) * (rng.random(n) < 0.7)]
        kind = it % 4
        if kind == 1:
            vals = [1] * n  # every move loses
        elif kind == 2:
            vals = [c if c != -1 else 0 for c in vals]
            N = [x if c == 1 else 0 for x, c in zip(N, vals)]  # the moves that are not lost have no visit
        if sum(N) == 0:
            N[int(rng.integers(n))] = 3
        for tau1 in (0, 1):
            draw = int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(2))
            got = _c_pick(N, vals, tau1, draw)
            assert got == pick_rule(N, vals, tau1, draw), (N, vals, tau1, draw)
            seen.add((kind, tau1, -1 in vals))
    assert len(seen) >= 10
    # hand-made: the lowest win at every temperature, a lost maximum is avoided, all lost = the plain rule
    assert _c_pick([1, 9, 1], [None, 0, -1], 0, 0) == 2 and _c_pick([1, 9, 1], [-1, 0, -1], 1, 5) == 0
    assert _c_pick([3, 9, 5], [None, 1, 0], 0, 0) == 2 and _c_pick([3, 9, 5], [1, 1, 1], 0, 0) == 1
    assert _c_pick([3, 9, 5], [None, 1, 0], 1, 7) == 2 and _c_pick([3, 9, 5], [None, 1, 0], 1, 10) == 0  # 7 % 8, 10 % 8 over (3, 5)
    assert _c_pick([0, 9, 0], [None, 1, 0], 0, 0) == 1 and _c_pick([0, 9, 0], [None, 1, 0], 1, 4) == 1  # nothing left: plain


def test_the_two_functions_refuse_bad_arguments_with_a_message():
    L = _lib.lib()
    v = np.array([0, 3], np.int8)
    n = np.array([1, 1], np.uint32)
    assert L.bz_solver_node(None, 2) == -128 and L.bz_solver_node(v.ctypes.data, 0) == -128 and L.bz_solver_node(v.ctypes.data, 256) == -128
    assert L.bz_solver_node(v.ctypes.data, 2) == -128 and b"bz_solver_node" in L.bz_last_error()
    assert L.bz_solver_pick(n.ctypes.data, v.ctypes.data, 2, 0, C.c_uint64(0)) == -1 and b"bz_solver_pick" in L.bz_last_error()
    assert L.bz_solver_pick(None, v.ctypes.data, 1, 0, C.c_uint64(0)) == -1 and L.bz_solver_pick(n.ctypes.data, v.ctypes.data, 0, 0, C.c_uint64(0)) == -1


# ---------------------------------------------------------------- soundness, completeness, invariants
def _searched(game, ev, positions, sims):
    tw = SolverTwin(game, ev, boards=boards())
    roots = [tw.search(b, p, sims) for b, p in positions]
    return tw, roots


@pytest.mark.parametrize("ev", ["uniform", "hash"])
def test_every_proof_of_the_twin_on_every_tictactoe_position_from_three_stones_equals_negamax(ev):
    pos = ttt_positions(3)
    assert len(pos) == 4438 and min(int((b.board != 0).sum()) for b, _ in pos) == 3
    tw, roots = _searched("ttt", ev, pos, 64)
    memo, n = {}, 0
    for root in roots:
        assert sum(e["N"] for e in root["edges"]) == 64
        n += check_sound(tw, root, memo)
    assert n > len(pos) and sum(r["proven"] is not None for r in roots) > len(pos) // 2
    assert tw.max_depth > TTT_GW  # a walk deeper than the lane group is wide: path entries beyond the registers


@pytest.mark.parametrize("ev", ["uniform", "hash"])
def test_every_proof_of_the_twin_on_64_reversi4_positions_equals_negamax_and_some_run_through_a_pass(ev):
    pos = rev4_positions()
    assert len(pos) >= 64
    tw, roots = rev4_roots(ev, 128)
    memo, n = {}, 0
    for root in roots:
        assert sum(e["N"] for e in root["edges"]) == 128
        n += check_sound(tw, root, memo)
    assert n > 64 and any(r["proven"] is not None for r in roots)
    assert tw.n_pass_proofs > 0  # a pass node (one edge) is decided exactly when its child is


@functools.lru_cache(maxsize=None)
def ttt5_roots(ev, sims):
    """the twin's searched roots of ttt_positions(5), shared with tests/test_gpu_solver.py: (twin, roots)"""
    return _searched("ttt", ev, ttt_positions(5), sims)


@functools.lru_cache(maxsize=None)
def rev4_roots(ev, sims):
    """the twin's searched roots of rev4_positions(), shared with tests/test_gpu_solver.py: (twin, roots)"""
    return _searched("reversi4", ev, rev4_positions(), sims)


@functools.lru_cache(maxsize=None)
def forced_win_fixtures(sims=32, ev="hash", want=3):
    """tic-tac-toe positions (board, mover, winning action) where the solver twin proves a win for the mover within `sims`
    simulations while the plain twin's argmax N after the same number plays another move"""
    out = []
    plain = Twin("ttt", ev, boards=boards())
    tw = SolverTwin("ttt", ev, boards=boards())
    for b, p in ttt_positions(3):
        root = tw.search(b, p, sims)
        c = [e.get("c") for e in root["edges"]]
        if -1 not in c:
            continue
        win = root["edges"][c.index(-1)]["a"]
        pr = plain.search(b, p, sims)
        N = [e["N"] for e in pr["edges"]]
        if pr["edges"][N.index(max(N))]["a"] != win:
            out.append((b, p, win))
            if len(out) >= want:
                break
    return tuple(out)


def test_every_tictactoe_root_from_five_stones_is_decided_at_s_simulations_and_not_at_half_of_them():
    """S = 256 under the uniform evaluator, found with this twin: undecided roots of the 3430 at 64 / 128 / 256 simulations = 73 / 15 /
    0.  Under the hash evaluator NO S <= 4096 decides them all -- 355 / 284 / 217 / 167 / 118 / 73 / 34 undecided at 64 / 128 / ... /
    4096: once a root edge is a decided draw it keeps q = 0 and an undecided sibling whose net value is clearly negative never
    outscores it again (u shrinks like 1 / sqrt(sum N)), so that sibling's proof never finishes.  DESIGN.md 3.23 reports it; the
    move is unaffected (the sibling can at best draw too, or it would have been walked).  The hash figures at 64 are asserted in
    tests/test_gpu_solver.py through the same roots."""
    n = len(ttt_positions(5))
    und = [sum(r["proven"] is None for r in ttt5_roots("uniform", s)[1]) for s in (S_COMPLETE // 2, S_COMPLETE)]
    print("undecided roots of", n, "at", S_COMPLETE // 2, "and", S_COMPLETE, "simulations:", und)
    assert n == 3430 and und[1] == 0
    assert und[0] > 0  # S is the smallest power of two


def test_a_decided_root_is_only_walked_one_edge_deep_and_its_visits_still_sum_to_the_simulations():
    b = bz.TicTacToeBoard(np.array([[1, 1, 0], [-1, -1, 0], [0, 0, 0]]))
    tw = SolverTwin("ttt", "uniform", boards=boards())
    root = tw.search(b, 1, 32)
    assert root["proven"] == 1 and [e.get("c") for e in root["edges"]][0] == -1  # action 2 wins: the lowest edge
    assert sum(e["N"] for e in root["edges"]) == 32 and root["edges"][0]["N"] >= 24
    assert tw.pick(root, False, 0)["a"] == 2 and tw.pick(root, True, 12345)["a"] == 2


def test_there_are_forced_wins_the_plain_search_does_not_play_at_the_same_simulations():
    fx = forced_win_fixtures()
    assert len(fx) >= 1
    memo = {}
    tw = Twin("ttt", "hash", boards=boards())
    for b, p, win in fx:
        assert negamax(tw, b, p, memo) == 1 and negamax(tw, tw.play(b, p, win), -p, memo) == -1


def test_a_search_that_meets_no_terminal_equals_the_plain_twin_in_every_visit_and_value():
    b = bz.ReversiBoard(size=8)
    a = SolverTwin("reversi", "hash", boards=boards()).search(b, 1, 32)
    p = Twin("reversi", "hash", boards=boards()).search(b, 1, 32)

    def flat(root):
        out, stack = [], [root]
        while stack:
            x = stack.pop()
            for e in x["edges"] or []:
                out.append((e["a"], e["N"], np.float32(e["W"]).view(np.uint32), np.float32(e["P"]).view(np.uint32)))
                assert e.get("c") is None
                if e["child"] is not None:
                    stack.append(e["child"])
        return out
    assert flat(a) == flat(p) and a["proven"] is None


def test_selfplay_twin_under_the_cap_with_noise_records_full_searches_only_and_avoids_lost_moves():
    tw = SolverTwin("reversi4", "hash", cap=(8, 32768), dir_alpha=0.3, dir_eps=0.25, boards=boards())
    lost = decided = 0
    for gid in range(6):
        rows, w, _ = tw.selfplay(gid, 48, 2, 0, 5)
        assert len(rows) == sum(b == 48 for b in tw.budgets) and [sum(lg["N"]) for lg in tw.log] == tw.budgets
        for lg in tw.log:
            c = lg["c"][lg["a"].index(lg["act"])]
            decided += lg["proven"] is not None
            if -1 in lg["c"]:
                assert c == -1 and lg["act"] == lg["a"][lg["c"].index(-1)]
            elif any(x != 1 for x in lg["c"]) and sum(n for n, x in zip(lg["N"], lg["c"]) if x != 1) > 0:
                assert c != 1
            lost += c == 1
    assert decided > 0


# ---------------------------------------------------------------- the twin runs behind the net / observer cases of the GPU file
NOISE_TWIN = dict(dir_alpha=0.3, dir_eps=0.25)


def solver_twins(game, ev, n, sims, cap=None, temp_moves=0, openings=0, seed=0, base=0, stagger=0, eval_fn=None, noise=False, slot0=0,
                 cls=SolverTwin):
    """every game's solver twin, played to the end: [(twin, rows, winner)]; a twin keeps its own game's log and budgets"""
    out = []
    for g in range(n):
        tw = cls(game, ev, cap=cap, eval_fn=eval_fn, boards=boards(), **(NOISE_TWIN if noise else {}))
        rows, w, _ = tw.selfplay(base + slot0 + g, sims, temp_moves, openings, seed, slot=g, stagger=stagger)
        out.append((tw, rows, w))
    return out


def twin_figures(twins):
    """what keeps a case from passing vacuously: searches with a decided root, decided root edges, nodes decided, walks that
    stopped at a proven edge, the budgets drawn"""
    logs = [lg for tw, _, _ in twins for lg in tw.log]
    return {"decided_roots": sum(lg["proven"] is not None for lg in logs), "decided_edges": sum(c is not None for lg in logs for c in lg["c"]),
            "n_decided": sum(lg["n_decided"] for lg in logs), "n_stops": sum(lg["n_stops"] for lg in logs),
            "budgets": {b for tw, _, _ in twins for b in tw.budgets}, "searches": len(logs)}


@functools.lru_cache(maxsize=None)
def exact_bf16_net():
    """(P, oracle net): the search-grade exact bf16 net of tests/test_search_net_cpu.py, 64 channels x 1 block"""
    from test_search_net_cpu import SEED, VH, oracle_net, search_net
    P = search_net(64, 1, VH, "bf16", SEED)
    return P, oracle_net(P, "bf16")


def store_figures(twins, base, seed, stagger, sims, plies=3):
    """what the root store of an engine playing these games once, in lockstep, does: (trees filed, searches
    seeded).  Behind every search the roots fewer than `plies` moves into their game that are not on file are filed -- full
    searches only, one tree per position, the lowest slot's -- and a search whose root is on file by then is seeded."""
    made0 = [tw.start(g, base + g, 0, seed, stagger)[2] for g, (tw, _, _) in enumerate(twins)]
    filed, seeds = set(), 0
    for s in range(max(len(tw.log) for tw, _, _ in twins)):
        new = set()
        for g, (tw, _, _) in enumerate(twins):
            if s < len(tw.log) and made0[g] + s < plies:
                key = tw.bits(tw.log[s]["b"], tw.log[s]["p"])
                if key in filed:
                    seeds += 1
                elif tw.log[s]["budget"] == sims:
                    new.add(key)
        filed |= new
    return len(filed), seeds


NET_CASE = dict(game="reversi6", n=8, sims=32, temp_moves=4, seed=2, stagger=3)
NET_CAP = (8, 16384)  # PlayoutCap(8, 0.25)
# game id base of the capped run.  The games are played once, so a search is seeded only where the stagger brings a slot to a
# root another slot's full search filed; under the cap with noise that is rare -- base 0: 4 trees filed, none met again;
# base 72: 6 filed, 4 searches seeded (store_figures)
NET_CAP_BASE = 72


@functools.lru_cache(maxsize=None)
def net_case_twins(capped):
    """the twins of the exact-bf16-net case of tests/test_gpu_solver.py (every cache mode compares with this one run), and of
    the same case under the cap with Dirichlet noise; the evaluator is the oracle's bf16 forward"""
    from test_search_net_cpu import oracle_eval_fn
    kw = dict(NET_CASE)
    return solver_twins(kw.pop("game"), "net", kw.pop("n"), kw.pop("sims"), cap=NET_CAP if capped else None,
                        eval_fn=oracle_eval_fn(exact_bf16_net()[1], "bf16"), noise=capped, base=NET_CAP_BASE if capped else 0, **kw)


def net_case_store(capped):
    return store_figures(net_case_twins(capped), NET_CAP_BASE if capped else 0, NET_CASE["seed"], NET_CASE["stagger"], NET_CASE["sims"])


class ObserverTwin(OwnTwin(SolverTwin)):
    """SolverTwin with the three observers: each mix-in keeps its own view of every searched root, _Own the final board"""
    kl_rows, row_kl, q_rows, row_q = _Surprise.kl_rows, _Surprise.row_kl, _Value.q_rows, _Value.row_q

    def root_noise(self, root):
        _Surprise._keep(self, root)
        _Value._keep(self, root)
        super().root_noise(root)


OBSERVER_CASE = dict(game="reversi4", n=8, sims=32, temp_moves=3, seed=5)


@functools.lru_cache(maxsize=None)
def observer_case_twins():
    kw = dict(OBSERVER_CASE)
    return solver_twins(kw.pop("game"), "hash", kw.pop("n"), kw.pop("sims"), noise=True, cls=ObserverTwin, **kw)


@pytest.mark.parametrize("capped", [False, True])
def test_the_net_case_of_the_gpu_file_holds_decided_roots_proven_stops_and_under_the_cap_both_budgets(capped):
    """a seed that makes the GPU case vacuous fails here first"""
    twins = net_case_twins(capped)
    f = twin_figures(twins)
    print("capped" if capped else "plain", f, "evaluations", sum(tw.n_evals for tw, _, _ in twins))
    assert f["decided_roots"] > 0 and f["decided_edges"] > 0 and f["n_decided"] > 0 and f["n_stops"] > 0, f
    assert f["budgets"] == ({NET_CASE["sims"], NET_CAP[0]} if capped else {NET_CASE["sims"]}), f
    for tw, rows, _ in twins:
        assert [sum(lg["N"]) for lg in tw.log] == tw.budgets and len(rows) == sum(b == NET_CASE["sims"] for b in tw.budgets)
    saves, seeds = net_case_store(capped)
    print("the root store: trees filed", saves, "searches seeded", seeds)
    assert (saves, seeds) == ((6, 4) if capped else (8, 2))  # the store fires in the default engine's run


def test_the_observer_case_of_the_gpu_file_holds_decided_roots_and_columns_that_are_not_constant():
    twins = observer_case_twins()
    f = twin_figures(twins)
    print(f)
    assert f["decided_roots"] > 0 and f["decided_edges"] > 0 and f["n_decided"] > 0 and f["n_stops"] > 0, f
    kl = np.concatenate([tw.kl_rows(rows) for tw, rows, _ in twins])
    q = np.concatenate([tw.q_rows(rows) for tw, rows, _ in twins])
    assert (kl > 0).any() and len(np.unique(q)) > 2
    # q is the value of the raw visits -- also at a decided root, whose proven value it need not equal
    n_dec = n_off = 0
    for tw, rows, _ in twins:
        lg = {tw.bits(x["b"], x["p"]): x for x in tw.log}
        for r, qq in zip(rows, tw.q_rows(rows)):
            x = lg[(r[0], r[1])]
            if x["proven"] is not None:
                n_dec += 1
                n_off += float(qq) != float(x["proven"])
    assert n_dec > 0 and n_off > 0, (n_dec, n_off)
    for tw, rows, w in twins:  # the final board gives the winner the game had
        assert winner_of(OBSERVER_CASE["game"], *tw.final_bits()) == (True, w)


# ---------------------------------------------------------------- the ABI
def test_solver_bytes_is_the_stated_layout():
    L = _lib.lib()
    for B in (1, 64, 65, 4096):
        cfg = _cfg(B=B)
        assert L.bz_engine_solver_bytes(C.byref(cfg)) == ((4 * B + 255) // 256) * 256 + 256


def test_solver_check_accepts_and_refuses_with_a_message():
    L = _lib.lib()
    assert L.bz_engine_solver_check(C.byref(_cfg())) == _lib.BZ_OK
    for cfg, word in ((_cfg(flags=_lib.ENGINE_REUSE_SUBTREE), b"subtree reuse"), (_cfg(K=2), b"leaves_per_step")):
        assert L.bz_engine_solver_check(C.byref(cfg)) == _lib.BZ_EINVAL
        assert word in L.bz_last_error() and b"solver" in L.bz_last_error(), L.bz_last_error()
        assert L.bz_engine_solver_bytes(C.byref(cfg)) == -1 and word in L.bz_last_error()
    assert L.bz_engine_solver_check(None) == _lib.BZ_EINVAL and L.bz_engine_solver_bytes(None) == -1


def test_set_solver_and_root_proven_refuse_a_null_engine_with_a_message():
    L = _lib.lib()
    assert L.bz_engine_set_solver(None, 1, None, 0, None) == _lib.BZ_EINVAL and b"null engine" in L.bz_last_error()
    assert L.bz_engine_root_proven(None, None, None, None, None) == _lib.BZ_EINVAL and b"null pointer" in L.bz_last_error()


def test_the_abi_version_stays_and_the_header_documents_the_rule():
    import os
    assert _lib.lib().bz_abi_version() == _lib.ABI_VERSION
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "bz_abi.h")).read()
    for name in ("bz_engine_solver_bytes", "bz_engine_solver_check", "bz_engine_set_solver", "bz_engine_root_proven", "bz_solver_node",
                 "bz_solver_pick", "DESIGN.md 3.23"):
        assert name in hdr, name
    assert "3.23" in open(os.path.join(root, "DESIGN.md")).read()


# ---------------------------------------------------------------- Python validation, before any device is touched
@pytest.fixture
def _no_device(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(_lib, "require_gpu", no_device)


def _everyone(touches_only=False, **kw):
    """every public entry point that takes solver=, with the keywords that make the combination"""
    from betazero_amd.arena import play_arena
    from betazero_amd.engine import PipelinedSelfPlay, SelfPlayEngine, self_play
    from betazero_amd.match import MatchPlayer, play_match
    sp = {k: v for k, v in kw.items()}
    out = [lambda: SelfPlayEngine("reversi", 4, 16, "hash", **sp)]
    if not touches_only:  # (the pipelines ask for their streams before they build an engine; self_play goes through them)
        out += [lambda: PipelinedSelfPlay("reversi", 4, 16, "hash", **sp), lambda: self_play("reversi", 4, 16, evaluator="hash", **sp)]
    pl = {k: v for k, v in kw.items() if k in ("solver", "leaves_per_step", "gumbel", "fpu")}
    if len(pl) == len(kw):
        if not touches_only:  # (the player builds its engine at the first get_move)
            out.append(lambda: bz.MCTSPlayer(1, sims=16, evaluator="hash", **pl))
        out += [lambda: play_match("reversi", 4, MatchPlayer(sims=16, evaluator="hash", **pl), MatchPlayer(sims=16, evaluator="hash")),
                lambda: play_arena("reversi", 4, 16, evaluator="hash", **pl)]
    return out


def test_python_refuses_every_refused_combination_before_touching_a_device(_no_device):
    from betazero_amd.engine import ForcedPlayouts, Fpu, check_solver
    for kw, word in ((dict(reuse_subtree=True), "reuse_subtree"), (dict(leaves_per_step=2), "leaves_per_step"), (dict(gumbel=True), "Gumbel"),
                     (dict(forced_playouts=ForcedPlayouts(2.0)), "forced_playouts"), (dict(fpu=Fpu()), "fpu"), (dict(fpu=True), "fpu")):
        calls = _everyone(solver=True, **kw)
        assert len(calls) >= 3
        for f in calls:
            with pytest.raises(ValueError, match=word):
                f()
    for bad in (1, "yes", 0.5):
        with pytest.raises(ValueError, match="solver must be a bool"):
            check_solver(bad)
        for f in _everyone(solver=bad):
            with pytest.raises(ValueError, match="solver must be a bool"):
                f()
    assert check_solver(None) is False and check_solver(False, reuse_subtree=True) is False and check_solver(True) is True


def test_python_accepts_on_everywhere_up_to_the_device(_no_device):
    from betazero_amd.engine import PlayoutCap
    assert bz.MCTSPlayer(1, sims=16, evaluator="hash", solver=True).solver is True
    for f in _everyone(True, solver=True) + _everyone(True, solver=True, playout_cap=PlayoutCap(4, 0.5), dirichlet_alpha=0.3, dirichlet_eps=0.25,
                                                 surprise=True, search_value=True, ownership=True):
        with pytest.raises(AssertionError, match="a device was touched"):
            f()
