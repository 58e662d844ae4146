"""Head-to-head matches without a GPU: the match twin -- pairing, opening draw, pass rule, move choice
per mode and winner exactly as the spec states them, on oracle.py_twin.Twin and the K-walk / Gumbel twins -- its
invariants, the exact mirror property, the opening draw of the library against the twin's, summary()'s arithmetic on
hand-computed results, and every refusal.  tests/test_gpu_match.py pins the engine's matches to this twin."""
import ctypes as C
import math

import numpy as np
import pytest

from betazero_amd import _lib
from betazero_amd.match import MatchPlayer, MatchResult, check_match, elo_of_score, play_match
from oracle.py_twin import Twin, rng_draw
from test_gumbel_cpu import GumbelTwin
from test_leaf_parallel_cpu import KTwin, boards

C_MATCH = 0x6D617463684F50E5
M64 = (1 << 64) - 1


def opening_index(seed, pair, ply, n_legal):
    return rng_draw((seed ^ C_MATCH) & M64, pair, ply) % n_legal


class Side:
    """one player of the twin match.  search: "twin" (the Python twins) or "oracle" (oracle.mcts_search: the same spec in
    C, PUCT with K = 1 only; orc_eval = (the oracle's eval kind, its net or None))"""

    def __init__(self, sims, ev="uniform", K=1, gumbel=None, eval_fn=None, c_puct=1.5, orc_eval=None):
        self.sims, self.ev, self.K, self.gumbel, self.eval_fn, self.c_puct, self.orc_eval = sims, ev, K, gumbel, eval_fn, c_puct, orc_eval
        self._tw = {}

    def twin(self, game):
        if game not in self._tw:
            kw = dict(c_puct=self.c_puct, boards=boards())
            if self.gumbel is not None:
                g = self.gumbel
                self._tw[game] = GumbelTwin(game, self.ev, m=g.max_considered, scale=g.scale, maxvisit_init=g.maxvisit_init,
                                            value_scale=g.value_scale, eval_fn=self.eval_fn, **kw)
            elif self.K > 1 or self.eval_fn is not None:
                self._tw[game] = KTwin(game, self.ev, leaves=self.K, eval_fn=self.eval_fn, **kw)
            else:
                self._tw[game] = Twin(game, self.ev, **kw)
        return self._tw[game]

    def move(self, game, rules, b, p):
        if self.orc_eval is not None:
            from oracle import oracle as orc
            og = {"ttt": orc.GAME_TTT, "reversi": orc.GAME_REVERSI, "reversi6": orc.GAME_REVERSI6, "reversi4": orc.GAME_REVERSI4}[game]
            own, opp = rules.bits(b, p)
            N = orc.mcts_search(og, own, opp, p, self.sims, self.orc_eval[0], c_puct=self.c_puct, net=self.orc_eval[1])[0]
            return int(np.argmax(N))  # first maximum of N
        tw = self.twin(game)
        if self.gumbel is not None:
            return int(tw.policy(tw.search(b, p, self.sims, False, (0, 0, 0)))[1])  # the Gumbel move, no noise
        root = tw.search(b, p, self.sims)
        pick, bn = root["edges"][0], 0
        for e in root["edges"]:  # first maximum of N (edges are in ascending action order)
            if e["N"] > bn:
                pick, bn = e, e["N"]
        return pick["a"]


class MatchTwin:
    """The match, restated: games 2k and 2k + 1 share the opening, A is X (+1, moves first) in 2k and O in 2k + 1; while a
    game has made t < opening_plies moves its move is the r-th legal move in ascending action order, r =
    rng_draw(seed ^ C_MATCH, k, t) mod n_legal; then the mover's search decides; the game ends by the board classes'
    is_game_over; a side without a move is passed over (the other side moves again, no log row)."""

    def __init__(self, game, a, b, opening_plies=0, seed=0):
        self.game, self.a, self.b, self.opening_plies, self.seed = game, a, b, opening_plies, seed
        self.rules = Twin(game, "uniform", boards=boards())  # (only its env calls are used)

    def play_game(self, g, check=False):
        """-> dict(actions, movers, winner, a_colour, passes, empties)"""
        tw = self.rules
        b = tw.TicTacToeBoard() if tw.game == "ttt" else tw.ReversiBoard(size=tw.size)
        a_colour = 1 if g % 2 == 0 else -1
        p, acts, movs, passes = 1, [], [], 0
        while True:
            mv = tw.moves(b, p)
            assert mv, "the side to move always has a move"
            t = len(acts)
            if t < self.opening_plies:
                a = mv[opening_index(self.seed, g // 2, t, len(mv))]
            else:
                a = (self.a if p == a_colour else self.b).move(self.game, tw, b, p)
            if check:
                assert a in mv, (g, t, a, mv)  # legal by the board class
            acts.append(a)
            movs.append(p)
            b = tw.play(b, p, a)
            over, w = tw.terminal(b)
            if over:
                if check:  # the winner is get_score / is_game_over of the final board
                    if tw.game == "ttt":
                        assert b.is_game_over() == (True, w)
                    else:
                        assert b.is_game_over() and b.get_score()[0] == w
                empties = int((np.asarray(b.board) == 0).sum())
                return {"actions": acts, "movers": movs, "winner": int(w), "a_colour": a_colour, "passes": passes, "empties": empties}
            if tw.moves(b, -p):
                p = -p
            else:
                passes += 1

    def play(self, n_games, check=False):
        games = [self.play_game(g, check) for g in range(n_games)]
        T = max(len(x["actions"]) for x in games)
        actions = np.full((T, n_games), 255, np.uint8)
        movers = np.zeros((T, n_games), np.int8)
        for g, x in enumerate(games):
            actions[:len(x["actions"]), g] = x["actions"]
            movers[:len(x["movers"]), g] = x["movers"]
        res = MatchResult(np.array([x["winner"] for x in games], np.int8), np.array([x["a_colour"] for x in games], np.int8),
                          np.array([len(x["actions"]) for x in games], np.int32), actions, movers)
        return res, games


def assert_same_match(res, ref, what=""):
    """a MatchResult against the twin's, bit for bit, every game"""
    assert np.array_equal(res.plies, ref.plies), (what, "plies", np.nonzero(res.plies != ref.plies)[0][:8])
    assert res.actions.shape == ref.actions.shape, (what, res.actions.shape, ref.actions.shape)
    bad = np.nonzero((res.actions != ref.actions).any(0) | (res.movers != ref.movers).any(0))[0]
    assert bad.size == 0, (what, "games", bad[:8], res.actions[:, bad[0]], ref.actions[:, bad[0]])
    assert np.array_equal(res.winner, ref.winner), (what, "winner", np.nonzero(res.winner != ref.winner)[0][:8])
    assert np.array_equal(res.a_colour, ref.a_colour), what


# ---------------------------------------------------------------- the twin's invariants
TWIN_CASES = [("ttt", Side(24, "hash"), Side(8, "uniform"), 2, 16), ("reversi4", Side(16, "hash"), Side(8, "uniform"), 2, 16),
              ("reversi4", Side(12, "hash", gumbel=MatchPlayer(gumbel=True).checked("reversi", 2, "a")[1]), Side(12, "hash", K=4), 0, 4),
              ("reversi6", Side(8, "hash"), Side(8, "uniform"), 4, 6)]


@pytest.mark.parametrize("game,a,b,opening,n", TWIN_CASES, ids=[f"{c[0]}-{i}" for i, c in enumerate(TWIN_CASES)])
def test_twin_match_invariants(game, a, b, opening, n):
    res, games = MatchTwin(game, a, b, opening, seed=3).play(n, check=True)  # (check: every move legal, the winner the board's)
    for k in range(n // 2):
        x, o = games[2 * k], games[2 * k + 1]
        assert x["a_colour"] == 1 and o["a_colour"] == -1
        assert x["actions"][:opening] == o["actions"][:opening] and x["movers"][:opening] == o["movers"][:opening]
    assert np.array_equal(res.score, res.winner * res.a_colour)
    assert np.array_equal(res.pair_score, res.score[0::2].astype(int) + res.score[1::2])
    assert ((res.actions != 255) == (res.movers != 0)).all() and ((res.movers != 0).sum(0) == res.plies).all()


def test_twin_small_boards_exercise_the_pass_rule_and_early_endings():
    _, g4 = MatchTwin("reversi4", Side(16, "hash"), Side(8, "uniform"), 2, seed=3).play(16)
    assert any(x["passes"] for x in g4) and any(x["empties"] for x in g4)


@pytest.mark.parametrize("game,side,opening,n", [("ttt", Side(16, "hash"), 2, 16), ("reversi4", Side(12, "hash"), 2, 16),
                                                 ("reversi4", Side(8, "hash", K=4), 1, 8), ("reversi6", Side(6, "hash"), 3, 4)])
def test_mirror_property_exact(game, side, opening, n):
    """a == b: the two games of every pair are the same game, and A's total score is exactly 0"""
    res, _ = MatchTwin(game, side, side, opening, seed=5).play(n)
    assert np.array_equal(res.actions[:, 0::2], res.actions[:, 1::2]) and np.array_equal(res.movers[:, 0::2], res.movers[:, 1::2])
    assert np.array_equal(res.winner[0::2], res.winner[1::2])
    assert int(res.score.sum()) == 0 and not res.pair_score.any()
    assert res.summary()["score"] == 0.5 and res.summary()["elo"] == 0.0


# ---------------------------------------------------------------- the opening draw
def test_opening_index_equals_the_twins_draw():
    L = _lib.lib()
    out = C.c_int32()
    for seed in (0, 1, 7, 2**63 + 5, 2**64 - 1):
        for pair in (0, 1, 2, 511, 2047, 2**23 - 1):
            for ply in (0, 1, 2, 3, 7, 59):
                for n_legal in range(1, 35):
                    assert L.bz_match_opening_index(seed, pair, ply, n_legal, C.byref(out)) == _lib.BZ_OK
                    assert out.value == opening_index(seed, pair, ply, n_legal), (seed, pair, ply, n_legal)
    assert len({opening_index(0, k, 0, 4) for k in range(64)}) == 4  # (the draw does vary)
    for bad in ((0, 0, -1, 4), (0, 0, 0, 0), (0, 0, 0, 65)):
        assert L.bz_match_opening_index(*bad, C.byref(out)) == _lib.BZ_EINVAL and b"bz_match_opening_index" in L.bz_last_error()


# ---------------------------------------------------------------- summary()
def _result(scores):
    """games with the given outcomes for A, colours alternating"""
    n = len(scores)
    col = np.where(np.arange(n) % 2 == 0, 1, -1).astype(np.int8)
    z = np.zeros((0, n))
    return MatchResult((np.array(scores, np.int8) * col).astype(np.int8), col, np.zeros(n, np.int32), z.astype(np.uint8), z.astype(np.int8))


def test_summary_on_hand_computed_results():
    # 8 games, pairs (+1,+1) (+1,-1) (0,+1) (-1,0): W 4 D 2 L 2 -> score (4 + 1) / 8 = 0.625
    r = _result([1, 1, 1, -1, 0, 1, -1, 0])
    s = r.summary()
    assert (s["games"], s["wins"], s["draws"], s["losses"]) == (8, 4, 2, 2)
    assert s["as_x"] == {"wins": 2, "draws": 1, "losses": 1} and s["as_o"] == {"wins": 2, "draws": 1, "losses": 1}
    assert list(r.pair_score) == [2, 0, 1, -1] and list(r.score) == [1, 1, 1, -1, 0, 1, -1, 0]
    assert s["score"] == 0.625
    assert s["elo"] == pytest.approx(-400 * math.log10(1 / 0.625 - 1)) and s["elo"] == pytest.approx(88.7390, abs=1e-3)
    # pair means 1, .5, .75, .25: mean .625, sample variance (.140625 + .015625 + .015625 + .140625) / 3 = 0.1041666...
    half = 1.96 * math.sqrt(0.3125 / 3 / 4)
    assert half == pytest.approx(0.316294, abs=1e-6)  # 1.96 x sqrt(0.0260417) = 1.96 x 0.161374
    assert s["elo_ci95"][0] == pytest.approx(-400 * math.log10(1 / (0.625 - half) - 1))
    assert s["elo_ci95"][1] == pytest.approx(-400 * math.log10(1 / (0.625 + half) - 1))
    assert s["elo_ci95"][0] < s["elo"] < s["elo_ci95"][1]


def test_summary_all_wins_all_draws_all_losses_and_one_pair():
    s = _result([1] * 6).summary()
    assert s["score"] == 1.0 and s["elo"] == math.inf and s["elo_ci95"] == [math.inf, math.inf] and s["wins"] == 6
    s = _result([0] * 6).summary()
    assert s["score"] == 0.5 and s["elo"] == 0.0 and s["elo_ci95"] == [0.0, 0.0] and s["draws"] == 6
    s = _result([-1] * 4).summary()
    assert s["score"] == 0.0 and s["elo"] == -math.inf and s["elo_ci95"] == [-math.inf, -math.inf]
    s = _result([1, 0]).summary()  # one pair: no variance to estimate
    assert s["score"] == 0.75 and s["elo"] == pytest.approx(190.8485, abs=1e-3) and s["elo_ci95"] == [-math.inf, math.inf]
    # the interval is clipped at the ends of the score range, not wrapped
    s = _result([1, 1, 1, 1, 1, -1]).summary()
    assert s["elo_ci95"][1] == math.inf and s["elo_ci95"][0] < s["elo"] < math.inf
    assert elo_of_score(0.5) == 0.0 and elo_of_score(0.0) == -math.inf and elo_of_score(1.0) == math.inf


# ---------------------------------------------------------------- refusals, before any device is touched
class _FakeNet:
    def __init__(self, max_batch):
        self.max_batch = max_batch


class DeviceMLP(_FakeNet):  # (check_match tells the MLP by its class name, so that it need not import torch)
    pass


def _refusals():
    P = MatchPlayer
    return [
        (dict(n_games=7), "n_games"), (dict(n_games=0), "n_games"), (dict(n_games=True), "n_games"), (dict(n_games=8.0), "n_games"),
        (dict(opening_plies=-1), "opening_plies"), (dict(opening_plies=1.5), "opening_plies"),
        (dict(game="go"), "game must be"), (dict(size=5), "8x8, 6x6 and 4x4"),
        (dict(a=P(sims=0)), "sims"), (dict(b=P(sims=9000)), "sims"),
        (dict(a=P(16, leaves_per_step=0)), "leaves_per_step"), (dict(b=P(16, leaves_per_step=33)), "leaves_per_step"),
        (dict(a=P(16, gumbel="yes")), "gumbel"), (dict(a=P(16, gumbel=True, leaves_per_step=2)), "gumbel"),
        (dict(b=P(16, eval_cache="off")), "eval_cache"),
        (dict(a=P(16, evaluator="external")), "evaluator"), (dict(a=P(16, evaluator="net_bf16")), "needs a net"),
        (dict(a="uniform"), "MatchPlayer"),
        (dict(game="ttt", a=P(16, net=_FakeNet(64))), "conv net evaluators serve the Reversi boards"),
        (dict(game="ttt", b=P(16, evaluator="net_f32", net=_FakeNet(64))), "conv net evaluators serve the Reversi boards"),
        (dict(b=P(16, net=DeviceMLP(64))), "serves tic-tac-toe, not Reversi"),
        (dict(a=P(16, evaluator="mlp_bf16", net=_FakeNet(64))), "serves tic-tac-toe, not Reversi"),
        (dict(n_games=8, a=P(16, net=_FakeNet(7))), "max_batch 7 < n_games 8"),
        (dict(n_games=8, b=P(16, net=_FakeNet(63), leaves_per_step=8)), "max_batch 63 < n_games 8 x leaves_per_step 8"),
        (dict(game="ttt", n_games=8, a=P(16, net=DeviceMLP(4))), "max_batch 4 < n_games 8"),
    ]


@pytest.mark.parametrize("kw,msg", _refusals(), ids=[f"{i}-{m.split()[0]}" for i, (_, m) in enumerate(_refusals())])
def test_play_match_refuses_before_touching_a_device(kw, msg, monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("touched a device")
    monkeypatch.setattr(_lib, "require_gpu", no_device)
    monkeypatch.setattr(_lib, "lib", no_device)
    args = dict(game="reversi", n_games=8, a=MatchPlayer(16), b=MatchPlayer(16), size=8, opening_plies=2)
    args.update(kw)
    with pytest.raises(ValueError, match=msg):
        play_match(args.pop("game"), args.pop("n_games"), args.pop("a"), args.pop("b"), **args)


def test_check_match_accepts_what_a_match_can_play():
    P = MatchPlayer
    assert check_match("reversi", 8, P(16, net=_FakeNet(64), leaves_per_step=8), P(16, gumbel=True), 6, 0)[0] == "reversi6"
    assert check_match("ttt", 2, P(16, net=DeviceMLP(2)), P(16, evaluator="hash"), 8, 4)[1][0] == "mlp_f32"
    assert check_match("reversi", np.int64(4), P(16, net=_FakeNet(4), evaluator="net_fp8", eval_cache="search"), P(1), 4, np.int32(3))[1][0] == "net_fp8"
    import betazero_amd
    assert betazero_amd.play_match is play_match and betazero_amd.MatchPlayer is MatchPlayer and betazero_amd.MatchResult is MatchResult


def test_workspace_bytes_answers_without_a_gpu_and_refuses_bad_arguments():
    L = _lib.lib()
    al = lambda n: (n + 255) & ~255  # noqa: E731
    for game, T in ((_lib.GAME_TTT, 9), (_lib.GAME_REVERSI, 60), (_lib.GAME_REVERSI6, 32), (_lib.GAME_REVERSI4, 12)):
        for B in (2, 256, 4096):
            want = 2 * al(8 * B) + 6 * al(B) + al(4 * B) + 2 * al(T * B) + al(32 * (T + 1))
            assert L.bz_match_workspace_bytes(game, B, 0) == want == L.bz_match_workspace_bytes(game, B, T), (game, B)
    assert L.bz_match_workspace_bytes(_lib.GAME_REVERSI, 64, 10) < L.bz_match_workspace_bytes(_lib.GAME_REVERSI, 64, 0)
    for bad in ((9, 8, 0), (-1, 8, 0), (1, 7, 0), (1, 0, 0), (1, -2, 0), (1, (1 << 24) + 2, 0), (1, 8, -1), (1, 8, 65)):
        assert L.bz_match_workspace_bytes(*bad) == -1, bad
        assert b"bz_match_workspace_bytes" in L.bz_last_error(), bad
    h = C.c_void_p()
    assert L.bz_match_create(1, 7, 0, 256, 1 << 20, C.byref(h)) == _lib.BZ_EINVAL
    assert L.bz_match_create(1, 8, 0, None, 1 << 20, C.byref(h)) == _lib.BZ_EINVAL
    if L.bz_device_count() <= 0:
        assert L.bz_match_create(1, 8, 0, 256, 1 << 20, C.byref(h)) == _lib.BZ_ENOGPU
    assert L.bz_engines_search(None, None, 2, 0) == _lib.BZ_EINVAL and L.bz_engines_search(None, None, 0, 0) == _lib.BZ_EINVAL
    assert L.bz_match_ply(None, None, None, None, None, None) == _lib.BZ_EINVAL
    assert L.bz_match_header(None, None, None) == _lib.BZ_EINVAL and L.bz_match_begin(None, 0, 0, None) == _lib.BZ_EINVAL
    assert C.sizeof(_lib.MatchHdr) == 32 and C.sizeof(_lib.MatchLayout) == 11 * 8 + 8
