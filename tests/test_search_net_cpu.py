"""Search-grade exact nets: the nets tests/test_gpu_search_net.py runs searches with, and their checks on the CPU.

tests/test_net_numerics_cpu.py's exact_net makes every sum of the forward exact, but as a player it is useless: its logits
reach hundreds (one-hot priors, one root child takes every visit) and its value is one number on every board.
search_net keeps exact_net's stem and tower and rebuilds the heads so that a search with it in the loop branches and backs
up many different values -- with power-of-two rescaling and sparse weights only, so every fp32 sum stays exact:
  value head  the 1x1 convolution +1 on the 4 tower channels that vary most, no biases behind it, the FCs on 2^-6 / 2^-3
              grids;
  scales      on a fixed calibration set (the 12 opening roots and golden 8x8 positions): the policy FC is multiplied by the
              power of two that brings the largest |logit| before the bias to at most LOGIT_CAL = 4 (the bias adds at most
              1/2), the last value FC by the one that brings the value's pre-activation on every calibration board to within
              VALUE_CAL = 1.5 of its median over the opening roots, and the value bias (on the 2^-6 grid) moves that
              median to about 0.
On these nets net_forward_ref (which asserts its own exactness) equals the oracle's forward in the mode bit for bit, so a
search with the net in the loop is a function of exact data: the GPU file compares the engine with the oracle's search (and
with the twins of tests/test_leaf_parallel_cpu.py / tests/test_gumbel_cpu.py, whose eval_fn here is the oracle's forward)
without a tolerance.  The checks below pin that -- exactness and agreement on >= 1000 golden positions of every size and
ply, and that the nets are usable for search (spread roots, many values of both signs)."""
import os
import threading

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from test_net_numerics_cpu import ORACLE_MODE, edge_boards, exact_net, flat_params, mode_params, net_forward_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
ORC_EVAL = {"bf16": orc.EVAL_NET_BF16, "fp8": orc.EVAL_NET_FP8}
ENGINE_EVAL = {"bf16": "net_bf16", "fp8": "net_fp8"}
# every (mode, C, NB) tests/test_gpu_search_net.py runs
CONFIGS = [("bf16", 64, 1), ("bf16", 128, 1), ("bf16", 256, 1), ("fp8", 128, 1), ("bf16", 128, 6), ("fp8", 128, 6)]
VH = 64
SEED = 1
LOGIT_CAL, VALUE_CAL = 4.0, 1.5


def threads(jobs):
    """the oracle's worker threads: min(16, jobs), never sized by the machine"""
    return max(1, min(16, jobs))


def run_threads(fn, jobs):
    """fn(i) for i in range(jobs) on threads(jobs) threads (the oracle's ctypes calls release the GIL); results in order"""
    out, err, it, lock = [None] * jobs, [], iter(range(jobs)), threading.Lock()

    def work():
        while True:
            with lock:
                i = None if err else next(it, None)
            if i is None:
                return
            try:
                out[i] = fn(i)
            except BaseException as e:  # (re-raised in the caller: a failure names its own cause)
                with lock:
                    err.append(e)
    th = [threading.Thread(target=work) for _ in range(threads(jobs))]
    [t.start() for t in th]
    [t.join() for t in th]
    if err:
        raise err[0]
    return out


# ---------------------------------------------------------------- positions
def opening_roots():
    """(own, opp, to_move, board) of the 12 openings (openings=1: game id % 12 picks the first two moves), game ids 0 .. 11"""
    from test_leaf_parallel_cpu import KTwin, boards
    tw = KTwin("reversi", "uniform", boards=boards())
    out = []
    for gid in range(12):
        b, p, _ = tw.start(0, gid, 1, 0, 0)
        own, opp = tw.bits(b, p)
        out.append((own, opp, p, b))
    return out


def golden_positions(n, seed=0):
    """n side-to-move positions of the golden games -- 8x8, 6x6 and 4x4 (reversi_random_games.npz) and the other sizes
    (reversi_other_sizes.npz) -- drawn from every ply: all plies of every size are represented"""
    rows = np.concatenate([np.load(os.path.join(G, f))["rows"] for f in ("reversi_random_games.npz", "reversi_other_sizes.npz")])
    cur = rows[:, 3].astype(np.int64) - 1
    own = np.where(cur == 1, rows[:, 4], rows[:, 5])
    opp = np.where(cur == 1, rows[:, 5], rows[:, 4])
    rng = np.random.default_rng(seed)
    pick = []
    for key in np.unique(rows[:, 1:3], axis=0):           # one of every (size, ply) first
        idx = np.nonzero((rows[:, 1] == key[0]) & (rows[:, 2] == key[1]))[0]
        pick.append(int(rng.choice(idx)))
    rest = np.setdiff1d(np.arange(len(rows)), pick)
    pick = np.concatenate([pick, rng.choice(rest, max(0, n - len(pick)), replace=False)])
    return own[pick].astype(np.uint64), opp[pick].astype(np.uint64), rows[pick, 1], rows[pick, 2]


def calibration_boards():
    own = [r[0] for r in opening_roots()]
    opp = [r[1] for r in opening_roots()]
    go, gp, size, _ = golden_positions(0, seed=5)
    keep = size == 8
    return np.concatenate([np.array(own, np.uint64), go[keep]]), np.concatenate([np.array(opp, np.uint64), gp[keep]])


# ---------------------------------------------------------------- the nets
def _pow2_at_most(m, target):
    """the power of two s with m s <= target < 2 m s (1 for m = 0)"""
    if m <= 0:
        return 1.0
    return 2.0 ** float(np.floor(np.log2(target / m)))


def search_net(C, NB, VH, mode, seed):
    """exact_net(C, NB, VH, mode, seed) with heads rebuilt for search (module docstring): float64 tensors, KEYS"""
    P = exact_net(C, NB, VH, mode, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    sign = lambda *s: torch.where(torch.rand(*s, generator=g) < 0.5, -1.0, 1.0).double()  # noqa: E731
    own, opp = calibration_boards()
    f = {}
    net_forward_ref(own, opp, P, mode, feats=f)
    # value head: +1 on the 4 tower channels that vary most over the calibration boards (a sum of ReLU outputs: never all
    # zero), nothing else; no biases behind it; sparse FCs on 2^-6 / 2^-3 grids
    var = f["x"].reshape(-1, C).var(0)
    val_w = torch.zeros(C, dtype=torch.float64)
    val_w[torch.argsort(var, descending=True, stable=True)[:4]] = 1.0
    P["val_w"], P["val_b"] = val_w.view(1, C, 1, 1), torch.zeros(1, dtype=torch.float64)
    P["v1_w"] = sign(VH, 64) * (torch.rand(VH, 64, generator=g) < 0.3) * 2.0 ** -6
    P["v1_b"] = torch.zeros(VH, dtype=torch.float64)
    P["v2_w"], P["v2_b"] = sign(1, VH) * 2.0 ** -3, torch.zeros(1, dtype=torch.float64)
    # the powers of two that bring the logits and the value's pre-activation into range on the calibration boards, and a
    # value bias (on the 2^-6 grid) that centres the pre-activation: values of both signs
    net_forward_ref(own, opp, P, mode, feats=f)
    P["polfc_w"] = P["polfc_w"] * _pow2_at_most(float((f["hf"] @ P["polfc_w"].t()).abs().max()), LOGIT_CAL)
    vpre = f["v1h"] @ P["v2_w"].reshape(-1)
    mid = vpre[:12].median()                            # (the opening roots: searches from them see both signs)
    s = _pow2_at_most(float((vpre - mid).abs().max()), VALUE_CAL)
    P["v2_w"] = P["v2_w"] * s
    P["v2_b"] = -torch.round(mid * s * 2.0 ** 6).view(1) * 2.0 ** -6
    return P


def oracle_net(P, mode):
    """the oracle's net holding what the mode's kernels compute with (test_gpu_net_numerics: the device takes P itself,
    the oracle mode_params(P, mode))"""
    C, L, vh = P["stem_w"].shape[0], P["tw"].shape[0], P["v1_w"].shape[0]
    return orc.Net(C, L // 2, vh, flat_params(mode_params(P, mode)))


def oracle_eval_fn(onet, mode):
    """eval_fn of the twins: the oracle's forward of one position in the mode"""
    def fn(own, opp):
        lg, v = onet.forward(np.array([own], np.uint64), np.array([opp], np.uint64), bf16=ORACLE_MODE[mode])
        return lg[0], np.float32(v[0])
    return fn


def search_roots_nodes(on, mode, roots, sims):
    """the oracle's search from every root (threads) and the nodes of the first: (results, own, opp, terminal)"""
    res = run_threads(lambda i: orc.mcts_search(orc.GAME_REVERSI, int(roots[i][0]), int(roots[i][1]), int(roots[i][2]), sims,
                                                ORC_EVAL[mode], net=on), len(roots))
    no, npp, term = orc.mcts_search_nodes(orc.GAME_REVERSI, int(roots[0][0]), int(roots[0][1]), int(roots[0][2]), sims,
                                          ORC_EVAL[mode], net=on)
    return res, no, npp, term


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


# ================================================================ checks (no GPU)
@pytest.mark.parametrize("mode,C,NB,seed", [c + (SEED,) for c in CONFIGS] + [("bf16", 128, 1, 2), ("fp8", 128, 1, 2)])
def test_search_net_is_exact_and_equals_the_oracle(mode, C, NB, seed):
    """net_forward_ref runs with its exactness asserts on the edge boards and >= 1000 golden positions (every size and ply)
    and gives the oracle's logits and value in the mode bit for bit -- for every net the GPU file runs (seed 2: the second
    net of its weight-update test)"""
    P = search_net(C, NB, VH, mode, seed)
    eo, ep = edge_boards()
    go, gp, size, ply = golden_positions(1000)
    assert set(np.unique(size).tolist()) >= {4, 6, 8} and len(np.unique(ply[size == 8])) >= 60
    own, opp = np.concatenate([eo, go]), np.concatenate([ep, gp])
    lg, v = net_forward_ref(own, opp, P, mode)
    on = oracle_net(P, mode)
    chunks = np.array_split(np.arange(own.size), threads(own.size // 64))
    out = run_threads(lambda i: on.forward(own[chunks[i]], opp[chunks[i]], bf16=ORACLE_MODE[mode]), len(chunks))
    olg, ov = np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])
    assert np.array_equal(_bits(lg.numpy()), _bits(olg)), mode
    assert np.array_equal(_bits(v.numpy()), _bits(ov)), mode


@pytest.mark.parametrize("mode,C,NB", CONFIGS)
def test_search_net_is_usable_for_search(mode, C, NB):
    """on the roots of the 12 openings an oracle search (200 simulations; 64 at 128x6) visits >= 3 root children and the
    largest prior is <= 0.9 in >= 9 of 12; |logit| <= 16 on the golden positions and on every node of a search; the nodes
    of one search take >= 32 distinct values of both signs, all with |v| < 0.99"""
    P = search_net(C, NB, VH, mode, SEED)
    on = oracle_net(P, mode)
    roots = opening_roots()
    res, no, npp, term = search_roots_nodes(on, mode, roots, 200 if NB == 1 else 64)
    kids = [int((n > 0).sum()) for n, _, _, _ in res]
    pmax = [float(p.max()) for _, _, p, _ in res]
    print(f"{mode} {C}x{NB}: root children visited {kids}, largest prior {np.round(pmax, 2).tolist()}")
    assert sum(k >= 3 for k in kids) >= 9 and sum(p <= 0.9 for p in pmax) >= 9
    go, gp, _, _ = golden_positions(200, seed=3)
    glg, _ = on.forward(go, gp, bf16=ORACLE_MODE[mode])
    nlg, nv = on.forward(no, npp, bf16=ORACLE_MODE[mode])
    assert np.abs(glg).max() <= 16 and np.abs(nlg).max() <= 16
    nv = nv[term == 0]
    print(f"  nodes of one search: {len(np.unique(nv))} distinct values in [{nv.min():.3f}, {nv.max():.3f}]")
    assert len(np.unique(nv)) >= 32 and nv.min() < 0 < nv.max() and np.abs(nv).max() < 0.99


@pytest.mark.parametrize("mode,C", [("bf16", 64), ("fp8", 128)])
def test_k_twin_with_the_oracle_forward_equals_the_oracle_search(mode, C):
    """KTwin(leaves=1) whose eval_fn is the oracle's forward in the mode equals orc.mcts_search with EVAL_NET_BF16 /
    EVAL_NET_FP8 (root N, W, P bits): the route tests/test_gpu_search_net.py takes for K > 1 and Gumbel"""
    from test_leaf_parallel_cpu import KTwin, boards
    P = search_net(C, 1, VH, mode, SEED)
    on = oracle_net(P, mode)
    fn = oracle_eval_fn(on, mode)
    roots = opening_roots()[:4]
    res = run_threads(lambda i: orc.mcts_search(orc.GAME_REVERSI, int(roots[i][0]), int(roots[i][1]), int(roots[i][2]), 100,
                                                ORC_EVAL[mode], net=on), len(roots))
    for (_, _, tm, b), (n, w, p, _) in zip(roots, res):
        tw = KTwin("reversi", "net", leaves=1, eval_fn=fn, boards=boards())
        root = tw.search(b, tm, 100)
        N, W, Pr = np.zeros(65, np.uint32), np.zeros(65, np.float32), np.zeros(65, np.float32)
        for e in root["edges"]:
            N[e["a"]], W[e["a"]], Pr[e["a"]] = e["N"], e["W"], e["P"]
        assert np.array_equal(N, n) and np.array_equal(_bits(W), _bits(w)) and np.array_equal(_bits(Pr), _bits(p))


@pytest.mark.parametrize("bad", ["off", "on", "Search", 1, 0, 2.0, "", [], "true"])
def test_python_refuses_bad_eval_cache_before_touching_a_device(bad, monkeypatch):
    """eval_cache takes True / "carry" / "search" / False / None only: any other value (a truthy "off" used to switch the
    cache on) raises ValueError before a device is touched"""
    from betazero_amd import _lib
    from betazero_amd.engine import PipelinedSelfPlay, SelfPlayEngine, check_eval_cache

    def no_device(*a, **k):
        raise AssertionError("touched a device")
    monkeypatch.setattr(_lib, "require_gpu", no_device)
    monkeypatch.setattr(_lib, "lib", no_device)
    with pytest.raises(ValueError, match="eval_cache"):
        check_eval_cache(bad)
    with pytest.raises(ValueError, match="eval_cache"):
        SelfPlayEngine("reversi", 4, 16, "net_bf16", eval_cache=bad)
    with pytest.raises(ValueError, match="eval_cache"):
        PipelinedSelfPlay("reversi", 4, 16, "net_bf16", eval_cache=bad)


def test_python_accepts_every_eval_cache_mode():
    from betazero_amd.engine import EVAL_CACHE_MODES, check_eval_cache
    for m in EVAL_CACHE_MODES:
        assert check_eval_cache(m) is m
