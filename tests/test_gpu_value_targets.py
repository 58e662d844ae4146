"""Search-value targets on the GPU: k_root_q / k_pack_f32 against the twins of tests/test_value_targets_cpu.py
and the engine's own root statistics, bz_value_targets against the numpy twin, k_train_heads_vt against k_train_heads, the fp64
reference and autograd.  "Equal" = bit for bit unless a tolerance is named.  The feature observes: with it on, every byte the
engine wrote without it is the same byte."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from betazero_amd import _lib
from betazero_amd.engine import ForcedPlayouts, GumbelConfig, PlayoutCap
from test_gpu_playout_cap import _bits, _run, _same_rows
from test_value_targets_cpu import value_games, value_targets_twin

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NOISE = dict(dirichlet_alpha=0.3, dirichlet_eps=0.25)
CONFIGS = {
    "plain": {},
    "noise": dict(NOISE),
    "cap": dict(playout_cap=PlayoutCap(4, 0.5), **NOISE),
    "forced_cap": dict(forced_playouts=ForcedPlayouts(2.0), playout_cap=PlayoutCap(4, 0.5), **NOISE),
    "gumbel": dict(gumbel=GumbelConfig(), temp_moves=3),
    "leaves8": dict(leaves_per_step=8, **NOISE),
    "reuse": dict(reuse_subtree=True, **NOISE),
}
# the twin's arguments of the configurations a twin exists for (test_value_targets_cpu.value_games)
TWINS = {
    "plain": ("plain", {}),
    "noise": ("plain", dict(noise=True)),
    "cap": ("cap", dict(noise=True, cap=(4, 32768))),
    "forced_cap": ("forced", dict(noise=True, cap=(4, 32768))),
    "gumbel": ("gumbel", dict(temp_moves=3)),
    "reuse": ("plain", dict(noise=True, reuse=True)),
}


def _engine(game, n, sims, ev="hash", **kw):
    from betazero_amd.engine import SelfPlayEngine
    return SelfPlayEngine(game, n, sims, ev, **kw)


def _gathered(eng):
    """ex_q of the finished games in (round, slot, ply) order"""
    _, lens = eng.winners()
    q = eng.search_value_rows().cpu().numpy()
    return np.concatenate([q[r, b, :max(0, lens[r, b])] for r in range(lens.shape[0]) for b in range(lens.shape[1])] or
                          [np.zeros(0, np.float32)])


# ---------------------------------------------------------------- observes only
@pytest.mark.parametrize("game", ["ttt", "reversi4", "reversi6", "reversi"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_search_value_on_and_off_write_the_same_bytes(game, config):
    kw = dict(temp_moves=4, openings=1, seed=11, game_id_base=5)
    kw.update(CONFIGS[config])
    sims = 16 if game != "ttt" else 24
    off, on = _engine(game, 8, sims, **kw), _engine(game, 8, sims, search_value=True, **kw)
    _, (w0, l0), c0 = _run(off)
    _, (w1, l1), c1 = _run(on)
    assert (l0 >= 0).all() and np.array_equal(w0, w1) and np.array_equal(l0, l1)
    assert torch.equal(off.example_block(), on.example_block())
    print(config, game, "counters off / on:", c0, c1)
    assert c0 == c1, (c0, c1)
    ex = on.examples()
    assert ex.q.shape == (int(l1.sum()),) and ex.q.dtype == np.float32 and (np.abs(ex.q) <= 1).all() and ex.kl is None
    assert off.examples().q is None
    with pytest.raises(RuntimeError, match="search_value=True"):
        off.search_value_rows()


# ---------------------------------------------------------------- pinned to the twins
def _pinned(config, game, n, sims, **twin_kw):
    kind, tkw = TWINS[config]
    tkw = dict(tkw, **twin_kw)
    ekw = dict(CONFIGS[config])
    ekw["temp_moves"] = tkw.get("temp_moves", 0)
    eng = _engine(game, n, sims, search_value=True, seed=tkw.get("seed", 0), game_id_base=tkw.get("base", 0),
                  openings=tkw.get("openings", 0), **ekw)
    ex, (winners, lens), _ = _run(eng)
    twins = value_games(kind, game, n, sims, **tkw)
    q = eng.search_value_rows().cpu().numpy()
    total = 0
    for g, (rows, want, w) in enumerate(twins):
        assert lens[0, g] == len(rows) and winners[0, g] == w, (g, lens[0, g], len(rows))
        _same_rows(ex, tkw.get("base", 0) + g, rows, w)
        assert np.array_equal(_bits(q[0, g, :len(rows)]), _bits(want)), (config, game, g, q[0, g, :len(rows)], want)
        assert np.array_equal(_bits(ex.q[ex.game == tkw.get("base", 0) + g]), _bits(want))
        total += len(rows)
    assert len(ex) == total > 0 and (ex.q != 0).any()
    return eng, ex


@pytest.mark.parametrize("config", list(TWINS))
def test_ex_q_equals_the_twin_ttt_and_reversi4(config):
    _pinned(config, "ttt", 8, 24, seed=3, base=2)
    eng, ex = _pinned(config, "reversi4", 8, 16, seed=4)
    if config == "cap":  # nothing was written behind a game's recorded rows: the buffer's zeros are still there
        _, lens = eng.winners()
        q = eng.search_value_rows().cpu().numpy()
        assert all(not q[0, g, lens[0, g]:].any() for g in range(8)) and 0 < len(ex) < 8 * 12


def test_ex_q_equals_the_twin_reversi6_and_reversi8_with_openings_and_temperature():
    _pinned("plain", "reversi6", 4, 16, seed=3, base=2)
    _pinned("noise", "reversi", 4, 16, seed=3, base=7, temp_moves=8, openings=1)


def _root_value(N, W):
    n, w, out = np.ascontiguousarray(N, np.uint32), np.ascontiguousarray(W, np.float32), C.c_float()
    assert _lib.lib().bz_root_value(n.ctypes.data, w.ctypes.data, len(n), C.addressof(out)) == 0
    return out.value


def _search_by_steps(eng):
    """one search through the step API with the engine's own evaluator (the sequence of SelfPlayEngine.search_external)"""
    eng.root_begin(); eng.evaluate(); eng.expand_backup()
    eng.root_noise()
    for s in range(0, eng.sims, eng.K):
        eng.select(s); eng.evaluate(); eng.expand_backup()


def _step_api_case(eng, n, by_steps=False):
    """play the games through search() -- or the step API -- / root_stats() / play(): every recorded row's q must be
    bz_root_value of the root statistics the engine itself reported before the play (an action without an edge has N = 0 and
    W = +0: adding it changes neither sum, so the NA actions in ascending order stand for the edges)"""
    eng.reset_games()
    stats = [[] for _ in range(n)]
    for _ in range(140):
        _, _, _, state = eng.positions()
        if by_steps:
            _search_by_steps(eng)
        else:
            eng.search()
        N, W, _ = eng.root_stats()
        for g in range(n):
            if state[g] == 0:
                stats[g].append(_root_value(N[g], W[g]))
        eng.play(False)
        if eng.status()[0] == 0:
            break
    ex = eng.examples()
    for g in range(n):
        m = ex.game == g
        assert int(m.sum()) == len(stats[g]) > 0
        assert np.array_equal(_bits(ex.q[m]), _bits(stats[g])), (g, ex.q[m], stats[g])
    assert (ex.q != 0).any() and (np.abs(ex.q) <= 1).all()
    return ex


@pytest.mark.parametrize("config,by_steps", [("noise", True), ("leaves8", True), ("leaves8", False), ("reuse", False), ("gumbel", False),
                                             ("forced", False)])
def test_ex_q_equals_root_value_of_the_engines_own_root_stats_taken_before_play(config, by_steps):
    kw = dict(forced_playouts=ForcedPlayouts(2.0), **NOISE) if config == "forced" else CONFIGS[config]
    _step_api_case(_engine("reversi4", 8, 16, search_value=True, seed=6, **dict(dict(temp_moves=2), **kw)), 8, by_steps)


def test_ex_q_with_the_bf16_net_equals_root_value_of_the_engines_own_root_stats():
    """the bf16 net in the loop, searched through the step API.  64 channels x 2 blocks: the smallest width the MFMA tower is
    built for (bz_net_forward_bf16 refuses 32 channels, so a 32-channel bf16 net cannot be searched with)"""
    from test_gpu_search_net import _dn, _net
    P, _ = _net("bf16", 64, 2)
    _step_api_case(_engine("reversi6", 8, 16, "net_bf16", net=_dn(P, 8), search_value=True, temp_moves=4, seed=2), 8, by_steps=True)


# ---------------------------------------------------------------- packing
def test_device_examples_q_is_ex_q_in_round_slot_ply_order_next_to_kl():
    eng = _engine("reversi4", 8, 16, search_value=True, surprise=True, temp_moves=4, seed=1, **NOISE)
    _run(eng)
    want = _gathered(eng)
    dx = eng.device_examples()
    assert dx.q.is_cuda and np.array_equal(_bits(dx.q.cpu().numpy()), _bits(want)) and len(dx) == len(want) > 0
    assert np.array_equal(_bits(eng.examples().q), _bits(want)) and np.array_equal(_bits(dx.cpu().q), _bits(want))
    assert dx.kl is not None and dx.kl.shape == dx.q.shape and dx.vt is None


def test_two_pipelines_append_at_the_right_offset_and_self_play_carries_q():
    from betazero_amd.engine import PipelinedSelfPlay, self_play
    kw = dict(temp_moves=4, seed=1, playout_cap=PlayoutCap(4, 0.5), **NOISE)  # (the cap: games of unequal row counts)
    sp = PipelinedSelfPlay("reversi4", 8, 16, "hash", pipelines=2, search_value=True, **kw)
    sp.run_iteration()
    assert sp.status()[0] == 0
    want = np.concatenate([_gathered(e) for e in sp.engines])
    dx, hx = sp.device_examples(), sp.examples()
    assert len(dx) == len(want) > 0 and np.array_equal(_bits(dx.q.cpu().numpy()), _bits(want)) and np.array_equal(_bits(hx.q), _bits(want))
    assert dx.kl is None and hx.kl is None
    blk, q = sp.pack_examples_with_search_value()
    assert np.array_equal(_bits(q[:len(want)].cpu().numpy()), _bits(want))
    one = _engine("reversi4", 8, 16, search_value=True, **kw)  # the same games on one engine: the same rows, the same q
    _run(one)
    ox = one.examples()
    assert np.array_equal(ox.game, hx.game) and np.array_equal(_bits(ox.pi), _bits(hx.pi)) and np.array_equal(_bits(ox.q), _bits(hx.q))
    _, _, _, sx = self_play("reversi4", 8, 16, seed=1, evaluator="hash", temp_moves=4, search_value=True, pipelines=2,
                            playout_cap=PlayoutCap(4, 0.5), **NOISE)
    assert np.array_equal(_bits(sx.q), _bits(want))
    assert self_play("reversi4", 4, 8, evaluator="hash")[3].q is None
    with pytest.raises(RuntimeError, match="search_value=True"):
        PipelinedSelfPlay("reversi4", 4, 8, "hash", pipelines=1).pack_examples_with_search_value()


def test_a_block_too_small_leaves_the_same_games_out_of_both_arrays():
    from betazero_amd.engine import _packed_views, packed_block_header
    eng = _engine("reversi4", 8, 16, search_value=True, temp_moves=4, seed=1, **NOISE)
    _run(eng)
    want = _gathered(eng)
    cap = len(want) // 2
    blk = eng.pack_examples(cap_rows=cap)
    q = torch.full((cap + 64,), -7.0, device=DEV)
    eng.pack_search_value(q, cap)
    h = packed_block_header(blk, strict=False)
    n = h["n_rows"]
    assert 0 < n <= cap and h["dropped_rows"] == len(want) - n
    q = q.cpu().numpy()
    assert np.array_equal(_bits(q[:n]), _bits(want[:n])) and (q[n:] == -7.0).all()  # (the games that fit are a prefix)
    games = _packed_views(blk, h)["game"].cpu().numpy()
    full = eng.examples()
    assert np.array_equal(games, full.game[:n]) and np.array_equal(_bits(q[:n]), _bits(full.q[:n]))


# ---------------------------------------------------------------- bz_value_targets
GUARD = 16


def _rows_from_lengths(lengths, seed, gaps=True):
    """rows of consecutive segments of the given lengths: game ids that change from segment to segment except where a
    falling ply alone marks the boundary, plies ascending with gaps (rows a fast search did not record), movers with
    repeats, z consistent with one winner per segment, q with NaN / inf / out-of-range values among ordinary ones"""
    g = np.random.default_rng(seed)
    q, z, m, game, ply = [], [], [], [], []
    gid = 100
    for k, T in enumerate(lengths):
        gid += int(g.integers(0, 2)) if k else 0  # (0: the same id as the previous segment -- the ply restarts at 0)
        mv = np.where(g.random(T) < 0.5, 1, -1).astype(np.int8)
        w = int(g.integers(-1, 2))
        steps = (1 + (g.random(T) < 0.2) * g.integers(1, 3, T)) if (gaps and T <= 80) else np.ones(T, np.int64)
        p = np.cumsum(steps) - steps[0]
        qq = (g.random(T) * 2 - 1).astype(np.float32)
        hit = g.random(T) < 0.1
        qq[hit] = g.choice(np.array([np.nan, np.inf, -np.inf, 1.0, -1.0, 2.5, -7.0], np.float32), int(hit.sum()))
        q.append(qq); z.append((mv * w).astype(np.int8)); m.append(mv); game.append(np.full(T, gid, np.int64)); ply.append(p.astype(np.int32))
    cat = lambda a, dt: np.concatenate(a).astype(dt) if a else np.zeros(0, dt)  # noqa: E731
    return cat(q, np.float32), cat(z, np.int8), cat(m, np.int8), cat(game, np.int64), cat(ply, np.int32)


def _value_targets(rows, lam, q_mix):
    """bz_value_targets on device copies of the rows: (vt with GUARD words behind it, the status word and the words behind it)"""
    q, z, m, game, ply = rows
    n = len(q)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    d = [t(q), t(z), t(m), t(game), t(ply)]
    vt = torch.full((n + GUARD,), -7.0, dtype=torch.float32, device=DEV)
    status = torch.full((1 + GUARD,), -7, dtype=torch.int64, device=DEV)
    _lib.check(_lib.lib().bz_value_targets(*(x.data_ptr() for x in d), n, lam, q_mix, vt.data_ptr(), status.data_ptr(),
                                           torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return vt.cpu().numpy(), status.cpu().numpy()


def _lengths(n, seed, forced_cuts=(), keep_whole=()):
    """segment lengths summing to n: random cuts (segments of 1 .. 60 rows), a boundary at every row of forced_cuts, none
    inside the (a, b) ranges of keep_whole"""
    g = np.random.default_rng(seed)
    cuts, at = set(), 0
    while at < n:
        cuts.add(at)
        at += int(g.integers(1, 61))
    cuts |= {c for c in forced_cuts if c < n}
    cuts = sorted(c for c in cuts if not any(a < c < b for a, b in keep_whole))
    return [b - a for a, b in zip(cuts, cuts[1:] + [n])]


# a workgroup holds 256 rows.  255 / 256 / 257: the last segment ends one row short of, at and one row behind the edge;
# 1025: a segment straddling row 256, boundaries exactly at rows 512 and 1024, a one-row segment in the fifth workgroup
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
@pytest.mark.parametrize("lam,q_mix", [(0.8, 0.25), (1.0, 0.0), (0.0, 1.0)])
def test_value_targets_equal_the_numpy_twin(n, lam, q_mix):
    lengths = _lengths(n, n, forced_cuts=(256, 512, 1024) if n != 1025 else (512, 1024), keep_whole=((250, 270),) if n == 1025 else ())
    assert sum(lengths) == n
    if n == 1025:
        starts = np.cumsum([0] + lengths[:-1])
        assert any(s < 256 < s + T for s, T in zip(starts, lengths)) and {512, 1024} <= set(starts) and lengths[-1] == 1
    rows = _rows_from_lengths(lengths, n)
    want, status = value_targets_twin(*rows, lam, q_mix)
    assert status == 0
    vt, st = _value_targets(rows, lam, q_mix)
    assert np.array_equal(_bits(vt[:n]), _bits(want)), (n, np.nonzero(_bits(vt[:n]) != _bits(want))[0][:8])
    assert (vt[n:] == -7.0).all() and st[0] == 0 and (st[1:] == -7).all() and (np.abs(vt[:n]) <= 1).all()
    vt2, st2 = _value_targets(rows, lam, q_mix)  # run to run: the same bits
    assert np.array_equal(_bits(vt), _bits(vt2)) and np.array_equal(st, st2)
    if (lam, q_mix) == (1.0, 0.0):
        assert np.array_equal(vt[:n], rows[1].astype(np.float32))  # the plain outcome, by value
    if (lam, q_mix) == (0.0, 1.0):
        with np.errstate(all="ignore"):
            assert np.array_equal(vt[:n], np.where(rows[0] != rows[0], 0, np.clip(rows[0], -1, 1)).astype(np.float32))


def test_value_targets_one_long_segment_all_one_row_segments_and_no_rows():
    one = _rows_from_lengths([300], 2, gaps=False)
    # (one game id throughout and a ply that never rises: every row is its own segment)
    singles = one[:3] + (np.zeros(300, np.int64), np.zeros(300, np.int32))
    for rows in (_rows_from_lengths([60], 1), singles, _rows_from_lengths([1, 1, 58, 1], 3)):
        want, status = value_targets_twin(*rows, 0.5, 0.5)
        vt, st = _value_targets(rows, 0.5, 0.5)
        n = len(rows[0])
        assert status == 0 and st[0] == 0 and np.array_equal(_bits(vt[:n]), _bits(want)) and (vt[n:] == -7.0).all()
    vt, st = _value_targets(tuple(a[:0] for a in rows), 0.5, 0.5)  # n = 0: the status word is still written
    assert st[0] == 0 and (vt == -7.0).all()


def test_a_segment_of_1025_rows_keeps_z_and_is_counted_its_neighbours_are_not_touched_by_it():
    rows = _rows_from_lengths([10, 1025, 1024, 7], 5, gaps=False)
    want, status = value_targets_twin(*rows, 0.8, 0.25)
    assert status == 1
    vt, st = _value_targets(rows, 0.8, 0.25)
    n = len(rows[0])
    assert st[0] == 1 and (st[1:] == -7).all() and np.array_equal(_bits(vt[:n]), _bits(want)) and (vt[n:] == -7.0).all()
    assert np.array_equal(vt[10:1035], rows[1][10:1035].astype(np.float32))     # the long segment: (float)z
    assert not np.array_equal(vt[1035:2059], rows[1][1035:2059].astype(np.float32))  # 1024 rows: still walked
    from betazero_amd.engine import DeviceExamples, Examples
    from betazero_amd.value_targets import value_targets
    q, z, m, game, ply = rows
    zeros = np.zeros(n, np.uint64)
    ex = DeviceExamples.from_host(Examples(zeros, zeros, np.zeros((n, 9), np.float32), z, m, np.zeros(n, np.uint8), game, ply, 3, q=q))
    with pytest.raises(RuntimeError, match="1 game"):
        value_targets(ex, 0.8, 0.25)
    ok = value_targets(select_first(ex, 10), 0.8, 0.25)
    assert np.array_equal(_bits(ok.vt.cpu().numpy()), _bits(want[:10])) and ok.q is not None and ex.vt is None


def select_first(ex, k):
    from betazero_amd.train import select_rows
    return select_rows(ex, torch.arange(k, device=DEV))


# ---------------------------------------------------------------- the head kernel
def _heads_setup(C, n, VH, seed):
    from betazero_amd.train_kernels import StepPlan
    from test_gpu_train_numerics import _batch, _boards, _heads_case, _net
    x, P, pi, z = _heads_case(C, n, VH, seed)
    net = _net(C, 1, VH, P=P)
    sp = StepPlan(net, n)
    own, opp = _boards(n, 1)
    sp.set_batch(*_batch(own, opp, pi, z))
    return x, P, pi, z, net, sp


def _run_heads_vt(sp, x, vt, n, C, VH):
    import ctypes as ct
    L, s, Ly = _lib.lib(), torch.cuda.current_stream().cuda_stream, sp.L
    slot = torch.tensor([vt.data_ptr()], dtype=torch.int64, device=DEV)
    sp.acts[Ly].copy_(x.to(DEV))
    _lib.check(L.bz_train_heads_vt(sp.acts[Ly].data_ptr(), sp.batch_desc.data_ptr(), slot.data_ptr(), n, C, VH, ct.byref(sp._head),
                                   sp.gs[Ly].data_ptr(), sp.hv.data_ptr(), sp.dl.data_ptr(), sp.dv1.data_ptr(), sp.heads_partial.data_ptr(), s))
    _lib.check(L.bz_train_heads_wgrad(sp.hv.data_ptr(), sp.dl.data_ptr(), sp.dv1.data_ptr(), n, VH, sp.heads_w_partial.data_ptr(), s))
    _lib.check(L.bz_train_finish(ct.byref(sp._partials), ct.byref(sp._grads), C, Ly, VH, n, sp.losses.data_ptr(), None, s))
    torch.cuda.synchronize()


def _snapshot(net, sp):
    out = {"g_top": sp.gs[sp.L], "hv": sp.hv, "dl": sp.dl, "dv1": sp.dv1, "partial": sp.heads_partial, "heads_w": sp.heads_w_partial,
           "losses": sp.losses}
    out.update({"grad " + k: p.grad for k, p in net.named_parameters()})
    return {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize("C,n,VH", [(64, 8, 64), (128, 20, 64)])
def test_heads_vt_with_vt_equal_to_z_is_bitwise_the_z_kernel(C, n, VH):
    from test_gpu_train_numerics import _run_heads
    x, P, pi, z, net, sp = _heads_setup(C, n, VH, 31 + n)
    _run_heads(net, sp, x, n, C, VH)
    want = _snapshot(net, sp)
    for t in (sp.gs[sp.L], sp.hv, sp.dl, sp.dv1, sp.heads_partial, sp.heads_w_partial):
        t.fill_(7.0)  # what the second run leaves is its own
    sp.losses[:3].fill_(7.0)  # (losses[3], the error word, accumulates)
    vt = z.to(DEV, torch.float32).contiguous()
    _run_heads_vt(sp, x, vt, n, C, VH)
    got = _snapshot(net, sp)
    assert set(got) == set(want) and float(want["losses"][2]) > 0 and bool((want["g_top"] != 0).any())
    for k in want:
        assert torch.equal(got[k].view(torch.uint8), want[k].view(torch.uint8)), k


@pytest.mark.parametrize("C,n,VH", [(64, 8, 64), (128, 20, 64)])
def test_heads_vt_with_dyadic_fractional_targets_within_the_derived_bounds(C, n, VH):
    """targets that are multiples of 2^-8 in [-1, 1] (exact in fp32, like z): the losses, all ten head gradients and g[L] within
    the bounds heads_ref derives for the kernel's fp32 operations -- the bounds of tests/test_gpu_train_numerics.py, unchanged"""
    from test_gpu_train_numerics import _check_heads
    from test_train_numerics_cpu import heads_ref
    x, P, pi, z, net, sp = _heads_setup(C, n, VH, 31 + n)
    g = torch.Generator().manual_seed(C + n)
    vt = torch.randint(-256, 257, (n,), generator=g).double() * 2.0 ** -8
    vt[0], vt[1], vt[2] = 1.0, -1.0, 2.0 ** -8
    assert bool(((vt != vt.round())).any())
    _run_heads_vt(sp, x, vt.to(DEV, torch.float32).contiguous(), n, C, VH)
    r = heads_ref(x.to(DEV), {k: v.to(DEV) for k, v in P.items()}, pi.to(DEV), vt.to(DEV))
    ambiguous = _check_heads(net, sp, r)
    assert ambiguous < 0.01 * x.numel() and float((sp.gs[sp.L] != 0).float().mean()) > 0.05
    rz = heads_ref(x.to(DEV), {k: v.to(DEV) for k, v in P.items()}, pi.to(DEV), z.to(DEV))
    assert float((r["mse"].v - rz["mse"].v).abs()) > 1e-3  # (the targets matter: not the z losses)


def _vt_examples(own, opp, pi, z, vt):
    from betazero_amd.engine import DeviceExamples
    n = own.shape[0]
    zero = lambda dt: torch.zeros(n, dtype=dt, device=DEV)  # noqa: E731
    return DeviceExamples(own, opp, pi, z, torch.ones(n, dtype=torch.int8, device=DEV), zero(torch.uint8), zero(torch.int64),
                          zero(torch.int32), 8, vt=vt)


def test_whole_step_with_value_targets_vs_train_step_autograd_fp32():
    """StepPlan(value_targets=True).grads against train_step(..., value_targets=True) -- autograd through the plain fp32 torch
    forward of the same module on the same batch and targets -- to the tolerance of tests/test_gpu_train_kernels.py's
    whole-step check: losses within 2 %, every gradient's cosine > 0.99 (stem 0.97), magnitudes within 10 %"""
    import torch.nn.functional as F
    from betazero_amd.train import make_optimizer, train_step
    from betazero_amd.train_kernels import StepPlan
    from test_gpu_train_kernels import _net_case
    C, NB, n = 64, 2, 64
    m, _, own, opp, pi, z = _net_case(C, NB, n, 23)
    plan = StepPlan(m, n, value_targets=True)
    g = torch.Generator().manual_seed(4)
    vt = (torch.rand(n, generator=g) * 2 - 1).to(DEV)
    with pytest.raises(ValueError, match="vt"):
        plan.set_batch(own, opp, pi, z)                      # a value-target plan needs the targets
    with pytest.raises(ValueError, match="vt"):
        plan.set_batch(own, opp, pi, z, vt=vt.double())
    with pytest.raises(ValueError, match="value_targets=True"):
        StepPlan(m, n).set_batch(own, opp, pi, z, vt=vt)     # ... and a plain plan refuses them
    plan = StepPlan(m, n, value_targets=True)                # (the plain plan above took the parameters' .grad)
    losses = plan.grads(own, opp, pi, z, vt=vt).clone()
    got = {k: p.grad.clone() for k, p in m.named_parameters()}
    assert float(losses[3]) == 0.0 and all(bool(torch.isfinite(x).all()) for x in got.values())
    z_losses = StepPlan(m, n).grads(own, opp, pi, z).clone()
    assert abs(float(z_losses[2]) - float(losses[2])) > 1e-3 and float(z_losses[1]) == float(losses[1])  # another MSE, the same CE
    ex = _vt_examples(own, opp, pi, z, vt)
    with pytest.raises(ValueError, match="vt"):
        train_step(m, None, _vt_examples(own, opp, pi, z, None), value_targets=True)
    want = train_step(m, make_optimizer(m, lr=0.0), ex, autocast=False, value_targets=True)   # (lr 0: the weights stay)
    assert np.allclose(losses[:3].cpu().numpy(), [float(w) for w in want], rtol=2e-2, atol=2e-3), (losses, want)
    ref = {k: p.grad for k, p in m.named_parameters()}
    cos = {k: float(F.cosine_similarity(got[k].flatten(), ref[k].flatten(), dim=0)) for k in got if got[k].numel() > 1}
    mag = {k: float(got[k].norm() / ref[k].norm().clamp(min=1e-20)) for k in got}
    print("cosine of kernel vs autograd gradients:", {k: round(c, 4) for k, c in cos.items()})
    for k, c in cos.items():
        assert c > (0.97 if k.startswith("stem") else 0.99), (k, c)
    assert all(0.9 < r < 1.1 for k, r in mag.items() if got[k].numel() >= 64), mag


def test_graphed_step_follows_set_batch_to_a_second_vt_tensor_without_recapture():
    from betazero_amd.train import GraphedTrainStep
    from betazero_amd.train_kernels import StepPlan
    from test_gpu_train_kernels import _net_case
    n, rows = 32, 96
    m, _, own, opp, pi, z = _net_case(64, 1, rows, 24)
    twin = copy.deepcopy(m)
    gen = torch.Generator(device=DEV).manual_seed(1)
    idx = torch.randint(0, rows, (n,), device=DEV, generator=gen)
    vt1 = (torch.rand(rows, device=DEV, generator=gen) * 2 - 1).contiguous()
    vt2 = (torch.rand(rows, device=DEV, generator=gen) * 2 - 1).contiguous()
    step = GraphedTrainStep(m, lr=1e-3, batch=n, value_targets=True)
    assert step.step_plan is not None and step.step_plan.value_targets
    with pytest.raises(ValueError, match="vt"):
        step(_vt_examples(own, opp, pi, z, None), idx)
    a = step(_vt_examples(own, opp, pi, z, vt1), idx)
    graph = step.graph
    b = step(_vt_examples(own, opp, pi, z, vt2), idx)
    step.check()
    assert step.graph is graph and graph is not None  # replayed, not recaptured
    # the same two steps, launched eagerly on a copy of the net
    plan = StepPlan(twin, n, value_targets=True)
    plan.enable_adam(1e-3)
    plan.set_batch(own, opp, pi, z, idx, vt=vt1)
    ea = plan.step().clone()
    plan.set_batch(own, opp, pi, z, idx, vt=vt2)
    eb = plan.step().clone()
    assert torch.equal(a, ea[:3]) and torch.equal(b, eb[:3]), (a, ea, b, eb)
    plan.set_batch(own, opp, pi, z, idx, vt=vt1)              # (the second tensor mattered: the same weights on the first)
    first = plan.grads()[:3].clone()
    assert not torch.equal(first, plan.grads(own, opp, pi, z, idx, vt=vt2)[:3])


def test_an_out_of_range_index_lands_in_the_error_word_with_value_targets_too():
    from betazero_amd.train_kernels import StepPlan
    from test_gpu_train_kernels import _net_case
    n, rows = 32, 304
    m, _, own, opp, pi, z = _net_case(64, 1, rows, 24)
    plan = StepPlan(m, n, value_targets=True)
    gen = torch.Generator(device=DEV).manual_seed(1)
    idx = torch.randint(0, rows, (n,), device=DEV, generator=gen)
    vt = (torch.rand(rows, device=DEV, generator=gen) * 2 - 1).contiguous()
    a = plan.grads(own, opp, pi, z, idx, vt=vt).clone()
    b = plan.grads(own[idx].contiguous(), opp[idx].contiguous(), pi[idx].contiguous(), z[idx].contiguous(), vt=vt[idx].contiguous()).clone()
    assert torch.equal(a, b) and float(a[3]) == 0.0  # vt is gathered by the same idx as the rest of the row
    bad, good = idx.clone(), idx.clone()
    bad[3], bad[7], bad[20] = rows + 1000, -5, rows
    good[3], good[7], good[20] = rows - 1, 0, rows - 1
    c = plan.grads(own, opp, pi, z, bad, vt=vt).clone()
    assert float(c[3]) == 3.0
    d = plan.grads(own, opp, pi, z, good, vt=vt).clone()
    assert torch.equal(c[:3], d[:3]) and float(d[3]) == 3.0  # clamped like z: row 0 / the last row, no fault
    with pytest.raises(IndexError, match="3 batch position"):
        plan.check_rows()


# ---------------------------------------------------------------- end to end
def test_value_targets_end_to_end_self_play_augment_one_graphed_step():
    from betazero_amd.augment import augment_examples
    from betazero_amd.engine import DeviceExamples, self_play
    from betazero_amd.net import PolicyValueNet
    from betazero_amd.train import GraphedTrainStep
    from betazero_amd.value_targets import value_targets
    _, _, _, hx = self_play("reversi", 8, 16, seed=2, evaluator="hash", temp_moves=6, openings=1, search_value=True,
                            playout_cap=PlayoutCap(4, 0.5), **NOISE)
    ex = DeviceExamples.from_host(hx)
    data = value_targets(ex, lam=0.8, q_mix=0.25)
    want, status = value_targets_twin(hx.q, hx.z, hx.mover, hx.game, hx.ply, 0.8, 0.25)
    assert status == 0 and data.vt.is_cuda and np.array_equal(_bits(data.vt.cpu().numpy()), _bits(want)) and len(data) > 64
    assert data.q is ex.q and ex.vt is None and (np.abs(want) <= 1).all() and not np.array_equal(want, hx.z.astype(np.float32))
    assert np.array_equal(value_targets(ex).vt.cpu().numpy(), hx.z.astype(np.float32))  # the defaults: the plain outcome
    aug = augment_examples(data, dedupe=True)
    assert len(data) < len(aug) <= 8 * len(data)
    src = {(int(g), int(p)): (a, b) for g, p, a, b in zip(hx.game, hx.ply, _bits(want), _bits(hx.q))}
    got = aug.cpu()
    assert all(src[(int(g), int(p))] == (a, b) for g, p, a, b in zip(got.game, got.ply, _bits(got.vt), _bits(got.q)))
    raw = augment_examples(data, dedupe=False)
    assert np.array_equal(_bits(raw.vt.cpu().numpy()), np.repeat(_bits(want), 8))
    torch.manual_seed(0)
    g = GraphedTrainStep(PolicyValueNet(64, 2, 64, fused_tower=True).cuda(), lr=1e-3, batch=64, value_targets=True)
    gen = torch.Generator(device=DEV).manual_seed(0)
    loss = g(aug, torch.randint(0, len(aug), (64,), device=DEV, generator=gen))
    g.check()
    assert np.isfinite(loss.cpu().numpy()).all()
