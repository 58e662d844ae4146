"""Policy surprise weighting on the GPU: k_surp_save / k_surp_note / k_surp_kl / k_pack_f32 and the resampler
(csrc/bz_surprise.hip) against the twins of tests/test_surprise_cpu.py.  "Equal" = bit for bit.  The feature observes: with it
on, every byte the engine wrote without it is the same byte."""
import ctypes as C

import numpy as np
import pytest
import torch

from betazero_amd import _lib
from betazero_amd.engine import ForcedPlayouts, GumbelConfig, PlayoutCap
from test_gpu_playout_cap import _bits, _run, _same_rows
from test_surprise_cpu import resample_twin, surprise_games

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


def _engine(game, n, sims, ev="hash", **kw):
    from betazero_amd.engine import SelfPlayEngine
    return SelfPlayEngine(game, n, sims, ev, **kw)


def _gathered(eng):
    """ex_kl of the finished games in (round, slot, ply) order"""
    _, lens = eng.winners()
    kl = eng.surprise_rows().cpu().numpy()
    return np.concatenate([kl[r, b, :max(0, lens[r, b])] for r in range(lens.shape[0]) for b in range(lens.shape[1])] or
                          [np.zeros(0, np.float32)])


# ---------------------------------------------------------------- observes only
@pytest.mark.parametrize("game", ["ttt", "reversi4", "reversi6", "reversi"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_surprise_on_and_off_write_the_same_bytes(game, config):
    kw = dict(temp_moves=4, openings=1, seed=11, game_id_base=5)
    kw.update(CONFIGS[config])
    sims = 16 if game != "ttt" else 24
    off, on = _engine(game, 64, sims, **kw), _engine(game, 64, sims, surprise=True, **kw)
    _, (w0, l0), c0 = _run(off)
    _, (w1, l1), c1 = _run(on)
    assert (l0 >= 0).all() and np.array_equal(w0, w1) and np.array_equal(l0, l1)
    assert torch.equal(off.example_block(), on.example_block())
    print(config, game, "counters off / on:", c0, c1)
    assert c0 == c1, (c0, c1)
    assert on.examples().kl.shape == (int(l1.sum()),)


# ---------------------------------------------------------------- pinned to the twin
def _pinned(kind, game, n, sims, engine_kw, **twin_kw):
    eng = _engine(game, n, sims, surprise=True, seed=twin_kw.get("seed", 0), game_id_base=twin_kw.get("base", 0),
                  temp_moves=twin_kw.get("temp_moves", 0), openings=twin_kw.get("openings", 0), **engine_kw)
    ex, (winners, lens), _ = _run(eng)
    twins = surprise_games(kind, game, n, sims, **twin_kw)
    kl = eng.surprise_rows().cpu().numpy()
    total = 0
    for g, (rows, want, w) in enumerate(twins):
        assert lens[0, g] == len(rows) and winners[0, g] == w, (g, lens[0, g], len(rows))
        _same_rows(ex, twin_kw.get("base", 0) + g, rows, w)
        assert np.array_equal(_bits(kl[0, g, :len(rows)]), _bits(want)), (g, kl[0, g, :len(rows)], want)
        assert np.array_equal(_bits(ex.kl[ex.game == twin_kw.get("base", 0) + g]), _bits(want))
        total += len(rows)
    assert len(ex) == total and (ex.kl >= 0).all()
    return eng, ex, twins


def test_plain_kl_equals_the_twin():
    for game, n, sims in (("ttt", 16, 24), ("reversi4", 16, 16), ("reversi6", 4, 16)):
        _, ex, _ = _pinned("plain", game, n, sims, {}, seed=3, base=2)
        assert (ex.kl > 0).any()


def test_kl_is_against_the_prior_before_the_dirichlet_noise():
    """the case that fails if the prior is read after the noise has rewritten it"""
    _pinned("plain", "reversi4", 16, 16, NOISE, seed=4, noise=True)
    _pinned("plain", "ttt", 16, 24, NOISE, seed=5, temp_moves=3, noise=True)


def test_kl_under_the_cap_fast_searches_record_no_row_and_no_kl():
    eng, ex, twins = _pinned("cap", "reversi4", 16, 16, dict(playout_cap=PlayoutCap(4, 0.5), **NOISE), seed=6, noise=True, cap=(4, 32768))
    _, lens = eng.winners()
    kl = eng.surprise_rows().cpu().numpy()
    for g in range(16):  # nothing was written behind a game's recorded rows: the buffer's zeros are still there
        assert not kl[0, g, lens[0, g]:].any()
    assert 0 < len(ex) < 16 * 12


def test_kl_with_forced_playouts_is_of_the_pruned_pi():
    _pinned("forced", "reversi4", 16, 16, dict(forced_playouts=ForcedPlayouts(2.0), **NOISE), seed=7, noise=True)
    _pinned("forced", "ttt", 12, 24, dict(forced_playouts=ForcedPlayouts(2.0), playout_cap=PlayoutCap(6, 0.5), **NOISE), seed=8,
            noise=True, cap=(6, 32768))


def test_kl_with_gumbel_is_of_the_improved_policy():
    _pinned("gumbel", "reversi4", 16, 16, dict(gumbel=GumbelConfig()), seed=9, temp_moves=3)


def test_kl_under_subtree_reuse_a_kept_root_has_its_raw_prior():
    _pinned("plain", "reversi4", 16, 16, dict(reuse_subtree=True, **NOISE), seed=10, noise=True, reuse=True)


def test_reversi8_with_openings_and_temperature_equals_the_twin():
    _pinned("plain", "reversi", 4, 16, NOISE, seed=3, base=7, temp_moves=8, openings=1, noise=True)


def test_bf16_net_kl_equals_the_host_function_on_the_engines_own_prior_and_pi():
    """tolerance 0: the engine's kl against bz_surprise_kl fed root_stats()' P of this noise-free run and the recorded pi"""
    from test_gpu_search_net import _dn, _net
    P, _ = _net("bf16", 64, 1)
    eng = _engine("reversi6", 8, 16, "net_bf16", net=_dn(P, 8), surprise=True, temp_moves=4, seed=2)
    eng.reset_games()
    priors = [[] for _ in range(8)]
    for _ in range(80):
        _, _, _, state = eng.positions()
        eng.search()
        N, _, Pr = eng.root_stats()
        for g in range(8):
            if state[g] == 0:
                priors[g].append((N[g].copy(), Pr[g].copy()))
        eng.play(False)
        if eng.status()[0] == 0:
            break
    ex = eng.examples()
    L = _lib.lib()
    checked = 0
    for g in range(8):
        m = ex.game == g
        assert int(m.sum()) == len(priors[g])
        for pi, kl, (N, Pr) in zip(ex.pi[m], ex.kl[m], priors[g]):
            a = np.nonzero((Pr > 0) | (N > 0))[0]  # the root's edges, ascending (an edge with P = 0 and N = 0 has pi = 0: never read)
            p, q, out = np.ascontiguousarray(pi[a]), np.ascontiguousarray(Pr[a]), C.c_float()
            assert L.bz_surprise_kl(p.ctypes.data, q.ctypes.data, len(a), C.addressof(out)) == 0
            assert _bits(out.value) == _bits(kl), (g, out.value, kl)
            checked += 1
    assert checked == len(ex) > 0 and (ex.kl > 0).any()


# ---------------------------------------------------------------- packing
def test_device_examples_kl_is_ex_kl_in_round_slot_ply_order():
    eng = _engine("reversi4", 64, 16, surprise=True, temp_moves=4, seed=1, **NOISE)
    _run(eng)
    want = _gathered(eng)
    dx = eng.device_examples()
    assert dx.kl.is_cuda and np.array_equal(_bits(dx.kl.cpu().numpy()), _bits(want)) and len(dx) == len(want) > 0
    assert np.array_equal(_bits(eng.examples().kl), _bits(want))
    assert np.array_equal(_bits(dx.cpu().kl), _bits(want))


def test_two_pipelines_append_at_the_right_offset_and_self_play_carries_kl():
    from betazero_amd.engine import PipelinedSelfPlay, self_play
    kw = dict(temp_moves=4, seed=1, playout_cap=PlayoutCap(4, 0.5), **NOISE)  # (the cap: games of unequal row counts)
    sp = PipelinedSelfPlay("reversi4", 16, 16, "hash", pipelines=2, surprise=True, **kw)
    sp.run_iteration()
    assert sp.status()[0] == 0
    want = np.concatenate([_gathered(e) for e in sp.engines])
    dx, hx = sp.device_examples(), sp.examples()
    assert len(dx) == len(want) > 0 and np.array_equal(_bits(dx.kl.cpu().numpy()), _bits(want)) and np.array_equal(_bits(hx.kl), _bits(want))
    one = _engine("reversi4", 16, 16, surprise=True, **kw)  # the same games on one engine: the same rows, the same kl
    _run(one)
    ox = one.examples()
    assert np.array_equal(ox.game, hx.game) and np.array_equal(_bits(ox.pi), _bits(hx.pi)) and np.array_equal(_bits(ox.kl), _bits(hx.kl))
    _, _, _, sx = self_play("reversi4", 16, 16, seed=1, evaluator="hash", temp_moves=4, surprise=True, pipelines=2,
                            playout_cap=PlayoutCap(4, 0.5), **NOISE)
    assert np.array_equal(_bits(sx.kl), _bits(want))
    assert self_play("reversi4", 4, 8, evaluator="hash")[3].kl is None


def test_a_block_too_small_leaves_the_same_games_out_of_both_arrays():
    from betazero_amd.engine import _packed_views, packed_block_header
    eng = _engine("reversi4", 64, 16, surprise=True, temp_moves=4, seed=1, **NOISE)
    _run(eng)
    want = _gathered(eng)
    cap = len(want) // 2
    blk = eng.pack_examples(cap_rows=cap)
    kl = torch.full((cap + 64,), -1.0, device=DEV)
    eng.pack_surprise(kl, cap)
    h = packed_block_header(blk, strict=False)
    n = h["n_rows"]
    assert 0 < n <= cap and h["dropped_rows"] == len(want) - n
    kl = kl.cpu().numpy()
    assert np.array_equal(_bits(kl[:n]), _bits(want[:n])) and (kl[n:] == -1.0).all()  # (the games that fit are a prefix)
    games = _packed_views(blk, h)["game"].cpu().numpy()
    full = eng.examples()
    assert np.array_equal(games, full.game[:n]) and np.array_equal(_bits(kl[:n]), _bits(full.kl[:n]))


# ---------------------------------------------------------------- the resampler
def _rows(n, seed):
    g = np.random.default_rng(seed)
    kl = (g.exponential(0.3, n) * (g.random(n) < 0.8)).astype(np.float32)
    if n >= 63:
        kl[[3, 17, 40]] = [np.nan, -2.0, 900.0]  # cleaned: 0, 0, 128
    return (kl, g.integers(0, 2 ** 40, n), g.integers(0, 64, n).astype(np.int32), g.integers(0, 2 ** 63, n).astype(np.uint64),
            g.integers(0, 2 ** 63, n).astype(np.uint64))


GUARD = 16


def _resample(rows, u, seed, idx_cap):
    """bz_surprise_resample on device copies of the rows: (count, idx buffer with GUARD words behind idx_cap, n_out, header)"""
    kl, game, ply, own, opp = rows
    n = len(kl)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    d = [t(kl), t(np.asarray(game, np.int64)), t(ply), t(own.view(np.int64)), t(opp.view(np.int64))]
    L = _lib.lib()
    wb = L.bz_surprise_resample_workspace_bytes(n)
    ws = torch.empty(wb + 256, dtype=torch.uint8, device=DEV)
    pad = (-ws.data_ptr()) & 255
    count = torch.full((n + GUARD,), -7, dtype=torch.int32, device=DEV)
    idx = torch.full((idx_cap + GUARD,), -7, dtype=torch.int64, device=DEV)
    n_out = torch.full((1 + GUARD,), -7, dtype=torch.int64, device=DEV)
    _lib.check(L.bz_surprise_resample(*(x.data_ptr() for x in d), n, u, seed, ws.data_ptr() + pad, wb, count.data_ptr(),
                                      idx.data_ptr(), idx_cap, n_out.data_ptr(), torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    head = ws[pad:pad + 24].view(torch.int64).cpu().numpy()
    return count.cpu().numpy(), idx.cpu().numpy(), n_out.cpu().numpy(), head


# 1025: the smallest size with two workgroups (a block holds 1024 rows); 2^20 + 1: the smallest whose block sums need a second
# pass of the one-workgroup scan
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025, (1 << 20) + 1])
def test_resampler_equals_the_numpy_twin(n):
    rows = _rows(n, n)
    want_c, want_i, total, _, _ = resample_twin(*rows, 0.5, 99)
    cap = total + 5
    c, i, no, head = _resample(rows, 0.5, 99, cap)
    assert np.array_equal(c[:n], want_c) and (c[n:] == -7).all()
    assert no[0] == total == head[1] and head[2] == 0 and (no[1:] == -7).all()
    assert np.array_equal(i[:total], want_i) and (i[total:] == -7).all()
    c2, i2, no2, head2 = _resample(rows, 0.5, 99, cap)  # run to run: the same bits
    assert np.array_equal(c, c2) and np.array_equal(i, i2) and np.array_equal(no, no2) and np.array_equal(head, head2)
    _, i, no, _ = _resample(rows, 1.0, 99, n)  # uniform_frac = 1: every row once
    assert no[0] == n and np.array_equal(i[:n], np.arange(n)) and (i[n:] == -7).all()
    zero = (np.zeros(n, np.float32),) + rows[1:]
    _, i, no, _ = _resample(zero, 0.5, 99, n)  # nothing surprising anywhere: every row once
    assert no[0] == n and np.array_equal(i[:n], np.arange(n))
    if total > 0:  # one entry short: one dropped entry, nothing written behind the end
        c, i, no, head = _resample(rows, 0.5, 99, total - 1)
        assert head[1] == total and head[2] == 1 and no[0] == total - 1
        assert np.array_equal(i[:total - 1], want_i[:total - 1]) and (i[total - 1:] == -7).all() and np.array_equal(c[:n], want_c)


def test_surprise_resample_on_device_examples_and_its_capacity_error():
    from betazero_amd.engine import DeviceExamples, Examples
    from betazero_amd.surprise import surprise_resample
    n = 3000
    kl, game, ply, own, opp = _rows(n, 5)
    ex = DeviceExamples.from_host(Examples(own, opp, np.zeros((n, 9), np.float32), np.zeros(n, np.int8), np.ones(n, np.int8),
                                           np.zeros(n, np.uint8), game, ply, 3, kl))
    want_c, want_i, total, _, _ = resample_twin(kl, game, ply, own, opp, 0.25, 7)
    res, counts = surprise_resample(ex, 0.25, seed=7, return_counts=True)
    assert res.is_cuda and res.dtype == torch.int64 and np.array_equal(res.cpu().numpy(), want_i) and np.array_equal(counts.cpu().numpy(), want_c)
    assert abs(len(res) / n - 1.0) < 0.1
    perm = np.random.default_rng(0).permutation(n)  # a row's count does not depend on where it stands in the window
    px = DeviceExamples.from_host(Examples(own[perm], opp[perm], np.zeros((n, 9), np.float32), np.zeros(n, np.int8), np.ones(n, np.int8),
                                           np.zeros(n, np.uint8), game[perm], ply[perm], 3, kl[perm]))
    assert np.array_equal(surprise_resample(px, 0.25, seed=7, return_counts=True)[1].cpu().numpy(), want_c[perm])
    with pytest.raises(RuntimeError, match="did not fit"):
        surprise_resample(ex, 0.25, seed=7, capacity=total - 1)
    assert len(surprise_resample(ex, 0.25, seed=7, capacity=total)) == total


# ---------------------------------------------------------------- augmentation and the training seam
def test_augmented_rows_keep_their_source_rows_kl():
    from betazero_amd.augment import augment_examples
    eng = _engine("reversi", 8, 16, surprise=True, temp_moves=6, openings=1, seed=2, **NOISE)
    _run(eng)
    ex = eng.device_examples()
    aug = augment_examples(ex, dedupe=True)
    assert len(ex) < len(aug) <= 8 * len(ex)
    src = {(int(g), int(p)): k for g, p, k in zip(ex.game.cpu().numpy(), ex.ply.cpu().numpy(), _bits(ex.kl.cpu().numpy()))}
    got = aug.cpu()
    assert all(src[(int(g), int(p))] == k for g, p, k in zip(got.game, got.ply, _bits(got.kl)))
    raw = augment_examples(ex, dedupe=False)
    assert np.array_equal(_bits(raw.kl.cpu().numpy()), np.repeat(_bits(ex.kl.cpu().numpy()), 8))


def test_one_graphed_train_step_on_resampled_indices_leaves_the_error_word_zero():
    from betazero_amd.net import PolicyValueNet
    from betazero_amd.surprise import surprise_resample
    from betazero_amd.train import GraphedTrainStep
    eng = _engine("reversi", 16, 16, surprise=True, temp_moves=6, openings=1, seed=2, **NOISE)
    _run(eng)
    data = eng.device_examples()
    res = surprise_resample(data, 0.5, seed=1)
    assert int(res.min()) >= 0 and int(res.max()) < len(data)
    torch.manual_seed(0)
    g = GraphedTrainStep(PolicyValueNet(64, 2, 64, fused_tower=True).cuda(), lr=1e-3, batch=128)
    gen = torch.Generator(device=DEV).manual_seed(0)
    loss = g(data, res[torch.randint(0, len(res), (128,), device=DEV, generator=gen)])
    g.check()  # raises on a non-zero error word (an out-of-range row index)
    assert np.isfinite(loss.cpu().numpy()).all()
