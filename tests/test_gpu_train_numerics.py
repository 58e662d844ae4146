"""The conv net's training kernels (csrc/bz_train.hip, csrc/bz_train_ends.hip) against the plain references of
tests/test_train_numerics_cpu.py:
- the tower (forward with saved activations, backward-data, weight gradients, k_train_finish's reduction) bit for bit on
  exact data, at every geometry the launcher picks (C = 64 half / full tile, C = 128 on the 16x16x32 path), 2 to 40 layers,
  weight-gradient slice counts that do and do not divide the batch's stages; the fragment packing's round-to-nearest-even;
- the stem bit for bit; the heads on exact nets within bounds derived from fp32 rounding; a whole StepPlan step chained;
- k_train_adam per element against its documented formula, from t = 1 to t = 10^6;
- non-finite values reaching the loss as torch's do, and bitwise determinism of a whole step."""
import ctypes as ct

import numpy as np
import pytest
import torch

from test_train_numerics_cpu import (B, adam_ref, bf16_rne, dyadic_pi, exact_head_params, exact_tower, heads_ref, lsb,
                                     pow2, stem_ref, stem_wgrad_ref, tower_backward_ref, tower_case_stats, tower_reference,
                                     tower_wgrad_ref)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _lib():
    from betazero_amd import _lib as m
    return m, m.lib(), torch.cuda.current_stream().cuda_stream


def _f64(t):
    return t.detach().to(DEV, torch.float64)


def _eq(got, want, what):
    got, want = _f64(got), _f64(want)
    bad = got != want
    assert not bool(bad.any()), (what, int(bad.sum()), got[bad][:5].tolist(), want[bad][:5].tolist())


def _within(got, ref, what, k=2.0):
    """|kernel - reference| <= k * derived bound, element by element (k = 2 covers the bounds' second-order terms)"""
    got, v, e = _f64(got), ref.v.to(DEV), ref.e.to(DEV)
    bad = (got - v).abs() > k * e
    assert not bool(bad.any()), (what, int(bad.sum()), got[bad][:4].tolist(), v[bad][:4].tolist(), e[bad][:4].tolist())


def _ref_on_gpu(x0, W, b, gy):
    return tower_reference(*(t.to(DEV) for t in (x0, W, b, gy)))


# every launcher geometry: C = 64 with n / 8 < 192 (4 positions per workgroup), C = 64 with n >= 1536 (8 per workgroup),
# C = 128 (16x16x32 path); 2, 12 (the bench shape (128, 12, 1024)), 20 and 40 layers.  Default slice counts
# bz_train_wgrad_splits: (64, 12, 2056) 21 over 514 stages (L S = 252), (128, 12, 1024) 10 over 512, (64, 20, 1528) 12 over 382
TOWERS = [(64, 2, 8), (64, 12, 40), (64, 20, 1528), (64, 2, 1536), (64, 12, 2056), (128, 2, 4), (128, 12, 12), (128, 12, 1024),
          (128, 20, 12), (64, 40, 8), (128, 40, 4)]
SEED = {(64, 40, 8): 7, (128, 40, 4): 5}   # (seeds whose 40-layer towers stay within exact range -- asserted)


@pytest.mark.parametrize("C,L,n", TOWERS)
def test_tower_bitexact_through_tower_apply_and_step_plan(C, L, n):
    """acts[1..L], gs[0..L], dx0, dW, db equal the exact reference bit for bit -- through tower_apply (TowerPlan, torch's sum
    of the slices) and through a StepPlan's buffers with k_train_finish reducing the slices into tower_w.grad / tower_b.grad"""
    from betazero_amd.net import PolicyValueNet
    from betazero_amd.train_kernels import StepPlan, TowerPlan, tower_apply_nhwc
    x0, W, b, gy = exact_tower(C, L, n, SEED.get((C, L, n), 11))
    acts, gs, dW, db = _ref_on_gpu(x0, W, b, gy)
    st = tower_case_stats(acts, W.to(DEV), b.to(DEV))
    assert st["zero"] > 0 and st["ties"] > 0 and st["neg_min"] > 0, st
    xd, Wd, bd, gyd = (t.to(DEV, torch.float32) for t in (x0, W, b, gy))
    plan = TowerPlan(C, L, n)
    xs, Ws, bs = (t.clone().requires_grad_(True) for t in (xd, Wd, bd))
    y = tower_apply_nhwc(xs, Ws, bs, plan)
    y.backward(gyd)
    torch.cuda.synchronize()
    for l in range(1, L + 1):
        _eq(plan.acts[l], acts[l], f"act[{l}]")
    for l in range(L + 1):
        _eq(plan.gs[l], gs[l], f"g[{l}]")
    _eq(xs.grad, gs[0], "dx0")
    _eq(Ws.grad, dW, "dW")
    _eq(bs.grad, db, "db")
    # the same through StepPlan's buffers and k_train_finish
    m, Lb, s = _lib()
    torch.manual_seed(0)
    net = PolicyValueNet(C, L // 2, 64, fused_tower=True).to(DEV)
    with torch.no_grad():
        net.tower_w.copy_(Wd); net.tower_b.copy_(bd)
    sp = StepPlan(net, n)
    sp.acts[0].copy_(xd)
    m.check(Lb.bz_train_pack_weights(net.tower_w.data_ptr(), C, L, sp.wf_fwd.data_ptr(), sp.wf_bwd.data_ptr(), s))
    m.check(Lb.bz_train_tower_fwd(sp.acts[0].data_ptr(), sp.wf_fwd.data_ptr(), net.tower_b.data_ptr(), C, L, n, sp.acts[1].data_ptr(),
                                  sp.masks.data_ptr(), s))
    torch.mul(gyd, sp.acts[L] > 0, out=sp.gs[L])
    m.check(Lb.bz_train_tower_bwd(sp.gs[L].data_ptr(), sp.wf_bwd.data_ptr(), sp.zeros_c.data_ptr(), sp.masks.data_ptr(), C, L, n,
                                  sp.gs[0].data_ptr(), s))
    m.check(Lb.bz_train_wgrad(sp.acts[0].data_ptr(), sp.gs[1].data_ptr(), C, L, n, sp.splits, sp.partial.data_ptr(), sp.db_partial.data_ptr(), s))
    m.check(Lb.bz_train_finish(ct.byref(sp._partials), ct.byref(sp._grads), C, L, sp.VH, n, sp.losses.data_ptr(), None, s))
    torch.cuda.synchronize()
    _eq(sp.acts[L], acts[L], "StepPlan act[L]")
    _eq(sp.gs[0], gs[0], "StepPlan g[0]")
    _eq(net.tower_w.grad, dW, "StepPlan tower_w.grad")
    _eq(net.tower_b.grad, db, "StepPlan tower_b.grad")


@pytest.mark.parametrize("C,L,n", [(64, 12, 40), (128, 6, 12), (64, 2, 1536)])
def test_wgrad_every_slice_count(C, L, n):
    """bz_train_wgrad with 1 slice, slice counts that do not divide the stages (L S not a multiple of 8) and one slice per
    stage: the sum of the slices is the reference's dW / db bit for bit"""
    from betazero_amd.train_kernels import TowerPlan, tower_apply_nhwc
    m, Lb, s = _lib()
    x0, W, b, gy = exact_tower(C, L, n, 12)
    acts, gs, dW, db = _ref_on_gpu(x0, W, b, gy)
    plan = TowerPlan(C, L, n)
    xs = x0.to(DEV, torch.float32).requires_grad_(True)
    tower_apply_nhwc(xs, W.to(DEV, torch.float32), b.to(DEV, torch.float32), plan).backward(gy.to(DEV, torch.float32))
    stages = n // (256 // C)
    for S in sorted({1, 3, 7, stages - 1, stages}):
        if not 1 <= S <= stages:
            continue
        part = torch.full((L, S, 9, C, C), float("nan"), device=DEV)
        dbp = torch.full((L, Lb.bz_train_wgrad_bias_rows(C, S), C), float("nan"), device=DEV)
        m.check(Lb.bz_train_wgrad(plan.acts[0].data_ptr(), plan.gs[1].data_ptr(), C, L, n, S, part.data_ptr(), dbp.data_ptr(), s))
        torch.cuda.synchronize()
        _eq(part.double().sum(1).view(L, 3, 3, C, C).permute(0, 4, 3, 1, 2), dW, f"dW, {S} slices")
        _eq(dbp.double().sum(1), db, f"db, {S} slices")


def test_half_batches_sum_to_the_full_batch_bitexact():
    from betazero_amd.train_kernels import TowerPlan, tower_apply_nhwc
    C, L, n = 64, 4, 48
    x0, W, b, gy = (t.to(DEV, torch.float32) for t in exact_tower(C, L, n, 13))

    def grads(lo, hi):
        Ws = W.clone().requires_grad_(True)
        tower_apply_nhwc(x0[lo:hi].contiguous(), Ws, b, TowerPlan(C, L, hi - lo)).backward(gy[lo:hi].contiguous())
        return Ws.grad
    full, a, c = grads(0, n), grads(0, n // 2), grads(n // 2, n)
    assert float(full.abs().max()) > 0
    _eq(a + c, full, "dW(first half) + dW(second half)")


def _stream_ref(W, C, L, m16):
    """the two fragment streams of k_pack_weights (m16 False) / k_pack_weights16 as documented in csrc/bz_train.hip, as
    int16 bf16 bits of RNE(W) -- [entries, 64 lanes, 8]"""
    Wr = bf16_rne(W.double()).float().bfloat16().view(torch.int16)   # exact: the values are bf16 already
    lane = torch.arange(64)
    if not m16:
        KC, MT = C // 16, C // 32
        r, h = lane % 32, lane // 32
        l, t, kc, mt = torch.meshgrid(torch.arange(L), torch.arange(9), torch.arange(KC), torch.arange(MT), indexing="ij")
        j = torch.arange(8)
        co = (32 * mt[..., None, None] + r[:, None]).expand(*mt.shape, 64, 8)
        ci = (16 * kc[..., None, None] + 8 * h[:, None] + j).expand(*mt.shape, 64, 8)
    else:
        KQ, MT = C // 32, C // 32
        c, g = lane % 16, lane // 16
        l, t, kc, mt, a = torch.meshgrid(torch.arange(L), torch.arange(9), torch.arange(KQ), torch.arange(MT), torch.arange(2), indexing="ij")
        j = torch.arange(8)
        co = (32 * mt[..., None, None] + 16 * a[..., None, None] + c[:, None]).expand(*mt.shape, 64, 8)
        ci = (32 * kc[..., None, None] + 8 * g[:, None] + j).expand(*mt.shape, 64, 8)
    ll, tt = l[..., None, None].expand_as(co), t[..., None, None].expand_as(co)
    fwd = Wr.view(L, C, C, 9)[ll, co, ci, tt].reshape(-1, 64, 8)
    # backward: slot of layer L-1-l, tap t holds W[l][co = k][ci = m][8 - t] with (m, k) the forward's (co, ci)
    bwd_src = Wr.view(L, C, C, 9)[ll, ci, co, 8 - tt]
    bwd = torch.empty_like(bwd_src)
    bwd[L - 1 - torch.arange(L)] = bwd_src
    return fwd, bwd.reshape(-1, 64, 8)


@pytest.mark.parametrize("C", [64, 128])
def test_pack_weights_round_to_nearest_even(C):
    """weights off the bf16 grid -- exact ties (both parities), just above / below a tie, random -- packed into both fragment
    streams: every fragment entry is RNE of its weight (k_pack_weights at 64 channels, k_pack_weights16 at 128)"""
    m, Lb, s = _lib()
    L = 4
    g = torch.Generator().manual_seed(C)
    base = (torch.randn(L, C, C, 3, 3, generator=g) * 0.5).bfloat16().float()
    ulp = pow2(torch.frexp(base)[1] - 8).float()
    kind = torch.randint(0, 5, base.shape, generator=g)
    off = torch.stack([0.5 * ulp, 0.5 * ulp * (1 + 2 ** -10), 0.5 * ulp * (1 - 2 ** -10), torch.rand(base.shape, generator=g) * ulp, -0.5 * ulp])
    W = (base + off.gather(0, kind[None]).squeeze(0)).float()
    assert int((kind == 0).sum()) > 1000
    Wd = W.to(DEV)
    nb = Lb.bz_train_wf_bytes(C, L)
    wf, wb = torch.zeros(nb, dtype=torch.uint8, device=DEV), torch.zeros(nb, dtype=torch.uint8, device=DEV)
    m.check(Lb.bz_train_pack_weights(Wd.data_ptr(), C, L, wf.data_ptr(), wb.data_ptr(), s))
    torch.cuda.synchronize()
    fwd, bwd = _stream_ref(W, C, L, C == 128)
    k = fwd.numel() * 2
    got_f = wf[:k].cpu().view(torch.int16).view(-1, 64, 8)
    got_b = wb[:k].cpu().view(torch.int16).view(-1, 64, 8)
    assert torch.equal(got_f, fwd) and torch.equal(got_b, bwd)
    assert not bool(wf[k:].any()) and not bool(wb[k:].any())   # the padding behind the streams stays zero


# ---------------------------------------------------------------- the ends
def _boards(n, seed):
    rng = np.random.default_rng(seed)
    own = rng.integers(0, 2 ** 63, n, dtype=np.int64).astype(np.uint64) | (rng.integers(0, 2, n).astype(np.uint64) << np.uint64(63))
    opp = (rng.integers(0, 2 ** 63, n, dtype=np.int64).astype(np.uint64) | (rng.integers(0, 2, n).astype(np.uint64) << np.uint64(63))) & ~own
    own[0], opp[0] = np.uint64(0), np.uint64(0)
    own[1], opp[1] = np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0)
    own[2], opp[2] = np.uint64(0x8181818181818181), np.uint64(0x7E000000000000FF) & ~np.uint64(0x8181818181818181)  # the edges
    return own, opp


def _net(C, NB, VH, P=None, stem=None, tower=None):
    from betazero_amd.net import PolicyValueNet
    torch.manual_seed(1)
    net = PolicyValueNet(C, NB, VH, fused_tower=True).to(DEV)
    with torch.no_grad():
        if P is not None:
            for k, v in P.items():
                mod, what = {"pol": net.pol, "val": net.val, "polfc": net.polfc, "v1": net.v1, "v2": net.v2}[k[:-2]], k[-1]
                (mod.weight if what == "w" else mod.bias).copy_(v.reshape((mod.weight if what == "w" else mod.bias).shape))
        if stem is not None:
            net.stem.weight.copy_(stem[0]); net.stem.bias.copy_(stem[1])
        if tower is not None:
            net.tower_w.copy_(tower[0]); net.tower_b.copy_(tower[1])
    return net


def _batch(own, opp, pi, z):
    t = lambda a: torch.as_tensor(a).to(DEV)  # noqa: E731
    return t(own.view(np.int64)), t(opp.view(np.int64)), pi.to(DEV, torch.float32).contiguous(), t(z.numpy().astype(np.int8))


@pytest.mark.parametrize("C,n", [(64, 8), (128, 1032)])
def test_stem_forward_and_weight_gradient_bitexact(C, n):
    """0/1 planes and dyadic stem weights: act[0] is RNE of the exact pre-activation's ReLU, bit for bit (sums past 8 bits:
    bf16 rounds, ties included); the weight / bias gradient from a given dyadic g[0] bit for bit.  Boards with stones on
    every edge cell: a tap that wrapped round the board instead of reading the zero padding would show."""
    m, Lb, s = _lib()
    g = torch.Generator().manual_seed(C + n)
    w = torch.randint(-600, 601, (C, 2, 3, 3), generator=g).double() * 2.0 ** -5
    b = torch.randint(-300, 301, (C,), generator=g).double() * 2.0 ** -5
    own, opp = _boards(n, C)
    net = _net(C, 1, 64, stem=(w.float(), b.float()))
    from betazero_amd.train_kernels import StepPlan
    sp = StepPlan(net, n)
    pi, z = dyadic_pi(n, 1), torch.zeros(n)
    sp.set_batch(*_batch(own, opp, pi, z))
    m.check(Lb.bz_train_stem_fwd(sp.batch_desc.data_ptr(), n, net.stem.weight.data_ptr(), net.stem.bias.data_ptr(), C, sp.acts[0].data_ptr(), s))
    want = stem_ref(own, opp, w, b)
    torch.cuda.synchronize()
    _eq(sp.acts[0], want, "act[0]")
    pre = (want != 0)
    assert bool(pre.any()) and bool((~pre).any())
    g0 = (torch.randint(-64, 65, (n, 64, C), generator=g) * (torch.rand(n, 64, C, generator=g) < 0.5)).double() * 2.0 ** -3
    sp.gs[0].copy_(g0.to(DEV))
    m.check(Lb.bz_train_stem_wgrad(sp.batch_desc.data_ptr(), sp.acts[0].data_ptr(), sp.gs[0].data_ptr(), n, C, sp.stem_partial.data_ptr(), s))
    m.check(Lb.bz_train_finish(ct.byref(sp._partials), ct.byref(sp._grads), C, sp.L, sp.VH, n, sp.losses.data_ptr(), None, s))
    dw, db, tw, tb = stem_wgrad_ref(own, opp, want, g0)
    assert float(tw.max()) < 2 ** 24 * 2 ** -3 and float(tb.max()) < 2 ** 24 * 2 ** -3   # exact in fp32 in any order
    torch.cuda.synchronize()
    _eq(net.stem.weight.grad, dw.view(C, 2, 3, 3), "stem.weight.grad")
    _eq(net.stem.bias.grad, db, "stem.bias.grad")


def _heads_case(C, n, VH, seed, saturate=False):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randint(0, 13, (n, 64, C), generator=g) * (torch.rand(n, 64, C, generator=g) < 0.6)).double()
    P = exact_head_params(C, VH, seed, saturate)
    pi, z = dyadic_pi(n, seed), torch.randint(-1, 2, (n,), generator=g).double()
    return x, P, pi, z


def _run_heads(net, sp, x, n, C, VH):
    m, Lb, s = _lib()
    Ly = sp.L
    sp.acts[Ly].copy_(x.to(DEV))
    m.check(Lb.bz_train_heads(sp.acts[Ly].data_ptr(), sp.batch_desc.data_ptr(), n, C, VH, ct.byref(sp._head), sp.gs[Ly].data_ptr(),
                              sp.hv.data_ptr(), sp.dl.data_ptr(), sp.dv1.data_ptr(), sp.heads_partial.data_ptr(), s))
    m.check(Lb.bz_train_heads_wgrad(sp.hv.data_ptr(), sp.dl.data_ptr(), sp.dv1.data_ptr(), n, VH, sp.heads_w_partial.data_ptr(), s))
    m.check(Lb.bz_train_finish(ct.byref(sp._partials), ct.byref(sp._grads), C, Ly, VH, n, sp.losses.data_ptr(), None, s))
    torch.cuda.synchronize()


HEAD_GRADS = {"pol_w": ("pol", "weight"), "pol_b": ("pol", "bias"), "val_w": ("val", "weight"), "val_b": ("val", "bias"),
              "polfc_w": ("polfc", "weight"), "polfc_b": ("polfc", "bias"), "v1_w": ("v1", "weight"), "v1_b": ("v1", "bias"),
              "v2_w": ("v2", "weight"), "v2_b": ("v2", "bias")}


def _check_heads(net, sp, r, what=""):
    for i, k in enumerate(("loss", "ce", "mse")):
        _within(sp.losses[i:i + 1], B(r[k].v.reshape(1), r[k].e.reshape(1)), what + k)
    for k, (mod, p) in HEAD_GRADS.items():
        _within(getattr(getattr(net, mod), p).grad, r[k], what + k)
    # g[L]: RNE of the fp32 value, which lies within the bound of the reference -> any bf16 between RNE(v - 2e) and RNE(v + 2e)
    g = _f64(sp.gs[sp.L])
    v, e = r["g_top"].v.to(DEV), r["g_top"].e.to(DEV)
    lo, hi = bf16_rne(v - 2 * e), bf16_rne(v + 2 * e)
    bad = (g < lo) | (g > hi)
    assert not bool(bad.any()), (what + "g[L]", int(bad.sum()), g[bad][:4].tolist(), v[bad][:4].tolist())
    return int((lo != hi).sum())


@pytest.mark.parametrize("C,n,VH", [(64, 8, 64), (128, 20, 64), (64, 1032, 24), (128, 1024, 64)])
def test_heads_on_exact_nets_within_derived_bounds(C, n, VH):
    """exact 1x1 convolutions and FC pre-activations (asserted): the losses, all ten head gradients and g[L] against the fp64
    reference, per element within the bound that fp32 rounding of the kernel's operations allows (exp / log / tanh 2 ulps);
    g[L] is RNE of its fp32 value -- it may differ from RNE of the fp64 value only where that lies within its bound of a
    rounding boundary"""
    from betazero_amd.train_kernels import StepPlan
    x, P, pi, z = _heads_case(C, n, VH, 31 + n)
    net = _net(C, 1, VH, P=P)
    sp = StepPlan(net, n)
    own, opp = _boards(n, 1)
    sp.set_batch(*_batch(own, opp, pi, z))
    _run_heads(net, sp, x, n, C, VH)
    r = heads_ref(x.to(DEV), {k: v.to(DEV) for k, v in P.items()}, pi.to(DEV), z.to(DEV))
    ambiguous = _check_heads(net, sp, r)
    assert ambiguous < 0.01 * x.numel() and float((sp.gs[sp.L] != 0).float().mean()) > 0.05
    assert bool((r["h"] == 0).any()) and bool((r["h"] > 0).any()) and bool((r["t"] < 0).any())   # ReLUs cut in both heads


@pytest.mark.parametrize("C,NB,n", [(64, 2, 64), (128, 6, 1024)])
def test_whole_step_chained_bitexact(C, NB, n):
    """StepPlan.grads on an exact net whose heads saturate (one policy logit 256 above the rest: soft-max, CE and d logit
    exact; v2 = 0): the heads' outputs within their bounds (which are 0 where exact), and the kernel's own g[L] fed into the
    reference backward -- the tower's and the stem's gradients of the whole step bit for bit"""
    from betazero_amd.train_kernels import StepPlan
    L = 2 * NB
    g = torch.Generator().manual_seed(n)
    sw = torch.randint(-2, 3, (C, 2, 3, 3), generator=g).double() * (torch.rand(C, 2, 3, 3, generator=g) < 0.4)
    sb = torch.randint(-1, 3, (C,), generator=g).double()
    _, W, b, _ = exact_tower(C, L, 4, 40 + L)
    P = exact_head_params(C, 64, 7, saturate=True)
    own, opp = _boards(n, 2)
    pi, z = dyadic_pi(n, 5, bits=4), torch.randint(-1, 2, (n,), generator=g).double()
    net = _net(C, NB, 64, P=P, stem=(sw.float(), sb.float()), tower=(W.float(), b.float()))
    sp = StepPlan(net, n)
    sp.grads(*_batch(own, opp, pi, z))
    torch.cuda.synchronize()
    act0 = stem_ref(own, opp, sw, sb).to(DEV)
    _eq(sp.acts[0], act0, "act[0]")
    acts = tower_reference(act0, W.to(DEV), b.to(DEV), torch.zeros_like(act0))[0]
    for l in range(1, L + 1):
        _eq(sp.acts[l], acts[l], f"act[{l}]")
    r = heads_ref(acts[L], {k: v.to(DEV) for k, v in P.items()}, pi.to(DEV), z.to(DEV))
    assert float(r["s"].max(1).values.sub(r["s"].topk(2, 1).values[:, 1]).min()) >= 128   # saturated
    _check_heads(net, sp, r)
    gL = _f64(sp.gs[L])
    unit = lsb(gL)
    assert unit > 0 and float(gL.abs().max()) > 0
    gs = tower_backward_ref(acts, W.to(DEV), gL, unit)
    dW, db = tower_wgrad_ref(acts, gs, unit)
    for l in range(L):
        _eq(sp.gs[l], gs[l], f"g[{l}]")
    _eq(net.tower_w.grad, dW, "tower_w.grad")
    _eq(net.tower_b.grad, db, "tower_b.grad")
    dw, dbs, tw, tb = stem_wgrad_ref(own, opp, act0.cpu(), gs[0].cpu())
    assert float(tw.max()) < 2 ** 24 * unit and float(tb.max()) < 2 ** 24 * unit
    _eq(net.stem.weight.grad, dw.view(C, 2, 3, 3), "stem.weight.grad")
    _eq(net.stem.bias.grad, dbs, "stem.bias.grad")


# ---------------------------------------------------------------- Adam
@pytest.mark.parametrize("case", ["t1", "warmup", "t1e4", "t1e6"])
def test_adam_kernel_per_element(case):
    """k_train_adam against an fp64 evaluation of its documented formula (float32 betas, 1 - powf(beta, t) in fp32,
    p -= (lr_t / bc1) m / (sqrt(v) bc2_rsqrt + eps)) from the kernel's own gradient and pre-step (p, m, v), per element within
    the bound derived from the fp32 operations: t = 1, the warm-up boundary (t = warm-up steps), and t = 10^4, 10^6 (powf
    underflows: both corrections become 1)"""
    from betazero_amd.train_kernels import StepPlan
    n = 64
    lr, b1, b2, eps, warm, done = {"t1": (3e-3, 0.9, 0.999, 1e-8, 0, 0), "warmup": (1e-3, 0.8, 0.95, 1e-3, 5, 4),
                                   "t1e4": (1e-3, 0.9, 0.999, 1e-8, 0, 9999), "t1e6": (1e-3, 0.9, 0.999, 1e-8, 100, 999999)}[case]
    net = _net(64, 1, 64)
    sp = StepPlan(net, n)
    own, opp = _boards(n, 3)
    sp.set_batch(*_batch(own, opp, dyadic_pi(n, 3), torch.randint(-1, 2, (n,)).double()))
    sp.enable_adam(lr, betas=(b1, b2), eps=eps, warmup_steps=warm)
    sp.reset_adam(steps_done=done)
    g = torch.Generator(device=DEV).manual_seed(9)
    with torch.no_grad():   # moments from earlier steps (v >= 0), some exact zeros
        for k in sp.NAMES:
            sp.adam_m[k].copy_(torch.randn(sp.adam_m[k].shape, device=DEV, generator=g) * 1e-3)
            sp.adam_v[k].copy_(torch.rand(sp.adam_v[k].shape, device=DEV, generator=g) ** 2 * 1e-6)
    p0 = {k: t.detach().clone() for k, t in sp.params.items()}
    m0 = {k: t.clone() for k, t in sp.adam_m.items()}
    v0 = {k: t.clone() for k, t in sp.adam_v.items()}
    sp.step()
    torch.cuda.synchronize()
    assert sp.adam_t == done + 1
    moved = 0
    for k, p in sp.params.items():
        r = adam_ref(p0[k].cpu(), m0[k].cpu(), v0[k].cpu(), p.grad.cpu(), lr, b1, b2, eps, done + 1, warm)
        _within(sp.adam_m[k], r["m"], f"m {k}")
        _within(sp.adam_v[k], r["v"], f"v {k}")
        _within(p, r["p"], f"p {k}")
        moved += int((p != p0[k]).sum())
    assert moved > 0


# ---------------------------------------------------------------- non-finite values, determinism
@pytest.mark.parametrize("where", ["tower_w", "tower_b", "pol_w", "v1_w"])
@pytest.mark.parametrize("bad", ["nan", "-nan", "inf", "-inf"])
def test_nonfinite_parameter_gives_nonfinite_loss(where, bad):
    """a NaN of either sign or an infinity in a tower weight / bias, pol.weight or v1.weight: wherever torch's fp32
    PolicyValueNet gives a non-finite loss, StepPlan.grads does too (before the fix the heads' fmaxf ReLU turned such NaNs
    into 0 and the loss came out finite)"""
    import torch.nn.functional as F
    from betazero_amd.net import PolicyValueNet
    from betazero_amd.train import planes_from_bits
    from betazero_amd.train_kernels import StepPlan
    bits = {"nan": 0x7FC00000, "-nan": -0x00400000, "inf": 0x7F800000, "-inf": -0x00800000}[bad]   # (-nan: 0xFFC00000)
    n = 16
    torch.manual_seed(4)
    net = PolicyValueNet(64, 1, 64, fused_tower=True).to(DEV)
    with torch.no_grad():
        t = {"tower_w": net.tower_w, "tower_b": net.tower_b, "pol_w": net.pol.weight, "v1_w": net.v1.weight}[where]
        t.view(-1)[37:38].view(torch.int32).fill_(bits)
    own, opp = _boards(n, 6)
    own_t, opp_t, pi, z = _batch(own, opp, dyadic_pi(n, 6), torch.randint(-1, 2, (n,)).double())
    sp = StepPlan(net, n)
    losses = sp.grads(own_t, opp_t, pi, z).clone()
    logits, v = net(planes_from_bits(own_t, opp_t))
    ref = -(pi * F.log_softmax(logits, dim=1)).sum(1).mean() + F.mse_loss(v, z.float())
    torch.cuda.synchronize()
    if not bool(torch.isfinite(ref)):
        assert not bool(torch.isfinite(losses[0])), (where, bad, float(ref), losses.tolist())
    if where != "tower_b":   # (37 = a weight that meets non-zero inputs: torch's loss is not finite here)
        assert not bool(torch.isfinite(ref))


def test_step_is_deterministic_at_the_bench_shape():
    """from the same parameters, moments and step count, two StepPlan.step() calls at (128 channels, 6 blocks, batch 1024) give
    the same bits in the losses, every gradient, m, v and p"""
    from betazero_amd.net import PolicyValueNet
    from betazero_amd.train_kernels import StepPlan
    n = 1024
    torch.manual_seed(8)
    net = PolicyValueNet(128, 6, 64, fused_tower=True).to(DEV)
    sp = StepPlan(net, n)
    own, opp = _boards(n, 8)
    rng = np.random.default_rng(8)
    pi = torch.from_numpy(rng.random((n, 65))).float()
    pi /= pi.sum(1, keepdim=True)
    sp.set_batch(*_batch(own, opp, pi, torch.from_numpy(rng.integers(-1, 2, n)).double()))
    sp.enable_adam(1e-3, warmup_steps=10)
    sp.step()                                # a first step: non-zero moments
    snap = lambda: ({k: p.detach().clone() for k, p in sp.params.items()}, {k: t.clone() for k, t in sp.adam_m.items()},  # noqa: E731
                    {k: t.clone() for k, t in sp.adam_v.items()}, sp.hyper.clone())
    p0, m0, v0, h0 = snap()
    runs = []
    for _ in range(2):
        with torch.no_grad():
            for k in sp.NAMES:
                sp.params[k].copy_(p0[k]); sp.adam_m[k].copy_(m0[k]); sp.adam_v[k].copy_(v0[k])
            sp.hyper.copy_(h0)
        losses = sp.step().clone()
        torch.cuda.synchronize()
        runs.append((losses, {k: p.grad.clone() for k, p in sp.params.items()}) + snap())
    a, b = runs
    bits = lambda t: t.contiguous().view(torch.int32)  # noqa: E731
    assert torch.equal(bits(a[0]), bits(b[0]))
    for i in (1, 2, 3, 4):
        for k in sp.NAMES:
            assert torch.equal(bits(a[i][k]), bits(b[i][k])), (i, k)
    assert bool(torch.isfinite(a[0][:3]).all())
