"""The ownership head's training kernels (k_train_heads_own, k_train_heads_own_vt, k_train_own_finish of csrc/bz_train_ends.hip;
DESIGN.md 12.2) against the references of tests/test_train_numerics_cpu.py (heads_ref(own=...), adam_ref) and
tests/test_train_optim_cpu.py (optim_ref), on the cases of tests/test_train_own_numerics_cpu.py:
- the head kernels per element within bounds derived from fp32 rounding, own_weight = 0 against k_train_heads bit for bit, a flat
  plane (o = 0) bit for bit;
- k_train_own_finish alone: its reduction bit for bit at 1, 2, 7, 8, 9 and 256 partial vectors, its Adam per element from t = 1
  to t = 10^6 under the plain and under the extended optimiser;
- the head together with the extended optimiser (12.1): a whole step per element, own_weight = 0 against a plan without the
  head, the captured graph against the eager step, the skip rule across the two optimisers, non-finite head parameters;
- a whole step with the head on, on the tower's own act[L].
Every tolerance is a derived bound with the project's factor 2 (_within), bit equality, or "non-finite where torch's is"."""
import copy
import ctypes as ct
import dataclasses

import numpy as np
import pytest
import torch

from test_gpu_train_numerics import DEV, HEAD_GRADS, _batch, _boards, _eq, _f64, _net, _within
from test_gpu_train_optim import _bits, _check_step, _grads, _same, _snap
from test_gpu_train_optim import _within as _within_cpu
from test_gpu_train_ownership import _examples, _run_heads
from test_train_numerics_cpu import (adam_ref, bf16_rne, dyadic_pi, exact_head_params, exact_own_params, exact_tower, heads_ref,
                                     stem_ref, tower_reference)
from test_train_optim_cpu import NAMES, f32, norm_ref
from test_train_own_numerics_cpu import AMBIGUOUS_CAP, SHAPES, WEIGHTS, B, own_case, own_ref, target_boards

pytestmark = pytest.mark.gpu
_SETUPS, _REFS = {}, {}


def _lib():
    from betazero_amd import _lib as m
    return m, m.lib(), torch.cuda.current_stream().cuda_stream


def _head(C, ow, ob):
    from betazero_amd.net import OwnershipHead
    head = OwnershipHead(C).to(DEV)
    with torch.no_grad():
        head.conv.weight.copy_(ow.reshape(1, C, 1, 1)); head.conv.bias.copy_(ob.reshape(1))
    return head


def _setup(C, n, VH, vt, flat=False):
    """own_case's data on an exact net with the head, and a StepPlan of the case's rows pointed at it (one per case for the
    whole module; own_weight is set per test through plan._own.weight, which every launch reads)"""
    from betazero_amd.train_kernels import StepPlan
    key = (C, n, VH, vt, flat)
    if key not in _SETUPS:
        case = own_case(C, n, VH, flat)
        rows = case["x"].shape[0]
        net, head = _net(C, 1, VH, P=case["P"]), _head(C, case["ow"], case["ob"])
        plan = StepPlan(net, rows, value_targets=vt, ownership=head)
        own, opp = _boards(rows, 1)
        plan.set_batch(*_batch(own, opp, case["pi"], case["z"]), vt=case["vt"].to(DEV, torch.float32).contiguous() if vt else None,
                       fown=case["fown"].to(DEV), fopp=case["fopp"].to(DEV))
        _SETUPS[key] = (case, net, plan)
    return _SETUPS[key]


def _ref(C, n, VH, vt, w, head=True, flat=False):
    """the reference of a case, computed once (float64 on the device) and shared"""
    key = (C, n, VH, vt, w if head else None, flat)
    if key not in _REFS:
        _REFS[key] = own_ref(own_case(C, n, VH, flat), vt, w, device=DEV, head=head)
    return _REFS[key]


def _run(plan, net, case, w, own=True):
    plan._own.weight = w
    out = _run_heads(plan, net, case["x"][:case["n"]], own=own, n=case["n"])
    torch.cuda.synchronize()
    return out


def _interval(r):
    v, e = r["g_top"].v, r["g_top"].e
    return bf16_rne(v - 2 * e), bf16_rne(v + 2 * e)


def _check_own(r, got, what=""):
    """_check_heads on the first n rows, extended by d ow, d ob, L_own and the four-term loss; returns the ambiguous g[L] count"""
    losses, grads, g_top, l_own, (d_ow, d_ob) = got
    one = lambda b: B(b.v.reshape(1), b.e.reshape(1))  # noqa: E731
    for i, k in enumerate(("loss", "ce", "mse")):
        _within(losses[i:i + 1], one(r[k]), what + k)
    _within(l_own, one(r["l_own"]), what + "l_own")
    for k in HEAD_GRADS:
        _within(grads[k], r[k], what + k)
    _within(d_ow, r["own_w"], what + "d ow")
    _within(d_ob, r["own_b"], what + "d ob")
    g = _f64(g_top)
    lo, hi = _interval(r)
    bad = (g < lo) | (g > hi)
    assert not bool(bad.any()), (what + "g[L]", int(bad.sum()), g[bad][:4].tolist(), r["g_top"].v[bad][:4].tolist())
    return int((lo != hi).sum())


# ---------------------------------------------------------------- 2. the head kernels
@pytest.mark.parametrize("own_weight", WEIGHTS)
@pytest.mark.parametrize("value_targets", [False, True])
@pytest.mark.parametrize("C,n,VH", SHAPES)
def test_own_heads_within_derived_bounds(C, n, VH, value_targets, own_weight):
    """the four losses, the ten head gradients, d ow, d ob and g[L] against heads_ref(own=...), per element within the bounds of
    the kernel's fp32 operations; the head's term is visible in g[L]: the kernel's value lies outside the interval of the
    reference WITHOUT the head on a share of the cells"""
    case, net, plan = _setup(C, n, VH, value_targets)
    got = _run(plan, net, case, own_weight)
    r, r0 = _ref(C, n, VH, value_targets, own_weight), _ref(C, n, VH, value_targets, own_weight, head=False)
    ambiguous = _check_own(r, got)
    g, x = _f64(got[2]), case["x"][:n].to(DEV)
    lo0, hi0 = _interval(r0)
    moved = float((((g < lo0) | (g > hi0)) & (x > 0)).double().sum() / (x > 0).double().sum())
    print(f"ambiguous g[L] cells {ambiguous} of {x.numel()}; the head's term moved g[L] on {moved:.3f} of the cells with x > 0")
    assert ambiguous < AMBIGUOUS_CAP * x.numel() and float((g != 0).double().mean()) > 0.05 and moved > 0
    assert float(got[4][0].abs().max()) > 0 and float(got[0][3]) == 0.0


@pytest.mark.parametrize("value_targets", [False, True])
@pytest.mark.parametrize("C,n,VH", SHAPES)
def test_own_weight_zero_is_the_plain_heads_kernel_bit_for_bit(C, n, VH, value_targets):
    """own_weight = 0 on the same data: the ten gradients, the three losses and g[L] carry the bits k_train_heads /
    k_train_heads_vt give; d ow and d ob are exactly 0; L_own is still reported, within its bound"""
    case, net, plan = _setup(C, n, VH, value_targets)
    l0, g0, top0, _, _ = _run(plan, net, case, 0.0, own=False)
    l1, g1, top1, l_own, (d_ow, d_ob) = _run(plan, net, case, 0.0, own=True)
    assert torch.equal(_bits(l0[:3]), _bits(l1[:3])) and torch.equal(_bits(top0.float()), _bits(top1.float())) and float(top0.abs().max()) > 0
    assert set(g0) == set(g1) and len(g0) == 10 and all(torch.equal(_bits(g0[k]), _bits(g1[k])) for k in g0)
    assert not bool(d_ow.any()) and not bool(d_ob.any())
    r = _ref(C, n, VH, value_targets, 1.0)
    _within(l_own, B(r["l_own"].v.reshape(1), r["l_own"].e.reshape(1)), "l_own")
    assert float(l_own) > 0.1


@pytest.mark.parametrize("value_targets", [False, True])
@pytest.mark.parametrize("C,n", [(64, 8), (128, 1024)])
def test_a_flat_plane_is_bit_exact(C, n, value_targets):
    """ow = 0, ob = 0, n and own_weight powers of two: o = 0, and d ow, d ob and L_own are exact dyadic sums (the reference
    asserts Sigma |terms| < 2^24 units by giving them a bound of 0) -- bit for bit, whatever the order of summation"""
    case, net, plan = _setup(C, n, 64, value_targets, flat=True)
    got = _run(plan, net, case, 0.5)
    r = _ref(C, n, 64, value_targets, 0.5, flat=True)
    for k in ("own_w", "own_b", "l_own"):
        assert float(r[k].e.abs().max()) == 0.0, k
    assert float(r["own_w"].v.abs().max()) > 0 and float(r["own_b"].v.abs()) > 0
    _eq(got[4][0], r["own_w"].v, "d ow")
    _eq(got[4][1], r["own_b"].v.reshape(1), "d ob")
    _eq(got[3], r["l_own"].v.reshape(1), "L_own")
    _check_own(r, got)


# ---------------------------------------------------------------- 3. k_train_own_finish alone
@pytest.mark.parametrize("C", [64, 128])
def test_own_finish_reduction_bit_for_bit_at_every_tail(C):
    """dyadic partial vectors whose sums are exact in any order, at n = 4, 8, 28, 32, 36, 1032 -- 1, 2, 7, 8, 9 and 256 vectors:
    strided_sum's eight-at-a-time body and its tail --: grad_w, grad_b, own_loss[0] and losses[0] + w L_own bit for bit; the rows
    behind the last vector hold NaN and are never read"""
    m, Lb, s = _lib()
    w = 0.7
    g = torch.Generator().manual_seed(C)
    keep = torch.zeros(4, dtype=torch.float32, device=DEV)   # (never dereferenced by this launch)
    for n in (4, 8, 28, 32, 36, 1032):
        parts = min(n // 4, 256)
        buf = torch.full((parts + 3, C + 2), float("nan"), dtype=torch.float32)
        buf[:parts] = torch.randint(-64, 65, (parts, C + 2), generator=g).float() * 2.0 ** -6
        buf[:parts, C + 1] = buf[:parts, C + 1].abs()
        dev = buf.to(DEV)
        own = m.TrainOwn(w=keep.data_ptr(), b=keep.data_ptr(), targets=keep.data_ptr(), weight=w, partial=dev.data_ptr())
        gw, gb, lo = (torch.full((k,), 7.0, dtype=torch.float32, device=DEV) for k in (C, 1, 1))
        losses = torch.tensor([1.625, 1.0, 0.625, 0.0], dtype=torch.float32, device=DEV)
        m.check(Lb.bz_train_own_finish(ct.byref(own), C, n, gw.data_ptr(), gb.data_ptr(), lo.data_ptr(), losses.data_ptr(), None, s))
        torch.cuda.synchronize()
        want = buf[:parts].double().sum(0)
        assert float(buf[:parts].double().abs().sum(0).max()) < 2 ** 24 * 2.0 ** -6 and bool((want[:C] != 0).any())
        _eq(gw, want[:C], f"grad_w at {parts} parts")
        _eq(gb, want[C:C + 1], f"grad_b at {parts} parts")
        _eq(lo, want[C + 1:], f"own_loss at {parts} parts")
        total = np.float32(1.625) + np.float32(w) * np.float32(float(want[C + 1]))   # two fp32 roundings
        assert losses.tolist() == [float(total), 1.0, 0.625, 0.0], (parts, losses.tolist(), float(total))


def _step_case(C, NB, VH, n, seed):
    """a randomly initialised net and head (the head's weights large enough for the tanh to bend) and a batch with value and
    ownership targets, on the device"""
    from betazero_amd.net import OwnershipHead, PolicyValueNet
    torch.manual_seed(seed)
    net, head = PolicyValueNet(C, NB, VH, fused_tower=True).to(DEV), OwnershipHead(C).to(DEV)
    with torch.no_grad():
        head.conv.weight.mul_(3.0)
        head.conv.bias.normal_(0.0, 0.2)
    own, opp = _boards(n, seed)
    g = torch.Generator().manual_seed(seed)
    o, p, pi, z = _batch(own, opp, dyadic_pi(n, seed), torch.randint(-1, 2, (n,), generator=g).double())
    fown, fopp = target_boards(n, seed + 1)
    batch = dict(own=o, opp=p, pi=pi, z=z, vt=(torch.rand(n, generator=g) * 2 - 1).to(DEV), fown=fown.to(DEV), fopp=fopp.to(DEV))
    return net, head, batch


def _seed_moments(sp, seed, calm=False):
    """moments as from earlier steps (v >= 0, some exact zeros) for the trunk, an EMA off the parameters, then the head's moments
    (last: a plan without the head draws the same numbers for the trunk)"""
    g = torch.Generator(device=DEV).manual_seed(seed)
    rnd = lambda t: torch.randn(t.shape, device=DEV, generator=g)  # noqa: E731

    def fill(m_, v_):
        m_.copy_(rnd(m_) * 1e-3)
        r = torch.rand(v_.shape, device=DEV, generator=g)
        v_.copy_((r + 0.5) * 1e-5 if calm else (r - 0.1).clamp(min=0) ** 2 * 1e-6)
    for k in NAMES:
        fill(sp.adam_m[k], sp.adam_v[k])
    if sp.ema is not None:
        for k in NAMES:
            sp.ema[k].add_(rnd(sp.ema[k]) * 1e-2)
    if sp._own is not None:
        for k in ("w", "b"):
            fill(sp.own_m[k], sp.own_v[k])


def _snap_head(sp):
    torch.cuda.synchronize()
    out = {("p", k): t.detach().clone() for k, t in sp.own_params.items()}
    out.update({("m", k): t.clone() for k, t in sp.own_m.items()})
    out.update({("v", k): t.clone() for k, t in sp.own_v.items()})
    return out


def _check_head(sp, before, t, lr, warm, betas=(0.9, 0.999), eps=1e-8, what=""):
    """the head's p, m, v after a step: plain Adam (adam_ref) at step t from `before` and the kernel's own gradient"""
    refs = {}
    for k, p in sp.own_params.items():
        r = refs[k] = adam_ref(before[("p", k)].cpu(), before[("m", k)].cpu(), before[("v", k)].cpu(), p.grad.cpu(), lr, betas[0], betas[1], eps, t, warm)
        _within_cpu(p, r["p"], f"{what} head p {k}")
        _within_cpu(sp.own_m[k], r["m"], f"{what} head m {k}")
        _within_cpu(sp.own_v[k], r["v"], f"{what} head v {k}")
    return refs


ADAM_CASES = {"t1": (3e-3, 0.9, 0.999, 1e-8, 0, 0), "warmup": (1e-3, 0.8, 0.95, 1e-3, 5, 4), "t1e4": (1e-3, 0.9, 0.999, 1e-8, 0, 9999),
              "t1e6": (1e-3, 0.9, 0.999, 1e-8, 100, 999999)}      # test_adam_kernel_per_element's: lr, betas, eps, warm-up, steps done


@pytest.mark.parametrize("extended", [False, True])
@pytest.mark.parametrize("case", list(ADAM_CASES))
def test_own_finish_adam_per_element(case, extended):
    """the head's p, m, v after StepPlan.step() against adam_ref fed the kernel's own gradient and the pre-step state, per
    element: t = 1, the warm-up boundary, t = 10^4, t = 10^6.  Under the extended optimiser (decay 0.1, a clip at a fiftieth of
    the norm, EMA) the head is still plain Adam at the t the counter holds after the step: no decay, no clip scale -- a head
    whose gradient had been clipped would lie hundreds of bounds away"""
    from betazero_amd.train_kernels import StepPlan
    lr, b1, b2, eps, warm, done = ADAM_CASES[case]
    n = 64
    net, head, batch = _step_case(64, 1, 64, n, 3)
    sp = StepPlan(net, n, value_targets=True, ownership=head, own_weight=0.7)
    sp.set_batch(**batch)
    opts = {}
    if extended:
        sp.grads()
        clip = f32(float(norm_ref(_grads(sp)).v) / 50.0)
        opts = dict(weight_decay=0.1, clip_norm=clip, ema_decay=0.999)
    sp.enable_adam(lr, betas=(b1, b2), eps=eps, warmup_steps=warm, **opts)
    sp.reset_adam(steps_done=done)
    _seed_moments(sp, 9)
    before = _snap_head(sp)
    sp.step()
    torch.cuda.synchronize()
    assert sp.adam_t == done + 1
    refs = _check_head(sp, before, done + 1, lr, warm, (b1, b2), eps, what=case)
    assert all(not torch.equal(sp.own_params[k].detach(), before[("p", k)]) for k in ("w", "b"))
    if extended:
        st = sp.optim_stats()
        assert st["clipped"] == 1 and st["skipped"] == 0 and abs(st["scale"] - 0.02) < 1e-4, st
        gw = sp.own_params["w"].grad.cpu()
        clipped = adam_ref(before[("p", "w")].cpu(), before[("m", "w")].cpu(), before[("v", "w")].cpu(), gw * st["scale"], lr, b1, b2, eps, done + 1, warm)
        far = (clipped["m"].v - refs["w"]["m"].v).abs() > 100 * refs["w"]["m"].e
        assert float(far.double().mean()) > 0.9   # (so the bound would tell a clipped head from an unclipped one)


# ---------------------------------------------------------------- 4. the head under the extended optimiser
EXT = {"small": (64, 1, 24, 8), "large": (128, 6, 64, 4)}      # test_gpu_train_optim's shapes and batches


def _ext_plan(shape, seed, own_weight, opts, lr=1e-2, warm=5, done=2, with_head=True, net=None, head=None, batch=None, clip_x=3.0, calm=False):
    """a plan at one of EXT's shapes with value targets, the head, and decay + clip (the norm / clip_x, from a first grads()) +
    EMA; moments seeded, t = done"""
    from betazero_amd.train_kernels import StepPlan
    C, NB, VH, n = EXT[shape]
    if net is None:
        net, head, batch = _step_case(C, NB, VH, n, seed)
    if with_head:
        sp = StepPlan(net, n, value_targets=True, ownership=head, own_weight=own_weight)
        sp.set_batch(**batch)
    else:
        sp = StepPlan(net, n, value_targets=True)
        sp.set_batch(**{k: v for k, v in batch.items() if k not in ("fown", "fopp")})
    opts = dict(opts)
    if opts.get("clip_norm") is None:
        sp.grads()
        opts["clip_norm"] = f32(float(norm_ref(_grads(sp)).v) / clip_x)
    sp.enable_adam(lr, warmup_steps=warm, **opts)
    sp.reset_adam(steps_done=done)
    _seed_moments(sp, seed + 50, calm)
    return sp, net, head, batch, opts


@pytest.mark.parametrize("shape", list(EXT))
def test_whole_step_with_the_head_under_the_extended_optimiser(shape):
    """one StepPlan.step() with ownership, value targets, decay, clip and EMA all on: every element of the trunk's p, m, v, ema
    within optim_ref's bounds from the kernel's own gradients, the head's within adam_ref's (no decay, no clip) at the same t,
    the counter advanced by one, and losses[0] = fp32(fp32(CE + MSE of a plan without the head) + fp32(w L_own)) in every bit"""
    from betazero_amd.train_kernels import StepPlan
    lr, warm, done, w = 1e-2, 5, 2, 0.7
    sp, net, head, batch, opts = _ext_plan(shape, 21, w, dict(weight_decay=0.05, clip_norm=None, ema_decay=0.99), lr, warm, done)
    plain = StepPlan(copy.deepcopy(net), EXT[shape][3], value_targets=True)
    l0 = plain.grads(**{k: v for k, v in batch.items() if k not in ("fown", "fopp")}).clone()
    before, hbefore = _snap(sp), _snap_head(sp)
    losses = sp.step().clone()
    torch.cuda.synchronize()
    assert sp.adam_t == done + 1
    scale = _check_step(sp, before, done + 1, lr, warm, wd=0.05, clip=opts["clip_norm"], d=0.99, what=shape)
    _check_head(sp, hbefore, done + 1, lr, warm, what=shape)
    st = sp.optim_stats()
    assert st["clipped"] == 1 and st["skipped"] == 0 and abs(st["scale"] - float(scale.v)) <= 2 * float(scale.e), st
    l_own = float(sp.own_loss[0])
    want = np.float32(float(l0[0])) + np.float32(w) * np.float32(l_own)
    assert l_own > 0.1 and float(losses[0]) == float(want) and torch.equal(_bits(losses[1:3]), _bits(l0[1:3])), (losses.tolist(), l0.tolist(), l_own)
    assert any(not torch.equal(sp.params[k].detach(), before[("p", k)]) for k in NAMES)


@pytest.mark.parametrize("shape", list(EXT))
def test_own_weight_zero_under_the_extended_optimiser_is_the_plan_without_the_head(shape):
    """two steps from the same state on the same batch: the trunk's p, m, v, ema, the counter and the statistics of a plan with
    the head at own_weight = 0 equal, bit for bit, those of a plan built without ownership="""
    opts = dict(weight_decay=0.05, clip_norm=None, ema_decay=0.99)
    a, net, head, batch, opts = _ext_plan(shape, 22, 0.0, opts, calm=True)   # (calm: two steps in a row stay finite)
    b, _, _, _, _ = _ext_plan(shape, 22, 0.0, opts, with_head=False, net=copy.deepcopy(net), batch=batch, calm=True)
    # (a's first grads() -- for the clip -- ran before b's net was copied: nothing had moved yet)
    _same(_snap(a), _snap(b), "the two plans' starting state")
    hb = _snap_head(a)
    for _ in range(2):
        a.step(); b.step()
    sa, sb = _snap(a), _snap(b)
    sa[("stats",)], sb[("stats",)] = a.stats.clone(), b.stats.clone()
    sa[("losses",)], sb[("losses",)] = a.losses.clone(), b.losses.clone()
    _same(sa, sb, "own_weight = 0 vs no head")
    assert a.adam_t == 4 and a.optim_stats()["clipped"] >= 1 and all(bool(torch.isfinite(t).all()) for t in sa.values())
    assert not bool(a.own_params["w"].grad.any()) and not bool(a.own_params["b"].grad.any())   # no gradient reaches the head ...
    assert not torch.equal(_snap_head(a)[("p", "w")], hb[("p", "w")])                           # ... whose moments still move it


def test_graphed_step_with_the_head_and_the_extended_optimiser_equals_the_eager_step():
    """GraphedTrainStep(value_targets, ownership, decay, clip, EMA) at batch 64 on a 64 x 2 net: four replays (the rate halved by
    set_lr after the second) and a fifth on a new data set -- the same graph object -- against eager StepPlan.step() calls on a
    deep copy started from the same state: the four losses of every step, every trunk tensor, the EMA, t, the statistics and
    the head's p, m, v in every bit"""
    from betazero_amd.net import OwnershipHead, PolicyValueNet
    from betazero_amd.train import GraphedTrainStep
    from betazero_amd.train_kernels import StepPlan
    torch.manual_seed(3)
    m1, h1 = PolicyValueNet(64, 2, 64, fused_tower=True).to(DEV), OwnershipHead(64).to(DEV)
    m2, h2 = copy.deepcopy(m1), copy.deepcopy(h1)
    hw0 = h1.conv.weight.detach().clone()
    ex = _examples(256, 7)
    lr, w, opts = 2e-3, 0.7, dict(weight_decay=1e-2, clip_norm=1.0, ema_decay=0.99)
    g = GraphedTrainStep(m1, lr=lr, batch=64, lr_warmup_steps=2, value_targets=True, ownership=h1, own_weight=w, **opts)
    idxs = [torch.randperm(256, device=DEV, generator=torch.Generator(device=DEV).manual_seed(s))[:64].contiguous() for s in range(5)]
    g.idx.copy_(idxs[0])
    g.step_plan.set_batch(ex.own, ex.opp, ex.pi, ex.z, g.idx, vt=ex.vt, fown=ex.fown, fopp=ex.fopp)
    g._capture()
    sp = g.step_plan
    torch.cuda.synchronize()
    for (k, a), (_, b) in list(zip(m1.named_parameters(), m2.named_parameters())) + list(zip(h1.named_parameters(), h2.named_parameters())):
        assert torch.equal(_bits(a), _bits(b)), k       # the capture's lr = 0 steps moved nothing
    assert sp.adam_t == 0 and all(float(t.abs().max()) == 0.0 for d in (sp.own_m, sp.own_v) for t in d.values())
    eager = StepPlan(m2, 64, value_targets=True, ownership=h2, own_weight=w)
    eager.enable_adam(lr, warmup_steps=2, **opts)
    graph = g.graph
    ex2 = dataclasses.replace(ex, own=ex.own.clone(), opp=ex.opp.clone(), pi=ex.pi.clone(), z=ex.z.clone(), vt=-ex.vt,
                              fown=torch.zeros_like(ex.fown), fopp=torch.zeros_like(ex.fopp))
    last = None
    for s, idx in enumerate(idxs):
        if s == 2:
            g.set_lr(lr / 2)
            eager.set_lr(lr / 2)
        e = ex2 if s == 4 else ex
        l1 = g(e, idx).clone()
        eager.set_batch(e.own, e.opp, e.pi, e.z, idx, vt=e.vt, fown=e.fown, fopp=e.fopp)
        l2 = torch.cat([eager.step()[:3], eager.own_loss])
        assert l1.shape == (4,) and torch.equal(_bits(l1), _bits(l2)) and bool(torch.isfinite(l1).all()), (s, l1.tolist(), l2.tolist())
        if s == 4:   # (all-zero targets are another L_own altogether: the replay did read the new arrays)
            assert abs(float(l1[3]) - float(last[3])) > 0.1, (l1.tolist(), last.tolist())
        last = l1
    assert g.graph is graph and float(sp.hyper[0]) == f32(lr / 2)
    a, b = _snap(sp), _snap(eager)
    a[("stats",)], b[("stats",)] = sp.stats.clone(), eager.stats.clone()
    _same(a, b, "graph vs eager: the trunk")
    _same(_snap_head(sp), _snap_head(eager), "graph vs eager: the head")
    assert sp.adam_t == 5 and g.optim_stats()["skipped"] == 0
    assert not torch.equal(h1.conv.weight.detach(), hw0) and float(sp.own_m["w"].abs().max()) > 0
    g.check()


def test_skip_rule_a_non_finite_trunk_skips_the_trunk_and_the_head_still_updates():
    """a NaN in one pi row: the trunk's norm is not finite -- p, m, v, ema keep their bits, skipped = 1 -- while the head's C + 1
    gradients are finite (its loss does not see pi): the head takes plain Adam's step at the advanced t.  The next, clean step
    updates both at t + 1, within bounds"""
    lr, warm, done = 1e-2, 4, 1
    sp, net, head, batch, opts = _ext_plan("small", 23, 0.7, dict(weight_decay=0.05, clip_norm=None, ema_decay=0.99), lr, warm, done, calm=True)
    clean = batch["pi"].clone()
    batch["pi"][3, 5] = float("nan")
    before, hbefore = _snap(sp), _snap_head(sp)
    losses = sp.step().clone()
    after = _snap(sp)
    st = sp.optim_stats(reset=False)
    assert float(after.pop(("t",))) == done + 1 and float(before.pop(("t",))) == done
    _same(before, after, "a skipped step wrote something of the trunk")
    assert st["skipped"] == 1 and st["clipped"] == 0 and st["scale"] == 0.0 and not np.isfinite(st["grad_norm"]), st
    assert not np.isfinite(float(losses[0])) and np.isfinite(float(sp.own_loss[0]))
    assert all(bool(torch.isfinite(p.grad).all()) for p in sp.own_params.values())
    _check_head(sp, hbefore, done + 1, lr, warm, what="skipped trunk")
    assert not torch.equal(sp.own_params["w"].detach(), hbefore[("p", "w")])
    batch["pi"].copy_(clean)
    before, hbefore = _snap(sp), _snap_head(sp)
    sp.step()
    torch.cuda.synchronize()
    assert sp.adam_t == done + 2
    _check_step(sp, before, done + 2, lr, warm, wd=0.05, clip=opts["clip_norm"], d=0.99, what="after the skip")
    _check_head(sp, hbefore, done + 2, lr, warm, what="after the skip")
    st = sp.optim_stats()
    assert st["skipped"] == 1 and st["clipped"] == 1, st
    assert all(not torch.equal(sp.params[k].detach(), before[("p", k)]) for k in NAMES)


def test_skip_rule_b_a_non_finite_head_moves_nothing():
    """an infinity in one weight of the head: L_own, the loss and the head's gradient are not finite, and through g[L] neither is
    the trunk's norm -- nothing moves, bit for bit: not the trunk, the EMA, the head or its moments; skipped = 1"""
    sp, net, head, batch, opts = _ext_plan("small", 24, 0.7, dict(weight_decay=0.05, clip_norm=None, ema_decay=0.99), done=1)
    with torch.no_grad():
        head.conv.weight.view(-1)[11] = float("inf")
    before, hbefore = _snap(sp), _snap_head(sp)
    losses = sp.step().clone()
    after, hafter = _snap(sp), _snap_head(sp)
    st = sp.optim_stats()
    assert float(after.pop(("t",))) == 2.0 and float(before.pop(("t",))) == 1.0
    _same(before, after, "the trunk")
    _same(hbefore, hafter, "the head")
    assert st["skipped"] == 1 and st["scale"] == 0.0, st
    assert not np.isfinite(float(losses[0])) and not np.isfinite(float(sp.own_loss[0]))
    assert not bool(torch.isfinite(torch.cat([p.grad.flatten() for p in sp.own_params.values()])).all())


@pytest.mark.parametrize("where", ["ow", "ob"])
@pytest.mark.parametrize("bad", ["nan", "-nan", "inf", "-inf"])
def test_nonfinite_head_parameter_gives_nonfinite_loss(where, bad):
    """test_nonfinite_parameter_gives_nonfinite_loss on the fourth plane: wherever torch's fp32 train_step(..., ownership=head)
    gives a non-finite loss, StepPlan.grads' losses[0] and own_loss[0] are not finite either"""
    from betazero_amd.net import OwnershipHead, PolicyValueNet
    from betazero_amd.train import train_step
    from betazero_amd.train_kernels import StepPlan
    bits = {"nan": 0x7FC00000, "-nan": -0x00400000, "inf": 0x7F800000, "-inf": -0x00800000}[bad]
    n = 16
    torch.manual_seed(4)
    net, head = PolicyValueNet(64, 1, 64, fused_tower=True).to(DEV), OwnershipHead(64).to(DEV)
    with torch.no_grad():
        t = head.conv.weight if where == "ow" else head.conv.bias
        t.view(-1)[(37 if where == "ow" else 0):][:1].view(torch.int32).fill_(bits)
    ex = _examples(n, 6)
    sp = StepPlan(net, n, ownership=head, own_weight=0.7)
    losses = sp.grads(ex.own, ex.opp, ex.pi, ex.z, fown=ex.fown, fopp=ex.fopp).clone()
    l_own = sp.own_loss.clone()
    n2, h2 = copy.deepcopy(net), copy.deepcopy(head)
    for p in list(n2.parameters()) + list(h2.parameters()):
        p.grad = None
    opt = torch.optim.SGD(list(n2.parameters()) + list(h2.parameters()), lr=0.0)
    ref = train_step(n2, opt, ex, autocast=False, ownership=h2, own_weight=0.7)
    torch.cuda.synchronize()
    if not bool(torch.isfinite(ref[0])):
        assert not bool(torch.isfinite(losses[0])) and not bool(torch.isfinite(l_own[0])), (where, bad, [float(t) for t in ref], losses.tolist())
    if where == "ow" or "nan" in bad:   # (a weight meets zero and non-zero activations; an infinite bias only saturates the tanh)
        assert not bool(torch.isfinite(ref[0]))
    else:
        assert bool(torch.isfinite(ref[0])) and bool(torch.isfinite(losses[0])) and bool(torch.isfinite(l_own[0]))


# ---------------------------------------------------------------- 5. the whole step chained, with the head on
def test_whole_step_chained_with_the_head():
    """test_whole_step_chained_bitexact's construction at (64, 2 blocks, 64) with ownership= and exact_own_params, through
    StepPlan.grads: the stem's and the tower's activations bit for bit, and on the tower's own act[L] the heads -- the fourth plane
    included -- within their bounds (the policy saturates and v2 = 0: of g[L] only the head's term rounds).  The backward is NOT
    chained bit for bit here as it is without the head: the head's term puts tanh-derived values over some fifty binades into
    g[L] (Sigma |terms| of a backward layer is 3.6e16 units of g[L]'s grid, against the 2^24 an order-free fp32 sum allows), so
    no exact reference of the tower's backward exists; with own_weight = 0 g[L] has the bits of the plan without the head, whose
    chain test_whole_step_chained_bitexact pins."""
    from betazero_amd.train_kernels import StepPlan
    C, NB, n, w = 64, 2, 64, 1.0
    L = 2 * NB
    g = torch.Generator().manual_seed(n)
    sw = torch.randint(-2, 3, (C, 2, 3, 3), generator=g).double() * (torch.rand(C, 2, 3, 3, generator=g) < 0.4)
    sb = torch.randint(-1, 3, (C,), generator=g).double()
    _, W, b, _ = exact_tower(C, L, 4, 40 + L)
    P = exact_head_params(C, 64, 7, saturate=True)
    ow, ob = exact_own_params(C, 7)
    own, opp = _boards(n, 2)
    fown, fopp = target_boards(n, 2)
    pi, z = dyadic_pi(n, 5, bits=4), torch.randint(-1, 2, (n,), generator=g).double()
    net = _net(C, NB, 64, P=P, stem=(sw.float(), sb.float()), tower=(W.float(), b.float()))
    sp = StepPlan(net, n, ownership=_head(C, ow, ob), own_weight=w)
    losses = sp.grads(*_batch(own, opp, pi, z), fown=fown.to(DEV), fopp=fopp.to(DEV)).clone()
    torch.cuda.synchronize()
    act0 = stem_ref(own, opp, sw, sb).to(DEV)
    acts = tower_reference(act0, W.to(DEV), b.to(DEV), torch.zeros_like(act0))[0]
    for l in range(L + 1):
        _eq(sp.acts[l], acts[l], f"act[{l}]")
    own_arg = {"ow": ow.to(DEV), "ob": ob.to(DEV), "fown": fown.to(DEV), "fopp": fopp.to(DEV), "own_weight": w}
    Pd = {k: v.to(DEV) for k, v in P.items()}
    r = heads_ref(acts[L], Pd, pi.to(DEV), z.to(DEV), own=own_arg)
    r0 = heads_ref(acts[L], Pd, pi.to(DEV), z.to(DEV))
    assert float(r["s"].max(1).values.sub(r["s"].topk(2, 1).values[:, 1]).min()) >= 128   # saturated
    assert float(r0["g_top"].e.max()) == 0.0 and float(r["g_top"].e.max()) > 0            # only the head's term rounds
    grads = {k: getattr(getattr(net, mod), p).grad for k, (mod, p) in HEAD_GRADS.items()}
    _check_own(r, (losses, grads, sp.gs[L].float(), sp.own_loss, (sp.own_params["w"].grad, sp.own_params["b"].grad)))
    assert float(r["own_w"].v.abs().max()) > 0 and float((r["o"].v.abs() > 0.5).double().mean()) > 0.1
    gL = _f64(sp.gs[L])
    moved = (gL < bf16_rne(r0["g_top"].v)) | (gL > bf16_rne(r0["g_top"].v))
    assert float(moved.double().mean()) > 0.01 and all(float(sp.gs[l].float().abs().max()) > 0 for l in range(L + 1))
