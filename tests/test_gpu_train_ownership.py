"""The ownership head in the fused training step on the GPU: k_train_heads_own / k_train_heads_own_vt against
torch autograd in fp32 on the same bf16 act[L] and against k_train_heads, k_train_own_finish against torch.optim.Adam, the whole
graphed step against the torch path (train_step(ownership=...)), and the loop tool."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from betazero_amd import _lib
from test_gpu_train_kernels import _byref, _heads_reference, _net_case, _rel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _targets(n, seed):
    """random disjoint target boards, int64 [n] device tensors: an all-empty row, one side owning everything (bit 63 set: the
    int64 sign), the other side owning everything"""
    rng = np.random.default_rng(seed)
    hi = lambda: rng.integers(0, 2, n).astype(np.uint64) << np.uint64(63)  # noqa: E731
    a = rng.integers(0, 2**63, n, dtype=np.int64).astype(np.uint64) | hi()
    b = (rng.integers(0, 2**63, n, dtype=np.int64).astype(np.uint64) | hi()) & ~a
    a[0], b[0] = np.uint64(0), np.uint64(0)
    a[1], b[1] = np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0)
    a[2], b[2] = np.uint64(0), np.uint64(0xFFFFFFFFFFFFFFFF)
    t = lambda x: torch.as_tensor(x.view(np.int64)).to(DEV)  # noqa: E731
    return t(a), t(b)


def _own_case(C, NB, n, seed, VH=64, own_weight=1.0, value_targets=False):
    """_net_case plus an ownership head (weights large enough that the tanh is exercised on both sides) and a plan with it"""
    from betazero_amd.net import OwnershipHead
    from betazero_amd.train_kernels import StepPlan
    m, _, own, opp, pi, z = _net_case(C, NB, n, seed, VH)
    head = OwnershipHead(C).cuda()
    with torch.no_grad():
        head.conv.weight.mul_(3.0)
        head.conv.bias.normal_(0.0, 0.2)
    plan = StepPlan(m, n, value_targets=value_targets, ownership=head, own_weight=own_weight)
    fown, fopp = _targets(n, seed + 100)
    vt = (torch.rand(n, device=DEV) * 2 - 1) if value_targets else None
    return m, head, plan, own, opp, pi, z, vt, fown, fopp


def _run_heads(plan, m, x, own=True, n=None):
    """the heads kernel (with or without the ownership head), the FC weight gradients, the finish and the head's own finish on
    act[L] = x: (losses [4], the ten head gradients, g_top, L_own or None, (d ow, d ob) or None).  n: the batch the kernels are
    launched with, the first n positions of the plan's (a StepPlan's batch is a multiple of 8, the head kernels' of 4)."""
    L, st, Ly, C, VH = _lib.lib(), torch.cuda.current_stream().cuda_stream, plan.L, plan.C, plan.VH
    n = plan.n if n is None else n
    plan.acts[Ly][:n].copy_(x)
    common = (n, C, VH, _byref(plan._head), plan.gs[Ly].data_ptr(), plan.hv.data_ptr(), plan.dl.data_ptr(), plan.dv1.data_ptr(),
              plan.heads_partial.data_ptr(), st)
    bd = plan.batch_desc.data_ptr()
    if own and plan.value_targets:
        _lib.check(L.bz_train_heads_own_vt(plan.acts[Ly].data_ptr(), bd, plan.vt_slot.data_ptr(), _byref(plan._own), *common))
    elif own:
        _lib.check(L.bz_train_heads_own(plan.acts[Ly].data_ptr(), bd, _byref(plan._own), *common))
    elif plan.value_targets:
        _lib.check(L.bz_train_heads_vt(plan.acts[Ly].data_ptr(), bd, plan.vt_slot.data_ptr(), *common))
    else:
        _lib.check(L.bz_train_heads(plan.acts[Ly].data_ptr(), bd, *common))
    _lib.check(L.bz_train_heads_wgrad(plan.hv.data_ptr(), plan.dl.data_ptr(), plan.dv1.data_ptr(), n, VH, plan.heads_w_partial.data_ptr(), st))
    _lib.check(L.bz_train_finish(_byref(plan._partials), _byref(plan._grads), C, Ly, VH, n, plan.losses.data_ptr(), None, st))
    l_own = d_own = None
    if own:
        w, b = plan.own_params["w"], plan.own_params["b"]
        _lib.check(L.bz_train_own_finish(_byref(plan._own), C, n, w.grad.data_ptr(), b.grad.data_ptr(), plan.own_loss.data_ptr(),
                                         plan.losses.data_ptr(), None, st))
        l_own, d_own = plan.own_loss.clone(), (w.grad.clone(), b.grad.clone())
    grads = {k + s: getattr(getattr(m, k), a).grad.clone() for k in ("pol", "polfc", "val", "v1", "v2") for s, a in (("_w", "weight"), ("_b", "bias"))}
    return plan.losses.clone(), grads, plan.gs[Ly][:n].float().clone(), l_own, d_own


# (64, 4): one pass of one workgroup; (64, 1032): several passes per workgroup, VH = 24 leaves lanes of the value head idle
@pytest.mark.parametrize("value_targets", [False, True])
@pytest.mark.parametrize("C,n,VH", [(64, 4, 64), (64, 8, 64), (128, 20, 64), (64, 1032, 24)])
def test_heads_own_kernel_losses_and_gradients_vs_torch_fp32(C, n, VH, value_targets):
    """the tolerances of test_heads_kernel_losses_and_gradients_vs_torch_fp32, now on four losses and twelve gradient tensors"""
    from betazero_amd.train import ownership_targets
    w_own = 0.7
    m, head, plan, own, opp, pi, z, vt, fown, fopp = _own_case(C, 1, max(n, 8), 31, VH, own_weight=w_own, value_targets=value_targets)
    x = torch.relu(torch.randn((n, 64, C), device=DEV) - 0.3).bfloat16()
    plan.set_batch(own, opp, pi, z, vt=vt, fown=fown, fopp=fopp)
    losses, got, g_top, l_own, (d_ow, d_ob) = _run_heads(plan, m, x, n=n)
    if n < plan.n:   # (n = 4: the kernels read the first four rows of the data set)
        pi, z, fown, fopp, vt = pi[:n], z[:n], fown[:n], fopp[:n], (vt[:n] if vt is not None else None)
    for p in list(m.parameters()) + list(head.parameters()):
        p.grad = None
    xr = x.float().requires_grad_(True)
    _, ce, mse = _heads_reference(m, xr, pi, vt if value_targets else z)
    o = head(xr.view(n, 8, 8, C).permute(0, 3, 1, 2))
    t = ownership_targets(fown, fopp)
    assert set(np.unique(t.cpu().numpy())) == {-1.0, 0.0, 1.0} and not t[0].any() and (t[1] == 1).all() and (t[2] == -1).all()
    want_own = torch.nn.functional.mse_loss(o, t)   # the mean over positions and all 64 cells
    total = ce + mse + w_own * want_own
    total.backward()
    four = np.concatenate([losses[:3].cpu().numpy(), l_own.cpu().numpy()])
    want = [float(total), float(ce), float(mse), float(want_own)]
    print("losses kernel / torch:", four, want)
    assert np.allclose(four, want, rtol=2e-5, atol=1e-6), (four, want)
    for k in ("pol", "polfc", "val", "v1", "v2"):
        assert _rel(got[k + "_w"], getattr(m, k).weight.grad) < 1e-4, (k, _rel(got[k + "_w"], getattr(m, k).weight.grad))
        assert _rel(got[k + "_b"], getattr(m, k).bias.grad) < 1e-4, (k, "bias")
    print("d ow, d ob rel:", _rel(d_ow, head.conv.weight.grad), _rel(d_ob, head.conv.bias.grad))
    assert _rel(d_ow, head.conv.weight.grad) < 1e-4 and _rel(d_ob, head.conv.bias.grad) < 1e-4
    assert float(d_ow.abs().max()) > 0
    gx = xr.grad * (x > 0)
    assert float((g_top - gx).abs().max()) <= 2.0 ** -8 * float(gx.abs().max()) + 1e-12, "g[L] more than bf16 rounding off"
    assert float(g_top.abs().max()) > 0 and float((g_top != 0).float().mean()) > 0.05
    assert float(losses[3]) == 0.0


@pytest.mark.parametrize("value_targets", [False, True])
@pytest.mark.parametrize("C,n,VH", [(64, 8, 64), (128, 20, 64), (64, 1032, 24)])
def test_own_weight_zero_leaves_every_output_of_the_heads_kernel_at_its_value(C, n, VH, value_targets):
    from betazero_amd.train import ownership_targets
    m, head, plan, own, opp, pi, z, vt, fown, fopp = _own_case(C, 1, n, 32, VH, own_weight=0.0, value_targets=value_targets)
    x = torch.relu(torch.randn((n, 64, C), device=DEV) - 0.3).bfloat16()
    plan.set_batch(own, opp, pi, z, vt=vt, fown=fown, fopp=fopp)
    l0, g0, top0, _, _ = _run_heads(plan, m, x, own=False)
    l1, g1, top1, l_own, (d_ow, d_ob) = _run_heads(plan, m, x, own=True)
    assert torch.equal(l0[:3], l1[:3]) and torch.equal(top0, top1) and float(top0.abs().max()) > 0
    assert set(g0) == set(g1) and len(g0) == 10 and all(torch.equal(g0[k], g1[k]) for k in g0)
    with torch.no_grad():   # L_own is still reported, and no gradient reaches the head
        want = torch.nn.functional.mse_loss(head(x.float().view(n, 8, 8, C).permute(0, 3, 1, 2)), ownership_targets(fown, fopp))
    assert np.allclose(float(l_own), float(want), rtol=2e-5, atol=1e-6) and float(want) > 0.1
    assert not d_ow.any() and not d_ob.any()


def test_own_finish_equals_torch_adam_and_skips_a_non_finite_gradient():
    """5 steps with warm-up: the head's parameters after k_train_own_finish against torch.optim.Adam fed the same gradients, to
    the tolerance of test_adam_kernel_equals_torch_adam; then a non-finite gradient leaves parameters and moments bit-identical"""
    lr, warmup, n, C = 3e-3, 4, 64, 64
    m, head, plan, own, opp, pi, z, vt, fown, fopp = _own_case(C, 2, n, 33)
    h2 = copy.deepcopy(head)
    h0 = copy.deepcopy(head)
    for p in h2.parameters():
        p.grad = None
    plan.enable_adam(lr, warmup_steps=warmup)
    opt = torch.optim.Adam(h2.parameters(), lr=lr)
    plan.set_batch(own, opp, pi, z, fown=fown, fopp=fopp)
    for t in range(1, 6):
        plan.step()
        for g in opt.param_groups:
            g["lr"] = lr * min(1.0, t / warmup)
        for a, b in zip(head.parameters(), h2.parameters()):
            b.grad = a.grad.clone()
        opt.step()
        for (k, a), (_, b) in zip(head.named_parameters(), h2.named_parameters()):
            assert float((a - b).abs().max()) <= 1e-5 * lr * t + 5e-7 * float(b.abs().max()), (t, k, float((a - b).abs().max()))
    assert plan.adam_t == 5
    assert max(float((a - b).abs().max()) for a, b in zip(head.parameters(), h0.parameters())) > 1e-3   # ... and they did move
    # the same launch on partial sums holding one infinity (then one NaN): gradient and loss are written, nothing is updated
    L, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    w, b = plan.own_params["w"], plan.own_params["b"]
    for bad, at in ((float("inf"), 5), (float("nan"), C)):   # (entry C: d ob)
        state = [t.clone() for t in (w, b, plan.own_m["w"], plan.own_m["b"], plan.own_v["w"], plan.own_v["b"])]
        keep = plan.own_partial.clone()
        plan.own_partial[1, at] = bad
        _lib.check(L.bz_train_own_finish(_byref(plan._own), C, n, w.grad.data_ptr(), b.grad.data_ptr(), plan.own_loss.data_ptr(), None,
                                         _byref(plan._own_adam), st))
        torch.cuda.synchronize()
        now = (w, b, plan.own_m["w"], plan.own_m["b"], plan.own_v["w"], plan.own_v["b"])
        assert all(torch.equal(a.view(torch.int32), c.view(torch.int32)) for a, c in zip(state, now)), bad
        assert not bool(torch.isfinite(torch.cat([w.grad.flatten(), b.grad.flatten()])).all())
        plan.own_partial.copy_(keep)
    _lib.check(L.bz_train_own_finish(_byref(plan._own), C, n, w.grad.data_ptr(), b.grad.data_ptr(), plan.own_loss.data_ptr(), None,
                                     _byref(plan._own_adam), st))
    assert not torch.equal(state[0], w)   # (finite again: the same launch does update)


def _examples(n, seed):
    from betazero_amd.engine import DeviceExamples, Examples
    rng = np.random.default_rng(seed)
    own = rng.integers(0, 2**63, n, dtype=np.int64).astype(np.uint64)
    opp = rng.integers(0, 2**63, n, dtype=np.int64).astype(np.uint64) & ~own
    pi = rng.random((n, 65)).astype(np.float32); pi /= pi.sum(1, keepdims=True)
    z = rng.integers(-1, 2, n).astype(np.int8)
    # targets a net can learn something about: the position's own stones plus a fixed pattern of the empty cells
    empty = ~(own | opp)
    fown, fopp = own | (empty & np.uint64(0x0F0F0F0F0F0F0F0F)), opp | (empty & np.uint64(0xF0F0F0F000000000))
    vt = (rng.random(n) * 2 - 1).astype(np.float32)
    return DeviceExamples.from_host(Examples(own, opp, pi, z, np.ones(n, np.int8), np.zeros(n, np.uint8), np.arange(n), np.zeros(n, np.int32),
                                             8, vt=vt, fown=fown, fopp=fopp))


def test_graphed_step_with_ownership_and_value_targets_tracks_the_torch_path():
    """test_graphed_train_step_on_the_tower_kernels_tracks_the_autograd_step with the ownership head and value targets on, within
    that test's tolerances (now on four losses); then a new data set after the capture (no recapture) and bad row indices"""
    import dataclasses
    from betazero_amd.net import OwnershipHead, PolicyValueNet
    from betazero_amd.train import GraphedTrainStep, train_step
    n, batch, w_own = 1024, 64, 1.0
    ex = _examples(n, 11)
    torch.manual_seed(5)
    m1, h1 = PolicyValueNet(64, 2, 64, fused_tower=True).cuda(), OwnershipHead(64).cuda()
    m2, h2 = copy.deepcopy(m1), copy.deepcopy(h1)
    w0, hw0 = m1.tower_w.detach().clone(), h1.conv.weight.detach().clone()
    g = GraphedTrainStep(m1, lr=1e-3, batch=batch, value_targets=True, ownership=h1, own_weight=w_own)
    assert g.step_plan is not None and g.step_plan.ownership is h1
    opt = torch.optim.Adam(list(m2.parameters()) + list(h2.parameters()), lr=1e-3)
    gen = torch.Generator(device=DEV).manual_seed(0)
    for step in range(8):
        idx = torch.randint(0, n, (batch,), device=DEV, generator=gen)
        l1 = g(ex, idx).cpu().numpy()
        l2 = torch.stack(train_step(m2, opt, ex, idx, value_targets=True, ownership=h2, own_weight=w_own)).cpu().numpy()
        assert l1.shape == (4,) and np.isfinite(l1).all() and np.abs(l1 - l2).max() < 3e-2 * max(1.0, np.abs(l2).max()), (step, l1, l2)
        assert abs(l1[0] - (l1[1] + l1[2] + w_own * l1[3])) < 1e-5 * max(1.0, abs(l1[0]))   # the loss gained the ownership term
    d1, d2 = (m1.tower_w.detach() - w0).flatten(), (m2.tower_w.detach() - w0).flatten()
    cos = float(torch.nn.functional.cosine_similarity(d1, d2, dim=0))
    print("cosine of the tower's weight updates after 8 steps, kernels vs autograd:", round(cos, 4), "last losses", l1, l2)
    assert float(d1.abs().max()) > 0 and cos > 0.9
    for name in ("stem", "pol", "polfc", "val", "v1", "v2"):
        a, b = getattr(m1, name).weight.detach().flatten(), getattr(m2, name).weight.detach().flatten()
        assert float(torch.nn.functional.cosine_similarity(a, b, dim=0)) > 0.999, name
    a, b = (h1.conv.weight.detach() - hw0).flatten(), (h2.conv.weight.detach() - hw0).flatten()
    assert float(a.abs().max()) > 0 and float(torch.nn.functional.cosine_similarity(a, b, dim=0)) > 0.9
    # a new data set after the capture: new tensors at new addresses, every ownership target 0 -- the same graph reads them
    graph = g.graph
    ex2 = dataclasses.replace(ex, own=ex.own.clone(), opp=ex.opp.clone(), pi=ex.pi.clone(), z=ex.z.clone(), vt=ex.vt.clone(),
                              fown=torch.zeros_like(ex.fown), fopp=torch.zeros_like(ex.fopp))
    idx = torch.randint(0, n, (batch,), device=DEV, generator=gen)
    m3, h3 = copy.deepcopy(m1), copy.deepcopy(h1)
    l1 = g(ex2, idx).cpu().numpy()
    opt3 = torch.optim.Adam(list(m3.parameters()) + list(h3.parameters()), lr=0.0)
    l3 = torch.stack(train_step(m3, opt3, ex2, idx, value_targets=True, ownership=h3, own_weight=w_own)).cpu().numpy()
    l_same = torch.stack(train_step(m3, opt3, ex, idx, value_targets=True, ownership=h3, own_weight=w_own)).cpu().numpy()
    assert g.graph is graph and np.abs(l1 - l3).max() < 3e-2 * max(1.0, np.abs(l3).max()), (l1, l3)
    # (all-zero targets are another loss altogether, several tolerances away: the step did read the new arrays)
    assert abs(l3[3] - l_same[3]) > 0.1, (l3, l_same)
    g.check()
    bad = idx.clone()
    bad[5] = n + 7
    g(ex2, bad)
    with pytest.raises(IndexError, match="1 batch position"):
        g.check()
    assert g.graph is graph
    with pytest.raises(ValueError, match="fown"):
        g(dataclasses.replace(ex, fown=None), idx)


def test_l_own_falls_on_one_fixed_batch():
    from betazero_amd.net import OwnershipHead, PolicyValueNet
    from betazero_amd.train import GraphedTrainStep
    ex = _examples(64, 12)
    torch.manual_seed(6)
    m, h = PolicyValueNet(64, 2, 64, fused_tower=True).cuda(), OwnershipHead(64).cuda()
    g = GraphedTrainStep(m, lr=1e-3, batch=64, ownership=h)
    idx = torch.arange(64, device=DEV)
    losses = torch.stack([g(ex, idx) for _ in range(100)]).cpu().numpy()
    print("L_own at steps 1, 10, 50, 100:", losses[[0, 9, 49, 99], 3])
    assert np.isfinite(losses).all() and losses[99, 3] < losses[0, 3]


def test_python_refusals_around_the_step():
    from betazero_amd.net import OwnershipHead, PolicyValueNet
    from betazero_amd.train import GraphedTrainStep
    from betazero_amd.train_kernels import StepPlan
    m = PolicyValueNet(64, 1, 64, fused_tower=True).cuda()
    with pytest.raises(ValueError, match="OwnershipHead"):
        StepPlan(m, 8, ownership=OwnershipHead(128).cuda())
    with pytest.raises(ValueError, match="OwnershipHead"):
        StepPlan(m, 8, ownership=torch.nn.Conv2d(64, 1, 1).cuda())
    plan = StepPlan(m, 8, ownership=OwnershipHead(64).cuda())
    ex = _examples(8, 1)
    with pytest.raises(ValueError, match="fown"):
        plan.set_batch(ex.own, ex.opp, ex.pi, ex.z)
    with pytest.raises(ValueError, match="fown"):
        plan.set_batch(ex.own, ex.opp, ex.pi, ex.z, fown=ex.fown, fopp=ex.fopp.to(torch.int32))
    with pytest.raises(ValueError, match="without ownership"):
        StepPlan(m, 8).set_batch(ex.own, ex.opp, ex.pi, ex.z, fown=ex.fown, fopp=ex.fopp)
    with pytest.raises(ValueError, match="all-kernel step"):
        GraphedTrainStep(PolicyValueNet(64, 1, 64), batch=8, ownership=OwnershipHead(64))
    L = _lib.lib()
    assert L.bz_train_heads_own(None, None, None, 64, 64, 64, None, None, None, None, None, None, None) == _lib.BZ_EINVAL
    assert b"bz_train_heads_own" in L.bz_last_error()
    assert L.bz_train_own_finish(None, 64, 64, None, None, None, None, None, None) == _lib.BZ_EINVAL and b"bz_train_own_finish" in L.bz_last_error()


def test_az_loop_runs_two_iterations_with_ownership_under_the_cap():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "az_loop.py"), "--iters", "2", "--games", "64", "--sims", "16",
                          "--ownership", "--fast-sims", "4", "--full-prob", "0.5", "--channels", "64", "--blocks", "1",
                          "--arena-games", "16", "--arena-sims", "8", "--depth", "1", "--final-depths", ""],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    its = [d for d in (json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")) if d.get("what") == "iteration"]
    assert [d["iter"] for d in its] == [1, 2]
    for d in its:
        assert 0 < d["rows_per_game"] < d["plies"] and np.isfinite(d["own"]) and 0 < d["own"] < 4 and d["own_weight"] == 1.0, d
        assert len(d["loss_last_tenth"]) == 4
