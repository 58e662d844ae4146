"""The extended optimiser of the all-kernel training step on the GPU (bz_train_optim_step: k_train_gnorm + k_train_optim,
DESIGN.md 12.1): bit-equality with k_train_adam when every option is off, the gradient norm against its derived bound and
its determinism, every element of p, m, v and the EMA against tests/test_train_optim_cpu.py's bounded reference, the skip
rule, the sticky counters, the captured graph against the eager step, torch's AdamW + clip_grad_norm_ + EMA fed the same
gradients, and the averaged net's way into the engine.  No forward pass except where a test is about the whole step: the
gradients are written into the plan's static .grad tensors and StepPlan.optim_step() runs the two launches alone.

Two nets at the smallest batch their plans accept (8 at 64 channels, 4 at 128; the optimiser never sees the batch): 64 x 1
blocks, value hidden 24 (about 90 blocks of 1024 elements -- fewer than k_train_gnorm's 256
workgroups, so the idle ones' partial slots matter; jobs of 1, 2, 24 and 65 elements) and 128 x 6, value hidden 64 (1728
tower blocks: seven trips per workgroup)."""
import copy
import types

import numpy as np
import pytest
import torch

from test_train_optim_cpu import NAMES, clip_scale_ref, f32, is_weight, norm_ref, optim_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = {"small": (64, 1, 24), "large": (128, 6, 64)}
BATCH = {"small": 8, "large": 4}      # the smallest a StepPlan takes at 64 / 128 channels (positions resident per workgroup)
BOTH = ["small", "large"]
MIXED = (1e-2, 1.0, 1e2, 1e-6, 1e-1, 1.0, 1e-3, 10.0, 1e-4, 1.0, 1e-5, 1e2, 1.0, 1e-6)   # a scale per tensor, in job order
_PLANS = {}


def _plan(shape):
    """one net and StepPlan per shape for the whole module (enable_adam is called anew by every test), and its initial parameters"""
    from betazero_amd.net import PolicyValueNet
    from betazero_amd.train_kernels import StepPlan
    if shape not in _PLANS:
        torch.manual_seed(11)
        net = PolicyValueNet(*SHAPES[shape], fused_tower=True).to(DEV)
        sp = StepPlan(net, BATCH[shape])
        _PLANS[shape] = (sp, {k: p.detach().clone() for k, p in sp.params.items()})
    return _PLANS[shape]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), (what, k, int((_bits(a[k]) != _bits(b[k])).sum()))


def _snap(sp):
    """every tensor the optimiser may write, and its counter"""
    torch.cuda.synchronize()
    out = {("p", k): t.detach().clone() for k, t in sp.params.items()}
    out.update({("m", k): t.clone() for k, t in sp.adam_m.items()})
    out.update({("v", k): t.clone() for k, t in sp.adam_v.items()})
    if sp.ema is not None:
        out.update({("ema", k): t.clone() for k, t in sp.ema.items()})
    out[("t",)] = sp.hyper[1:2].clone()
    return out


def _start(shape, seed=5, steps_done=0, lr=3e-3, warm=0, betas=(0.9, 0.999), eps=1e-8, calm=False, **opts):
    """the plan of `shape` with a fresh optimiser (options `opts`) on the initial parameters, moments as from earlier steps
    (v >= 0, some exact zeros; calm: v >= 5e-6 everywhere, so that m / sqrt(v) < 1 and a run of whole steps stays finite)
    and, with an EMA, averaged weights near the parameters but not on them"""
    sp, p0 = _plan(shape)
    with torch.no_grad():
        for k, p in sp.params.items():
            p.copy_(p0[k])
    sp.enable_adam(lr, betas=betas, eps=eps, warmup_steps=warm, **opts)
    sp.reset_adam(steps_done=steps_done)
    g = torch.Generator(device=DEV).manual_seed(seed)
    for k in NAMES:
        sp.adam_m[k].copy_(torch.randn(sp.adam_m[k].shape, device=DEV, generator=g) * 1e-3)
        r = torch.rand(sp.adam_v[k].shape, device=DEV, generator=g)
        sp.adam_v[k].copy_((r + 0.5) * 1e-5 if calm else (r - 0.1).clamp(min=0) ** 2 * 1e-6)
        if sp.ema is not None:
            sp.ema[k].add_(torch.randn(sp.ema[k].shape, device=DEV, generator=g) * 1e-2)
    return sp


def _set_grads(sp, seed, scales=MIXED, size=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    for k, s in zip(NAMES, scales):
        gr = sp.params[k].grad
        gr.copy_(torch.randn(gr.shape, device=DEV, generator=g) * (s * size))


def _grads(sp):
    return [sp.params[k].grad.detach().cpu() for k in NAMES]


def _within(got, ref, what, k=2.0):
    """|kernel - reference| <= k * derived bound, element by element (k = 2 covers the bounds' second-order terms)"""
    got, v, e = got.detach().cpu().double(), ref.v, ref.e
    bad = ~((got - v).abs() <= k * e)
    assert not bool(bad.any()), (what, int(bad.sum()), got[bad][:4].tolist(), v[bad][:4].tolist(), e[bad][:4].tolist())


def _boards(n, seed):
    rng = np.random.default_rng(seed)
    own = rng.integers(0, 2 ** 63, n, dtype=np.int64)
    opp = rng.integers(0, 2 ** 63, n, dtype=np.int64) & ~own
    pi = torch.rand(n, 65, generator=torch.Generator().manual_seed(seed)) ** 4
    z = torch.from_numpy(rng.integers(-1, 2, n).astype(np.int8))
    return torch.from_numpy(own).to(DEV), torch.from_numpy(opp).to(DEV), (pi / pi.sum(1, keepdim=True)).to(DEV).contiguous(), z.to(DEV)


# ---------------------------------------------------------------- 1. off is the old kernel
@pytest.mark.parametrize("shape", BOTH)
def test_extended_with_every_option_off_is_k_train_adam_bit_for_bit(shape):
    """5 whole steps (the same batch, so the same gradients, kernel for kernel) from the same p, m, v through
    enable_adam(extended=True) -- eleven launches -- and through the plain enable_adam -- ten: p, m, v and the counter equal
    in every bit, and the extended path reports no clip and no skip"""
    batch = _boards(BATCH[shape], 2)
    out = []
    for extended in (True, False):
        sp = _start(shape, lr=2e-3, warm=3, calm=True, **({"extended": True} if extended else {}))
        assert (sp._optim is not None) == extended and (sp._adam is not None) != extended
        sp.set_batch(*batch)
        for _ in range(5):
            sp.step()
        out.append(_snap(sp))
        if extended:
            st = sp.optim_stats()
            assert st["scale"] == 1.0 and st["skipped"] == 0 and st["clipped"] == 0 and np.isfinite(st["grad_norm"]) and st["grad_norm"] > 0, st
    _same(out[0], out[1], "extended vs plain")
    assert float(out[0][("t",)]) == 5.0
    _, p0 = _plan(shape)
    assert any(not torch.equal(out[0][("p", k)], p0[k]) for k in NAMES)


# ---------------------------------------------------------------- 2. the norm
@pytest.mark.parametrize("shape", BOTH)
def test_gradient_norm_within_its_derived_bound_deterministic_and_needs_no_zeroed_memory(shape):
    """gradients at scales 1e-6 .. 1e2 per tensor: the stored norm within 2 x the bound of the documented summation order
    (a bound below 1e-4 relative: ~1.4e-6 at 128 x 6) of the fp64 norm; the same state run again gives the same bits in the norm and in
    every tensor; and so does a run whose partials buffer was filled with NaN beforehand"""
    runs = []
    for nan_partials in (False, False, True):
        sp = _start(shape, clip_norm=1.0, weight_decay=0.01, ema_decay=0.99)
        _set_grads(sp, 21)
        if nan_partials:
            sp.optim_partials.fill_(float("nan"))
        sp.optim_step()
        snap = _snap(sp)
        snap[("stats",)] = sp.stats.clone()
        runs.append(snap)
    ref = norm_ref(_grads(sp))
    rel = float(ref.e / ref.v)
    print(f"norm bound ({shape}): {rel:.3e} relative; kernel {float(runs[0][('stats',)][0])!r}, fp64 {float(ref.v)!r}")
    assert 0 < rel < 1e-4
    assert abs(float(runs[0][("stats",)][0].double()) - float(ref.v)) <= 2 * float(ref.e)
    _same(runs[0], runs[1], "second run")
    _same(runs[0], runs[2], "NaN-filled partials")
    assert bool(torch.isfinite(sp.optim_partials).all())       # every slot was written, the idle workgroups' included
    blocks = sum((sp.params[k].numel() + 1023) // 1024 for k in NAMES)
    if blocks < 256:
        assert bool((sp.optim_partials[blocks:] == 0).all()) and bool((sp.optim_partials[:blocks] > 0).all())


# ---------------------------------------------------------------- 3. per element
def _check_step(sp, before, t, lr, warm, betas=(0.9, 0.999), eps=1e-8, wd=0.0, clip=0.0, d=None, decay_biases=False, what=""):
    """every element of p, m, v (and the EMA) after one optim_step against optim_ref from the state `before`; the clip scale
    enters as the interval that the fp64 norm and its derived bound give, not as the value the kernel stored"""
    grads = dict(zip(NAMES, _grads(sp)))
    scale = clip_scale_ref(norm_ref(list(grads.values())), clip)
    for k in NAMES:
        r = optim_ref(before[("p", k)].cpu(), before[("m", k)].cpu(), before[("v", k)].cpu(), grads[k], lr, betas[0], betas[1], eps, t, warm,
                      wd=wd if is_weight(k) or decay_biases else 0.0, scale=scale,
                      ema=before[("ema", k)].cpu() if d is not None else None, d=d or 0.0)
        _within(sp.params[k], r["p"], f"{what} p {k}")
        _within(sp.adam_m[k], r["m"], f"{what} m {k}")
        _within(sp.adam_v[k], r["v"], f"{what} v {k}")
        if d is not None:
            _within(sp.ema[k], r["ema"], f"{what} ema {k}")
    return scale


@pytest.mark.parametrize("shape", BOTH)
def test_decay_only_per_element_and_the_biases(shape):
    """wd = 0.1: every element within the reference's bounds; the biases (and their moments) keep the bits of the wd = 0 step,
    the weights do not; with decay_biases the biases decay too (within the reference's bounds with their wd)"""
    lr = 1e-2
    snaps = {}
    for name, opts in (("wd0", dict(extended=True)), ("wd", dict(weight_decay=0.1)), ("wd_b", dict(weight_decay=0.1, decay_biases=True))):
        sp = _start(shape, lr=lr, **opts)
        _set_grads(sp, 31)
        before = _snap(sp)
        sp.optim_step()
        snaps[name] = _snap(sp)
        if name != "wd0":
            _check_step(sp, before, 1, lr, 0, wd=0.1, decay_biases=name == "wd_b", what=name)
    for k in NAMES:
        for part in ("p", "m", "v"):
            same = torch.equal(_bits(snaps["wd"][(part, k)]), _bits(snaps["wd0"][(part, k)]))
            assert same == (part != "p" or not is_weight(k)), (part, k)
        if not is_weight(k):
            assert not torch.equal(snaps["wd_b"][("p", k)], snaps["wd0"][("p", k)]), k


@pytest.mark.parametrize("shape", BOTH)
def test_clip_far_above_the_norm_is_the_unclipped_step_bit_for_bit(shape):
    snaps = []
    for clip in (0.0, 1e4):
        sp = _start(shape, **({"clip_norm": clip} if clip else {"extended": True}))
        _set_grads(sp, 33, size=1e-2)
        sp.optim_step()
        snaps.append(_snap(sp))
        st = sp.optim_stats()
        assert st["scale"] == 1.0 and st["clipped"] == 0 and 0.1 < st["grad_norm"] < 100.0, st
    _same(snaps[0], snaps[1], "clip far above the norm")


@pytest.mark.parametrize("shape", BOTH)
@pytest.mark.parametrize("case", ["clip50", "all_t1", "all_warmup", "all_t1e4", "ema"])
def test_per_element_within_derived_bounds(shape, case):
    """clip with the norm ~50 x max_norm; decay + clip + EMA together at t = 1, inside the warm-up (t = 3 of 5) and at
    t = 10^4 (powf underflows for beta1); the EMA alone at d = 0.999"""
    sp0, _ = _plan(shape)
    lr, done, warm, wd, clip_x, d = {"clip50": (3e-3, 0, 0, 0.0, 50.0, None), "all_t1": (3e-3, 0, 0, 0.05, 50.0, 0.99),
                                     "all_warmup": (1e-2, 2, 5, 0.05, 3.0, 0.99), "all_t1e4": (1e-3, 9999, 100, 0.05, 50.0, 0.99),
                                     "ema": (3e-3, 0, 0, 0.0, 0.0, 0.999)}[case]
    clip = 0.0
    if clip_x:      # max_norm from the fp64 norm of the gradients this case will use
        _set_grads(sp0, 40)
        clip = f32(float(norm_ref(_grads(sp0)).v) / clip_x)
    opts = {k: v for k, v in (("weight_decay", wd), ("clip_norm", clip)) if v}
    if d is not None:
        opts["ema_decay"] = d
    sp = _start(shape, lr=lr, warm=warm, steps_done=done, **opts)
    _set_grads(sp, 40)
    before = _snap(sp)
    sp.optim_step()
    torch.cuda.synchronize()
    assert sp.adam_t == done + 1
    scale = _check_step(sp, before, done + 1, lr, warm, wd=wd, clip=clip, d=d, what=case)
    st = sp.optim_stats()
    if clip_x:
        assert abs(st["scale"] - float(scale.v)) <= 2 * float(scale.e) and st["clipped"] == 1 and abs(float(scale.v) - 1 / clip_x) < 1e-3
    else:
        assert st["scale"] == 1.0 and st["clipped"] == 0
    assert st["skipped"] == 0
    assert any(not torch.equal(sp.params[k].detach(), before[("p", k)]) for k in NAMES)


# ---------------------------------------------------------------- 4. skip
def _where(sp, where):
    k, at = {"tower_w": ("tower_w", sp.params["tower_w"].numel() // 2 + 3), "v2_b": ("v2_b", 0),
             "polfc_w_last": ("polfc_w", 65 * 128 - 1)}[where]
    return sp.params[k].grad.view(-1), at


@pytest.mark.parametrize("shape", BOTH)
@pytest.mark.parametrize("where,bad", [(w, b) for w in ("tower_w", "v2_b", "polfc_w_last") for b in ("nan", "inf", "-inf")] + [("tower_w", "1e20")])
def test_a_non_finite_norm_skips_the_step_and_the_next_one_updates_normally(shape, where, bad):
    """one NaN / +-inf among the gradients -- or one finite 1e20, whose square overflows -- and nothing of p, m, v, ema is
    written, `skipped` and t advance by one; the following step with finite gradients is, bit for bit, the step a plan that
    never skipped takes from the same state at that t"""
    opts = dict(lr=3e-3, warm=4, weight_decay=0.05, clip_norm=1.0, ema_decay=0.99)
    sp = _start(shape, steps_done=1, **opts)
    _set_grads(sp, 50)
    flat, at = _where(sp, where)
    flat[at] = float(bad)
    before = _snap(sp)
    sp.optim_step()
    after = _snap(sp)
    st = sp.optim_stats(reset=False)
    assert float(after.pop(("t",))) == 2.0 and float(before.pop(("t",))) == 1.0
    _same(before, after, "a skipped step wrote something")
    assert st["skipped"] == 1 and st["clipped"] == 0 and st["scale"] == 0.0, st
    assert not np.isfinite(st["grad_norm"])
    _set_grads(sp, 51)
    sp.optim_step()
    nxt = _snap(sp)
    st = sp.optim_stats(reset=False)
    assert st["skipped"] == 1 and st["clipped"] == 1 and 0 < st["scale"] < 1 and float(nxt[("t",)]) == 3.0, st
    twin = _start(shape, steps_done=2, **opts)      # (the same plan, started anew: same p, m, v, ema; t already where the skip left it)
    _set_grads(twin, 51)
    twin.optim_step()
    _same(nxt, _snap(twin), "the step after a skip")
    assert all(not torch.equal(nxt[("p", k)], before[("p", k)]) for k in NAMES)


# ---------------------------------------------------------------- 5. sticky counters
@pytest.mark.parametrize("shape", BOTH)
def test_skipped_and_clipped_accumulate_until_reset(shape):
    sp = _start(shape, clip_norm=1.0)
    for step, kind in enumerate(("small", "big", "small", "nan", "big", "small")):
        _set_grads(sp, 60 + step, scales=(1.0,) * 14, size={"small": 1e-5, "big": 1.0, "nan": 1e-5}[kind])
        if kind == "nan":
            sp.params["stem_b"].grad[7] = float("nan")
        sp.optim_step()
    st = sp.optim_stats(reset=False)
    assert st["clipped"] == 2 and st["skipped"] == 1 and st["scale"] == 1.0 and sp.adam_t == 6, st
    assert sp.optim_stats() == st                      # the resetting read returns the counts it clears
    st = sp.optim_stats()
    assert st["clipped"] == 0 and st["skipped"] == 0 and st["grad_norm"] > 0


# ---------------------------------------------------------------- 6. the captured graph
def test_graphed_step_equals_the_eager_step_bit_for_bit_and_follows_set_lr():
    """GraphedTrainStep with decay, clip and EMA, batch 64: right after the capture (three lr = 0 steps, then reset_adam) the
    parameters are untouched, the EMA equals them bit for bit, t and the sticky counters are 0; four replays -- the rate
    halved by set_lr after the second, with no recapture -- leave p, m, v, ema, t and the statistics of a StepPlan driven
    eagerly from the same state on the same batches"""
    from betazero_amd.net import PolicyValueNet
    from betazero_amd.train import GraphedTrainStep
    from betazero_amd.train_kernels import StepPlan
    torch.manual_seed(3)
    m1 = PolicyValueNet(*SHAPES["small"], fused_tower=True).to(DEV)
    m2 = copy.deepcopy(m1)
    own, opp, pi, z = _boards(256, 7)
    ex = types.SimpleNamespace(own=own, opp=opp, pi=pi, z=z, vt=None)
    lr, opts = 2e-3, dict(weight_decay=1e-2, clip_norm=1.0, ema_decay=0.99)
    g = GraphedTrainStep(m1, lr=lr, batch=64, lr_warmup_steps=2, **opts)
    idxs = [torch.randperm(256, device=DEV, generator=torch.Generator(device=DEV).manual_seed(s))[:64].contiguous() for s in range(4)]
    g.idx.copy_(idxs[0])
    g.step_plan.set_batch(own, opp, pi, z, g.idx)
    g._capture()
    sp = g.step_plan
    torch.cuda.synchronize()
    for (k, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(_bits(a), _bits(b)), k
    for k in NAMES:
        assert torch.equal(_bits(sp.ema[k]), _bits(sp.params[k])), k
        assert float(sp.adam_m[k].abs().max()) == 0.0 and float(sp.adam_v[k].abs().max()) == 0.0
    assert sp.adam_t == 0 and sp.stats.tolist() == [0.0, 0.0, 0.0, 0.0]
    eager = StepPlan(m2, 64)
    eager.enable_adam(lr, warmup_steps=2, **opts)
    graph = g.graph
    for s, idx in enumerate(idxs):
        if s == 2:
            g.set_lr(lr / 2)
            eager.set_lr(lr / 2)
        g(ex, idx)
        eager.set_batch(own, opp, pi, z, idx)
        eager.step()
    assert g.graph is graph and float(sp.hyper[0]) == f32(lr / 2)
    a, b = _snap(sp), _snap(eager)
    a[("stats",)], b[("stats",)] = sp.stats.clone(), eager.stats.clone()
    _same(a, b, "graph vs eager")
    assert sp.adam_t == 4 and g.optim_stats()["skipped"] == 0
    assert all(not torch.equal(sp.ema[k], sp.params[k].detach()) for k in ("tower_w", "polfc_w"))


# ---------------------------------------------------------------- 7. against torch
def test_optim_kernel_equals_torch_adamw_clip_and_ema():
    """6 steps at the small shape against torch.optim.AdamW (two parameter groups) after torch.nn.utils.clip_grad_norm_, and
    an EMA by hand, fed the SAME gradients: every parameter and every averaged weight equal to 1e-5 of an lr-sized step plus
    a few fp32 ulps after each step (test_adam_kernel_equals_torch_adam's tolerance); three of the steps clip"""
    lr, wd, clip, d, warm = 3e-3, 0.05, 1.0, 0.9, 4
    sp, p0 = _plan("small")
    with torch.no_grad():
        for k, p in sp.params.items():
            p.copy_(p0[k])
    sp.enable_adam(lr, warmup_steps=warm, weight_decay=wd, clip_norm=clip, ema_decay=d)
    twin = {k: p0[k].clone().requires_grad_(True) for k in NAMES}
    opt = torch.optim.AdamW([{"params": [twin[k] for k in NAMES if is_weight(k)], "weight_decay": wd},
                             {"params": [twin[k] for k in NAMES if not is_weight(k)], "weight_decay": 0.0}], lr=lr)
    ema = {k: p0[k].clone() for k in NAMES}
    for t in range(1, 7):
        _set_grads(sp, 70 + t, scales=(1.0,) * 14, size=1e-1 if t % 2 else 1e-4)
        sp.optim_step()
        for gr in opt.param_groups:
            gr["lr"] = lr * min(1.0, t / warm)
        for k in NAMES:
            twin[k].grad = sp.params[k].grad.clone()
        torch.nn.utils.clip_grad_norm_(list(twin.values()), clip)
        opt.step()
        for k in NAMES:
            ema[k] += (1.0 - d) * (twin[k].detach() - ema[k])
            for what, a, b in (("p", sp.params[k].detach(), twin[k].detach()), ("ema", sp.ema[k], ema[k])):
                assert float((a - b).abs().max()) <= 1e-5 * lr * t + 5e-7 * float(b.abs().max()), (t, k, what, float((a - b).abs().max()))
    st = sp.optim_stats()
    assert sp.adam_t == 6 and st["clipped"] == 3 and st["skipped"] == 0
    assert max(float((sp.params[k].detach() - p0[k]).abs().max()) for k in NAMES) > 1e-3


# ---------------------------------------------------------------- 8. to the engine
def test_ema_module_reaches_the_engine_and_a_nan_in_it_is_refused():
    """refresh_device_net(dnet, step.ema_module()): DeviceNet.forward (the bf16 path, as the other refresh tests compare) then
    returns, bit for bit, what a net created from the bf16-rounded EMA weights returns -- not the last iterate's; a NaN in
    an EMA tensor raises FloatingPointError and leaves the engine's net alone"""
    from betazero_amd.net import DeviceNet, PolicyValueNet
    from betazero_amd.train import GraphedTrainStep, refresh_device_net
    torch.manual_seed(9)
    module = PolicyValueNet(*SHAPES["small"], fused_tower=True).to(DEV)
    step = GraphedTrainStep(module, lr=1e-2, batch=BATCH["small"], ema_decay=0.9)
    sp = step.step_plan
    dnet = DeviceNet.from_module(copy.deepcopy(module).cpu().round_to_bf16_(), 16)
    for s in range(3):
        _set_grads(sp, 80 + s, scales=(1.0,) * 14)
        sp.optim_step()
    em = step.ema_module()
    for k, p in sp._named(em).items():
        assert torch.equal(_bits(p), _bits(sp.ema[k])) and p.grad is None
        assert not torch.equal(p.detach(), sp.params[k].detach()) and p.data_ptr() != sp.ema[k].data_ptr()
    own, opp, _, _ = _boards(16, 4)
    first = dnet.forward(own, opp)[0].clone()
    refresh_device_net(dnet, em)
    lg, v = (t.clone() for t in dnet.forward(own, opp))
    want = DeviceNet.from_module(copy.deepcopy(em).cpu().round_to_bf16_(), 16)
    wl, wv = want.forward(own, opp)
    assert torch.equal(_bits(lg), _bits(wl)) and torch.equal(_bits(v), _bits(wv))
    last = DeviceNet.from_module(copy.deepcopy(module).cpu().round_to_bf16_(), 16)
    assert not torch.equal(lg, last.forward(own, opp)[0]) and not torch.equal(lg, first)
    sp.ema["pol_b"][1] = float("nan")
    with pytest.raises(FloatingPointError, match="pol.bias"):
        refresh_device_net(dnet, step.ema_module())
    assert torch.equal(_bits(dnet.forward(own, opp)[0]), _bits(lg))
