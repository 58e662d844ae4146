"""The training step under every combination of its five options, on the GPU.  tests/test_step_options_cpu.py
names the options (V value targets, O ownership head, Q fp8 QAT, S per-row symmetry, X extended optimiser) and enumerates the
lattice.  What a combination adds is the plumbing between kernels -- which head kernel runs, which rows the slots point at,
which hyper block the head's Adam reads, the order of the last launches -- so the checks are relations between plans:

1. every edge (T, o) of the lattice, o in {V, O, S, X}: plan(T) fed o's neutral input equals plan(T minus o) bit for bit --
   one grads() and two step()s; and every T with Q equals plan({Q}) in everything plan({Q}) computes.  Each combination is
   thereby joined to {} or {Q}, which the single-option suites hold to references;
2. all five on against the torch statement of the same step, train_step(value_targets=, ownership=, fp8_qat=, sym=), at
   tests/test_gpu_qat.py's tolerances; the head kernels' losses against an fp64 evaluation of the heads on the fake-quantised
   rows (not the masters); the ownership gradient masked by the stored fp8 activation;
3. the skip rules across the trunk / head seam with all five on;
4. the captured graph against eager steps, a saved state loaded into a fresh step, and the launches of one step.

Shapes: the smallest a plan takes -- 128 x 1 blocks, value hidden 64, and 64 x 1, value hidden 24, at batch 8 (two tower
workgroups at 128 channels, half a staging wave); 3 n + 5 rows on the 8 x 8 board, row numbers with repeats, all eight symmetries."""
import copy
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from betazero_amd.examples import DeviceExamples
from test_gpu_qat import _bits_eq, _counted, _exact_fp8_net
from test_gpu_train_optim import _check_step, _grads, _snap
from test_gpu_train_symmetry import _draw, _equal_plans, _examples, _net, _twin
from test_step_options_cpu import OPTIONS, SHAPES, edges, subsets, without
from test_train_optim_cpu import f32, norm_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LR, WARM, OWN_W = 1e-3, 2, 0.5
EXT = dict(weight_decay=1e-2, ema_decay=0.9)       # and clip_norm = half the first step's fp64 gradient norm, so that it clips
LOSS_TOL = dict(rtol=2e-2, atol=2e-3)              # tests/test_gpu_qat.py's, step against torch
_DATA, _Q_ONLY = {}, {}


# ---------------------------------------------------------------- data, nets, plans
def _data(C, seed=0):
    """one data set per width for the whole module (left unchanged: a test that writes into a column clones it first): ex, the
    3 n + 5 rows with vt and ownership targets; idx / sym, the batch; tw, the n rows the host twin transformed"""
    if (C, seed) not in _DATA:
        n = SHAPES[C][3]
        ex = _examples(3 * n + 5, 8, 7 * n + C + seed, vt=True, own=True, payloads=False)
        idx, sym = _draw(len(ex), n, n + C + seed)
        idx[n - 1] = idx[0]                        # (a repeat for certain: the same row under two symmetries)
        assert len(set(sym.tolist())) == 8 and sym[n - 1] != sym[0]
        up = lambda e: DeviceExamples.from_host(e, DEV)  # noqa: E731
        _DATA[(C, seed)] = types.SimpleNamespace(ex=up(ex), tw=up(_twin(ex, idx, sym)), idx=torch.as_tensor(idx).to(DEV),
                                                 sym=torch.as_tensor(sym).to(DEV))
    return _DATA[(C, seed)]


def _pair(C, seed, NB=None):
    """a net of SHAPES[C] (test_gpu_train_symmetry's recipe) and an ownership head whose tanh bends, on the device"""
    from betazero_amd.net import OwnershipHead
    _, nb, VH, _ = SHAPES[C]
    net = _net(C, NB or nb, VH, seed)
    head = OwnershipHead(C).to(DEV)
    with torch.no_grad():
        head.conv.weight.mul_(3.0)
        head.conv.bias.normal_(0.0, 0.2)
    return net, head


def _plan(T, net, head, own_weight=OWN_W, n=None):
    from betazero_amd.train_kernels import StepPlan
    kw = dict(ownership=head, own_weight=own_weight) if "O" in T else {}
    return StepPlan(net, n or SHAPES[net.C][3], value_targets="V" in T, fp8_qat="Q" in T, symmetry="S" in T, **kw)


def _feed(plan, T, d, vt="data", ex=None):
    """set_batch: with S the data set, idx and sym; without it the twin's rows and no idx -- the same rows either way.
    vt: 'data' (the rows' random value targets) or 'z' (the outcome as floats: V's neutral input)"""
    src = (ex or d.ex) if "S" in T else d.tw
    kw = {}
    if "V" in T:
        kw["vt"] = src.vt if vt == "data" else src.z.to(torch.float32)
    if "O" in T:
        kw.update(fown=src.fown, fopp=src.fopp)
    if "S" in T:
        kw.update(idx=d.idx, sym=d.sym)
    plan.set_batch(src.own, src.opp, src.pi, src.z, **kw)


def _clip(plan):
    """half the fp64 norm of the gradients the plan holds: the first step clips"""
    return f32(float(norm_ref(_grads(plan)).v) / 2.0)


def _adam(plan, T, clip=None, on=True):
    if "X" not in T:
        plan.enable_adam(LR, warmup_steps=WARM)
    elif on:
        plan.enable_adam(LR, warmup_steps=WARM, clip_norm=clip, **EXT)
    else:
        plan.enable_adam(LR, warmup_steps=WARM, extended=True)


def _same(a, b, what):
    """the same bits (a NaN equals the NaN of the same pattern; -0 is not +0)"""
    a, b = a.detach().contiguous(), b.detach().contiguous()
    assert a.shape == b.shape and a.dtype == b.dtype, what
    bits = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[a.element_size()]
    bad = a.view(bits) != b.view(bits)
    assert not bool(bad.any()), (what, int(bad.sum()), a[bad][:4].tolist(), b[bad][:4].tolist())


def _same_head(a, b, what, grads=True):
    for k in ("w", "b"):
        _same(a.own_params[k], b.own_params[k], (what, "head", k))
        if grads:
            _same(a.own_params[k].grad, b.own_params[k].grad, (what, "head grad", k))
        if a._own_adam is not None:
            _same(a.own_m[k], b.own_m[k], (what, "head m", k))
            _same(a.own_v[k], b.own_v[k], (what, "head v", k))
    if grads:
        _same(a.own_loss, b.own_loss, (what, "L_own"))


def _equal(a, b, la, lb, what, head):
    """the four losses, the 14 gradients, parameters, both moments and the EMA of two plans, and -- head -- the ownership head's
    w, b, gradients, moments and L_own: the same bits"""
    _same(la, lb, (what, "losses", la.tolist(), lb.tolist()))
    for k in a.NAMES:
        _same(a.params[k].grad, b.params[k].grad, (what, "grad", k))
        _same(a.params[k], b.params[k], (what, "param", k))
        if a.adam_m is not None:
            _same(a.adam_m[k], b.adam_m[k], (what, "m", k))
            _same(a.adam_v[k], b.adam_v[k], (what, "v", k))
        if a.ema is not None and b.ema is not None:
            _same(a.ema[k], b.ema[k], (what, "ema", k))
    if head:
        _same_head(a, b, what)
    if (a.ownership is None) == (b.ownership is None) and (a.ema is None) == (b.ema is None):
        _equal_plans(a, b, what)       # (test_gpu_train_symmetry's statement of the same, by value)


def _moved(plan, net0, what):
    assert all(not torch.equal(plan.params[k].detach(), plan._named(net0)[k].detach()) for k in ("tower_w", "stem_w", "polfc_w", "v1_w")), what


# ---------------------------------------------------------------- 1. the lattice
EDGES = [(C, T, o) for C in (128, 64) for T, o in edges(C)]


def _x_edge(C, T, d):
    """the extended optimiser with every option off is plain Adam over both steps; with decay, clip and EMA on, the first step's
    gradients are plan(T minus X).grads()'s, p, m, v and the EMA lie within optim_ref's bounds from the pre-step state -- and the
    ownership head, where there is one, takes the X-less plan's step bit for bit: plain Adam with the rate, warm-up and t of the
    step's hyper block, although the trunk was clipped and decayed"""
    U, head_on = without(T, "X"), "O" in T
    net, head = _pair(C, 11)
    net0 = copy.deepcopy(net)
    for on in (False, True):
        (n1, h1), (n2, h2) = (copy.deepcopy(net0), copy.deepcopy(head)), (copy.deepcopy(net0), copy.deepcopy(head))
        a, b = _plan(T, n1, h1), _plan(U, n2, h2)
        _feed(a, T, d), _feed(b, U, d)
        lb = b.grads().clone()
        if not on:
            la = a.grads().clone()
            _equal(a, b, la, lb, "grads", head_on)
            _adam(a, T, on=False), _adam(b, U)
            for t in range(2):
                la, lb = a.step().clone(), b.step().clone()
                _equal(a, b, la, lb, f"every option off, step {t}", head_on)
            st = a.optim_stats()
            assert st["scale"] == 1.0 and st["skipped"] == 0 and st["clipped"] == 0 and a.adam_t == 2 == b.adam_t, st
            _moved(a, net0, "every option off")
            continue
        clip = _clip(b)
        grads_b = {k: b.params[k].grad.clone() for k in b.NAMES}
        _adam(a, T, clip), _adam(b, U)
        before = _snap(a)
        la = a.step().clone()
        _same(la, lb, ("the first step's losses", la.tolist(), lb.tolist()))
        for k in a.NAMES:
            _same(a.params[k].grad, grads_b[k], ("the first step's gradient", k))
        scale = _check_step(a, before, 1, LR, WARM, wd=EXT["weight_decay"], clip=clip, d=EXT["ema_decay"], what=f"{T} step 1")
        st = a.optim_stats()
        assert st["clipped"] == 1 and st["skipped"] == 0 and abs(st["scale"] - float(scale.v)) <= 2 * float(scale.e) and a.adam_t == 1, st
        assert abs(float(scale.v) - 0.5) < 1e-3
        if head_on:
            hb = {k: t.detach().clone() for k, t in b.own_params.items()}
            b.step()
            _same_head(a, b, "the head beside a clipped and decayed trunk")
            assert all(not torch.equal(b.own_params[k].detach(), hb[k]) for k in ("w", "b"))
            assert not torch.equal(a.params["tower_w"].detach(), b.params["tower_w"].detach())
        assert a.bad_rows() == 0 and b.bad_rows() == 0


@pytest.mark.parametrize("C,T,o", EDGES, ids=[f"{C}-{T}-minus-{o}" for C, T, o in EDGES])
def test_plan_with_one_option_neutralised_is_the_plan_without_it(C, T, o):
    """S: (idx, sym) on the data set against the twin's rows; V: vt = z as floats against z; O: own_weight = 0 against no head
    (everything the net owns); X: see _x_edge.  Every OTHER option of T keeps its non-neutral setting on both sides: the rows'
    random vt, own_weight 0.5, decay + a clip that clips + EMA + warm-up, random symmetries"""
    d = _data(C)
    if o == "X":
        return _x_edge(C, T, d)
    U = without(T, o)
    net, head = _pair(C, 11)
    net0, net2, head2 = copy.deepcopy(net), copy.deepcopy(net), copy.deepcopy(head)
    a, b = _plan(T, net, head, own_weight=0.0 if o == "O" else OWN_W), _plan(U, net2, head2)
    _feed(a, T, d, vt="z" if o == "V" else "data"), _feed(b, U, d)
    head_on = "O" in U
    la, lb = a.grads().clone(), b.grads().clone()
    _equal(a, b, la, lb, "grads", head_on)
    assert bool(torch.isfinite(la).all()) and float(la[1]) > 0 and float(la[2]) > 0 and float(la[3]) == 0.0, la
    if "O" in T:
        assert float(a.own_loss[0]) > 0.1        # (L_own is reported at own_weight = 0 too)
        if o != "O":
            assert abs(float(la[0]) - (float(la[1]) + float(la[2]) + OWN_W * float(a.own_loss[0]))) < 1e-5 * max(1.0, float(la[0]))
    clip = _clip(a) if "X" in U else None
    _adam(a, T, clip), _adam(b, U, clip)
    for t in range(2):
        la, lb = a.step().clone(), b.step().clone()
        _equal(a, b, la, lb, f"step {t}", head_on)
        assert bool(torch.isfinite(la).all()), (t, la)
    assert a.bad_rows() == 0 and b.bad_rows() == 0 and a.adam_t == 2 == b.adam_t
    _moved(a, net0, "two steps")
    if "X" in U:
        sa, sb = a.optim_stats(reset=False), b.optim_stats(reset=False)
        assert sa == sb and sa["clipped"] >= 1 and sa["skipped"] == 0, (sa, sb)
    if o == "O":       # the head at own_weight = 0 receives no gradient
        assert not bool(a.own_params["w"].grad.any()) and not bool(a.own_params["b"].grad.any())


def _q_only(d):
    """plan({Q}) on the twin's rows, once: what tests/test_gpu_qat.py pins to quant.qat_forward and the engine's fp8 forward"""
    if not _Q_ONLY:
        net, head = _pair(128, 11)
        q = _plan("Q", net, head)
        _feed(q, "Q", d)
        losses = q.grads().clone()
        _Q_ONLY.update(acts=q.acts.clone(), masks=q.masks.clone(), scales=q.qat_scales.clone(), head=q.qat_head.clone(), losses=losses)
        assert bool(q.masks.any()) and float(q.acts[q.L].float().abs().max()) > 0 and bool(torch.isfinite(losses).all())
    return _Q_ONLY


def _equals_q_only(a, losses, ref, what, mse):
    _same(a.acts, ref["acts"], (what, "acts[0..L]"))
    _same(a.masks, ref["masks"], (what, "the ReLU words"))
    _same(a.qat_scales, ref["scales"], (what, "qat_scales"))
    _same(a.qat_head, ref["head"], (what, "qat_head"))
    _same(losses[1], ref["losses"][1], (what, "CE"))
    if mse:
        _same(losses[2], ref["losses"][2], (what, "MSE"))
    assert a._head.pol_w == a.qat_head.data_ptr() and a._head.val_w == a.qat_head[2].data_ptr()


@pytest.mark.parametrize("T", [T for T in subsets(128) if "Q" in T and T != "Q"])
def test_every_plan_with_qat_computes_what_the_qat_only_plan_computes(T):
    """Q has no neutral input; instead acts[0..L], the ReLU words, the scales, the shadow head rows and CE of plan(T) equal
    plan({Q})'s on the same rows (with S: the staged rows are the twin's), and MSE where the value target is z (V off, or vt = z).
    The same holds for the forward of a whole step() under T's optimiser, which runs on the weights before the update"""
    d = _data(128)
    ref = _q_only(d)
    net, head = _pair(128, 11)
    a = _plan(T, net, head)
    _feed(a, T, d)
    _equals_q_only(a, a.grads().clone(), ref, "grads", mse="V" not in T)
    if "V" in T:
        _feed(a, T, d, vt="z")
        _equals_q_only(a, a.grads().clone(), ref, "grads, vt = z", mse=True)
        _feed(a, T, d)
    _adam(a, T, _clip(a) if "X" in T else None)
    _equals_q_only(a, a.step().clone(), ref, "step", mse="V" not in T)     # (the forward runs on the weights before the update)
    assert a.bad_rows() == 0


# ---------------------------------------------------------------- 2. all five on against the torch definition
def _heads_f64(net, rows, x, pi, target):
    """CE and MSE of the heads on act[L] = x [n, 64, C] in fp64, with `rows` [3, C] as the policy / value conv1x1 weights"""
    m = copy.deepcopy(net).double()
    n, C = x.shape[0], x.shape[2]
    with torch.no_grad():
        m.pol.weight.copy_(rows[:2].double().view(2, C, 1, 1))
        m.val.weight.copy_(rows[2:].double().view(1, C, 1, 1))
        a = x.double().view(n, 8, 8, C).permute(0, 3, 1, 2)
        logits = m.polfc(F.relu(m.pol(a)).flatten(1))
        v = torch.tanh(m.v2(F.relu(m.v1(F.relu(m.val(a)).flatten(1))))).squeeze(-1)
        return float(-(pi.double() * F.log_softmax(logits, dim=1)).sum(1).mean()), float(F.mse_loss(v, target.double()))


@pytest.mark.parametrize("T", ["Q", "VQ", "OQ", "VOQ", OPTIONS])
def test_each_head_kernel_under_qat_reads_the_fake_quantised_rows(T):
    """CE and MSE of the four head kernels (plain, _vt, _own, _own_vt) on a QAT plan against an fp64 evaluation of the heads on
    the stored act[L] with the fake-quantised policy / value rows, at the tolerance tests/test_gpu_train_ownership.py holds the
    head kernels' losses to (rtol 2e-5, atol 1e-6).  The masters are the e4m3 grid values times 1.02 -- inside the rounding
    interval of the same grid value (half a step is at least 3.1 %, bf16 adds 0.4 %), all off it to the same side -- so the
    same evaluation with the masters lies well over two tolerances away: a head kernel handed the masters, itself within one
    tolerance of that, would fail in CE (pol_w) and in MSE (val_w)"""
    from betazero_amd import quant
    d = _data(128)
    net, head = _pair(128, 11)
    with torch.no_grad():
        for conv in (net.pol, net.val):
            conv.weight.copy_(quant.fake_quant_weight(conv.weight.view(-1, 128)).view_as(conv.weight) * 1.02)
    a = _plan(T, net, head)
    _feed(a, T, d)
    losses = a.grads().clone().cpu().numpy()
    masters = torch.cat([net.pol.weight, net.val.weight]).detach().view(3, 128)
    _bits_eq(a.qat_head, quant.fake_quant_weight(masters), "shadow rows")
    target = d.tw.vt if "V" in T else d.tw.z
    want = _heads_f64(net, a.qat_head, a.acts[a.L], d.tw.pi, target)
    off = _heads_f64(net, masters, a.acts[a.L], d.tw.pi, target)
    print(f"{T}: kernel CE / MSE {losses[1]!r} {losses[2]!r}; fp64 on the shadow rows {want}; on the masters {off}")
    for k in (0, 1):
        tol = 2e-5 * abs(want[k]) + 1e-6
        assert abs(float(losses[1 + k]) - want[k]) <= tol, (k, losses, want)
        assert abs(off[k] - want[k]) > 2 * tol, (k, off, want)
    assert not torch.equal(a.qat_head, masters) and float((a.qat_head * 1.02 - masters).abs().max()) < 2.0 ** -7 * float(masters.abs().max())


@pytest.mark.parametrize("NB,n", [(1, 8), (1, 64), (2, 8), (2, 64)])
def test_all_five_on_against_train_step_through_autograd(NB, n):
    """StepPlan with V, O, Q, S on (.grads(): the optimiser takes no part) against train_step(value_targets=True, ownership=head,
    own_weight=0.5, fp8_qat=True, sym=) with an optimiser that moves nothing -- fp32 autograd through quant.qat_forward, the head
    on its last stored activation, the rows through torch_sym_rows.  tests/test_gpu_qat.py's tolerances, unchanged: four losses
    rtol 2e-2 / atol 2e-3; every gradient, the head's included, cosine > 0.99 (0.97 for the stem); norms within 10 % for tensors
    of 64 elements and more.  The measured cosines and loss differences are printed (DESIGN.md 12.6 records them)"""
    from betazero_amd.train import train_step
    net, head = _pair(128, 20 + NB, NB=NB)
    net2, head2 = copy.deepcopy(net), copy.deepcopy(head)
    rows = 3 * n + 5
    ex = DeviceExamples.from_host(_examples(rows, 8, 9 * n + NB, vt=True, own=True, payloads=False), DEV)
    idx, sym = (torch.as_tensor(t).to(DEV) for t in _draw(rows, n, n + NB))
    sp = _plan("VOQS", net, head, n=n)
    losses = sp.grads(ex.own, ex.opp, ex.pi, ex.z, idx, vt=ex.vt, fown=ex.fown, fopp=ex.fopp, sym=sym).clone()
    got = {k: p.grad.clone() for k, p in net.named_parameters()}
    got.update({"own." + k: p.grad.clone() for k, p in head.named_parameters()})
    assert sp.bad_rows() == 0 and all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in got.values())
    for p in list(net2.parameters()) + list(head2.parameters()):
        p.grad = None
    params = list(net2.parameters()) + list(head2.parameters())
    want_l = torch.stack(train_step(net2, torch.optim.SGD(params, lr=0.0), ex, idx, value_targets=True, ownership=head2, own_weight=OWN_W,
                                    fp8_qat=True, sym=sym)).cpu().numpy()
    want = {k: p.grad for k, p in net2.named_parameters()}
    want.update({"own." + k: p.grad for k, p in head2.named_parameters()})
    four = np.concatenate([losses[:3].cpu().numpy(), sp.own_loss.cpu().numpy()])
    cos = {k: float(F.cosine_similarity(got[k].flatten(), want[k].flatten(), dim=0)) for k in got if got[k].numel() > 1}
    mag = {k: float(got[k].norm() / want[k].norm().clamp(min=1e-20)) for k in got}
    print(f"NB={NB} n={n}: losses kernel {four.tolist()} torch {want_l.tolist()} max |d| {float(np.abs(four - want_l).max()):.2e}")
    print("cosines:", {k: round(c, 5) for k, c in cos.items()}, "smallest", min(cos.values()))
    assert np.allclose(four, want_l, **LOSS_TOL), (four, want_l)
    assert float(want_l[3]) > 0.1 and abs(four[0] - (four[1] + four[2] + OWN_W * four[3])) < 1e-5 * max(1.0, abs(four[0]))
    for k, c in cos.items():
        assert c > (0.97 if k.startswith("stem") else 0.99), (k, c)
    assert all(0.9 < r < 1.1 for k, r in mag.items() if got[k].numel() >= 64), mag
    assert set(cos) >= {"own.conv.weight", "tower_w", "pol.weight", "val.weight"}


def test_ownership_gradient_under_qat_is_masked_by_the_stored_activation():
    """the one thing only Q x O can get wrong.  On test_gpu_qat's exact fp8 net channel 6 of tower layer 1 holds positive
    pre-activations that round to 0 in fp8.  That net has almost no weight leaving the channel, so every output channel of
    layer 2 is given one (the row's own maximum at the centre tap: on the e4m3 grid, the row's scale unchanged -- and the
    forward unchanged, the channel's stored value being 0).  With the ownership head on and own_weight > 0 the gradient that
    arrives at the channel -- backward-data of the kernel's own g[L] through those weights, taken on the host -- is not zero,
    and g at that layer is: the stored value decides, not the pre-activation.  At the top, where the head's own term enters,
    g[L] is zero wherever the stored act[L] is"""
    from betazero_amd.net import OwnershipHead
    from test_gpu_train_numerics import _batch
    from test_gpu_train_ownership import _targets
    from test_net_numerics_cpu import boards, to_module
    from test_train_numerics_cpu import dyadic_pi
    n = 8
    net = to_module(_exact_fp8_net(1, 32), torch.float32).to(DEV)
    with torch.no_grad():
        top = net.tower_w[1].abs().amax((1, 2, 3))
        net.tower_w[1][:, 6, 1, 1] = torch.where(top > 0, top, torch.ones_like(top))
    torch.manual_seed(4)
    head = OwnershipHead(128).to(DEV)
    with torch.no_grad():
        head.conv.weight.mul_(3.0)
    own, opp = boards(n, seed=5)
    fown, fopp = _targets(n, 9)
    sp = _plan("OQ", net, head)
    plain = _plan("Q", copy.deepcopy(net), None)
    batch = _batch(own, opp, dyadic_pi(n, 1), torch.zeros(n))
    sp.grads(*batch, fown=fown, fopp=fopp)
    plain.grads(*batch)
    torch.cuda.synchronize()
    L, act, g = sp.L, sp.acts.float(), sp.gs.float()
    _same(sp.acts, plain.acts, "the head does not touch the forward")
    assert L == 2 and bool((act[1][:, :, 6] == 0).all()) and bool((act[1][:, :, 7] == 2.0 ** -12).all())
    nchw = lambda t: t.double().view(n, 8, 8, 128).permute(0, 3, 1, 2)  # noqa: E731
    arriving = F.conv_transpose2d(nchw(g[L]), net.tower_w[1].detach().double(), padding=1)     # before layer 1's mask
    assert float(arriving[:, 6].abs().max()) > 1e-4, "nothing arrives at channel 6: the mask would not show"
    assert not bool(g[1][:, :, 6].any()), "a gradient passed where the stored activation is 0"
    assert float(net.tower_b.grad[0, 6]) == 0.0 and bool(g[1].any()) and not bool(g[1][act[1] == 0].any())
    assert not bool(g[L][act[L] == 0].any()) and bool((act[L] == 0).any()) and bool(g[L].any())
    assert not torch.equal(sp.gs[L], plain.gs[L]) and float(sp.own_loss[0]) > 0      # the head's term is in g[L]
    assert bool(head.conv.weight.grad.any())


# ---------------------------------------------------------------- 3. skip and clip across the trunk / head seam
def _all_on(d, seed=11, net=None, head=None, ex=None):
    """the all-on plan with decay, a clip at half the first gradient's norm, EMA and warm-up: (plan, net, head, clip)"""
    if net is None:
        net, head = _pair(128, seed)
    a = _plan(OPTIONS, net, head)
    _feed(a, OPTIONS, d, ex=ex)
    return a, net, head


def _copy_state(dst, src, skip=("stats",)):
    """everything a step reads from one replay to the next but the sticky statistics, copied in place"""
    with torch.no_grad():
        for k, t in src._state_tensors().items():
            if k not in skip:
                dst._state_tensors()[k].copy_(t)


def _same_states(a, b, what, skip=("stats",)):
    ta, tb = a._state_tensors(), b._state_tensors()
    assert set(ta) == set(tb)
    for k in ta:
        if k not in skip:
            _same(ta[k], tb[k], (what, k))


def _never_skipped(a, net, head, d, clip):
    """an all-on plan that has run no step, holding a's state (the parameters, moments, EMA, hyper block, the head's) on copies"""
    c, _, _ = _all_on(d, net=copy.deepcopy(net), head=copy.deepcopy(head))
    _adam(c, OPTIONS, clip)
    _copy_state(c, a)
    return c


def _trunk(plan):
    s = _snap(plan)
    t = float(s.pop(("t",)))
    return s, t


def _bits_of(d):
    return {k: t.detach().clone() for k, t in d.items()}


def test_all_on_a_non_finite_trunk_skips_the_trunk_and_the_head_follows_its_own_rule():
    """a NaN in one pi row (staged under its symmetry): the trunk's p, m, v and EMA keep their bits, skipped = 1, t advances;
    the head's C + 1 gradients do not see pi and are finite, so the head takes the step an X-less plan's head takes from the
    same state at that t, bit for bit; the next, finite step is the step of a plan that never skipped"""
    d = _data(128)
    a, net, head = _all_on(d)
    a.grads()
    clip = _clip(a)
    _adam(a, OPTIONS, clip)
    a.step()                                          # one clean step: moments, t = 1
    bad = copy.copy(d.ex)
    bad.pi = d.ex.pi.clone()
    bad.pi[int(d.idx[3]), 5] = float("nan")
    _feed(a, OPTIONS, d, ex=bad)
    U = without(OPTIONS, "X")
    b = _plan(U, copy.deepcopy(net), copy.deepcopy(head))       # the X-less plan: the same net and head, the head's moments, t = 1
    _feed(b, U, d, ex=bad)
    _adam(b, U)
    b.reset_adam(steps_done=1)
    for k in ("w", "b"):
        b.own_m[k].copy_(a.own_m[k]), b.own_v[k].copy_(a.own_v[k])
    before, t0 = _trunk(a)
    hbefore = _bits_of(a.own_params)
    la = a.step().clone()
    b.step()
    after, t1 = _trunk(a)
    st = a.optim_stats(reset=False)
    assert (t0, t1) == (1.0, 2.0) and b.adam_t == 2
    for k in before:
        _same(before[k], after[k], ("a skipped step wrote the trunk's", k))
    assert st["skipped"] == 1 and st["scale"] == 0.0 and not np.isfinite(st["grad_norm"]) and not np.isfinite(float(la[0])), st
    finite = all(bool(torch.isfinite(p.grad).all()) for p in a.own_params.values())      # (on the host: the head's own rule)
    assert finite and np.isfinite(float(a.own_loss[0]))
    _same_head(a, b, "the head beside a skipped trunk")
    assert all(not torch.equal(a.own_params[k].detach(), hbefore[k]) for k in ("w", "b"))
    c = _never_skipped(a, net, head, d, clip)
    _feed(a, OPTIONS, d)
    la, lc = a.step().clone(), c.step().clone()
    _same(la, lc, "the losses of the step after the skip")
    _same_states(a, c, "the step after the skip")
    _same_head(a, c, "the step after the skip")
    sa, sc = a.optim_stats(), c.optim_stats()
    assert a.adam_t == 3 and sa["skipped"] == 1 and sc["skipped"] == 0 and (sa["grad_norm"], sa["scale"]) == (sc["grad_norm"], sc["scale"])
    assert bool(torch.isfinite(la).all()) and not torch.equal(after[("p", "tower_w")], a.params["tower_w"].detach())


def test_all_on_a_non_finite_head_leaves_the_head_untouched_and_the_trunk_skips_with_it():
    """the opposite seam.  A NaN in one weight of the head makes its C + 1 gradients non-finite: k_train_own_finish leaves the
    head's w, b and moments as they are.  The trunk does NOT update beside it: the head's term dp3 enters every g[L] of its cell
    ("the skip rule across the two optimisers", case b), so the trunk's norm is not finite either and the
    extended optimiser skips -- nothing moves but t.  With the weight put back, the next step is the step of a plan that never
    skipped"""
    d = _data(128)
    a, net, head = _all_on(d)
    a.grads()
    clip = _clip(a)
    _adam(a, OPTIONS, clip)
    a.step()
    keep = head.conv.weight.detach().clone()
    with torch.no_grad():
        head.conv.weight.view(-1)[11] = float("nan")
    before, t0 = _trunk(a)
    hbefore = {**_bits_of(a.own_params), **{"m" + k: t.clone() for k, t in a.own_m.items()}, **{"v" + k: t.clone() for k, t in a.own_v.items()}}
    la = a.step().clone()
    after, t1 = _trunk(a)
    st = a.optim_stats(reset=False)
    assert (t0, t1) == (1.0, 2.0)
    assert not bool(torch.isfinite(torch.cat([p.grad.flatten() for p in a.own_params.values()])).all())
    for k in ("w", "b"):
        _same(a.own_params[k], hbefore[k], ("the head's", k))
        _same(a.own_m[k], hbefore["m" + k], ("the head's m", k))
        _same(a.own_v[k], hbefore["v" + k], ("the head's v", k))
    for k in before:
        _same(before[k], after[k], ("the trunk's", k))
    assert st["skipped"] == 1 and st["scale"] == 0.0 and not np.isfinite(float(la[0])) and not np.isfinite(float(a.own_loss[0])), st
    with torch.no_grad():
        head.conv.weight.copy_(keep)
    c = _never_skipped(a, net, head, d, clip)
    la, lc = a.step().clone(), c.step().clone()
    _same(la, lc, "the losses of the step after the skip")
    _same_states(a, c, "the step after the skip")
    _same_head(a, c, "the step after the skip")
    assert a.adam_t == 3 and bool(torch.isfinite(la).all()) and a.optim_stats()["skipped"] == 1 and c.optim_stats()["skipped"] == 0
    assert not torch.equal(a.own_params["w"].detach(), keep) and not torch.equal(after[("p", "tower_w")], a.params["tower_w"].detach())


# ---------------------------------------------------------------- 4. the captured graph, the state, the launches
def _graphed(net, head, clip):
    from betazero_amd.train import GraphedTrainStep
    return GraphedTrainStep(net, lr=LR, batch=SHAPES[128][3], lr_warmup_steps=WARM, value_targets=True, ownership=head, own_weight=OWN_W,
                            fp8_qat=True, symmetry=True, clip_norm=clip, **EXT)


def _first_clip(d, net, head):
    """the clip the graphed tests use: half the norm of the first batch's gradients, from an all-on plan on copies"""
    a, _, _ = _all_on(d, net=copy.deepcopy(net), head=copy.deepcopy(head))
    a.grads()
    return _clip(a)


def _batches(sets, k0, k1):
    n = SHAPES[128][3]
    for t in range(k0, k1):
        ex = sets[t >= 2]
        idx, sym = _draw(len(ex), n, 300 + t, shift=t)
        yield t, ex, torch.as_tensor(idx).to(DEV), torch.as_tensor(sym).to(DEV)


def _four(plan, losses):
    return torch.cat([losses[:3], plan.own_loss])


def test_all_on_graphed_step_equals_eager_steps_bit_for_bit():
    """GraphedTrainStep with all five on, batch 8: right after the capture the parameters and the head are untouched, EMA ==
    parameters, moments and t are 0 and both error words (the step's and the staging kernel's) are 0; four replays on new
    (idx, sym) -- the last two on a second data set, the rate halved by set_lr in between, one graph -- equal an eager all-on
    StepPlan driven from the same state in every tensor of _state_tensors(), the four returned values and optim_stats()"""
    d, d2 = _data(128), _data(128, seed=1)
    sets = [d.ex, d2.ex]
    net, head = _pair(128, 14)
    net0, net2, head2 = copy.deepcopy(net), copy.deepcopy(net), copy.deepcopy(head)
    clip = _first_clip(d, net, head)
    g = _graphed(net, head, clip)
    sp = g.step_plan
    g.idx.copy_(d.idx), g.sym.copy_(d.sym)
    sp.set_batch(d.ex.own, d.ex.opp, d.ex.pi, d.ex.z, g.idx, vt=d.ex.vt, fown=d.ex.fown, fopp=d.ex.fopp, sym=g.sym)
    g._capture()
    torch.cuda.synchronize()
    for (k, p), q in list(zip(net.named_parameters(), net2.parameters())) + list(zip(head.named_parameters(), head2.parameters())):
        _same(p, q, ("the capture moved", k))
    for k in sp.NAMES:
        _same(sp.ema[k], sp.params[k], ("ema after the capture", k))
        assert not bool(sp.adam_m[k].any()) and not bool(sp.adam_v[k].any())
    assert all(not bool(t.any()) for m in (sp.own_m, sp.own_v) for t in m.values())
    assert sp.adam_t == 0 and sp.stats.tolist() == [0.0] * 4 and float(sp.losses[3]) == 0.0 and int(sp.sym_stage.bad.sum()) == 0
    eager, _, _ = _all_on(d, net=net2, head=head2)
    _adam(eager, OPTIONS, clip)
    graph = g.graph
    for t, ex, idx, sym in _batches(sets, 0, 4):
        if t == 2:
            g.set_lr(LR / 2), eager.set_lr(LR / 2)
        got = g.step(ex, idx, sym).clone()
        eager.set_batch(ex.own, ex.opp, ex.pi, ex.z, idx, vt=ex.vt, fown=ex.fown, fopp=ex.fopp, sym=sym)
        want = _four(eager, eager.step())
        assert got.shape == (4,) and bool(torch.isfinite(got).all()) and float(got[3]) > 0.1, (t, got)
        _same(got, want, ("the four values of replay", t, got.tolist(), want.tolist()))
        _same_states(sp, eager, f"replay {t}", skip=())
        assert g.optim_stats(reset=False) == eager.optim_stats(reset=False)
    assert g.graph is graph and sp.adam_t == 4 and float(sp.hyper[0]) == f32(LR / 2)
    st = g.optim_stats()
    assert st["skipped"] == 0 and st["clipped"] >= 1, st
    g.check()
    _moved(sp, net0, "four replays")


def test_all_on_state_saved_after_two_replays_continues_in_a_fresh_step():
    """state_dict() after two replays, loaded into a fresh all-on GraphedTrainStep (another net, another head) before its first
    call: both take two more steps and stay bit-identical; the saved state names every optional part"""
    d, d2 = _data(128), _data(128, seed=1)
    sets = [d.ex, d2.ex]
    net, head = _pair(128, 14)
    clip = _first_clip(d, net, head)
    g1 = _graphed(net, head, clip)
    for t, ex, idx, sym in _batches(sets, 0, 2):
        g1.step(ex, idx, sym)
    sd = g1.state_dict()
    desc = g1.step_plan._describe()
    assert {k: sd[k] for k in desc} == desc and all(desc[k] is True for k in ("extended", "has_ema", "has_ownership", "fp8_qat"))
    assert sd["value_targets"] is True and sd["steps_done"] == 2 and sd["hyper"].shape == (8,) and float(sd["hyper"][1]) == 2.0
    assert {"stats", "ema.tower_w", "own.w", "own_m.b", "own_v.w", "adam_v.v2_b", "param.stem_w"} <= set(sd)
    assert (sd["weight_decay"], sd["clip_norm"], sd["ema_decay"]) == (EXT["weight_decay"], clip, EXT["ema_decay"])
    net2, head2 = _pair(128, 15)
    assert not torch.equal(net2.tower_w, net.tower_w)
    g2 = _graphed(net2, head2, clip)
    g2.load_state_dict(sd)
    for t, ex, idx, sym in _batches(sets, 2, 4):
        got, want = g2.step(ex, idx, sym).clone(), g1.step(ex, idx, sym).clone()
        _same(got, want, ("the four values of step", t, got.tolist(), want.tolist()))
        _same_states(g2.step_plan, g1.step_plan, f"step {t}", skip=())
        assert bool(torch.isfinite(got).all())
    assert g1.step_plan.adam_t == 4 == g2.step_plan.adam_t and g2.graph is not None
    assert not torch.equal(sd["param.tower_w"], g1.step_plan.params["tower_w"].detach().cpu())
    g1.check(), g2.check()


def test_all_on_step_is_thirteen_entry_points_fourteen_kernels_in_this_order(monkeypatch):
    """one eager all-on step(): the nine launches of the plain step, with the four k_qat_* entry points in place of stem / pack /
    tower forward (+ 1), the staging kernel in front (+ 1), bz_train_optim_step's two kernels through its one entry point (+ 2)
    and the head's finish behind it (+ 1): 14 kernels through 13 entry-point calls; bz_train_heads_own_vt is the only head
    kernel called"""
    from betazero_amd import _lib as lm
    d = _data(128)
    a, _, _ = _all_on(d)
    a.grads()
    _adam(a, OPTIONS, _clip(a))
    counts, real = {}, lm.lib()
    monkeypatch.setattr(lm, "_lib", _counted(real, counts))
    a.step()
    monkeypatch.setattr(lm, "_lib", real)
    order = ["bz_train_sym_batch", "bz_train_qat_stem_fwd", "bz_train_qat_scales", "bz_train_qat_pack_weights", "bz_train_qat_tower_fwd",
             "bz_train_heads_own_vt", "bz_train_tower_bwd", "bz_train_wgrad", "bz_train_stem_wgrad", "bz_train_heads_wgrad",
             "bz_train_finish", "bz_train_optim_step", "bz_train_own_finish"]
    assert list(counts) == order and set(counts.values()) == {1}, counts
    kernels = sum(2 if k == "bz_train_optim_step" else 1 for k in counts)
    assert kernels == 9 + 1 + 1 + 2 + 1 == 14 and [k for k in counts if "heads" in k and "wgrad" not in k] == ["bz_train_heads_own_vt"]
    assert a.adam_t == 1 and a.bad_rows() == 0
