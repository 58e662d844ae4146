"""fp8 quantisation-aware training on the GPU: the device form of the activation rule against the host's,
k_qat_scales / k_qat_pack against the packing of fake-quantised weights, k_qat_stem / k_qat_fwd bit for bit against
quant.qat_forward on exact-sum fp8 nets (ties, saturation at 28, positive values that round to 0), the training forward
against the engine's fp8 forward, the gradients against autograd through qat_forward, the captured step, and one small closed
loop on net_fp8.  Shapes: 128 channels, 2 and 4 layers, batch 8 (two workgroups) and 64."""
import copy
import ctypes as ct
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_train_numerics import _batch, _eq
from test_net_numerics_cpu import boards, exact_net, flat_params, net_forward_ref, to_module
from test_qat_cpu import act_inputs
from test_train_numerics_cpu import dyadic_pi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C = 128


def _lib():
    from betazero_amd import _lib as m
    return m, m.lib(), torch.cuda.current_stream().cuda_stream


def _bits_eq(got, want, what):
    got, want = got.detach().float().cpu().contiguous(), want.detach().float().cpu().contiguous()
    bad = (got.view(torch.int32) != want.view(torch.int32)) & ~(torch.isnan(got) & torch.isnan(want))
    assert not bool(bad.any()), (what, int(bad.sum()), got[bad][:4].tolist(), want[bad][:4].tolist())


# ---------------------------------------------------------------- 1. the device form of the activation rule
def test_device_activation_rule_equals_the_host_function_bit_for_bit():
    m, L, s = _lib()
    v = act_inputs()
    want = np.array([L.bz_qat_act(float(x)) for x in v], np.float32)
    x = torch.from_numpy(v).to(DEV)
    out = torch.full_like(x, 7.0)
    m.check(L.bz_qat_act_batch(x.data_ptr(), out.data_ptr(), x.numel(), s))
    _bits_eq(out, torch.from_numpy(want), "bz_qat_act_batch vs bz_qat_act")
    assert int(torch.isnan(out).sum()) == int(np.isnan(v).sum()) > 0


# ---------------------------------------------------------------- 2. scales and packing
def _qat_weights(L, seed):
    """random tower / head weights: an all-zero output channel, weights off the bf16 grid (ties among them) and -- after the
    scaling -- off the e4m3 grid (ties among them: the channel's maximum is a power of two and others sit on half steps)"""
    g = torch.Generator().manual_seed(seed)
    W = torch.randn(L, C, C, 3, 3, generator=g) * 0.05
    W[0, 5] = 0.0
    W[L - 1, C - 1] = 0.0
    W[1, 7] = W[1, 7].bfloat16().float()
    W[1, 7, 0, 0, 0] = 0.25                                                    # s = 1024: e4m3 steps at |w| s in [16, 32) are 2
    W[1, 7, 1] = (torch.randint(8, 16, (3, 3), generator=g) * 2 + 1).float() / 1024  # odd integers: e4m3 ties
    ulp = torch.ldexp(torch.ones(()), torch.frexp(W[0, 9])[1] - 8)
    W[0, 9] = W[0, 9].bfloat16().float() + 0.5 * ulp * (torch.rand(C, 3, 3, generator=g) < 0.5)   # bf16 ties
    pol, val = torch.randn(2, C, 1, 1, generator=g) * 0.3, torch.randn(1, C, 1, 1, generator=g) * 0.3
    pol[1, 3] = 0.0
    return W, pol, val


@pytest.mark.parametrize("L", [2, 4])
def test_scales_and_both_fragment_streams_equal_the_packing_of_fake_quantised_weights(L):
    from betazero_amd import quant
    m, Lb, s = _lib()
    W, pol, val = _qat_weights(L, 20 + L)
    Wq = quant.fake_quant_weight(W.view(L * C, -1)).view_as(W)
    assert not torch.equal(Wq, W.bfloat16().float())
    Wd, Wqd, pd, vd = (t.to(DEV).contiguous() for t in (W, Wq, pol, val))
    nb = Lb.bz_train_wf_bytes(C, L)
    bufs = [torch.zeros(nb, dtype=torch.uint8, device=DEV) for _ in range(4)]
    scales, head = torch.full((L * C + 3,), -1.0, device=DEV), torch.full((3, C), -1.0, device=DEV)
    m.check(Lb.bz_train_qat_scales(Wd.data_ptr(), pd.data_ptr(), vd.data_ptr(), C, L, scales.data_ptr(), head.data_ptr(), s))
    m.check(Lb.bz_train_qat_pack_weights(Wd.data_ptr(), scales.data_ptr(), C, L, bufs[0].data_ptr(), bufs[1].data_ptr(), s))
    m.check(Lb.bz_train_pack_weights(Wqd.data_ptr(), C, L, bufs[2].data_ptr(), bufs[3].data_ptr(), s))
    torch.cuda.synchronize()
    assert torch.equal(bufs[0], bufs[2]) and torch.equal(bufs[1], bufs[3]) and bool(bufs[0].any())
    rows = torch.cat([W.view(L * C, -1).bfloat16().float(), F.pad(torch.cat([pol, val]).view(3, C).bfloat16().float(), (0, C * 8))])
    _bits_eq(scales, torch.from_numpy(quant.channel_scale(rows.numpy())), "scales")
    assert float(scales[5]) == 1.0                                             # the all-zero channel
    _bits_eq(head, quant.fake_quant_weight(torch.cat([pol, val]).view(3, C)), "the shadow head rows")


# ---------------------------------------------------------------- 3. / 4. exact-sum nets
def _exact_fp8_net(NB, seed):
    """test_net_numerics_cpu.exact_net's fp8 construction (e4m3 ties, saturation above 28, subnormal codes) plus positive values
    that round to 0 and a tie at the smallest step, in the stem and in tower layer 0 (channels with zero weights)"""
    P = exact_net(C, NB, 64, "fp8", seed)
    P["stem_w"][[3, 4]] = 0.0
    P["stem_b"][3], P["stem_b"][4] = 2.0 ** -14, 3 * 2.0 ** -14              # 16 v = 2^-10 -> 0 (tie to even); 1.5 2^-9 -> 2 2^-9
    P["tw"][0, [6, 7]] = 0.0
    P["tb"][0, 6], P["tb"][0, 7] = 2.0 ** -15, 3 * 2.0 ** -14
    return P


def _mask_words(act_pos):
    """[n, 64, C] bool (stored value > 0) -> the ReLU words k_train_fwd's 16x16x32 epilogue writes: [n / 4, 256 threads, 4];
    thread 64 w + 16 g + c, word 2 a + b, bit 4 u + i <-> position 2 b + (c >> 3), cell 8 u + (c & 7), channel 32 w + 16 a + 4 g + i"""
    n = act_pos.shape[0]
    A = act_pos.view(n // 4, 2, 2, 8, 8, 4, 2, 4, 4)            # blk, b, chi, u, x, w, a, g, i
    A = A.permute(0, 5, 7, 2, 4, 6, 1, 3, 8).reshape(n // 4, 256, 4, 32).long()   # blk, (w, g, chi, x), (a, b), (u, i)
    return (A << torch.arange(32, device=A.device)).sum(-1)


@pytest.mark.parametrize("NB,n", [(1, 8), (2, 64)])
def test_qat_stem_and_tower_forward_bit_for_bit_and_equal_to_the_engines_fp8_forward(NB, n):
    from betazero_amd import quant
    from betazero_amd.net import DeviceNet
    from betazero_amd.train_kernels import StepPlan
    L = 2 * NB
    P = _exact_fp8_net(NB, 31 + NB)
    own, opp = boards(n, seed=5)
    stats, feats = {}, {}
    rl, rv = net_forward_ref(own, opp, {k: v.to(DEV) for k, v in P.items()}, "fp8", stats=stats, feats=feats)   # (asserts every sum exact)
    tot = {k: sum(st[k] for st in stats.values()) for k in ("ties", "sat", "sub", "zero", "neg")}
    assert all(v > 0 for v in tot.values()) and stats[0]["sat"] > 0 and tot["sat"] > stats[0]["sat"], stats   # ties, saturation (tower too)
    m64 = to_module(P)                                                          # fp64, fused tower
    t = lambda a: torch.as_tensor(a.view(np.int64))  # noqa: E731
    with torch.no_grad():
        _, _, want = quant.qat_forward(m64, t(own), t(opp), acts=True)
    want = [a.permute(0, 2, 3, 1).reshape(n, 64, C) for a in want]
    assert bool((want[0][:, :, 3] == 0).all()) and bool((want[0][:, :, 4] == 2.0 ** -12).all())     # rounds to 0 / ties to even
    assert bool((want[1][:, :, 6] == 0).all()) and bool((want[1][:, :, 7] == 2.0 ** -12).all())
    assert float(want[0].max()) == 28.0 and max(float(a.max()) for a in want[1:]) == 28.0       # saturation, stem and tower
    net = to_module(P, torch.float32).to(DEV)
    sp = StepPlan(net, n, fp8_qat=True)
    sp.grads(*_batch(own, opp, dyadic_pi(n, 1), torch.zeros(n)))
    torch.cuda.synchronize()
    masks = sp.masks.view(torch.int32).view(L, n // 4, 256, 4)
    for l in range(L + 1):
        _eq(sp.acts[l], want[l], f"act[{l}]")
        if l:
            got = masks[l - 1].long() & 0xFFFFFFFF
            assert torch.equal(got, _mask_words((want[l] > 0).to(DEV))), f"ReLU words of act[{l}]"
    # the positive pre-activation that rounds to 0 has its bit clear: channel 6 = 32 * 0 + 16 * 0 + 4 * 1 + 2 -> wave 0, g = 1, word 0 / 1, bit 4 u + 2
    w0 = masks[0][:, 16:32, :2].long()
    assert not bool((w0 & 0x44444444).any()) and bool((w0 & 0x88888888).any())
    # the training forward IS the engine's fp8 forward: act[L] equals the fp8 emulation's last activation (the reference the fp8
    # parity tests hold DeviceNet.forward(fp8=True) to), and the engine's logits / values are that reference's
    _eq(sp.acts[L], feats["x"], "act[L] vs the fp8 reference's tower output")
    dn = DeviceNet(C, NB, 64, flat_params(P), n)
    lg, v = dn.forward(t(own).to(DEV), t(opp).to(DEV), fp8=True)
    _eq(lg, rl, "engine fp8 logits vs the reference")
    _eq(v, rv, "engine fp8 values vs the reference")


# ---------------------------------------------------------------- 4b. / 5. random nets
def _random_case(NB, n, seed, hot=False):
    """a random net (test_gpu_train_kernels._net_case's recipe), bf16-rounded so that the engine's copy holds the very same
    parameters; hot: stem biases that put a quarter of the channels above 28, where the fp8 net saturates"""
    from betazero_amd.net import PolicyValueNet
    torch.manual_seed(seed)
    m = PolicyValueNet(C, NB, 64, fused_tower=True)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.normal_(0.0, 0.2)
        m.pol.weight.mul_(3.0); m.val.weight.mul_(3.0); m.polfc.weight.mul_(2.0)
        if hot:
            m.stem.bias[::4] += 40.0
    m.round_to_bf16_()
    rng = np.random.default_rng(seed)
    own, opp = boards(n, seed=seed)
    pi = rng.random((n, 65)).astype(np.float32) ** 4
    pi /= pi.sum(1, keepdims=True)
    z = rng.integers(-1, 2, n).astype(np.int8)
    t = lambda a: torch.as_tensor(a).to(DEV)  # noqa: E731
    return m.to(DEV), t(own.view(np.int64)), t(opp.view(np.int64)), t(pi), t(z)


def _losses_of(logits, v, pi, z):
    ce = -(pi * F.log_softmax(logits, dim=1)).sum(1).mean()
    mse = F.mse_loss(v, z.float())
    return [float(ce + mse), float(ce), float(mse)]


@pytest.mark.parametrize("NB,n", [(1, 8), (2, 64)])
def test_step_losses_are_the_fp8_engines_and_the_plain_steps_are_not(NB, n):
    """CE and MSE of StepPlan(fp8_qat=True).grads() against those of the engine's fp8 logits / values on the same rows, within
    the tolerance of test_gpu_train_kernels' step-vs-reference comparison (rtol 2e-2, atol 2e-3).  On a net with activations
    above 28 the plain step does NOT agree with the fp8 engine to that tolerance -- the QAT step still does."""
    from betazero_amd.net import DeviceNet
    from betazero_amd.train_kernels import StepPlan
    for hot in (False, True):
        m, own, opp, pi, z = _random_case(NB, n, 40 + NB, hot=hot)
        dn = DeviceNet.from_module(m, n)
        lg, v = dn.forward(own, opp, fp8=True)
        want = _losses_of(lg, v, pi, z)
        got = StepPlan(m, n, fp8_qat=True).grads(own, opp, pi, z)[:3].cpu().numpy()
        plain = StepPlan(m, n).grads(own, opp, pi, z)[:3].cpu().numpy()
        print(f"NB={NB} n={n} hot={hot}: engine fp8 {want}, qat step {got.tolist()}, plain step {plain.tolist()}")
        assert np.allclose(got, want, rtol=2e-2, atol=2e-3), (hot, got, want)
        if hot:
            assert not np.allclose(plain, want, rtol=2e-2, atol=2e-3), (plain, want)


@pytest.mark.parametrize("NB,n", [(1, 8), (2, 64)])
def test_gradients_vs_autograd_through_qat_forward(NB, n):
    """every parameter's gradient against torch.autograd through quant.qat_forward (fp32, straight-through), with the
    tolerances of test_whole_step_on_the_kernels_vs_torch_autograd_fp32: cosine > 0.99 (0.97 for the stem), norms within 10 %
    for tensors of 64 elements and more.  The masters receive the gradients; the shadow rows have none."""
    from betazero_amd import quant
    from betazero_amd.train_kernels import StepPlan
    m, own, opp, pi, z = _random_case(NB, n, 50 + NB)
    sp = StepPlan(m, n, fp8_qat=True)
    losses = sp.grads(own, opp, pi, z).clone()
    got = {k: p.grad.clone() for k, p in m.named_parameters()}
    assert all(bool(torch.isfinite(g).all()) for g in got.values()) and sp.qat_head.grad is None and sp.qat_scales.grad is None
    assert float(got["pol.weight"].abs().max()) > 0 and float(got["val.weight"].abs().max()) > 0
    _bits_eq(sp.qat_head, quant.fake_quant_weight(torch.cat([m.pol.weight, m.val.weight]).view(3, C)), "shadow rows")
    for p in m.parameters():
        p.grad = None
    logits, v = quant.qat_forward(m, own, opp)
    ce = -(pi * F.log_softmax(logits, dim=1)).sum(1).mean()
    mse = F.mse_loss(v, z.float())
    (ce + mse).backward()
    assert np.allclose(losses[:3].cpu().numpy(), [float(ce.detach() + mse.detach()), float(ce.detach()), float(mse.detach())], rtol=2e-2, atol=2e-3)
    cos = {k: float(F.cosine_similarity(got[k].flatten(), p.grad.flatten(), dim=0)) for k, p in m.named_parameters() if p.numel() > 1}
    mag = {k: float(got[k].norm() / p.grad.norm().clamp(min=1e-20)) for k, p in m.named_parameters()}
    print("cosine of kernel vs autograd gradients:", {k: round(c, 4) for k, c in cos.items()})
    for k, c in cos.items():
        assert c > (0.97 if k.startswith("stem") else 0.99), (k, c)
    assert all(0.9 < r < 1.1 for k, r in mag.items() if got[k].numel() >= 64), mag


# ---------------------------------------------------------------- 6. the captured step
def _counted(L, counts):
    class Counting:
        def __getattr__(self, name):
            fn = getattr(L, name)
            if not name.startswith("bz_train_"):
                return fn

            def call(*a):
                counts[name] = counts.get(name, 0) + 1
                return fn(*a)
            return call
    return Counting()


def test_graphed_qat_step_equals_eager_steps_and_the_plain_step_is_unchanged(monkeypatch):
    from betazero_amd import _lib as lm
    from betazero_amd.train import GraphedTrainStep
    from betazero_amd.train_kernels import StepPlan
    n = 64
    m1, own, opp, pi, z = _random_case(2, 256, 60)
    m0, m2 = copy.deepcopy(m1), copy.deepcopy(m1)
    ex = types.SimpleNamespace(own=own, opp=opp, pi=pi, z=z, vt=None, fown=None, fopp=None)
    idxs = [torch.randperm(256, device=DEV, generator=torch.Generator(device=DEV).manual_seed(s))[:n].contiguous() for s in range(2)]
    g = GraphedTrainStep(m1, lr=1e-3, batch=n, fp8_qat=True)
    outs = [g(ex, i).clone() for i in idxs]
    sp = StepPlan(m2, n, fp8_qat=True)
    sp.enable_adam(1e-3)
    idx = torch.zeros(n, dtype=torch.int64, device=DEV)
    for k, i in enumerate(idxs):
        idx.copy_(i)
        sp.set_batch(own, opp, pi, z, idx)
        _bits_eq(sp.launch(adam=True)[:3], outs[k], f"losses of step {k}")
    torch.cuda.synchronize()
    for (k, a), b in zip(m1.named_parameters(), m2.parameters()):
        _bits_eq(a, b, k)
        assert not torch.equal(a, dict(m0.named_parameters())[k]), k     # ... and they moved
    # without the option: the launches of the step as it was (9 + nothing new), and their results
    m3, m4, m5 = copy.deepcopy(m2), copy.deepcopy(m2), copy.deepcopy(m2)
    counts = {}
    real = lm.lib()
    monkeypatch.setattr(lm, "_lib", _counted(real, counts))
    plain = StepPlan(m3, n)
    out3 = plain.grads(own, opp, pi, z, idx).clone()
    n_plain, counts_plain = sum(counts.values()) - counts.get("bz_train_ends_sizes", 0), dict(counts)
    counts.clear()
    qat = StepPlan(m5, n, fp8_qat=True)
    qat.grads(own, opp, pi, z, idx)
    n_qat = sum(counts.values()) - counts.get("bz_train_ends_sizes", 0)
    monkeypatch.setattr(lm, "_lib", real)
    launches = lambda c: {k: v for k, v in c.items() if k not in ("bz_train_ends_sizes", "bz_train_positions_per_workgroup", "bz_train_mask_bytes",  # noqa: E731
                                                                  "bz_train_wf_bytes", "bz_train_wgrad_splits", "bz_train_wgrad_bias_rows")}
    assert launches(counts_plain) == {k: 1 for k in ("bz_train_stem_fwd", "bz_train_pack_weights", "bz_train_tower_fwd", "bz_train_heads",
                                                     "bz_train_tower_bwd", "bz_train_wgrad", "bz_train_stem_wgrad", "bz_train_heads_wgrad",
                                                     "bz_train_finish")}, counts_plain
    assert len(launches(counts)) == 10 and n_qat == n_plain + 1
    # the plain step against the same nine entry points called by hand
    L, s = real, torch.cuda.current_stream().cuda_stream
    hand = StepPlan(m4, n)
    hand.set_batch(own, opp, pi, z, idx)
    p, Ly = hand.params, hand.L
    chk = lm.check
    chk(L.bz_train_stem_fwd(hand.batch_desc.data_ptr(), n, p["stem_w"].data_ptr(), p["stem_b"].data_ptr(), C, hand.acts[0].data_ptr(), s))
    chk(L.bz_train_pack_weights(p["tower_w"].data_ptr(), C, Ly, hand.wf_fwd.data_ptr(), hand.wf_bwd.data_ptr(), s))
    chk(L.bz_train_tower_fwd(hand.acts[0].data_ptr(), hand.wf_fwd.data_ptr(), p["tower_b"].data_ptr(), C, Ly, n, hand.acts[1].data_ptr(),
                             hand.masks.data_ptr(), s))
    chk(L.bz_train_heads(hand.acts[Ly].data_ptr(), hand.batch_desc.data_ptr(), n, C, hand.VH, ct.byref(hand._head), hand.gs[Ly].data_ptr(),
                         hand.hv.data_ptr(), hand.dl.data_ptr(), hand.dv1.data_ptr(), hand.heads_partial.data_ptr(), s))
    chk(L.bz_train_tower_bwd(hand.gs[Ly].data_ptr(), hand.wf_bwd.data_ptr(), hand.zeros_c.data_ptr(), hand.masks.data_ptr(), C, Ly, n,
                             hand.gs[0].data_ptr(), s))
    chk(L.bz_train_wgrad(hand.acts[0].data_ptr(), hand.gs[1].data_ptr(), C, Ly, n, hand.splits, hand.partial.data_ptr(),
                         hand.db_partial.data_ptr(), s))
    chk(L.bz_train_stem_wgrad(hand.batch_desc.data_ptr(), hand.acts[0].data_ptr(), hand.gs[0].data_ptr(), n, C, hand.stem_partial.data_ptr(), s))
    chk(L.bz_train_heads_wgrad(hand.hv.data_ptr(), hand.dl.data_ptr(), hand.dv1.data_ptr(), n, hand.VH, hand.heads_w_partial.data_ptr(), s))
    chk(L.bz_train_finish(ct.byref(hand._partials), ct.byref(hand._grads), C, Ly, hand.VH, n, hand.losses.data_ptr(), None, s))
    torch.cuda.synchronize()
    _bits_eq(out3, hand.losses, "the plain step's losses")
    _bits_eq(plain.acts, hand.acts, "acts")
    _bits_eq(plain.gs, hand.gs, "gs")
    for (k, a), b in zip(m3.named_parameters(), m4.parameters()):
        _bits_eq(a.grad, b.grad, f"{k}.grad")
    assert not hasattr(plain, "qat_head") and plain._head.pol_w == m3.pol.weight.data_ptr()


# ---------------------------------------------------------------- 7. one small closed loop
def test_closed_loop_on_the_fp8_net():
    """8 games of net_fp8 self-play at 16 simulations -> 3 quantisation-aware steps -> refresh_device_net -> a second search on
    the refreshed fp8 net, with no error flag; the engine then derives, from the bf16-rounded masters, the very scales and
    weights the training step used (its fp8 forward equals qat_forward of the module to the step-loss tolerance)"""
    from betazero_amd import quant
    from betazero_amd.engine import SelfPlayEngine
    from betazero_amd.net import DeviceNet, PolicyValueNet
    from betazero_amd.train import GraphedTrainStep, refresh_device_net
    torch.manual_seed(7)
    module = PolicyValueNet(C, 1, 64, fused_tower=True)
    dnet = DeviceNet.from_module(module.round_to_bf16_(), 64)
    eng = SelfPlayEngine("reversi", 8, 16, "net_fp8", net=dnet, temp_moves=4, seed=3)
    eng.run_iteration()
    eng.status()
    ex = eng.device_examples()
    assert len(ex) >= 64
    step = GraphedTrainStep(module, lr=1e-3, batch=64, fp8_qat=True)
    gen = torch.Generator(device=DEV).manual_seed(1)
    losses = [step(ex, torch.randint(0, len(ex), (64,), device=DEV, generator=gen)) for _ in range(3)]
    step.check()
    assert bool(torch.isfinite(torch.stack(losses)).all())
    refresh_device_net(dnet, module)
    eng2 = SelfPlayEngine("reversi", 8, 16, "net_fp8", net=dnet, temp_moves=4, seed=4)
    eng2.run_iteration(max_plies=3)
    eng2.status()
    # refresh_device_net is unchanged: the engine rounds the masters to bf16 and derives scales and codes itself -- the rule the
    # step trained against.  Same rows, the module's masters: engine fp8 losses vs qat_forward's.
    own, opp, pi, z = ex.own[:64].contiguous(), ex.opp[:64].contiguous(), ex.pi[:64], ex.z[:64]
    lg, v = dnet.forward(own, opp, fp8=True)
    with torch.no_grad():
        ql, qv = quant.qat_forward(copy.deepcopy(module).round_to_bf16_(), own, opp)
    assert np.allclose(_losses_of(lg, v, pi, z), _losses_of(ql, qv, pi, z), rtol=2e-2, atol=2e-3)
    m, L, s = _lib()
    wq, sc = torch.zeros(C * 9), ct.c_float()
    w0 = module.tower_w[0, 0].detach().cpu().contiguous().view(-1)
    m.check(L.bz_qat_weight_row(w0.data_ptr(), w0.numel(), wq.data_ptr(), ct.byref(sc)))
    wb = w0.bfloat16().float()
    assert sc.value == float(quant.channel_scale(wb.numpy()[None])[0])       # masters -> bf16 -> the engine's scale
