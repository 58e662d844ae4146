"""fp8 quantisation-aware training, the parts that need no GPU: the rule of csrc/bz_qat.h through its host
entry points (bz_qat_weight_row, bz_qat_act) against quant.py's numpy statement of it and against what the engine's host
packing makes of the same weights; the torch restatement (FakeQuantFp8, qat_forward); the ABI and the refusals.  (The register
budget of the four k_qat_* kernels is in tests/test_kernel_resources.py's table.)"""
import ctypes as ct
import os

import numpy as np
import pytest
import torch

from betazero_amd import _lib, quant

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    ok = (_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))
    assert ok.all(), (what, int((~ok).sum()), got[~ok][:4], want[~ok][:4])


def _bf16(w):
    return torch.from_numpy(np.asarray(w, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def _row(w):
    w = np.ascontiguousarray(w, dtype=np.float32)
    wq, s = np.full_like(w, np.nan), ct.c_float(-1.0)
    _lib.check(_lib.lib().bz_qat_weight_row(w.ctypes.data, w.size, wq.ctypes.data, ct.byref(s)))
    return wq, np.float32(s.value)


def qat_rows():
    """random rows at many magnitudes, then the edge rows: all zero, a single subnormal, the maximum exactly at a power of two,
    values off the bf16 grid (ties of both parities among them), values whose scaled image saturates or ties in e4m3"""
    rng = np.random.default_rng(5)
    rows = [(rng.standard_normal(n) * 10.0 ** rng.integers(-8, 6)).astype(np.float32) for n in (1152, 128) for _ in range(40)]
    rows.append(np.zeros(128, np.float32))
    sub = np.zeros(128, np.float32); sub[7] = 1e-40
    rows.append(sub)
    sub2 = np.zeros(128, np.float32); sub2[3] = 1e-45           # (bf16 rounds it to 0: an all-zero channel after all)
    rows.append(sub2)
    for p in (-20, -1, 0, 3, 8, 9):                              # max |w| = 2^p, others below
        r = (rng.random(128) * 2.0 ** p).astype(np.float32); r[11] = -(2.0 ** p)
        rows.append(r)
    base = _bf16(rng.standard_normal(1152).astype(np.float32))
    ulp = np.ldexp(np.float32(1), np.frexp(base)[1] - 8).astype(np.float32)
    for k in (0.5, -0.5, 0.25, 0.5 * (1 + 2.0 ** -10)):          # bf16 ties, and just off them
        rows.append((base + np.float32(k) * ulp).astype(np.float32))
    # e4m3 ties after scaling: max = 448 / s exactly, others at odd multiples of half an e4m3 step
    r = np.array([448.0, 17.0, 19.0, 9.5, 10.5, 0.0009765625, 0.0029296875, 25.0, 27.0, 417.0, 447.9, 440.0, -232.0, -17.0], np.float32) / np.float32(64)
    rows.append(r)
    rows.append(np.array([1.0e38, 1.0, -0.5e38], np.float32))  # a scale far below 1
    rows.append(np.array([0.0, -0.0, 2.0 ** -126], np.float32))
    return rows


def test_weight_rows_equal_the_numpy_rule_bit_for_bit():
    for i, w in enumerate(qat_rows()):
        wb = _bf16(w)
        s = quant.channel_scale(wb[None])[0]
        want = quant.e4m3_round(wb * s) / s
        got, gs = _row(w)
        assert gs == s, (i, gs, s)
        _same(got, want, f"row {i}")
        _same(quant.fake_quant_weight(torch.from_numpy(w)[None]).numpy()[0], want, f"row {i}, torch")
        _same(_bf16(got), got, f"row {i}: w_q is exact in bf16")


def test_an_all_zero_channel_and_a_nan_weight_behave_as_in_the_host_packing():
    """bz_net.hip's upload_params: the channel maximum is an fmaxf chain (a NaN is skipped), pow2_scale(0) = 1, f2e4m3(NaN) = the
    NaN code"""
    got, s = _row(np.zeros(1152, np.float32))
    assert s == 1.0 and not got.any() and not np.signbit(got).any()
    w = np.array([0.5, np.nan, -3.0, 0.75], np.float32)
    got, s = _row(w)
    assert s == 128.0 and np.isnan(got[1])
    _same(got[[0, 2, 3]], w[[0, 2, 3]], "the finite weights next to a NaN")
    got, s = _row(np.full(4, np.nan, np.float32))
    assert s == 1.0 and np.isnan(got).all()
    t = quant.fake_quant_weight(torch.from_numpy(w)[None]).numpy()[0]
    assert np.isnan(t[1])
    _same(t[[0, 2, 3]], w[[0, 2, 3]], "torch: the finite weights next to a NaN")


def test_weight_rows_equal_fake_quantize_and_the_engines_flat_parameters():
    """the engine derives its e4m3 codes and dequantisation factors from the flat parameter vector; fake_quantize_fp8_ is the
    statement of that packing which the fp8 parity tests hold the engine to (tests/test_gpu_net_numerics.py).  Row by row,
    bz_qat_weight_row of the raw weights gives the fake-quantised module's weights."""
    from betazero_amd.net import PolicyValueNet
    torch.manual_seed(3)
    m = PolicyValueNet(128, 1, 64)
    with torch.no_grad():
        m.c1[0].weight[5] = 0.0
        m.c2[0].weight.mul_(7.3)
    raw = {k: v.detach().clone() for k, v in m.state_dict().items()}
    quant.fake_quantize_fp8_(m)
    for name in ("c1.0.weight", "c2.0.weight", "pol.weight", "val.weight"):
        w, q = raw[name].numpy(), m.state_dict()[name].numpy()
        for co in range(w.shape[0]):
            _same(_row(w[co].reshape(-1))[0], q[co].reshape(-1), f"{name}[{co}]")


def act_inputs():
    """every bf16 bit pattern taken as fp32; every midpoint between neighbouring e4m3 grid values, divided by 16, with its two
    fp32 neighbours; +-0, +inf, NaNs of both signs"""
    v = (np.arange(65536, dtype=np.uint32) << 16).view(np.float32)
    codes = np.arange(0, 0x7F, dtype=np.uint8)                   # the non-negative finite codes 0 .. 448
    e, mnt = (codes >> 3).astype(np.int32), (codes & 7).astype(np.float64)
    grid = np.where(e == 0, mnt * 2.0 ** -9, (1 + mnt / 8) * 2.0 ** (e - 7))
    assert grid[-1] == 448.0 and grid[1] == 2.0 ** -9
    mid = ((grid[:-1] + grid[1:]) / 2 / 16).astype(np.float32)
    assert (mid.astype(np.float64) * 16 * 2 == grid[:-1] + grid[1:]).all()
    extra = np.array([0.0, -0.0, np.inf, -np.inf, 28.0, 29.0, 1e30], np.float32)
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001], np.uint32).view(np.float32)
    return np.concatenate([v, mid, np.nextafter(mid, np.float32(np.inf)), np.nextafter(mid, np.float32(-np.inf)), extra, nans])


def act_want(v):
    with np.errstate(all="ignore"):
        return (quant.e4m3_round(np.float32(16) * np.maximum(v, np.float32(0))) / np.float32(16)).astype(np.float32)


def test_activations_equal_the_numpy_rule_on_every_bf16_pattern_and_every_tie():
    L = _lib.lib()
    v = act_inputs()
    want = act_want(v)
    got = np.array([L.bz_qat_act(float(x)) if x == x else L.bz_qat_act(float("nan")) for x in v], np.float32)
    _same(got, want, "bz_qat_act")
    assert L.bz_qat_act(float("inf")) == 28.0 and L.bz_qat_act(1e30) == 28.0
    assert np.isnan(L.bz_qat_act(float("nan")))
    for z in (0.0, -0.0, -1.0, -float("inf")):
        assert _bits(np.float32(L.bz_qat_act(z)))[()] == 0, z                  # +0, not -0
    assert L.bz_qat_act(2.0 ** -14) == 0.0 and L.bz_qat_act(3 * 2.0 ** -14) == 2 * 2.0 ** -13   # ties go to even
    assert not np.signbit(want[v == 0]).any()
    _same(quant.FakeQuantFp8.apply(torch.from_numpy(v)).numpy(), want, "FakeQuantFp8")


def test_fake_quant_backward_is_the_identity_where_the_output_is_positive():
    v = torch.tensor([-1.0, 0.0, 2.0 ** -14, 3 * 2.0 ** -14, 0.3, 27.9, 28.0, 1000.0, float("inf")], requires_grad=True)
    a = quant.FakeQuantFp8.apply(v)
    g = torch.arange(1.0, 10.0)
    a.backward(g)
    want = torch.where(a > 0, g, torch.zeros_like(g))
    assert torch.equal(v.grad, want)
    assert v.grad.tolist() == [0.0, 0.0, 0.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0]     # rounds to 0: masked; saturated at 28: not masked
    w = torch.randn(4, 8, requires_grad=True)
    gw = torch.randn(4, 8)
    quant.fake_quant_weight(w).backward(gw)
    assert torch.equal(w.grad, gw)                                               # weights: straight through


def test_qat_forward_of_a_quantised_net_with_activations_on_the_grid_is_the_plain_forward():
    """a fake-quantised net whose every activation is a small integer, on the e4m3 / 16 grid: the fake quantisation changes nothing,
    so qat_forward is PolicyValueNet.forward (fp64: exact sums on both sides)"""
    from betazero_amd.net import PolicyValueNet
    g = torch.Generator().manual_seed(2)
    m = PolicyValueNet(128, 1, 64).double()
    with torch.no_grad():
        sw = torch.zeros(128, 18, dtype=torch.float64)          # one tap of one plane per channel: integer sums
        sw[torch.arange(128), torch.randint(0, 18, (128,), generator=g)] = 1.0
        m.stem.weight.copy_(sw.view(128, 2, 3, 3))
        m.stem.bias.copy_(torch.randint(0, 3, (128,), generator=g).double())
        for c in (m.c1[0], m.c2[0]):                            # one +-1 per output channel: integers up to 8 (every integer
            w = torch.zeros_like(c.weight)                      # up to 16 is an e4m3 value / 16)
            idx = torch.randint(0, 128 * 9, (128,), generator=g)
            w.view(128, -1)[torch.arange(128), idx] = torch.where(torch.rand(128, generator=g) < 0.5, 1.0, -1.0).double()
            c.weight.copy_(w)
            c.bias.copy_(torch.randint(-1, 2, (128,), generator=g).double())
    quant.fake_quantize_fp8_(m)
    own = torch.randint(-2 ** 63, 2 ** 63 - 1, (6,), generator=g, dtype=torch.int64)
    opp = torch.randint(-2 ** 63, 2 ** 63 - 1, (6,), generator=g, dtype=torch.int64) & ~own
    from betazero_amd.train import planes_from_bits
    with torch.no_grad():
        lg, v, acts = quant.qat_forward(m, own, opp, acts=True)
        pl, pv, trunk = m(planes_from_bits(own, opp).double(), trunk=True)
    for a in acts:     # on the grid, below saturation, and not all zero
        assert float(a.max()) < 28 and float(a.max()) > 0 and torch.equal(quant.e4m3_round_t(16 * a) / 16, a)
    assert torch.equal(acts[-1], trunk) and torch.equal(lg, pl) and torch.equal(v, pv)


def test_abi_symbols_and_refusals():
    from betazero_amd.net import PolicyValueNet
    from betazero_amd.train import GraphedTrainStep, train_step
    from betazero_amd.train_kernels import StepPlan
    L = _lib.lib()
    assert L.bz_abi_version() == 7 and _lib.ABI_VERSION == 7
    sigs = {"bz_qat_weight_row": 4, "bz_qat_act": 1, "bz_qat_act_batch": 4, "bz_train_qat_scales": 8, "bz_train_qat_pack_weights": 7,
            "bz_train_qat_tower_fwd": 9, "bz_train_qat_stem_fwd": 7}
    hdr = open(os.path.join(ROOT, "include", "bz_abi.h")).read()
    for name, nargs in sigs.items():
        assert name in _lib.ABI_SYMBOLS and len(getattr(L, name).argtypes) == nargs and f" {name}(" in hdr, name
    # the library refuses other channel counts itself (BZ_EINVAL, before it looks for a device)
    one = ct.c_void_p(256)
    for rc in (L.bz_train_qat_scales(one, one, one, 64, 2, one, one, None), L.bz_train_qat_pack_weights(one, one, 64, 2, one, one, None),
               L.bz_train_qat_tower_fwd(one, one, one, 64, 2, 8, one, one, None), L.bz_train_qat_stem_fwd(one, 8, one, one, 64, one, None)):
        assert rc == _lib.BZ_EINVAL and "C == 128" in _lib.last_error()
    m64 = PolicyValueNet(64, 1, 64, fused_tower=True)
    with pytest.raises(ValueError, match="128 channels"):
        StepPlan(m64, 8, fp8_qat=True)
    with pytest.raises(ValueError, match="128 channels"):
        GraphedTrainStep(m64, batch=8, fp8_qat=True)
    with pytest.raises(ValueError, match="128 channels"):
        train_step(m64, None, None, fp8_qat=True)
    stock, fused = PolicyValueNet(128, 1, 64), PolicyValueNet(128, 1, 64, fused_tower=True)
    for mod, kw in ((stock, {}), (fused, {"step_kernels": False}), (fused, {"autocast": False}), (fused, {"tower_kernels": False, "step_kernels": False})):
        with pytest.raises(ValueError, match="all-kernel step"):
            GraphedTrainStep(mod, batch=8, device="cpu", fp8_qat=True, **kw)


def test_qat_forward_equals_the_fp8_reference_on_an_exact_net():
    """on test_net_numerics_cpu's exact fp8 net (ties, saturation, subnormal codes) qat_forward in fp64 gives the tower output
    and the logits of net_forward_ref's fp8 mode -- the emulation the engine's fp8 forward is pinned to -- bit for bit"""
    from test_net_numerics_cpu import boards, exact_net, net_forward_ref, to_module
    P = exact_net(128, 1, 64, "fp8", 32)
    own, opp = boards(8, seed=5)
    feats = {}
    rl, _ = net_forward_ref(own, opp, P, "fp8", feats=feats)
    with torch.no_grad():
        lg, _, acts = quant.qat_forward(to_module(P), torch.as_tensor(own.view(np.int64)), torch.as_tensor(opp.view(np.int64)), acts=True)
    assert torch.equal(acts[-1].permute(0, 2, 3, 1).reshape(8, 64, 128), feats["x"]) and torch.equal(lg, rl)
    assert float(acts[0].max()) == 28.0
