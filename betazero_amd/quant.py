"""fp8 (OCP e4m3fn) fake-quantisation of the policy/value net for the fp8 MFMA path
(BASELINE config 5).  Specification ("fp8 net"):
  * tower conv weights and the two head conv1x1 weights: per OUTPUT CHANNEL power-of-two scale
    s = 2^floor(log2(448 / max|w|)), w_q = e4m3(w * s) (RNE, saturating), effective weight w_q / s;
  * tower activations are stored as e4m3(x * 16) (fixed activation scale 2^4, saturating at 448);
  * stem weights, biases and the FC layers stay as in the bf16 net;
  * ReLU is torch's, IEEE maximum(x, +0): a NaN (weight or activation) passes and is stored as the e4m3fn NaN code, +inf
    saturates to 448 like any value above it, -0 becomes +0.
The engine derives the same scales from the effective weights, so passing the fake-quantised
parameter vector to bz_net_create is all that is needed."""
import numpy as np
import torch


def e4m3_round(x):
    """round float array to the nearest e4m3fn value (RNE, saturate at +-448, subnormal step 2^-9)"""
    x = np.asarray(x, dtype=np.float32)
    a = np.minimum(np.abs(x), np.float32(448.0))
    _, ex = np.frexp(np.maximum(a, np.float32(2.0 ** -20)))
    e = np.maximum(ex - 1, -6)
    step = np.ldexp(np.float32(1.0), e - 3).astype(np.float32)
    q = np.minimum(np.round(a / step) * step, np.float32(448.0)).astype(np.float32)
    return np.where(a == 0, np.float32(0.0), np.copysign(q, x)).astype(np.float32)


def channel_scale(w_rows):
    """power-of-two scale per row so that max|row| * s lands in (224, 448]"""
    m = np.abs(w_rows).reshape(w_rows.shape[0], -1).max(1)
    mant, ex = np.frexp(np.where(m > 0, np.float32(448.0) / np.maximum(m, 1e-30), 1.0).astype(np.float32))
    return np.ldexp(np.float32(1.0), ex - 1).astype(np.float32)


# ---- quantisation-aware training: the same rule as differentiable torch, the reference of the k_qat_* kernels
def e4m3_round_t(x):
    """e4m3_round on a torch tensor (any float dtype; the result is exact in it): RNE, saturating at +-448, a NaN stays a NaN"""
    a = x.abs().clamp(max=448.0)
    _, ex = torch.frexp(torch.where(a > 2.0 ** -20, a, torch.full_like(a, 2.0 ** -20)))
    step = torch.ldexp(torch.ones_like(a), (ex - 1).clamp(min=-6) - 3)
    q = (torch.round(a / step) * step).clamp(max=448.0)          # (torch.round: half to even)
    return torch.where(torch.isnan(x), x, torch.where(a == 0, torch.zeros_like(q), torch.copysign(q, x)))


def channel_scale_t(w_rows):
    """channel_scale for a torch tensor of bf16-rounded rows [rows, ...]: a NaN is skipped by the maximum (as the engine's host
    packing does with fmaxf), m == 0 gives 1"""
    a = w_rows.detach().abs().reshape(w_rows.shape[0], -1).float()
    m = torch.where(torch.isnan(a), torch.zeros_like(a), a).amax(1)
    _, ex = torch.frexp(torch.where(m > 0, 448.0 / m.clamp(min=1e-30), torch.ones_like(m)))
    return torch.ldexp(torch.ones_like(m), ex - 1)


class _FakeQuantWeight(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w):
        wb = w.to(torch.bfloat16).to(w.dtype)
        s = channel_scale_t(wb).to(w.dtype).reshape(-1, *([1] * (w.dim() - 1)))
        return e4m3_round_t(wb * s) / s

    @staticmethod
    def backward(ctx, g):
        return g


def fake_quant_weight(w):
    """w [rows, ...] -> w_q = e4m3(bf16(w) s) / s per row, with the straight-through estimator: d w_q / d w = 1 (the gradient
    with respect to the quantised weight is the master weight's)"""
    return _FakeQuantWeight.apply(w)


class FakeQuantFp8(torch.autograd.Function):
    """the fp8 net's activation store, a = e4m3(16 maximum(v, +0)) / 16 from the fp32 value v (one rounding; a NaN passes, +inf
    becomes 28), with the straight-through estimator: the gradient passes wherever the stored value is > 0 -- so not where a
    positive v rounds to 0, and unmasked where v saturates at 28"""

    @staticmethod
    def forward(ctx, v):
        r = torch.maximum(v.float(), torch.zeros((), dtype=torch.float32, device=v.device)) + 0.0   # (a NaN passes; -0 -> +0)
        a = (e4m3_round_t(16.0 * r) / 16.0).to(v.dtype)
        ctx.save_for_backward(a)
        return a

    @staticmethod
    def backward(ctx, g):
        a, = ctx.saved_tensors
        return g * (a > 0).to(g.dtype)


def qat_forward(module, own, opp, acts=False):
    """PolicyValueNet's forward as the fp8 net computes it (bz_net_forward_fp8), differentiable: tower and head conv1x1
    weights fake-quantised per output channel, the stem's and every tower layer's output through FakeQuantFp8; stem weights,
    biases and the FC layers as they are.  own / opp: int64 tensors holding the uint64 bitboards [n].  Runs in the module's
    dtype (fp32: the reference of StepPlan(fp8_qat=True)'s gradients; fp64 on an exact-sum net gives the same bits).
    acts=True: also the stored activations [act[0] .. act[L]], each [n, C, 8, 8]."""
    import torch.nn.functional as F
    from .train import planes_from_bits
    dt = module.stem.weight.dtype
    x = planes_from_bits(own, opp).to(dt)
    act = FakeQuantFp8.apply
    if module.fused_tower:
        layers = [(module.tower_w[l], module.tower_b[l]) for l in range(2 * module.NB)]
    else:
        layers = [(m.weight, m.bias) for pair in zip(module.c1, module.c2) for m in pair]
    a = act(F.conv2d(x, module.stem.weight, module.stem.bias, padding=1))
    saved = [a]
    for blk in range(module.NB):
        (w1, b1), (w2, b2) = layers[2 * blk], layers[2 * blk + 1]
        h = act(F.conv2d(a, fake_quant_weight(w1), b1, padding=1))
        a = act(F.conv2d(h, fake_quant_weight(w2), b2, padding=1) + a)
        saved += [h, a]
    p = module.polfc(F.relu(F.conv2d(a, fake_quant_weight(module.pol.weight), module.pol.bias)).flatten(1))
    hv = F.relu(F.conv2d(a, fake_quant_weight(module.val.weight), module.val.bias)).flatten(1)
    v = torch.tanh(module.v2(F.relu(module.v1(hv)))).squeeze(-1)
    return (p, v, saved) if acts else (p, v)


@torch.no_grad()
def fake_quantize_fp8_(module):
    """in place: bf16-round everything, then e4m3 fake-quantise the tower / head conv weights"""
    module.round_to_bf16_()
    convs = [c for pair in zip(module.c1, module.c2) for c in pair] + [module.pol, module.val]
    for c in convs:
        w = c.weight.detach().cpu().numpy()
        s = channel_scale(w).reshape(-1, 1, 1, 1)
        c.weight.copy_(torch.from_numpy(e4m3_round(w * s) / s))
    return module
