"""The reference that tests/test_gpu_train_optim.py holds the extended optimiser to (bz_train_optim_step: k_train_gnorm and
k_train_optim of csrc/bz_train_ends.hip), built from the bounded arithmetic of test_train_numerics_cpu.py, and
what of the feature can be checked without a GPU: the reference's value track against torch.optim.AdamW (two parameter
groups) + torch.nn.utils.clip_grad_norm_ + a hand-written EMA in fp64, the struct against the header, every refusal of the
entry points, and GraphedTrainStep's refusal of the options without the fused optimiser."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from test_train_numerics_cpu import ETA, B, adam_ref, fma, sum_rounding

# the kernels' job order (k_train_adam's) and which tensors are weights
NAMES = ("tower_w", "tower_b", "stem_w", "stem_b", "pol_w", "pol_b", "polfc_w", "polfc_b", "val_w", "val_b", "v1_w", "v1_b", "v2_w", "v2_b")
GNORM_GROUPS = 256      # k_train_gnorm's fixed grid = bz_train_optim_partials()


def f32(x):
    return float(np.float32(x))


def counts(C_, L, VH):
    """elements of every job of a (channels, conv layers, value hidden) net, in job order"""
    return dict(zip(NAMES, (L * C_ * C_ * 9, L * C_, C_ * 18, C_, 2 * C_, 2, 65 * 128, 65, C_, 1, VH * 64, VH, VH, 1)))


def norm_depth(sizes):
    """the longest chain of fp32 roundings a term of the norm's sum goes through: a thread's fmaf chain of 4 elements per
    1024-element block over ceil(blocks / 256) trips, the 8 levels of the workgroup's LDS tree, the 8 levels of the tree
    over the 256 partials"""
    blocks = sum((n + 1023) // 1024 for n in sizes)
    trips = (blocks + GNORM_GROUPS - 1) // GNORM_GROUPS
    return 4 * trips + 8 + 8


def norm_ref(grads):
    """sqrtf of the fixed-order fp32 sum of g^2 over `grads` (tensors in job order), as a B: every term is non-negative and
    passes through at most norm_depth roundings, so the sum is within gamma_depth Sigma g^2 (+ one subnormal step per
    element: squares below 2^-126) of the fp64 one; one more rounding for the square root"""
    g = [torch.as_tensor(t, dtype=torch.float64).reshape(-1) for t in grads]
    S = sum((t * t).sum() for t in g)
    depth, n = norm_depth([t.numel() for t in g]), sum(t.numel() for t in g)
    e = sum_rounding(S, torch.tensor(1.0, dtype=torch.float64), 0.0, depth + 1) + n * ETA   # (esum != 0: no exactness claimed)
    return B(S, e).sqrt()


def clip_scale_ref(norm, max_norm):
    """fminf(1, max_norm / (norm + 1e-6f)) from a bounded norm (torch.nn.utils.clip_grad_norm_'s rule); exactly 1 where the
    whole interval of the quotient lies above 1, and without a clip"""
    if not max_norm > 0:
        return B(1.0)
    q = B(f32(max_norm)) / (norm + B(f32(1e-6)))
    if float(q.v - q.e) >= 1.0:
        return B(1.0)
    assert float(q.v + q.e) < 1.0, "the clip decision is not determined at this norm: choose another case"
    return q


def optim_ref(p, m, v, g, lr, b1, b2, eps, t, warm, wd=0.0, scale=None, ema=None, d=0.0):
    """one update of k_train_optim's documented formula with bounds (adam_ref's operations, plus): g' = g scale;
    p' = p (1 - lr_t wd) - (lr_t / bc1) m' / (sqrtf(v') bc2_rsqrt + eps); ema' = fmaf(1 - d, p' - ema, ema).  scale: a B (an
    interval, clip_scale_ref) or None for 1; wd: this tensor's decay (0 for a bias without decay_biases)."""
    f = f32
    b1, b2, eps, lr, wd, d = f(b1), f(b2), f(eps), f(lr), f(wd), f(d)
    c1, c2 = 1.0 - b1, 1.0 - b2                    # exact in fp32 (Sterbenz: beta in [0.5, 1])
    g, m, v, p = (torch.as_tensor(a, dtype=torch.float64) for a in (g, m, v, p))
    gs = B(g) * (scale if scale is not None else B(1.0))
    mn = fma(b1, B(m), B(c1) * gs)
    vn = fma(b2, B(v), (B(c2) * gs) * gs)
    lr_t = B(lr) * B.rnd(torch.tensor(min(1.0, t / warm)), torch.tensor(0.0)) if warm > 0 else B(lr)

    def pow_(b):
        x = torch.tensor(b, dtype=torch.float64) ** t
        return B(x, 2 * 4 * 2.0 ** -24 * x)        # powf: 4 ulps
    bc1 = 1.0 - pow_(b1)
    bc2r = B(1.0) / (1.0 - pow_(b2)).sqrt()
    keep = 1.0 - lr_t * B(wd)
    step = ((lr_t / bc1) * mn) / (vn.sqrt() * bc2r + eps)
    out = {"m": mn, "v": vn, "p": B(p) * keep - step}
    if ema is not None:
        a = B(torch.as_tensor(ema, dtype=torch.float64))
        out["ema"] = fma(B(1.0) - B(d), out["p"] - a, a)
    return out


def is_weight(name):
    return name.endswith("_w")


# ================================================================ the reference's own checks (no GPU)
def test_optim_ref_with_everything_off_is_adam_ref():
    g = torch.Generator().manual_seed(0)
    p, m, gr = (torch.randn(500, generator=g).float().double() for _ in range(3))
    v = torch.rand(500, generator=g).float().double() * 1e-3
    for t, warm in ((1, 0), (3, 5), (10000, 0)):
        a = adam_ref(p, m, v, gr, 3e-3, 0.9, 0.999, 1e-8, t, warm)
        o = optim_ref(p, m, v, gr, 3e-3, 0.9, 0.999, 1e-8, t, warm)
        for k in ("p", "m", "v"):
            assert torch.equal(a[k].v, o[k].v) and torch.equal(a[k].e, o[k].e), (t, k)


def test_norm_reference_bound_is_a_few_ulps_and_covers_fp32_sums():
    """the bound of the documented order is ~ depth / 2 ulps of the norm (1.4e-6 at the 128 x 6 net), and fp32 sums of the same
    squares in other orders of no greater depth lie inside it"""
    sizes = list(counts(128, 12, 64).values())
    assert norm_depth(sizes) == 4 * 7 + 16 and norm_depth(list(counts(64, 2, 24).values())) == 4 + 16
    g = torch.Generator().manual_seed(1)
    grads = [torch.randn(n, generator=g).float() * s for n, s in zip(sizes, (1e-2, 1.0, 1e2, 1e-6, 1e-1, 1.0, 1e-3, 10.0, 1e-4, 1.0, 1e-5, 1e2, 1.0, 1e-6))]
    r = norm_ref(grads)
    rel = float(r.e / r.v)
    assert 1e-6 < rel < 4e-6, rel
    sq = torch.cat([t * t for t in grads])          # fp32 squares, summed pairwise in fp32 (a tree of depth 21 + the squares' rounding)
    assert abs(float(torch.sqrt(sq.sum())) - float(r.v)) <= float(r.e)


def test_clip_scale_reference():
    assert float(clip_scale_ref(B(0.5, 1e-6), 0.0).v) == 1.0 and float(clip_scale_ref(B(0.5, 1e-6), 1.0).e) == 0.0
    q = clip_scale_ref(B(50.0, 1e-4), 1.0)
    assert abs(float(q.v) - 1 / 50.000001) < 1e-9 and 1e-4 / 2500 < float(q.e) < 2e-4 / 2500 + 1e-8
    with pytest.raises(AssertionError):
        clip_scale_ref(B(1.0, 1e-3), 1.0)


@pytest.mark.parametrize("decay_biases", [False, True])
def test_reference_value_track_against_torch_adamw_clip_and_ema(decay_biases):
    """20 steps: torch.optim.AdamW (fp64, two parameter groups: the weights decay, the biases only with decay_biases) after
    torch.nn.utils.clip_grad_norm_, and ema += (1 - d) (p - ema) by hand, against the reference fed the same gradients and
    its own fp64 values: torch's p, m, v and the EMA lie inside the reference's bounds at every step"""
    torch.manual_seed(3)
    lr, b1, b2, eps, warm, wd, max_norm, d = f32(2e-3), f32(0.9), f32(0.999), f32(1e-8), 5, f32(0.1), f32(1.0), f32(0.99)
    shapes = {"a_w": (40, 7), "a_b": (40,), "c_w": (3, 5, 2), "c_b": (1,)}
    P = {k: torch.randn(s, dtype=torch.float32).double().requires_grad_(True) for k, s in shapes.items()}
    groups = [{"params": [P[k] for k in P if is_weight(k)], "weight_decay": wd},
              {"params": [P[k] for k in P if not is_weight(k)], "weight_decay": wd if decay_biases else 0.0}]
    opt = torch.optim.AdamW(groups, lr=lr, betas=(b1, b2), eps=eps)
    ema = {k: p.detach().clone() for k, p in P.items()}
    ref = {k: {"p": p.detach().clone(), "m": torch.zeros_like(p), "v": torch.zeros_like(p), "ema": p.detach().clone()} for k, p in P.items()}
    clipped = 0
    for t in range(1, 21):
        size = 10.0 if t % 3 == 0 else 0.01          # every third step's norm is far above max_norm, the others far below
        grads = {k: (torch.randn(s, dtype=torch.float32) * size).double() for k, s in shapes.items()}
        for k, p in P.items():
            p.grad = grads[k].clone()
        for gr in opt.param_groups:
            gr["lr"] = lr * min(1.0, t / warm)
        total = torch.nn.utils.clip_grad_norm_(list(P.values()), max_norm)
        opt.step()
        norm = B(torch.sqrt(sum((g * g).sum() for g in grads.values())), 0.0)
        assert abs(float(total) - float(norm.v)) < 1e-12
        scale = clip_scale_ref(norm, max_norm)
        clipped += float(scale.v) < 1.0
        for k, p in P.items():
            ema[k] += (1.0 - d) * (p.detach() - ema[k])
            s = ref[k]
            r = optim_ref(s["p"], s["m"], s["v"], grads[k], lr, b1, b2, eps, t, warm, wd=wd if is_weight(k) or decay_biases else 0.0,
                          scale=scale, ema=s["ema"], d=d)
            st = opt.state[p]
            for what, got in (("p", p.detach()), ("m", st["exp_avg"]), ("v", st["exp_avg_sq"]), ("ema", ema[k])):
                assert bool(((got - r[what].v).abs() <= r[what].e).all()), (t, k, what, float((got - r[what].v).abs().max()), float(r[what].e.min()))
                assert float((r[what].e / r[what].v.abs().clamp(min=1e-30)).median()) < 1e-5, (t, k, what)   # ... and the bounds are no wider than a few ulps
                s[what] = r[what].v
    assert clipped == 6


# ================================================================ the ABI
def _lib():
    from betazero_amd import _lib as m
    return m, m.lib()


def test_struct_matches_the_header():
    m, _ = _lib()
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
    import tempfile
    with tempfile.TemporaryDirectory() as dd:
        src = os.path.join(dd, "s.c")
        with open(src, "w") as f:
            f.write('#include <stdio.h>\n#include <stddef.h>\n#include "bz_abi.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", '
                    "sizeof(bz_train_optim), offsetof(bz_train_optim, stats), offsetof(bz_train_optim, partials), offsetof(bz_train_optim, beta1), "
                    "offsetof(bz_train_optim, decay_biases), offsetof(bz_train_optim, p), offsetof(bz_train_optim, ema)); return 0; }\n")
        subprocess.check_call(["gcc", "-I", inc, "-o", os.path.join(dd, "s"), src])
        got = [int(x) for x in subprocess.check_output([os.path.join(dd, "s")]).split()]
    T = m.TrainOptim
    assert got == [C.sizeof(T), T.stats.offset, T.partials.offset, T.beta1.offset, T.decay_biases.offset, T.p.offset, T.ema.offset], got
    assert C.sizeof(T) == 3 * 8 + 4 * 4 + 3 * 14 * 8 + 8


def _valid(m, with_ema=True):
    """a bz_train_optim whose pointers are all non-null (never dereferenced on the host: refusals come before any launch)"""
    keep = C.create_string_buffer(64)
    a = C.addressof(keep)
    T = m.TrainTensors
    full = lambda: T(**{k: a for k, _ in T._fields_})  # noqa: E731
    ema = full()
    opt = m.TrainOptim(hyper=a, stats=a, partials=a, beta1=0.9, beta2=0.999, eps=1e-8, decay_biases=0, p=full(), m=full(), v=full(),
                       ema=C.pointer(ema) if with_ema else None)
    return opt, full(), (keep, ema)


def test_hyper_block_layout_and_refusals():
    m, L = _lib()
    assert L.bz_train_optim_partials() == GNORM_GROUPS
    blk = (C.c_float * 8)(*([7.0] * 8))
    assert L.bz_train_optim_hyper(2e-3, 5.0, 300.0, 1e-4, 1.0, 0.99, blk) == m.BZ_OK
    assert list(blk) == [f32(2e-3), 5.0, 300.0, f32(1e-4), 1.0, f32(0.99), 0.0, 0.0]
    assert L.bz_train_optim_hyper(2e-3, 0.0, 0.0, 0.0, 0.0, 0.0, blk) == m.BZ_OK
    nan, inf = float("nan"), float("inf")
    for args, word in (((2e-3, 0, 0, -1e-4, 0, 0), b"weight_decay"), ((2e-3, 0, 0, nan, 0, 0), b"weight_decay"), ((2e-3, 0, 0, inf, 0, 0), b"weight_decay"),
                       ((2e-3, 0, 0, 0, -1.0, 0), b"max_norm"), ((2e-3, 0, 0, 0, nan, 0), b"max_norm"), ((2e-3, 0, 0, 0, inf, 0), b"max_norm"),
                       ((2e-3, 0, 0, 0, 0, -0.1), b"ema_decay"), ((2e-3, 0, 0, 0, 0, 1.0), b"ema_decay"), ((2e-3, 0, 0, 0, 0, 1.5), b"ema_decay"),
                       ((2e-3, 0, 0, 0, 0, nan), b"ema_decay"), ((-1.0, 0, 0, 0, 0, 0), b"rate"), ((nan, 0, 0, 0, 0, 0), b"rate"),
                       ((2e-3, -1, 0, 0, 0, 0), b"step count"), ((2e-3, 0, -1, 0, 0, 0), b"warm-up")):
        assert L.bz_train_optim_hyper(*[float(x) for x in args], blk) == m.BZ_EINVAL and word in L.bz_last_error(), args
    assert L.bz_train_optim_hyper(2e-3, 0.0, 0.0, 0.0, 0.0, 0.0, None) == m.BZ_EINVAL


def test_optim_step_refusals_and_no_device():
    m, L = _lib()
    opt, G, keep = _valid(m)
    call = lambda g, o, C_=64, Ly=4, VH=24: L.bz_train_optim_step(C.byref(g) if g is not None else None, C.byref(o) if o is not None else None, C_, Ly, VH, None)  # noqa: E731
    assert call(None, opt) == m.BZ_EINVAL and call(G, None) == m.BZ_EINVAL and b"null" in L.bz_last_error()
    for C_, Ly, VH in ((96, 4, 24), (64, 1, 24), (64, 4, 0), (64, 4, 65)):
        assert call(G, opt, C_, Ly, VH) == m.BZ_EINVAL and b"shape" in L.bz_last_error(), (C_, Ly, VH)
    g2 = m.TrainTensors.from_buffer_copy(G)
    g2.v2_b = None
    assert call(g2, opt) == m.BZ_EINVAL and b"gradient" in L.bz_last_error()
    for field in ("hyper", "stats", "partials"):
        o, _, k = _valid(m)
        setattr(o, field, None)
        assert call(G, o) == m.BZ_EINVAL and b"optimiser block" in L.bz_last_error(), field
    for field in ("p", "m", "v"):
        o, _, k = _valid(m)
        getattr(o, field).polfc_w = None
        assert call(G, o) == m.BZ_EINVAL and b"optimiser block" in L.bz_last_error(), field
    o, _, k = _valid(m)
    k[1].tower_b = None                              # an EMA set with a hole (ema = NULL as a whole is fine)
    assert call(G, o) == m.BZ_EINVAL and b"optimiser block" in L.bz_last_error()
    for b1, b2, eps in ((1.0, 0.999, 1e-8), (-0.1, 0.999, 1e-8), (0.9, 1.0, 1e-8), (0.9, 0.999, 0.0), (float("nan"), 0.999, 1e-8)):
        o, _, k = _valid(m)
        o.beta1, o.beta2, o.eps = b1, b2, eps
        assert call(G, o) == m.BZ_EINVAL and b"beta" in L.bz_last_error(), (b1, b2, eps)
    if L.bz_device_count() <= 0:                     # valid arguments: refused only for want of a device (with one they would launch)
        for with_ema in (True, False):
            o, _, k = _valid(m, with_ema)
            assert call(G, o) == m.BZ_ENOGPU and b"no HIP device" in L.bz_last_error()


def test_graphed_step_refuses_the_options_without_the_fused_optimiser():
    """before a device is touched: the module stays where it is"""
    from betazero_amd.net import PolicyValueNet
    from betazero_amd.train import GraphedTrainStep
    net = PolicyValueNet(64, 1, 24, fused_tower=True)
    for kw in (dict(weight_decay=0.1), dict(clip_norm=1.0), dict(ema_decay=0.99), dict(decay_biases=True)):
        with pytest.raises(ValueError, match="fused_adam"):
            GraphedTrainStep(net, batch=8, fused_adam=False, **kw)
        with pytest.raises(ValueError, match="fused_adam"):
            GraphedTrainStep(net, batch=8, step_kernels=False, **kw)
    with pytest.raises(ValueError, match="fused_adam"):
        GraphedTrainStep(PolicyValueNet(64, 1, 24), batch=8, weight_decay=0.1)
    assert all(p.device.type == "cpu" for p in net.parameters())
