"""The reference that tests/test_gpu_train_own_numerics.py holds the ownership head's training kernels to (k_train_heads_own,
k_train_heads_own_vt, k_train_own_finish of csrc/bz_train_ends.hip) -- heads_ref(..., own=...) of
test_train_numerics_cpu.py -- with the cases both files share, and the reference's own checks on the CPU: its values against
float64 autograd of the torch modules, a plain float32 evaluation of the same expressions inside every bound, the data reaching
every kind of cell, and the cap on ambiguous g[L] cells for each case the GPU file runs."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_train_numerics_cpu import B, U, bf16_rne, dyadic_pi, exact_head_params, exact_own_params, heads_ref, heads_torch

# (C, n, VH) of the GPU file: one workgroup and one pass; two workgroups; CPL = 2, five workgroups; 258 groups of four over 256
# workgroups (two of them run a second pass), idle value-head lanes
SHAPES = [(64, 4, 64), (64, 8, 64), (128, 20, 64), (64, 1032, 24)]
WEIGHTS = [0.7, 1.0]          # 0.7 is not dyadic: its rounding to fp32 and the product's are inside the bounds
AMBIGUOUS_CAP = 0.01          # of the elements of x: g[L] cells whose fp64 value lies within its bound of a bf16 rounding boundary
# exact_own_params' (seed, density) per shape.  Three quarters of the cells with x > 0 get their g[L] from the head's term alone
# (the ReLUs of the other three planes cut), and from |d3| ~ 4.5 on the bound of 1 - o o -- a few u, absolute -- is wider than a
# bf16 step of it: such a cell is ambiguous in every channel with a weight.  At density 0.25 that is 3 - 8 % of x, so the
# density is 0.1 - 0.12, and the seeds are ones whose few weights still saturate tanhf somewhere (all asserted below).
OWN_PARAMS = {(64, 4, 64): (866, 0.1), (64, 8, 64): (584, 0.1), (128, 20, 64): (48, 0.12), (64, 1032, 24): (44, 0.12)}


def heads_case(C, n, VH, seed, saturate=False):
    """test_gpu_train_numerics._heads_case's data (activations: integers 0..12 at density 0.6)"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randint(0, 13, (n, 64, C), generator=g) * (torch.rand(n, 64, C, generator=g) < 0.6)).double()
    P = exact_head_params(C, VH, seed, saturate)
    pi, z = dyadic_pi(n, seed), torch.randint(-1, 2, (n,), generator=g).double()
    return x, P, pi, z


def target_boards(n, seed):
    """disjoint target boards as int64 tensors [n] holding the uint64 bits: row 0 all empty, row 1 every cell the mover's (bit 63:
    the int64 sign), row 2 every cell the opponent's, the others random with bit 63 on either side"""
    rng = np.random.default_rng(seed)
    hi = lambda: rng.integers(0, 2, n).astype(np.uint64) << np.uint64(63)  # noqa: E731
    a = rng.integers(0, 2 ** 63, n, dtype=np.int64).astype(np.uint64) | hi()
    b = (rng.integers(0, 2 ** 63, n, dtype=np.int64).astype(np.uint64) | hi()) & ~a
    a[0], b[0] = np.uint64(0), np.uint64(0)
    a[1], b[1] = np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0)
    a[2], b[2] = np.uint64(0), np.uint64(0xFFFFFFFFFFFFFFFF)
    return torch.from_numpy(a.view(np.int64).copy()), torch.from_numpy(b.view(np.int64).copy())


def dyadic_vt(C, n):
    """test_heads_vt_with_dyadic_fractional_targets_within_the_derived_bounds' value targets: multiples of 2^-8 in [-1, 1]"""
    g = torch.Generator().manual_seed(C + n)
    vt = torch.randint(-256, 257, (n,), generator=g).double() * 2.0 ** -8
    vt[0], vt[1], vt[2] = 1.0, -1.0, 2.0 ** -8
    assert bool((vt != vt.round()).any())
    return vt


@functools.lru_cache(maxsize=None)
def own_case(C, n, VH, flat=False):
    """the data of one (C, n, VH): rows = max(n, 8) rows (a StepPlan's batch is a multiple of 8; the kernels are launched on the
    first n), as CPU tensors -- x [rows, 64, C], P, pi, z, vt, fown, fopp, ow, ob.  flat: ow = 0 and ob = 0 (o = 0 exactly)."""
    rows = max(n, 8)
    x, P, pi, z = heads_case(C, rows, VH, 31 + n)
    fown, fopp = target_boards(rows, 131 + n)
    ow, ob = exact_own_params(C, *OWN_PARAMS.get((C, n, VH), (231 + n, 0.25)))
    if flat:
        ow, ob = torch.zeros_like(ow), torch.zeros_like(ob)
    return {"x": x, "P": P, "pi": pi, "z": z, "vt": dyadic_vt(C, rows), "fown": fown, "fopp": fopp, "ow": ow, "ob": ob, "n": n}


def own_ref(case, value_targets, own_weight, device="cpu", head=True):
    """heads_ref on the first n rows of `case`; head=False: the same without the ownership head"""
    n = case["n"]
    to = lambda t: t[:n].to(device)  # noqa: E731
    own = {"ow": case["ow"].to(device), "ob": case["ob"].to(device), "fown": to(case["fown"]), "fopp": to(case["fopp"]), "own_weight": own_weight}
    return heads_ref(to(case["x"]), {k: v.to(device) for k, v in case["P"].items()}, to(case["pi"]), to(case["vt"] if value_targets else case["z"]),
                     own=own if head else None)


def g_top_counts(r, r0, x):
    """of the reference alone: how many g[L] cells are ambiguous (RNE of v - 2e and of v + 2e differ: _check_heads' interval), and
    on what share of the cells with x > 0 the head's term moved g[L] by at least one bf16 step (against r0, the same without)"""
    v, e = r["g_top"].v, r["g_top"].e
    ambiguous = int((bf16_rne(v - 2 * e) != bf16_rne(v + 2 * e)).sum())
    moved = (bf16_rne(v) != bf16_rne(r0["g_top"].v)) & (x > 0)
    return ambiguous, float(moved.double().sum() / (x > 0).double().sum())


TEN = ("pol_w", "pol_b", "val_w", "val_b", "polfc_w", "polfc_b", "v1_w", "v1_b", "v2_w", "v2_b")


# ================================================================ the reference's own checks (no GPU)
@pytest.mark.parametrize("own_weight", WEIGHTS + [0.0])
@pytest.mark.parametrize("C,n,VH", [(64, 16, 24), (128, 8, 64)])
def test_own_reference_equals_autograd(C, n, VH, own_weight):
    """heads_ref(own=...)'s values equal float64 autograd of heads_torch + OwnershipHead + own_weight * mse_loss to 1e-12; the ten
    other head gradients, CE and MSE keep the values AND the bounds they have without the head"""
    from betazero_amd.net import OwnershipHead
    from betazero_amd.train import ownership_targets
    case = own_case(C, n, VH)
    w = float(np.float32(own_weight))
    r, r0 = own_ref(case, False, own_weight), own_ref(case, False, own_weight, head=False)
    for k in TEN + ("ce", "mse"):
        assert torch.equal(r[k].v, r0[k].v) and torch.equal(r[k].e, r0[k].e), k
    x, pi, z = case["x"][:n], case["pi"][:n], case["z"][:n]
    Pt = {k: v.clone().requires_grad_(True) for k, v in case["P"].items()}
    xt = x.clone().requires_grad_(True)
    head = OwnershipHead(C).double()
    with torch.no_grad():
        head.conv.weight.copy_(case["ow"].reshape(1, C, 1, 1)); head.conv.bias.copy_(case["ob"])
    _, ce, mse = heads_torch(xt, Pt, pi, z)
    tgt = ownership_targets(case["fown"][:n], case["fopp"][:n]).double()
    l_own = F.mse_loss(head(xt.view(n, 8, 8, C).permute(0, 3, 1, 2)), tgt)     # the mean over positions and all 64 cells
    loss = ce + mse + w * l_own
    loss.backward()
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))  # noqa: E731
    assert torch.equal(r["own_t"], tgt)
    assert close(r["loss"].v, loss.detach()) and close(r["l_own"].v, l_own.detach())
    assert close(r["g_top"].v, xt.grad * (x > 0))
    assert r["own_w"].v.shape == head.conv.weight.grad.shape and close(r["own_w"].v, head.conv.weight.grad)
    assert r["own_b"].v.shape == head.conv.bias.grad.shape and close(r["own_b"].v, head.conv.bias.grad)
    for k in TEN:
        assert close(r[k].v, Pt[k].grad), k
    if own_weight:
        assert float(r["own_w"].v.abs().max()) > 0 and float(r["own_w"].e.min()) > 0 and float((r["g_top"].v - r0["g_top"].v).abs().max()) > 0
    else:   # no gradient reaches the head or, through it, the trunk -- exactly
        assert not bool(r["own_w"].v.any()) and not bool(r["own_w"].e.any()) and not bool(r["own_b"].v.any()) and not bool(r["own_b"].e.any())
        assert torch.equal(r["g_top"].v, r0["g_top"].v)   # (the GPU file asserts the kernels' bits equal here; the bound counts the fmaf)
        assert float(r["l_own"].v) > 0.1


@pytest.mark.parametrize("own_weight", WEIGHTS)
@pytest.mark.parametrize("C,n,VH", [(64, 8, 64), (128, 20, 64)])
def test_a_float32_evaluation_of_the_own_plane_lies_inside_every_bound(C, n, VH, own_weight):
    """the kernel's expressions for the fourth plane in plain float32 torch (sums in torch's own order; the three-term part of
    g[L] taken as the fp32 number nearest the reference's value, the fmaf's single rounding made in float64) within 1 x the bound"""
    case = own_case(C, n, VH)
    r, r0 = own_ref(case, False, own_weight), own_ref(case, False, own_weight, head=False)
    x = case["x"][:n].float()
    ow, ob, w = case["ow"].float(), case["ob"].float(), torch.tensor(own_weight, dtype=torch.float32)
    d3 = ob + x @ ow
    assert torch.equal(d3.double(), r["d3"])                       # exact: any order
    o = torch.tanh(d3)
    diff = o - r["own_t"].float()
    inv = (torch.tensor(1.0, dtype=torch.float32) / n) * (1.0 / 64.0)
    dp3 = w * 2.0 * diff * (1.0 - o * o) * inv
    terms = (diff * diff) * inv
    l_own, d_ob, d_ow = terms.sum(), dp3.sum(), dp3.reshape(-1) @ x.reshape(-1, C)
    three = r0["g_top"].v.float()
    g_top = ((dp3.double()[:, :, None] * ow.double() + three.double()).float() * (x > 0)).double()
    loss = r0["loss"].v.float() + w * l_own
    inside = lambda got, ref: bool(((got.double() - ref.v).abs() <= ref.e).all())  # noqa: E731
    assert inside(o, r["o"]) and inside(dp3, r["dp3"])
    assert inside(l_own, r["l_own"]) and inside(d_ob.reshape(1), r["own_b"]) and inside(d_ow.reshape(1, C, 1, 1), r["own_w"])
    assert inside(g_top, r["g_top"]) and inside(loss, r["loss"])
    # ... and the bounds are a few ulps, not a tolerance: relative to Sigma |terms| for the sums, to the value for the plane
    assert float((r["o"].e / r["o"].v.abs().clamp(min=1e-30)).max()) <= 5 * U
    f = r["dp3"].v.abs().reshape(-1)
    k = 4 * 64 * n   # (gamma_(64 n) Sigma |terms| for the order, as much again for the terms' own roundings, the tanh's 2 ulps twice)
    assert float(r["own_b"].e) < k * U * float(f.sum())
    assert float((r["own_w"].e.reshape(-1) / (f @ case["x"][:n].reshape(-1, C)).clamp(min=1e-30)).max()) < k * U
    assert float(r["l_own"].e / r["l_own"].v) < k * U


@pytest.mark.parametrize("C,n,VH", SHAPES)
def test_every_case_reaches_every_kind_of_cell_and_stays_under_the_ambiguous_cap(C, n, VH):
    """exact_own_params on the cases' activations: cells with |o| < 0.5, cells where tanhf saturates to +-1 exactly, cells with
    d3 = 0 exactly; all three target values; o and t of opposite signs somewhere; and for every variant the GPU file runs, of the
    reference alone: ambiguous g[L] cells under the cap, g[L] non-zero on more than 5 % of cells, the head's term visible"""
    case = own_case(C, n, VH)
    x = case["x"][:n]
    for vt in (False, True):
        for w in WEIGHTS:
            r = own_ref(case, vt, w)
            ambiguous, moved = g_top_counts(r, own_ref(case, vt, w, head=False), x)
            print(f"({C}, {n}, {VH}) vt={vt} w={w}: ambiguous {ambiguous} of {x.numel()}, moved by the head {moved:.3f} of the cells with x > 0")
            assert ambiguous < AMBIGUOUS_CAP * x.numel()
            assert float((bf16_rne(r["g_top"].v) != 0).double().mean()) > 0.05 and moved > 0
    o32 = torch.tanh(r["d3"]).float()
    small, sat, zero = (o32.abs() < 0.5).double().mean(), (o32.abs() == 1).double().mean(), (r["d3"] == 0).double().mean()
    print(f"({C}, {n}, {VH}): |o| < 0.5 on {float(small):.3f} of cells, saturated {float(sat):.3f}, d3 = 0 on {float(zero):.4f}")
    assert small > 0 and sat > 0 and zero > 0
    t = r["own_t"]
    assert set(t.unique().tolist()) == {-1.0, 0.0, 1.0} and not bool(t[0].any()) and bool((t[1] == 1).all()) and bool((t[2] == -1).all())
    assert bool((r["o"].v * t < 0).any())
    # (saturated cells: 1 - o o = 0 exactly in fp32 as in fp64 up to the bound -- their dp3 is bounded by a few u, not by 0)
    assert float(r["dp3"].e[o32.abs() == 1].max()) < 1e-6


@pytest.mark.parametrize("C,n", [(64, 8), (128, 1024)])
def test_the_flat_plane_is_exact(C, n):
    """ow = 0, ob = 0, n and own_weight powers of two: o = 0 exactly, dp3 = -+ 2 own_weight t / (64 n), and d ow, d ob and L_own are
    sums of dyadic terms with Sigma |terms| < 2^24 units -- the reference's bounds are 0, and the values are not"""
    case = own_case(C, n, 64, flat=True)
    r = own_ref(case, False, 0.5)
    for k in ("o", "dp3", "own_w", "own_b", "l_own"):
        assert float(r[k].e.abs().max()) == 0.0, k
    assert not bool(r["o"].v.any()) and float(r["own_w"].v.abs().max()) > 0 and float(r["own_b"].v.abs()) > 0
    t = r["own_t"]
    assert float(r["l_own"].v) == float((t * t).mean()) and torch.equal(r["dp3"].v, -t * 2.0 ** -6 / n)
