"""The plain references that tests/test_gpu_train_numerics.py holds the conv net's training kernels to (csrc/bz_train.hip,
csrc/bz_train_ends.hip), and their own checks on the CPU.

- Exact towers: integer activations, sparse integer weights in {+-1, +-2}, integer biases, sparse ternary output gradients.
  Every fp32 sum the kernels form is then exact in any order (each Sigma |terms| < 2^24 is asserted), so the MFMA's summation
  order cannot matter and a mapping error is a bit difference.  The reference reproduces every value the kernels store:
  act[l+1] = bf16_RNE(relu(conv + bias [+ skip])), g[l] = bf16_RNE((act[l] > 0) * (conv_bwd [+ skip])), dW, db summed over
  (position, cell) -- convolutions as im2col + an fp64 matmul (exact here; no F.conv2d, whose GPU algorithms need not be).
- Bounded values: `B` carries an fp64 value and a bound on how far an fp32 computation of it may lie (one rounding of u per
  operation, gamma_k * Sigma |terms| per k-term sum, the inputs' bounds carried through, 2 ulps per exp / log / tanh, 1 per
  sqrt, 4 per pow, and one subnormal step per rounding -- 2^-126 for the library functions, which may flush).  The heads and Adam are checked against it.
Layouts are the kernels': activations / gradients [n, 64 cells (8 y + x), C]; tower weights torch's [L, co, ci, 3, 3]."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

U = 2.0 ** -24          # fp32 unit roundoff
ETA = 2.0 ** -149       # absolute error of one fp32 rounding in the subnormal range (the smallest subnormal)
ETA_LIB = 2.0 ** -126   # ... of a library exp / log / tanh / sqrt, which may flush a subnormal result
EXACT = 2.0 ** 24       # an fp32 sum of integers is exact in any order while Sigma |terms| < 2^24


def gam(k):
    return k * U / (1 - k * U)


# ---------------------------------------------------------------- rounding
def pow2(k):
    """2^k as float64, exactly (int64 k in -1022 .. 1023; torch.ldexp multiplies by pow(2, k), which need not be exact on a GPU)"""
    return ((k.long() + 1023) << 52).view(torch.float64)


def bf16_rne(x):
    """round float64 values to the nearest bf16 (ties to even; subnormals included: quantum 2^-133), as float64"""
    x = torch.as_tensor(x, dtype=torch.float64)
    e = torch.frexp(x)[1]
    assert bool((e[x != 0] < 128).all()), "bf16_rne: beyond bf16's range"
    q = pow2((e - 8).clamp(min=-133))
    return torch.round(x / q) * q                 # torch.round: half to even; both scalings by q are exact


# ---------------------------------------------------------------- the tower
def im2col(a):
    """[n, 64, C] -> [n * 64, 9 * C]: column (tap, ci) of row (pos, cell) = a[pos, neighbour of cell at tap, ci] (zero off
    the board); tap = 3 ky + kx, neighbour (y + ky - 1, x + kx - 1) -- conv2d(padding=1)'s cross-correlation"""
    n, _, C = a.shape
    p = F.pad(a.view(n, 8, 8, C), (0, 0, 1, 1, 1, 1))
    cols = [p[:, ky:ky + 8, kx:kx + 8, :] for ky in range(3) for kx in range(3)]
    return torch.stack(cols, 3).reshape(n * 64, 9 * C)


def _wmat(W):   # [co, ci, 3, 3] -> [(tap, ci), co]
    return W.permute(2, 3, 1, 0).reshape(-1, W.shape[0])


def conv(a, W):
    """conv3x3(padding=1) of a [n, 64, C] with W [co, ci, 3, 3] -> [n, 64, co], and Sigma |terms| of every output"""
    n = a.shape[0]
    cols = im2col(a)
    return (cols @ _wmat(W)).view(n, 64, -1), (cols.abs() @ _wmat(W).abs()).view(n, 64, -1)


def conv_t(g, W):
    """d conv / d input: the transposed convolution (taps mirrored, co <-> ci)"""
    return conv(g, W.flip(2, 3).transpose(0, 1))


def _exact(terms, unit, what):
    worst = float(terms.max()) / unit if terms.numel() else 0.0
    assert worst < EXACT, f"{what}: Sigma |terms| = {worst:.3g} units >= 2^24, fp32 would round"


def tower_forward_ref(x0, W, b):
    """acts[0 .. L] (float64, [n, 64, C]) as the kernels store them; x0 integer, W / b integer (asserted exact)"""
    acts = [x0]
    for l in range(W.shape[0]):
        z, t = conv(acts[l], W[l])
        z, t = z + b[l], t + b[l].abs()
        if l % 2:
            z, t = z + acts[l - 1], t + acts[l - 1].abs()
        _exact(t, 1.0, f"forward layer {l}")
        acts.append(bf16_rne(torch.relu(z)))
    return acts


def tower_backward_ref(acts, W, g_top, unit=1.0):
    """gs[0 .. L] from g[L] (d loss / d pre-activation of act[L], as stored): g[2k+1] = bf16((act[2k+1] > 0) conv_t(g[2k+2])),
    g[2k] = bf16((act[2k] > 0) (conv_t(g[2k+1]) + g[2k+2])), g[0] unmasked (the stem's ReLU is not the tower's).  Every
    gradient is a multiple of `unit` (asserted)."""
    L = W.shape[0]
    gs = [None] * (L + 1)
    gs[L] = g_top
    for blk in range(L // 2 - 1, -1, -1):
        hi = gs[2 * blk + 2]
        z, t = conv_t(hi, W[2 * blk + 1])
        _exact(t, unit, f"backward layer {2 * blk + 1}")
        gs[2 * blk + 1] = bf16_rne(z * (acts[2 * blk + 1] > 0))
        z, t = conv_t(gs[2 * blk + 1], W[2 * blk])
        z, t = z + hi, t + hi.abs()
        _exact(t, unit, f"backward layer {2 * blk}")
        gs[2 * blk] = bf16_rne(z * (acts[2 * blk] > 0) if blk > 0 else z)
    for g in gs:
        assert bool((torch.remainder(g, unit) == 0).all()), "a gradient off its grid"
    return gs


def tower_wgrad_ref(acts, gs, unit=1.0):
    """dW [L, co, ci, 3, 3], db [L, C]: sums over (position, cell) of act[l] (shifted by the tap) x g[l + 1]"""
    L, C = len(acts) - 1, acts[0].shape[2]
    dW, db = [], []
    for l in range(L):
        cols, g = im2col(acts[l]), gs[l + 1].reshape(-1, C)
        d, t = cols.t() @ g, cols.abs().t() @ g.abs()
        _exact(t, unit, f"dW of layer {l}")
        _exact(g.abs().sum(0), unit, f"db of layer {l}")
        dW.append(d.view(3, 3, C, C).permute(3, 2, 0, 1))
        db.append(g.sum(0))
    return torch.stack(dW), torch.stack(db)


def exact_tower(C, L, n, seed, hot=True):
    """(x0, W, b, gy) on which the tower's fp32 sums are exact.  Weights: 1 or 2 nonzeros in {+-1, +-2} per output channel,
    then one more wherever a (tap, 32-channel chunk) of either the forward's ci or the backward's co would stay empty --
    every weight fragment the kernels stream carries data.  x0: small integers, a quarter zeros; with `hot`, a few
    positions hold values in the hundreds (bf16 must round them -- ties included -- all the way up).  gy: ternary, mostly 0."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi, s, generator=g).double()  # noqa: E731
    x0 = ri(0, 5, n, 64, C) * (torch.rand(n, 64, C, generator=g) > 0.25)
    if hot:
        for p in torch.randperm(n, generator=g)[:max(1, n // 64)].tolist():
            sel = torch.rand(64, C, generator=g) < 0.05
            x0[p][sel] = bf16_rne(ri(120, 400, int(sel.sum())))   # (act[0] is stored in bf16 too)
    W = torch.zeros(L, C, C, 3, 3, dtype=torch.float64)
    for l in range(L):
        k = 1 + (torch.rand(C, generator=g) < 0.5).long()
        for co in range(C):
            ci, tap = torch.randint(0, C, (int(k[co]),), generator=g), torch.randint(0, 9, (int(k[co]),), generator=g)
            val = torch.where(torch.rand(int(k[co]), generator=g) < 0.2, 2.0, 1.0).double()
            val = val * torch.where(torch.rand(int(k[co]), generator=g) < 0.5, -1.0, 1.0).double()
            W[l, co, ci, tap // 3, tap % 3] = val
        for tap in range(9):
            for ch in range(0, C, 32):
                if not bool((W[l, :, ch:ch + 32, tap // 3, tap % 3] != 0).any()):
                    W[l, int(torch.randint(0, C, (1,), generator=g)), ch + int(torch.randint(0, 32, (1,), generator=g)), tap // 3, tap % 3] = 1.0
                if not bool((W[l, ch:ch + 32, :, tap // 3, tap % 3] != 0).any()):
                    W[l, ch + int(torch.randint(0, 32, (1,), generator=g)), int(torch.randint(0, C, (1,), generator=g)), tap // 3, tap % 3] = -1.0
    b = ri(-3, 2, L, C)
    b[1::2] -= 2                        # (the residual stream: drifts down, which keeps deep towers in range)
    gy = ri(-1, 2, n, 64, C) * (torch.rand(n, 64, C, generator=g) < 0.15)
    check_fragments(W)
    return x0, W, b, gy


def check_fragments(W):
    """every (layer, tap, 32-channel chunk) of both fragment streams holds a nonzero weight"""
    L, C = W.shape[:2]
    nz = (W != 0).reshape(L, C, C, 9)
    fwd = nz.view(L, C, C // 32, 32, 9).any(3).any(1)        # [L, ci chunk, tap]
    bwd = nz.view(L, C // 32, 32, C, 9).any(2).any(2)        # [L, co chunk, tap]
    assert bool(fwd.all()) and bool(bwd.all()), "a weight fragment is all zero: a K-chunk would go untested"


def tower_case_stats(acts, W, b):
    """the data reaches what random floats never do: exact-zero pre-activations, stored values above 256 that bf16 had to
    round (ties among them), negative pre-activations in every layer"""
    zero = tie = rounded = 0
    neg = []
    for l in range(W.shape[0]):
        z = conv(acts[l], W[l])[0] + b[l] + (acts[l - 1] if l % 2 else 0)
        zero += int((z == 0).sum())
        neg.append(int((z < 0).sum()))
        big = z[z > 256]
        rounded += int((bf16_rne(big) != big).sum())
        m, e = torch.frexp(big)
        frac = m * 256 - torch.floor(m * 256)
        tie += int((frac == 0.5).sum())
    return {"zero": zero, "ties": tie, "rounded": rounded, "neg_min": min(neg)}


def tower_reference(x0, W, b, gy):
    """everything the tower kernels store for output gradient gy (g[L] = bf16(gy (act[L] > 0))): acts, gs, dW, db"""
    acts = tower_forward_ref(x0, W, b)
    gs = tower_backward_ref(acts, W, bf16_rne(gy * (acts[-1] > 0)))
    dW, db = tower_wgrad_ref(acts, gs)
    return acts, gs, dW, db


# ---------------------------------------------------------------- the stem
def planes_np(own, opp):
    """uint64 bitboards [n] -> [n, 64 cells, 18] 0/1: feature 9 plane + tap = stone of plane at the tap's neighbour"""
    n = own.shape[0]
    bits = np.stack([(own[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1),
                     (opp[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)], 1).astype(np.float64).reshape(n, 2, 8, 8)
    p = np.pad(bits, ((0, 0), (0, 0), (1, 1), (1, 1)))
    f = np.stack([p[:, pl, ky:ky + 8, kx:kx + 8] for pl in range(2) for ky in range(3) for kx in range(3)], -1)
    return torch.from_numpy(f.reshape(n, 64, 18))


def stem_ref(own, opp, w, b):
    """act[0] = bf16(relu(b + Sigma_k f_k w[c][k])) (fp64; exact when w, b share a grid and the sums fit, asserted by the caller)"""
    f = planes_np(own, opp)
    return bf16_rne(torch.relu(f @ w.reshape(w.shape[0], 18).t().double() + b.double()))


def stem_wgrad_ref(own, opp, act0, g0):
    f = planes_np(own, opp).reshape(-1, 18)
    gm = (g0 * (act0 > 0)).reshape(-1, g0.shape[2])
    return (gm.t() @ f), gm.sum(0), (gm.abs().t() @ f), gm.abs().sum(0)


# ---------------------------------------------------------------- values with bounds
class B:
    """an fp32 computation as its fp64 value `v` and a bound `e` on |fp32 result - v| (first order in u)"""

    def __init__(self, v, e=0.0):
        self.v = torch.as_tensor(v, dtype=torch.float64)
        self.e = torch.as_tensor(e, dtype=torch.float64).expand_as(self.v).clone() if torch.is_tensor(e) else torch.full_like(self.v, float(e))

    @staticmethod
    def lift(x):
        return x if isinstance(x, B) else B(x)

    @staticmethod
    def rnd(v, e):
        """one correctly rounded fp32 operation: + u |v|; or, where the exact result v is an fp32 number, + e (the computed
        result is then the fp32 number nearest to a value within e of v, so within 2 e of v; 0 when the inputs are exact)"""
        return B(v, e + torch.where(v.float().double() == v, e, U * v.abs() + ETA))

    def __add__(a, b):
        b = B.lift(b)
        return B.rnd(a.v + b.v, a.e + b.e)

    def __sub__(a, b):
        b = B.lift(b)
        return B.rnd(a.v - b.v, a.e + b.e)

    def __rsub__(a, b):
        return B.lift(b) - a

    def __mul__(a, b):
        b = B.lift(b)
        return B.rnd(a.v * b.v, a.v.abs() * b.e + b.v.abs() * a.e + a.e * b.e)

    __rmul__ = __mul__

    def __truediv__(a, b):
        b = B.lift(b)
        q = a.v / b.v
        lo = (b.v.abs() - b.e).clamp(min=1e-300)
        return B.rnd(q, (a.e + q.abs() * b.e) / lo)

    def __neg__(a):
        return B(-a.v, a.e)

    def where(self, mask):              # mask decided exactly (asserted by the caller): a select, no rounding
        return B(torch.where(mask, self.v, torch.zeros_like(self.v)), torch.where(mask, self.e, torch.zeros_like(self.e)))

    # exp(0) = 1, log(1) = 0 and tanh(0) = 0 exactly (C Annex F), exp below -104 underflows to 0
    def exp(a, ulps=2):
        v = torch.exp(a.v)
        e = v * torch.expm1(a.e) + 2 * ulps * U * v * torch.exp(a.e) + ETA_LIB
        under = (a.e == 0) & (a.v < -104)
        v = torch.where(under, torch.zeros_like(v), v)
        return B(v, torch.where((a.e == 0) & (a.v == 0) | under, torch.zeros_like(v), e))

    def log(a, ulps=2):
        v = torch.log(a.v)
        e = -torch.log1p(-a.e / a.v) + 2 * ulps * U * v.abs() + ETA_LIB
        return B(v, torch.where((a.e == 0) & (a.v == 1), torch.zeros_like(v), e))

    def tanh(a, ulps=2):
        v = torch.tanh(a.v)
        return B(v, a.e + 2 * ulps * U * v.abs() + torch.where(a.v == 0, 0.0, ETA_LIB))

    def sqrt(a, ulps=1):
        v = torch.sqrt(a.v)
        lo = torch.sqrt((a.v - a.e).clamp(min=0))
        return B(v, torch.where(v + lo > 0, a.e / (v + lo).clamp(min=1e-300), a.e.sqrt()) + 2 * ulps * U * v + ETA_LIB)

    def sum(a, dim):
        """a sum of k computed terms in any order: gamma_(k-1) Sigma |terms| plus the terms' bounds (no rounding where the
        terms are exact and fit one fp32 grid: every partial sum is then an fp32 number)"""
        k = a.v.shape[dim]
        ab, es = a.v.abs().sum(dim), a.e.sum(dim)
        return B(a.v.sum(dim), es + sum_rounding(ab, es, lsb(a.v), k))

    def __getitem__(self, i):
        return B(self.v[i], self.e[i])


def fma(a, b, c):
    a, b, c = B.lift(a), B.lift(b), B.lift(c)
    return B.rnd(a.v * b.v + c.v, a.v.abs() * b.e + b.v.abs() * a.e + a.e * b.e + c.e)


def lsb(t):
    """the largest power of two of which every value of t is a multiple (1 for an all-zero t; 0 unless all are fp32 numbers)"""
    t = t[t != 0]
    if t.numel() == 0:
        return 1.0
    if not bool((t.float().double() == t).all()):
        return 0.0                      # not fp32 values: no exactness claimed
    m, e = torch.frexp(t)
    m24 = (m.abs() * 2.0 ** 24).long()
    return float((pow2(e - 24) * (m24 & -m24).double()).min())


def sum_rounding(absum, esum, unit, k):
    """the rounding of a k-term fp32 sum with Sigma |terms| = absum: none where the terms are exact (esum = 0) multiples of
    `unit` and absum < 2^24 units, else gamma_(k-1) absum (+ k subnormal roundings)"""
    return torch.where((esum == 0) & (absum < EXACT * unit), torch.zeros_like(absum), gam(max(k - 1, 0)) * absum + k * ETA)


def matsum(x, W, k):
    """x @ W (x a B, W exact) as a k-term fmaf chain / any-order sum"""
    ab, es = x.v.abs() @ W.abs(), x.e @ W.abs()
    return B(x.v @ W, es + sum_rounding(ab, es, lsb(x.v) * lsb(W), k))


def dot(x, W, dim_terms):
    return matsum(x, W, dim_terms)


def heads_ref(x, P, pi, z, own=None):
    """the heads and losses of k_train_heads / k_train_heads_wgrad / k_train_finish on act[L] x [n, 64, C] (float64 values
    of the stored bf16) with parameters P (torch tensors, fp64 values of the fp32 parameters), in the kernels' operation
    order.  Requires exact 1x1 convolutions and FC pre-activations (asserted through `exact_units`): then the ReLU masks are
    exact and only exp / log / tanh and what follows round.  Returns {name: B} for the three losses, g[L] (before its bf16
    rounding) and the ten head gradients.

    own (k_train_heads_own / k_train_heads_own_vt and k_train_own_finish): a dict of the ownership head's
    `ow` [C] and `ob` (float64 values of the fp32 parameters), the rows' target boards `fown` / `fopp` (int64 tensors [n] holding
    the uint64 bits) and `own_weight`.  Adds own_w [1, C, 1, 1], own_b [1], l_own, the plane's o [n, 64] (B) and d3 (exact),
    and replaces loss (CE + MSE + own_weight L_own) and g_top (the head's term added last); the rest is what it is without."""
    n, _, C = x.shape
    inv_n = B.rnd(torch.tensor(1.0 / n), torch.tensor(0.0))     # 1.0f / n: one rounding
    hw = torch.cat([P["pol_w"].reshape(2, C), P["val_w"].reshape(1, C)])          # [3, C]
    hb = torch.cat([P["pol_b"], P["val_b"]])
    d = x @ hw.t() + hb                                           # [n, 64, 3]
    exact_units(x.abs() @ hw.abs().t() + hb.abs(), "1x1 convolutions")
    h = torch.relu(d)
    hf = torch.cat([h[:, :, 0], h[:, :, 1]], 1)                   # [n, 128]: torch's flatten of [2, 8, 8]
    Wp, bp = P["polfc_w"], P["polfc_b"]
    s = hf @ Wp.t() + bp                                          # [n, 65] logits
    exact_units(hf.abs() @ Wp.abs().t() + bp.abs(), "policy FC")
    V1, b1, v2w, v2b = P["v1_w"], P["v1_b"], P["v2_w"].reshape(-1), P["v2_b"]
    t = h[:, :, 2] @ V1.t() + b1                                  # [n, VH]
    exact_units(h[:, :, 2].abs() @ V1.abs().t() + b1.abs(), "value FC 1")
    v1h = torch.relu(t)
    vpre = v1h @ v2w + v2b
    exact_units(v1h.abs() @ v2w.abs() + v2b.abs(), "value FC 2")
    # soft-max, cross-entropy, d logit (pi: exact dyadic rows summing to 1, so spi = 1 exactly -- asserted by the caller)
    m = s.max(1, keepdim=True).values
    e = B(s - m).exp()
    S = e.sum(1)                                                  # (a 64-lane butterfly + 1: fewer than 65 additions)
    lse = B(m[:, 0]) + S.log()
    t_ce = B(pi) * _bsub_col(s, lse)
    ce = -(t_ce.sum(1))
    q = e / _bcol(S)
    da = (q - B(pi)) * inv_n                                      # (e / sum * spi - pa) * inv_n, spi = 1
    # value head
    v = B(vpre).tanh()
    diff = v - B(z)
    dpre2 = ((2.0 * diff) * inv_n) * (1.0 - v * v)
    dv1 = (_bcol(dpre2) * B(v2w.expand(n, -1))).where(t > 0)     # [n, VH]
    # losses: per position ce * inv_n and diff^2 * inv_n, summed over the batch
    ce_n = ce * inv_n
    mse_n = fma(diff * diff, inv_n, B(torch.zeros(n, dtype=torch.float64, device=x.device)))
    CE, MSE = ce_n.sum(0), mse_n.sum(0)
    both = B(torch.cat([ce_n.v, mse_n.v]), torch.cat([ce_n.e, mse_n.e])).sum(0)
    # back through the FCs to the three planes (65- and VH-term chains), their ReLUs
    a0 = dot(da, Wp[:, :64], 65)
    a1 = dot(da, Wp[:, 64:], 65)
    a2 = dot(dv1, V1, V1.shape[0])
    dp = [a.where(h[:, :, j] > 0) for j, a in enumerate((a0, a1, a2))]       # [n, 64] each
    # g[L] = (x > 0) * (dp0 hw0 + dp1 hw1 + dp2 hw2), a 3-term chain
    dps = B(torch.stack([d.v for d in dp], -1), torch.stack([d.e for d in dp], -1))   # [n, 64, 3]
    g_top = matsum(dps, hw, 3).where(x > 0)
    # parameter gradients: sums over (position, cell) / positions
    flat = lambda a: B(a.v.reshape(-1, *a.v.shape[2:]), a.e.reshape(-1, *a.e.shape[2:]))  # noqa: E731
    xr = x.reshape(-1, C)
    d_hw = []
    for j in range(3):
        dj = flat(dp[j])
        d_hw.append(matsum(B(dj.v.t(), dj.e.t()), xr, 64 * n))
    d_hb = [flat(dp[j]).sum(0) for j in range(3)]
    g_polfc_w = matsum(B(da.v.t(), da.e.t()), hf, n)
    g_v1_w = matsum(B(dv1.v.t(), dv1.e.t()), h[:, :, 2], n)
    g_v2_w = matsum(B(dpre2.v[None, :], dpre2.e[None, :]), v1h, n)[0]
    out = {"loss": both, "ce": CE, "mse": MSE, "g_top": g_top,
           "pol_w": B(torch.stack([d_hw[0].v, d_hw[1].v]).reshape(2, C, 1, 1), torch.stack([d_hw[0].e, d_hw[1].e]).reshape(2, C, 1, 1)),
           "val_w": B(d_hw[2].v.reshape(1, C, 1, 1), d_hw[2].e.reshape(1, C, 1, 1)),
           "pol_b": B(torch.stack([d_hb[0].v, d_hb[1].v]), torch.stack([d_hb[0].e, d_hb[1].e])),
           "val_b": B(d_hb[2].v.reshape(1), d_hb[2].e.reshape(1)),
           "polfc_w": g_polfc_w, "polfc_b": da.sum(0), "v1_w": g_v1_w, "v1_b": dv1.sum(0),
           "v2_w": B(g_v2_w.v.reshape(1, -1), g_v2_w.e.reshape(1, -1)), "v2_b": B(dpre2.sum(0).v.reshape(1), dpre2.sum(0).e.reshape(1)),
           "h": h, "s": s, "t": t}
    if own is not None:
        out.update(_own_plane_ref(x, own, inv_n, both, matsum(dps, hw, 3)))
    return out


def _own_plane_ref(x, own, inv_n, both, three):
    """the fourth plane of train_heads_body<C, kVT, true> and k_train_own_finish's sums, in their operation order.  both: CE + MSE
    as k_train_finish stores it; three: the three-term expression of g_top before its mask.  The plane has no ReLU and no mask:
    all 64 cells of every position count."""
    n, _, C = x.shape
    ow = torch.as_tensor(own["ow"], dtype=torch.float64, device=x.device).reshape(C)
    ob = torch.as_tensor(own["ob"], dtype=torch.float64, device=x.device).reshape(())
    w = float(np.float32(own["own_weight"]))                      # (the kernel argument is a float)
    d3 = x @ ow + ob                                              # [n, 64]: one ascending fmaf chain from ob
    exact_units(x.abs() @ ow.abs() + ob.abs(), "ownership 1x1")
    sh = torch.arange(64, dtype=torch.int64, device=x.device)
    bit = lambda b: (torch.as_tensor(b, dtype=torch.int64, device=x.device)[:, None] >> sh) & 1  # noqa: E731  (arithmetic shift: & 1 keeps bit 63)
    tgt = (bit(own["fown"]) - bit(own["fopp"])).double()          # [n, 64] in {-1, 0, 1}
    o = B(d3).tanh()
    diff = o - B(tgt)
    inv = B(inv_n.v * 2.0 ** -6, inv_n.e * 2.0 ** -6)             # inv_n * (1.0f / 64.0f): a scaling by a power of two, exact
    dp3 = (((B(w) * 2.0) * diff) * (1.0 - o * o)) * inv           # [n, 64]
    lo_t = fma(diff * diff, inv, B(torch.zeros_like(d3)))
    flat = lambda a: B(a.v.reshape(-1), a.e.reshape(-1))          # noqa: E731
    l_own = flat(lo_t).sum(0)
    d_ob = flat(dp3).sum(0)
    f = flat(dp3)
    d_ow = matsum(B(f.v[None, :], f.e[None, :]), x.reshape(-1, C), 64 * n)[0]
    g_top = fma(B(dp3.v[:, :, None], dp3.e[:, :, None]), B(ow.expand(n, 64, C)), three).where(x > 0)
    loss = both + B(w) * l_own                                    # losses[0] + weight * L_own: two roundings
    return {"own_w": B(d_ow.v.reshape(1, C, 1, 1), d_ow.e.reshape(1, C, 1, 1)), "own_b": B(d_ob.v.reshape(1), d_ob.e.reshape(1)),
            "l_own": l_own, "loss": loss, "g_top": g_top, "o": o, "d3": d3, "own_t": tgt, "dp3": dp3}


def _bcol(a):   # B [n] -> B [n, 1]
    return B(a.v[:, None], a.e[:, None])


def _bsub_col(s, lse):   # s [n, 65] exact minus lse [n] (a B): one rounding
    return B.rnd(s - lse.v[:, None], lse.e[:, None].expand_as(s).clone())


def exact_units(terms, what, unit=None):
    """Sigma |terms| of an exact sum in units of its grid (the caller's `HEAD_UNIT[what]`) < 2^24"""
    u = unit if unit is not None else HEAD_UNIT[what]
    _exact(terms, u, what)


# the grid of each exact head sum for exact_head_net's parameters (powers of two): x and the 1x1 weights integers,
# polfc / v1 weights multiples of 2^-6, v2 multiples of 2^-8
HEAD_UNIT = {"1x1 convolutions": 1.0, "policy FC": 2.0 ** -6, "value FC 1": 2.0 ** -6, "value FC 2": 2.0 ** -14,
             "ownership 1x1": 2.0 ** -4}   # (exact_own_params: x integers, ow and ob multiples of 2^-4)


def exact_own_params(C, seed, density=0.25):
    """the ownership head's (ow [C], ob) on which its pre-activation is exact on integer activations: ow multiples of 2^-4 in
    [-4, 4] / 16 at `density`, ob a multiple of 2^-4 in [-1/2, 1/2] -- on _heads_case's activations the plane then has cells
    with |o| < 0.5, cells where tanhf saturates to +-1 exactly and cells with d3 = 0 exactly (the callers assert which)"""
    g = torch.Generator().manual_seed(seed)
    ow = torch.randint(-4, 5, (C,), generator=g).double() * 2.0 ** -4 * (torch.rand(C, generator=g) < density)
    ob = torch.randint(-8, 9, (1,), generator=g).double() * 2.0 ** -4
    return ow, ob


def exact_head_params(C, VH, seed, saturate=False):
    """head parameters on which k_train_heads' 1x1 convolutions and FC pre-activations are exact (HEAD_UNIT).  saturate: the
    policy logit of action 7 is 256 above every other (every other exp underflows to 0: soft-max, CE and d logit exact)
    and v2 = 0 (v = tanh(0) = 0): the whole head backward is exact too."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi, s, generator=g).double()  # noqa: E731
    sparse = lambda *s: ri(-1, 2, *s) * (torch.rand(*s, generator=g) < 0.25)  # noqa: E731
    P = {"pol_w": sparse(2, C, 1, 1), "pol_b": ri(-2, 3, 2), "val_w": sparse(1, C, 1, 1), "val_b": ri(-2, 3, 1),
         "polfc_w": ri(-16, 17, 65, 128) * 2.0 ** -6 * (torch.rand(65, 128, generator=g) < 0.3),
         "polfc_b": ri(-32, 33, 65) * 2.0 ** -6,
         "v1_w": ri(-16, 17, VH, 64) * 2.0 ** -6 * (torch.rand(VH, 64, generator=g) < 0.3), "v1_b": ri(-32, 33, VH) * 2.0 ** -6,
         "v2_w": ri(-4, 5, 1, VH) * 2.0 ** -8, "v2_b": ri(-8, 9, 1) * 2.0 ** -8}
    if saturate:
        P["polfc_w"] = ri(-1, 2, 65, 128) * 2.0 ** -2 * (torch.rand(65, 128, generator=g) < 0.05)
        P["polfc_b"] = ri(-4, 5, 65)
        P["polfc_b"][7] = 256.0
        P["v2_w"].zero_(); P["v2_b"].zero_()
    return P


def dyadic_pi(n, seed, bits=8):
    """policy targets [n, 65]: multiples of 2^-bits summing to exactly 1, most of the mass on a few actions, some rows one-hot"""
    g = torch.Generator().manual_seed(seed)
    q = (torch.rand(n, 65, generator=g) ** 6 * 2 ** bits).floor()
    q[:, 64] += 1
    tot = q.sum(1)
    for i in range(n):   # trim / pad to exactly 2^bits units
        diff = int(2 ** bits - tot[i])
        j = int(torch.argmax(q[i]))
        q[i, j] += diff
        if q[i, j] < 0:
            q[i] = 0; q[i, j] = 2 ** bits
    q[0] = 0; q[0, 64] = 2 ** bits                     # all mass on "pass"
    assert bool((q >= 0).all()) and bool((q.sum(1) == 2 ** bits).all())
    return q.double() * 2.0 ** -bits


def heads_torch(x, P, pi, z):
    """the same heads in plain torch autograd (float64): PolicyValueNet's head definition and train.py's losses"""
    n, _, C = x.shape
    xc = x.view(n, 8, 8, C).permute(0, 3, 1, 2)
    p = F.linear(F.relu(F.conv2d(xc, P["pol_w"], P["pol_b"])).flatten(1), P["polfc_w"], P["polfc_b"])
    hv = F.relu(F.conv2d(xc, P["val_w"], P["val_b"])).flatten(1)
    v = torch.tanh(F.linear(F.relu(F.linear(hv, P["v1_w"], P["v1_b"])), P["v2_w"], P["v2_b"])).squeeze(-1)
    ce = -(pi * F.log_softmax(p, dim=1)).sum(1).mean()
    mse = ((v - z) ** 2).mean()
    return ce + mse, ce, mse


# ---------------------------------------------------------------- Adam (k_train_adam)
def adam_ref(p, m, v, g, lr, b1, b2, eps, t, warm):
    """one update of k_train_adam's documented formula from (p, m, v) and the kernel's gradient g, with bounds: float32 betas,
    lr_t = lr min(1, t / warm), bc1 = 1 - powf(b1, t), bc2_rsqrt = 1 / sqrtf(1 - powf(b2, t)) in fp32;
    m' = fmaf(b1, m, (1 - b1) g), v' = fmaf(b2, v, (1 - b2) g g), p' = p - (lr_t / bc1) m' / (sqrtf(v') bc2_rsqrt + eps)"""
    f = lambda x: float(np.float32(x))  # noqa: E731
    b1, b2, eps, lr = f(b1), f(b2), f(eps), f(lr)
    c1, c2 = 1.0 - b1, 1.0 - b2                    # exact in fp32 (Sterbenz: beta in [0.5, 1])
    g, m, v, p = (torch.as_tensor(a, dtype=torch.float64) for a in (g, m, v, p))
    mn = fma(b1, B(m), B(c1) * B(g))
    vn = fma(b2, B(v), (B(c2) * B(g)) * B(g))
    lr_t = B(lr) * B.rnd(torch.tensor(min(1.0, t / warm)), torch.tensor(0.0)) if warm > 0 else B(lr)

    def pow_(b):
        x = torch.tensor(b, dtype=torch.float64) ** t
        return B(x, 2 * 4 * U * x)                 # powf: 4 ulps
    bc1 = 1.0 - pow_(b1)
    bc2r = B(1.0) / (1.0 - pow_(b2)).sqrt()
    step = ((lr_t / bc1) * mn) / (vn.sqrt() * bc2r + eps)
    return {"m": mn, "v": vn, "p": B(p) - step}


# ================================================================ the references' own checks (no GPU)
def test_bf16_rne_matches_torch_and_rounds_ties_to_even():
    x = torch.tensor([1.0, 257.0, 259.0, 258.0, 513.0, 514.0, 515.0, -257.0, -259.0, 1 + 2 ** -8, 1 + 3 * 2 ** -8, 2 ** -134,
                      3 * 2 ** -134, 2 ** -140, -5 * 2 ** -134], dtype=torch.float64)
    want = torch.tensor([1.0, 256.0, 260.0, 258.0, 512.0, 512.0, 516.0, -256.0, -260.0, 1.0, 1 + 2 ** -6, 0.0,
                         2 ** -132, 0.0, -2 ** -132], dtype=torch.float64)
    assert torch.equal(bf16_rne(x), want)
    r = torch.cat([torch.randn(100000, dtype=torch.float64) * 1000, torch.randn(1000, dtype=torch.float64) * 2.0 ** -128])
    assert torch.equal(bf16_rne(r.float().double()), r.float().bfloat16().double())   # torch's own fp32 -> bf16 is RNE


def _tower_autograd(x0, W, b, gy, relu_masks):
    """tower_reference's definition in float64 torch autograd (conv2d, ReLU given by masks computed from the reference's
    own forward, the stored values rounded to bf16 with gradients rounded at the same points)"""
    class Rnd(torch.autograd.Function):   # bf16 rounding of the value AND of the gradient that passes back
        @staticmethod
        def forward(ctx, t):
            return bf16_rne(t)

        @staticmethod
        def backward(ctx, g):
            return bf16_rne(g)
    n, _, C = x0.shape
    nchw = lambda t: t.view(n, 8, 8, -1).permute(0, 3, 1, 2)  # noqa: E731
    a = nchw(x0)
    outs = []
    for blk in range(W.shape[0] // 2):
        hpre = F.conv2d(a, W[2 * blk], b[2 * blk], padding=1)
        hh = Rnd.apply(hpre * nchw(relu_masks[2 * blk]))
        apre = F.conv2d(hh, W[2 * blk + 1], b[2 * blk + 1], padding=1) + a
        a = Rnd.apply(apre * nchw(relu_masks[2 * blk + 1]))
        outs += [hh, a]
    return outs


@pytest.mark.parametrize("C,L,n", [(64, 2, 2), (64, 4, 3), (128, 6, 2)])
def test_tower_reference_equals_autograd(C, L, n):
    """the hand-written forward / backward / weight gradient equal float64 autograd of the same tower (conv2d, ReLU by masks
    from the stored activations, bf16 rounding of every stored value and gradient) bit for bit on exact data"""
    x0, W, b, gy = exact_tower(C, L, n, 100 + L)
    acts, gs, dW, db = tower_reference(x0, W, b, gy)
    masks = [acts[l + 1] > 0 for l in range(L)]
    xs, Ws, bs = (t.clone().requires_grad_(True) for t in (x0, W, b))
    outs = _tower_autograd(xs, Ws, bs, gy, masks)
    for l in range(L):
        assert torch.equal(outs[l].permute(0, 2, 3, 1).reshape(n, 64, C), acts[l + 1]), l
    outs[-1].backward(gy.view(n, 8, 8, C).permute(0, 3, 1, 2))
    assert torch.equal(xs.grad, gs[0])
    assert torch.equal(Ws.grad, dW) and torch.equal(bs.grad, db)
    # and the masks are the plain ReLU's: the forward through F.relu gives the same activations
    a = x0.view(n, 8, 8, C).permute(0, 3, 1, 2)
    for blk in range(L // 2):
        hh = bf16_rne(F.relu(F.conv2d(a, W[2 * blk], b[2 * blk], padding=1)))
        a = bf16_rne(F.relu(F.conv2d(hh, W[2 * blk + 1], b[2 * blk + 1], padding=1) + a))
    assert torch.equal(a.permute(0, 2, 3, 1).reshape(n, 64, C), acts[-1])


def test_exact_tower_data_reaches_the_edges():
    """the generator's data has zero pre-activations, rounded values above 256 with ties among them, negatives in every
    layer, and every weight fragment populated -- at the smallest and a deep shape"""
    for C, L, n in ((64, 2, 8), (128, 12, 4), (64, 40, 8)):
        x0, W, b, gy = exact_tower(C, L, n, 7)
        acts, gs, dW, db = tower_reference(x0, W, b, gy)
        st = tower_case_stats(acts, W, b)
        assert st["zero"] > 0 and st["ties"] > 0 and st["rounded"] > st["ties"] and st["neg_min"] > 0, (C, L, n, st)
        assert all(bool((g != 0).any()) for g in gs) and bool((dW != 0).any())


def test_stem_reference_equals_torch_conv():
    rng = np.random.default_rng(3)
    own = rng.integers(0, 2 ** 63, 6, dtype=np.int64).astype(np.uint64) | np.uint64(1 << 63)
    opp = rng.integers(0, 2 ** 63, 6, dtype=np.int64).astype(np.uint64) & ~own
    w = torch.randint(-64, 64, (64, 2, 3, 3)).double() * 2.0 ** -4
    b = torch.randint(-64, 64, (64,)).double() * 2.0 ** -4
    x = torch.stack([torch.from_numpy(((own[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(np.float64)),
                     torch.from_numpy(((opp[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(np.float64))], 1).view(6, 2, 8, 8)
    want = bf16_rne(F.relu(F.conv2d(x, w, b, padding=1))).permute(0, 2, 3, 1).reshape(6, 64, 64)
    assert torch.equal(stem_ref(own, opp, w, b), want)
    g0 = torch.randint(-8, 9, (6, 64, 64)).double()
    act0 = stem_ref(own, opp, w, b)
    ws, bs = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    pre = F.conv2d(x, ws, bs, padding=1).permute(0, 2, 3, 1).reshape(6, 64, 64)
    (pre * g0 * (act0 > 0)).sum().backward()
    dw, db, _, _ = stem_wgrad_ref(own, opp, act0, g0)
    assert torch.equal(dw.view(64, 2, 3, 3), ws.grad) and torch.equal(db, bs.grad)


@pytest.mark.parametrize("saturate", [False, True])
def test_heads_reference_equals_autograd(saturate):
    """the hand-written heads (values of B) equal float64 autograd of PolicyValueNet's heads and losses; their bounds are
    positive where the value is not exact and, with saturate, zero everywhere (the whole head backward exact)"""
    n, C, VH = 16, 64, 24
    P = exact_head_params(C, VH, 5, saturate)
    g = torch.Generator().manual_seed(1)
    x = (torch.randint(0, 9, (n, 64, C), generator=g) * (torch.rand(n, 64, C, generator=g) < 0.6)).double()
    pi, z = dyadic_pi(n, 2), torch.randint(-1, 2, (n,), generator=g).double()
    r = heads_ref(x, P, pi, z)
    Pt = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    xt = x.clone().requires_grad_(True)
    loss, ce, mse = heads_torch(xt, Pt, pi, z)
    loss.backward()
    close = lambda a, b: float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))  # noqa: E731
    assert close(r["loss"].v, loss.detach()) and close(r["ce"].v, ce.detach()) and close(r["mse"].v, mse.detach())
    assert close(r["g_top"].v, xt.grad * (x > 0))
    for k in ("pol_w", "pol_b", "val_w", "val_b", "polfc_w", "polfc_b", "v1_w", "v1_b", "v2_w", "v2_b"):
        assert r[k].v.shape == Pt[k].grad.shape and close(r[k].v, Pt[k].grad), k
    if saturate:
        assert all(float(r[k].e.abs().max()) == 0.0 for k in ("loss", "g_top", "pol_w", "polfc_w", "v2_w"))
    else:
        assert float(r["loss"].e) > 0 and float(r["g_top"].e.max()) > 0


def test_bounded_arithmetic_covers_fp32():
    """B's bounds hold for fp32 evaluations of random expressions (the kernels' operation shapes) and are not loose by more
    than a few u"""
    g = torch.Generator().manual_seed(0)
    a, b, c = (torch.rand(10000, generator=g, dtype=torch.float64) + 0.5 for _ in range(3))
    a, b, c = a.float().double(), b.float().double(), c.float().double()
    A, Bb, Cc = B(a), B(b), B(c)
    r = ((A * Bb + Cc) / (Bb - 0.25)).sqrt()
    f32 = torch.sqrt(((a.float() * b.float() + c.float()) / (b.float() - 0.25))).double()
    assert bool(((f32 - r.v).abs() <= r.e).all()) and float((r.e / r.v).max()) < 8 * U
    s = B(a.view(100, 100)).sum(1)
    f32s = a.float().view(100, 100).sum(1).double()
    assert bool(((f32s - s.v).abs() <= s.e).all())


def test_adam_reference_at_large_t():
    """powf underflows at large t: the bias corrections become 1 exactly and the bound stays a few u of the step"""
    r = adam_ref(torch.ones(4), torch.zeros(4), torch.zeros(4), torch.tensor([1e-3, -2.0, 0.0, 5.0]), 1e-3, 0.9, 0.999, 1e-8, 1e6, 0)
    assert torch.allclose(r["p"].v[:2], torch.tensor([1 - 1e-3 * 0.1 * 1e-3 / (np.sqrt(np.float32(0.001) * 1e-6) + 1e-8), 1 + 1e-3 * 0.2 / (np.sqrt(np.float32(0.001) * 4) + 1e-8)], dtype=torch.float64), rtol=1e-6)
    step = (r["p"].v - 1).abs()
    assert bool((r["p"].e - U * r["p"].v.abs() <= 16 * U * step).all())    # p's own rounding + a few u of the step
