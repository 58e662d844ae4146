"""The plain reference that tests/test_gpu_net_numerics.py holds the policy/value net's inference forwards to (csrc/bz_net.hip:
k_tower_bf16 at every geometry, f8::k_tower_fp8, and the f32 path k_stem / k_conv_f32 / k_heads), the exact nets it runs on,
and their own checks on the CPU.

net_forward_ref(own, opp, P, mode) builds the input planes from the bitboards and runs the stem, the residual tower (im2col +
an fp64 matmul, tests/test_train_numerics_cpu.py's `conv`) and the heads in float64, storing every activation the way the mode
specifies:
  f32   fp32 (the values are asserted to be fp32 numbers);
  bf16  bf16_RNE(relu(.)) -- the stem, tower and head-conv weights rounded to bf16 (RNE) as the host packing does;
  fp8   e4m3_RNE(16 relu(.)) / 16, saturating at 448 -- quant.py's spec: tower and head-conv weights e4m3 with a power-of-two
        scale per output channel, the skip added as the stored value, stem weights and biases as in bf16.
ReLU is IEEE maximum(y, +0) (torch's: a NaN passes).  Every sum is asserted exact (Sigma |terms| < 2^24 units of its grid), so
the kernels' summation order cannot matter; the value comes out through oracle.tanhf, the fp32 restatement of tanhf_spec, the
only function here that rounds."""
import os

import numpy as np
import pytest
import torch

from test_train_numerics_cpu import EXACT, bf16_rne, check_fragments, conv, exact_head_params, exact_tower, planes_np, pow2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ("f32", "bf16", "fp8")
ORACLE_MODE = {"f32": 0, "bf16": 1, "fp8": 2}


# ---------------------------------------------------------------- rounding
def e4m3_rne(x):
    """float64 -> the nearest OCP e4m3fn value (ties to even, subnormal quantum 2^-9), saturating at +-448; a NaN passes"""
    x = torch.as_tensor(x, dtype=torch.float64)
    fin = torch.isfinite(x)
    xf = torch.where(fin, x, torch.zeros_like(x))
    e = torch.frexp(xf)[1]
    q = pow2((e - 4).clamp(min=-9))
    r = (torch.round(xf / q) * q).clamp(-448.0, 448.0)
    return torch.where(fin, r, torch.where(torch.isnan(x), x, torch.sign(x) * 448.0))


def relu(z):
    """torch's ReLU, IEEE maximum(z, +0): a NaN passes, -0 and negatives become +0"""
    return torch.where(torch.isnan(z), z, z.clamp(min=0.0) + 0.0)


def pow2_scale(m):
    """quant.py's per-output-channel scale: the largest power of two s with m s <= 448 (1 for m = 0)"""
    m = torch.as_tensor(m, dtype=torch.float64)
    k = torch.floor(torch.log2(448.0 / torch.where(m > 0, m, torch.ones_like(m))))
    s = pow2(k)
    s = torch.where(m * s > 448.0, s / 2, s)            # (log2 rounding: exact powers of two only)
    return torch.where(m * s * 2 <= 448.0, s * 2, s)


def fp8_weights(W):
    """tower / head-conv weights [co, ...] as the fp8 path holds them: e4m3(w s) / s per output channel"""
    s = pow2_scale(W.abs().reshape(W.shape[0], -1).max(1).values).view(-1, *([1] * (W.dim() - 1)))
    return e4m3_rne(W * s) / s


def store(z, mode):
    """an activation as stored after its ReLU"""
    y = relu(z)
    if mode == "bf16":
        return bf16_rne(y)
    if mode == "fp8":
        return e4m3_rne(16.0 * y) / 16.0
    return y


def lsb64(t):
    """the largest power of two of which every (finite) value of t is a multiple (1 for an all-zero t)"""
    t = t[torch.isfinite(t) & (t != 0)]
    if t.numel() == 0:
        return 1.0
    m, e = torch.frexp(t.double())
    m53 = (m.abs() * 2.0 ** 53).long()
    return float((pow2(e - 53) * (m53 & -m53).double()).min())


def _exact(terms, unit, what):
    worst = float(terms.max()) / unit if terms.numel() else 0.0
    assert worst < EXACT, f"{what}: Sigma |terms| = {worst:.3g} units of {unit:g} >= 2^24: fp32 would round"


def _is_f32(t, what):
    assert bool((t.float().double() == t).all()), f"{what}: not fp32 numbers"


# ---------------------------------------------------------------- parameters
KEYS = ("stem_w", "stem_b", "tw", "tb", "pol_w", "pol_b", "polfc_w", "polfc_b", "val_w", "val_b", "v1_w", "v1_b", "v2_w", "v2_b")


def flat_params(P):
    """the flat fp32 vector of bz_net_create / the oracle (PolicyValueNet.flat_params' order)"""
    parts = [P["stem_w"], P["stem_b"]]
    for l in range(P["tw"].shape[0]):
        parts += [P["tw"][l], P["tb"][l]]
    parts += [P[k] for k in ("pol_w", "pol_b", "polfc_w", "polfc_b", "val_w", "val_b", "v1_w", "v1_b", "v2_w", "v2_b")]
    return torch.cat([p.reshape(-1).cpu() for p in parts]).float().numpy().copy()


def to_module(P, dtype=torch.float64):
    """PolicyValueNet holding P (fused tower form)"""
    from betazero_amd.net import PolicyValueNet
    C, L, VH = P["stem_w"].shape[0], P["tw"].shape[0], P["v1_w"].shape[0]
    m = PolicyValueNet(C, L // 2, VH, fused_tower=True).to(dtype)
    with torch.no_grad():
        m.stem.weight.copy_(P["stem_w"]); m.stem.bias.copy_(P["stem_b"])
        m.tower_w.copy_(P["tw"]); m.tower_b.copy_(P["tb"])
        for mod, k in ((m.pol, "pol"), (m.polfc, "polfc"), (m.val, "val"), (m.v1, "v1"), (m.v2, "v2")):
            mod.weight.copy_(P[k + "_w"].reshape(mod.weight.shape)); mod.bias.copy_(P[k + "_b"].reshape(mod.bias.shape))
    return m


def mode_params(P, mode):
    """the parameters the mode's kernels compute with (host packing): bf16 / fp8 round the stem, tower and head-conv weights"""
    if mode == "f32":
        return P
    Q = dict(P)
    for k in ("stem_w", "pol_w", "val_w"):
        Q[k] = bf16_rne(P[k])
    Q["tw"] = bf16_rne(P["tw"])
    if mode == "fp8":
        Q["tw"] = torch.stack([fp8_weights(w) for w in Q["tw"]]) if Q["tw"].shape[0] else Q["tw"]
        hw = fp8_weights(torch.cat([Q["pol_w"].reshape(2, -1), Q["val_w"].reshape(1, -1)]))
        Q["pol_w"], Q["val_w"] = hw[:2].reshape(P["pol_w"].shape), hw[2:].reshape(P["val_w"].shape)
    return Q


# ---------------------------------------------------------------- the reference
def net_forward_ref(own, opp, P, mode, stats=None, feats=None):
    """(logits [n, 65], value [n]) as float64 tensors holding the kernels' fp32 results (P: float64 tensors, KEYS; on the
    device the tower runs on).  stats: a dict that receives per-layer counts of what the stores met; feats: a dict that
    receives the tower's output ("x" [n, 64, C]) and the inputs of the policy FC ("hf" [n, 128]) and of the second value FC
    ("v1h" [n, VH])."""
    assert mode in MODES
    Q = mode_params(P, mode)
    dev = Q["tw"].device
    own, opp = np.asarray(own, dtype=np.uint64), np.asarray(opp, dtype=np.uint64)
    n, C, L = own.shape[0], Q["stem_w"].shape[0], Q["tw"].shape[0]
    f = planes_np(own, opp).to(dev)

    def record(l, z, x):
        if stats is None:
            return
        s = stats.setdefault(l, {"zero": 0, "neg": 0, "ties": 0, "sat": 0, "sub": 0, "negzero": 0})
        y = relu(z)
        s["zero"] += int((z == 0).sum())
        s["neg"] += int((z < 0).sum())
        s["negzero"] += int(((z == 0) & (torch.signbit(z))).sum())
        if mode == "bf16":
            big = y[y > 256]
            m, _ = torch.frexp(big)
            fr = m * 256 - torch.floor(m * 256)
            s["ties"] += int((fr == 0.5).sum())
        if mode == "fp8":
            y16 = 16 * y
            s["sat"] += int((y16 > 448).sum())
            s["sub"] += int(((x > 0) & (16 * x < 2.0 ** -6)).sum())
            q = pow2((torch.frexp(y16)[1] - 4).clamp(min=-9))
            fr = y16 / q - torch.floor(y16 / q)
            s["ties"] += int(((fr == 0.5) & (y16 <= 448)).sum())

    # stem: planes (0 / 1) x weights + bias
    ws = Q["stem_w"].reshape(C, 18).t()
    z = f @ ws + Q["stem_b"]
    _exact(f @ ws.abs() + Q["stem_b"].abs(), min(lsb64(ws), lsb64(Q["stem_b"])), "stem")
    x = store(z, mode)
    record(0, z, x)
    acts = [x]
    for l in range(L):
        W, b = Q["tw"][l], Q["tb"][l]
        z, t = conv(acts[-1], W)
        z, t = z + b, t + b.abs()
        if l % 2:
            z, t = z + acts[-2], t + acts[-2].abs()
        _exact(t, min(lsb64(acts[-1]) * lsb64(W), lsb64(b), lsb64(acts[-2]) if l % 2 else 1.0), f"tower layer {l}")
        x = store(z, mode)
        record(l + 1, z, x)
        if l % 2:
            acts[-2:] = [x]
        else:
            acts.append(x)
    x = acts[-1] if L else acts[0]
    if mode == "f32":
        _is_f32(x, "activations")
    # heads: 1x1 convolutions -> ReLU (fp32 values) -> the FCs (fp32 fmaf chains, exact here)
    hw = torch.cat([Q["pol_w"].reshape(2, C), Q["val_w"].reshape(1, C)])
    hb = torch.cat([Q["pol_b"], Q["val_b"]])
    d = x @ hw.t() + hb                                                     # [n, 64, 3]
    _exact(x.abs() @ hw.abs().t() + hb.abs(), min(lsb64(x) * lsb64(hw), lsb64(hb)), "head 1x1 convolutions")
    h = relu(d)
    hf = torch.cat([h[:, :, 0], h[:, :, 1]], 1)                              # torch's flatten of [2, 8, 8]
    Wp, bp = Q["polfc_w"], Q["polfc_b"]
    logits = hf @ Wp.t() + bp
    _exact(hf.abs() @ Wp.abs().t() + bp.abs(), min(lsb64(hf) * lsb64(Wp), lsb64(bp)), "policy FC")
    t = h[:, :, 2] @ Q["v1_w"].t() + Q["v1_b"]
    _exact(h[:, :, 2].abs() @ Q["v1_w"].abs().t() + Q["v1_b"].abs(), min(lsb64(h[:, :, 2]) * lsb64(Q["v1_w"]), lsb64(Q["v1_b"])),
           "value FC 1")
    v1h = relu(t)
    v2w = Q["v2_w"].reshape(-1)
    vpre = v1h @ v2w + Q["v2_b"]
    _exact(v1h.abs() @ v2w.abs() + Q["v2_b"].abs(), min(lsb64(v1h) * lsb64(v2w), lsb64(Q["v2_b"])), "value FC 2")
    if feats is not None:
        feats.update(x=x, hf=hf, v1h=v1h)
    _is_f32(logits, "logits")
    _is_f32(vpre, "value pre-activation")
    import oracle.oracle as orc
    tanh = np.vectorize(lambda a: float(orc.tanhf(a)), otypes=[np.float64])
    value = torch.from_numpy(tanh(vpre.cpu().numpy().astype(np.float32))).to(dev)
    return logits, value


# ---------------------------------------------------------------- exact nets
def exact_net(C, NB, VH, mode, seed):
    """parameters (float64 tensors) on which every sum of the mode's forward is exact.
    Stem: dyadic weights, integer biases, a few odd ones in 257..511 (bf16 ties from layer 0 on).  Tower: exact_tower's
    sparse weights in {+-1, +-2} with every (layer, tap, 32-channel chunk) fragment nonzero, integer biases.  Heads:
    exact_head_params (FC weights dyadic on 2^-6 / 2^-8).
    fp8: the stem and tower biases are multiples of 1/16 (odd multiples above 1: e4m3 ties at 16 x = 17, 19, ..), a few stem
    biases above 28 (16 x > 448: saturation), a few channels with zero stem weights and biases k 2^-13 (subnormal codes),
    a tenth of the tower biases on the 2^-13 grid; the heads' weights are sparse powers of two (exactness on the 2^-13 grid)."""
    g = torch.Generator().manual_seed(seed)
    ri = lambda lo, hi, *s: torch.randint(lo, hi, s, generator=g).double()  # noqa: E731
    L = 2 * NB
    if L:
        _, W, b, _ = exact_tower(C, L, 1, seed, hot=False)
    else:
        W, b = torch.zeros(0, C, C, 3, 3, dtype=torch.float64), torch.zeros(0, C, dtype=torch.float64)
    P = exact_head_params(C, VH, seed + 1)
    sp = lambda *s: (torch.where(torch.rand(*s, generator=g) < 0.5, -1.0, 1.0).double()  # noqa: E731
                     * (torch.rand(*s, generator=g) < 0.04))

    def pow2_heads():                   # sparse powers of two: exact sums over activations on any grid, of any size
        P["pol_w"], P["val_w"] = sp(2, C, 1, 1), sp(1, C, 1, 1)
        P["pol_w"][:, 0] = P["val_w"][:, 0] = 1.0
        P["polfc_w"] = sp(65, 128) * 2.0 ** -4
        P["v1_w"] = sp(VH, 64) * 2.0 ** -3
        P["v2_w"] = sp(1, VH) * 2.0 ** -2
    if L > 12:                          # deep towers: a residual stream that drifts down faster
        b[1::2] -= 2
        pow2_heads()
    if mode == "fp8":
        stem_w = ri(-6, 7, C, 2, 3, 3) / 16 * (torch.rand(C, 2, 3, 3, generator=g) < 0.5)
        stem_b = ri(-8, 40, C) / 16
        hot = torch.randperm(C, generator=g)[:max(2, C // 16)]
        stem_b[hot] = ri(440, 520, hot.numel()) / 16                              # saturate (and ties just below 448)
        sub = torch.randperm(C, generator=g)[:max(2, C // 16)]
        stem_w[sub] = 0
        stem_b[sub] = ri(1, 8, sub.numel()) * 2.0 ** -13                         # subnormal codes 2^-9 .. 7 2^-9
        stem_b[sub[0]], stem_b[sub[1]] = 0.0, 9 * 2.0 ** -13                     # (+0; the smallest normal's neighbour)
        b = b / 2 + ri(-8, 9, L, C) / 16
        fine = torch.rand(L, C, generator=g) < 0.1
        b = torch.where(fine, b + ri(1, 8, L, C) * 2.0 ** -13, b)
        pow2_heads()
        P["pol_b"], P["val_b"] = ri(-8, 9, 2) / 16, ri(-8, 9, 1) / 16
        P["polfc_b"] = ri(-32, 33, 65) * 2.0 ** -6
        P["v1_b"] = ri(-16, 17, VH) * 2.0 ** -6
        P["v2_b"] = ri(-8, 9, 1) * 2.0 ** -6
    else:
        stem_w = ri(-8, 9, C, 2, 3, 3) / 2 * (torch.rand(C, 2, 3, 3, generator=g) < 0.6)
        stem_b = ri(-4, 6, C)
        hot = torch.randperm(C, generator=g)[:max(2, C // 16)]
        stem_b[hot] = 2 * ri(128, 256, hot.numel()) + 1                          # odd integers in 257 .. 511
        stem_w[hot] = stem_w[hot].round()                                        # (integral sums there: ties survive)
    P.update(stem_w=stem_w, stem_b=stem_b, tw=W, tb=b)
    if L:
        check_fragments(W)
    return P


# boards beyond legal positions
def edge_boards():
    """(own, opp) uint64 arrays: empty, full own, full opp, overlapping own / opp bits, stones only on the edges and corners,
    a checkerboard, random 64-bit words"""
    full = np.uint64(0xFFFFFFFFFFFFFFFF)
    edge = np.uint64(0xFF818181818181FF)
    corners = np.uint64(0x8100000000000081)
    rng = np.random.default_rng(0)
    rnd = rng.integers(0, 2 ** 63, (8, 2), dtype=np.int64).astype(np.uint64) * np.uint64(2) + rng.integers(0, 2, (8, 2)).astype(np.uint64)
    rows = [(0, 0), (full, 0), (0, full), (full, full), (edge, 0), (0, edge), (edge, corners), (corners, corners),
            (0xAA55AA55AA55AA55, 0x55AA55AA55AA55AA), (0x00000000000000FF, 0xFF00000000000000), (0x0101010101010101, 0x8080808080808080)]
    rows += [tuple(r) for r in rnd]
    own = np.array([np.uint64(a) for a, _ in rows], dtype=np.uint64)
    opp = np.array([np.uint64(b) for _, b in rows], dtype=np.uint64)
    return own, opp


def golden_boards(n, seed=1):
    """n rows of the golden Reversi games (8x8)"""
    d = np.load(os.path.join(ROOT, "tests", "golden", "reversi_random_games.npz"))
    rows = d["rows"][d["rows"][:, 1] == 8]
    idx = np.random.default_rng(seed).choice(len(rows), n, replace=n > len(rows))
    return rows[idx, 4].astype(np.uint64), rows[idx, 5].astype(np.uint64)


def boards(n, seed=1):
    """the edge boards first, then golden rows, n in all"""
    eo, ep = edge_boards()
    go, gp = golden_boards(max(n - eo.size, 1), seed)
    return np.concatenate([eo, go])[:n], np.concatenate([ep, gp])[:n]


# ================================================================ the reference's own checks (no GPU)
def _planes_t(own, opp, dtype=torch.float64):
    from betazero_amd.net import bits_to_planes
    return bits_to_planes(own, opp).to(dtype)


@pytest.mark.parametrize("C,NB,VH", [(32, 1, 33), (64, 2, 64), (128, 1, 1)])
def test_f32_reference_equals_torch_module_in_fp64(C, NB, VH):
    """mode f32 is PolicyValueNet's forward: on exact data the fp64 module gives the same logits and values (up to the
    value's fp32 tanh)"""
    P = exact_net(C, NB, VH, "f32", 3)
    own, opp = boards(40)
    lg, v = net_forward_ref(own, opp, P, "f32")
    with torch.no_grad():
        tl, tv = to_module(P)(_planes_t(own, opp))
    assert torch.equal(lg, tl)
    assert float((v - tv).abs().max()) < 2e-7


@pytest.mark.parametrize("mode,C,NB", [("f32", 64, 1), ("f32", 128, 2), ("bf16", 64, 1), ("bf16", 128, 2), ("fp8", 128, 2)])
def test_reference_equals_the_oracle_bit_for_bit(mode, C, NB):
    """on exact data the oracle (fmaf chains, its own bf16 / e4m3 stores) gives the same bits in all three modes"""
    import oracle.oracle as orc
    P = exact_net(C, NB, 64, mode, 5)
    Q = mode_params(P, mode)
    own, opp = boards(48)
    lg, v = net_forward_ref(own, opp, P, mode)
    olg, ov = orc.Net(C, NB, 64, flat_params(Q)).forward(own, opp, bf16=ORACLE_MODE[mode])
    assert np.array_equal(lg.numpy().astype(np.float32).view(np.uint32), olg.view(np.uint32))
    assert np.array_equal(v.numpy().astype(np.float32).view(np.uint32), ov.view(np.uint32))


@pytest.mark.parametrize("mode,C,NB", [("bf16", 64, 1), ("bf16", 128, 6), ("bf16", 256, 1), ("fp8", 128, 1), ("fp8", 128, 6),
                                       ("bf16", 64, 20)])
def test_exact_data_reaches_the_edges(mode, C, NB):
    """the stores meet what random floats never do: exact-zero and negative pre-activations in every layer, bf16 ties above
    256 (from the stem on), e4m3 ties, saturation above 448 / 16 and subnormal codes"""
    P = exact_net(C, NB, 64, mode, 1)
    st = {}
    own, opp = boards(64)
    net_forward_ref(own, opp, P, mode, st)
    for l, s in st.items():
        assert s["zero"] > 0 and s["neg"] > 0, (l, s)
    assert st[0]["ties"] > 0, st[0]
    assert sum(s["ties"] for s in st.values()) > len(st), st
    if mode == "fp8":
        assert st[0]["sat"] > 0 and st[0]["sub"] > 0, st[0]
        assert sum(1 for s in st.values() if s["sat"] > 0) >= len(st) // 2, st
        assert sum(s["sub"] for l, s in st.items() if l > 0) > 0, st


def _e4m3_table():
    """the 127 non-negative finite e4m3fn values, by code 0x00 .. 0x7E"""
    v = []
    for c in range(0x7F):
        e, m = c >> 3, c & 7
        v.append(m * 2.0 ** -9 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7))
    return np.array(v)


def test_e4m3_rounding_matches_an_enumeration_of_the_codes():
    """quant.e4m3_round, the reference's e4m3_rne and the oracle agree with a plain enumeration of the e4m3fn codes:
    every code, every midpoint (ties to the even code), points just off the midpoints, saturation, both signs"""
    import oracle.oracle as orc
    from betazero_amd.quant import e4m3_round
    tab = _e4m3_table()
    mids = (tab[1:] + tab[:-1]) / 2
    off = np.concatenate([np.nextafter(mids.astype(np.float32), np.float32(0)), np.nextafter(mids.astype(np.float32), np.float32(1e9))])
    x = np.concatenate([tab, mids, off, [448.0, 460.0, 464.0, 470.0, 480.0, 1e6, 2.0 ** -11, 2.0 ** -10, 3 * 2.0 ** -11]]).astype(np.float32)
    x = np.concatenate([x, -x])

    def nearest(a):
        i = np.abs(tab[None, :] - np.abs(a)[:, None]).argmin(1)
        d = np.abs(tab[i] - np.abs(a))
        j = np.minimum(i + 1, len(tab) - 1)
        tie = (np.abs(tab[j] - np.abs(a)) == d) & (j != i)
        i = np.where(tie & (i % 2 == 1), j, i)                      # ties: the even code
        return np.copysign(tab[i], a)
    want = nearest(x.astype(np.float64))
    assert np.array_equal(e4m3_round(x).astype(np.float64), want)
    assert np.array_equal(e4m3_rne(torch.from_numpy(x.astype(np.float64))).numpy(), want)
    assert np.array_equal(np.array([orc.lib().orc_e4m3_round(float(a)) for a in x]), want)
    assert bool(torch.isnan(e4m3_rne(torch.tensor([float("nan")]))).all())


def test_channel_scale_is_the_largest_power_of_two_that_fits():
    from betazero_amd.quant import channel_scale
    rng = np.random.default_rng(1)
    m = np.concatenate([rng.uniform(1e-3, 1e3, 2000), 448.0 / 2.0 ** np.arange(-8, 20), 448.0 / 2.0 ** np.arange(-8, 20) * (1 + 2.0 ** -20),
                        448.0 / 2.0 ** np.arange(-8, 20) * (1 - 2.0 ** -20)]).astype(np.float32)
    want = []
    for a in m.astype(np.float64):
        k = max(k for k in range(-40, 40) if a * 2.0 ** k <= 448.0)
        want.append(2.0 ** k)
    got = channel_scale(m.reshape(-1, 1))
    assert np.array_equal(got.astype(np.float64), np.array(want))
    assert np.array_equal(pow2_scale(torch.from_numpy(m.astype(np.float64))).numpy(), np.array(want))
    assert float(channel_scale(np.zeros((1, 4), np.float32))[0]) == 1.0


def test_relu_store_semantics():
    """ReLU is IEEE maximum(y, +0): NaN of either sign passes, -0 becomes +0; fp8 saturates at 448 / 16, +inf too"""
    z = torch.tensor([float("nan"), -float("nan"), -0.0, -1.0, 3.0, float("inf"), -float("inf"), 100.0], dtype=torch.float64)
    y = relu(z)
    assert bool(torch.isnan(y[:2]).all()) and not bool(torch.signbit(y[2])) and float(y[3]) == 0.0
    s8 = store(z, "fp8")
    assert bool(torch.isnan(s8[:2]).all()) and s8[5:].tolist() == [28.0, 0.0, 28.0]
    sb = store(z, "bf16")
    assert bool(torch.isnan(sb[:2]).all()) and float(sb[5]) == float("inf")
    # torch's relu agrees on the NaNs
    assert bool(torch.isnan(torch.relu(torch.tensor([float("nan"), -float("nan")]))).all())
