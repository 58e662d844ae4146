"""The policy/value net's inference forwards (csrc/bz_net.hip, csrc/bz_tower.h) against net_forward_ref of
tests/test_net_numerics_cpu.py, bit for bit on exact nets: every logit (the pass logit, a wave reduction of its own, included)
and the value, for
- bf16: k_tower_bf16 at all six geometries (C = 64: Tw<64,2> / Tw<64,8>; C = 128: Tw<128,1> / Tw<128,4,true>, the 16x16x32 path;
  C = 256: Tw<256,1> / Tw<256,2>), NB in {0, 1, 6, 20}, VH in {1, 33, 64}, batches of 1, ragged sizes, 256 and 257 (the
  latency / throughput switch), 1848 (a bench-sized launch) and 8192;
- fp8: f8::k_tower_fp8 with its e4m3 ties, saturation and subnormal codes all reached;
- f32: k_stem / k_conv_f32 / k_heads at C = 32 .. 256 against the fp64 reference (not only against the oracle);
- the host packing: off-grid weights give the net of their rounded values, a zero output channel, a NaN weight stays a NaN;
- non-finite parameters: wherever torch's fp32 PolicyValueNet gives a non-finite logit or value, the kernels do too, and an
  engine search with such a net raises ERR_EVAL_NONFINITE.
References run on the GPU in fp64 (im2col + torch.matmul; never F.conv2d)."""
import numpy as np
import pytest
import torch

from test_net_numerics_cpu import ORACLE_MODE, boards, bf16_rne, exact_net, flat_params, net_forward_ref, to_module

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 1          # (exact at every configuration below: asserted by the reference)


def _u64(a):
    return torch.as_tensor(np.asarray(a, dtype=np.uint64).view(np.int64)).to(DEV)


def _dn(P, max_batch):
    from betazero_amd.net import DeviceNet
    C, L, VH = P["stem_w"].shape[0], P["tw"].shape[0], P["v1_w"].shape[0]
    return DeviceNet(C, L // 2, VH, flat_params(P), max_batch)


def _fwd(dn, own, opp, mode):
    lg, v = dn.forward(_u64(own), _u64(opp), bf16=mode != "f32", fp8=mode == "fp8")
    torch.cuda.synchronize()
    return lg.double(), v.double()


def _on(P, dev=DEV):
    return {k: t.to(dev) for k, t in P.items()}


def _bits_eq(got, want, what):
    g = got.float().cpu().numpy().view(np.uint32)
    w = want.float().cpu().numpy().view(np.uint32)
    bad = g != w
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got.cpu().numpy()[bad][:5].tolist(),
                           want.cpu().numpy()[bad][:5].tolist())


def _rows(n):
    """the rows compared with the reference: all up to 300, else a strided sample plus the last 9"""
    if n <= 300:
        return np.arange(n)
    return np.unique(np.concatenate([np.arange(0, n, max(1, n // 96)), np.arange(n - 9, n)]))


def _check(P, dn, mode, n, what, small_chunk=200):
    own, opp = boards(n, seed=n)
    lg, v = _fwd(dn, own, opp, mode)
    rows = _rows(n)
    rl, rv = net_forward_ref(own[rows], opp[rows], _on(P), mode)
    _bits_eq(lg[rows], rl, f"{what} n={n}: logits")
    _bits_eq(v[rows], rv, f"{what} n={n}: value")
    if n > 300:   # every row equals the same row from a small batch (another geometry: the latency shape)
        for lo in range(0, n, small_chunk):
            hi = min(n, lo + small_chunk)
            l2, v2 = _fwd(dn, own[lo:hi], opp[lo:hi], mode)
            _bits_eq(lg[lo:hi], l2, f"{what} n={n} rows {lo}..{hi} vs a small batch: logits")
            _bits_eq(v[lo:hi], v2, f"{what} n={n} rows {lo}..{hi} vs a small batch: value")


BF16 = [(64, 0, 1), (64, 1, 33), (64, 6, 64), (64, 20, 64), (128, 0, 33), (128, 1, 1), (128, 6, 64), (128, 20, 33),
        (256, 0, 64), (256, 1, 33), (256, 6, 1), (256, 20, 64)]


@pytest.mark.parametrize("C,NB,VH", BF16)
def test_bf16_net_bitexact_at_every_geometry(C, NB, VH):
    P = exact_net(C, NB, VH, "bf16", SEED)
    sizes = [1, 7, 37, 256, 257] + ([1848] if NB <= 6 else []) + ([8192] if (C, NB) == (128, 6) else [])
    dn = _dn(P, max(sizes))
    for n in sizes:
        _check(P, dn, "bf16", n, f"bf16 C={C} NB={NB} VH={VH}")


@pytest.mark.parametrize("NB,VH", [(0, 64), (1, 33), (6, 1), (6, 64)])
def test_fp8_net_bitexact(NB, VH):
    P = exact_net(128, NB, VH, "fp8", SEED)
    st = {}
    own, opp = boards(257, seed=257)
    net_forward_ref(own, opp, _on(P), "fp8", st)
    assert st[0]["ties"] > 0 and st[0]["sat"] > 0 and st[0]["sub"] > 0, st[0]
    if NB:
        assert sum(s["ties"] for l, s in st.items() if l) > 0 and sum(s["sat"] for l, s in st.items() if l) > 0, st
    sizes = [1, 7, 37, 256, 257] + ([1848, 8192] if NB == 6 and VH == 64 else [])
    dn = _dn(P, max(sizes))
    for n in sizes:
        _check(P, dn, "fp8", n, f"fp8 NB={NB} VH={VH}")


@pytest.mark.parametrize("C,NB,VH", [(32, 2, 64), (64, 1, 33), (128, 2, 1), (256, 1, 64), (64, 0, 64)])
def test_f32_net_bitexact_against_the_fp64_reference(C, NB, VH):
    P = exact_net(C, NB, VH, "f32", SEED)
    dn = _dn(P, 257)
    for n in (1, 37, 257):
        _check(P, dn, "f32", n, f"f32 C={C} NB={NB}")


# ---------------------------------------------------------------- host packing
def _perturb_bf16(w, g):
    """values that round (RNE) back to w, for w on the bf16 grid with an even last mantissa bit: + half an ulp (a tie),
    +- a quarter of one"""
    m, e = torch.frexp(w)
    ulp = torch.ldexp(torch.ones_like(w), e - 8)
    k = torch.randint(0, 4, w.shape, generator=g).double()
    d = torch.where(k == 1, ulp / 2, torch.where(k == 2, ulp / 4, torch.where(k == 3, -ulp / 4, torch.zeros_like(w))))
    return torch.where(w != 0, w + d * torch.sign(w), w)


def _even_bf16(w):
    bits = torch.from_numpy(w.float().numpy().view(np.uint32).astype(np.int64))
    return bool((((bits >> 16) & 1) == 0)[w != 0].all())


@pytest.mark.parametrize("C", [64, 128, 256])
def test_bf16_packing_rounds_weights_to_nearest_even(C):
    """tower, stem and head-conv weights off the bf16 grid (ties among them) give the net of their RNE values, bit for bit"""
    P = exact_net(C, 1, 64, "bf16", SEED)
    g = torch.Generator().manual_seed(3)
    Q = dict(P)
    for k in ("stem_w", "tw", "pol_w", "val_w"):
        assert _even_bf16(P[k]), k
        Q[k] = _perturb_bf16(P[k], g)
        assert torch.equal(bf16_rne(Q[k]), P[k]) and not torch.equal(Q[k], P[k]), k
    dn, dq = _dn(P, 300), _dn(Q, 300)
    for n in (5, 300):
        own, opp = boards(n, seed=9)
        a, b = _fwd(dn, own, opp, "bf16"), _fwd(dq, own, opp, "bf16")
        _bits_eq(b[0], a[0], f"C={C} n={n}: off-grid weights, logits")
        _bits_eq(b[1], a[1], f"C={C} n={n}: off-grid weights, value")
        rl, rv = net_forward_ref(own, opp, _on(P), "bf16")
        _bits_eq(b[0], rl, f"C={C} n={n}: logits vs reference")


def _fp8_module(P):
    """PolicyValueNet (per-layer modules) holding P in fp32, fake-quantised by quant.fake_quantize_fp8_"""
    from betazero_amd.net import PolicyValueNet
    from betazero_amd.quant import fake_quantize_fp8_
    C, L, VH = P["stem_w"].shape[0], P["tw"].shape[0], P["v1_w"].shape[0]
    m = PolicyValueNet(C, L // 2, VH)
    with torch.no_grad():
        for p, x in zip(m.parameters(), _param_list(P)):
            p.copy_(x.reshape(p.shape))
    return fake_quantize_fp8_(m)


def _param_list(P):
    out = [P["stem_w"], P["stem_b"]]
    for l in range(P["tw"].shape[0] // 2):
        out += [P["tw"][2 * l], P["tb"][2 * l]]
    for l in range(P["tw"].shape[0] // 2):
        out += [P["tw"][2 * l + 1], P["tb"][2 * l + 1]]
    return out + [P[k] for k in ("pol_w", "pol_b", "polfc_w", "polfc_b", "val_w", "val_b", "v1_w", "v1_b", "v2_w", "v2_b")]


def test_fp8_packing_matches_fake_quantize():
    """tower and head-conv weights on the bf16 grid but off the e4m3 grid (e4m3 ties among them) give quant.fake_quantize_fp8_'s
    net bit for bit -- and that is the reference's net of the exact weights they round to"""
    from betazero_amd.net import DeviceNet
    P = exact_net(128, 2, 64, "fp8", SEED)
    g = torch.Generator().manual_seed(4)
    Q = dict(P)
    for k in ("tw", "pol_w", "val_w"):
        w = P[k]
        e = torch.frexp(w)[1]
        ulp8 = torch.ldexp(torch.ones_like(w), e - 4)                 # e4m3's step at |w|
        kk = torch.randint(0, 4, w.shape, generator=g).double()
        d = torch.where(kk == 1, ulp8 / 2, torch.where(kk == 2, ulp8 / 4, torch.where(kk == 3, -ulp8 / 8, torch.zeros_like(w))))
        Q[k] = torch.where(w != 0, w + d * torch.sign(w), w)
        assert torch.equal(bf16_rne(Q[k]), Q[k])
    m = _fp8_module(Q)
    fq = m.flat_params()
    dq = _dn(Q, 300)
    df = DeviceNet(128, 2, 64, fq, 300)
    for n in (5, 300):
        own, opp = boards(n, seed=10)
        a, b = _fwd(dq, own, opp, "fp8"), _fwd(df, own, opp, "fp8")
        _bits_eq(a[0], b[0], f"n={n}: off-grid fp8 weights vs fake_quantize_fp8_, logits")
        _bits_eq(a[1], b[1], f"n={n}: value")
        rl, rv = net_forward_ref(own, opp, _on(P), "fp8")
        _bits_eq(a[0], rl, f"n={n}: logits vs reference")
        _bits_eq(a[1], rv, f"n={n}: value vs reference")


@pytest.mark.parametrize("mode,C", [("bf16", 64), ("bf16", 128), ("bf16", 256), ("fp8", 128), ("f32", 64)])
def test_an_all_zero_output_channel(mode, C):
    P = exact_net(C, 1, 64, mode, SEED)
    P["tw"] = P["tw"].clone()
    P["tw"][0, 5] = 0.0
    P["tw"][1, C - 1] = 0.0
    dn = _dn(P, 300)
    for n in (3, 300):
        own, opp = boards(n, seed=11)
        lg, v = _fwd(dn, own, opp, mode)
        rl, rv = net_forward_ref(own, opp, _on(P), mode)
        _bits_eq(lg, rl, f"{mode} C={C} n={n}: logits")
        _bits_eq(v, rv, f"{mode} C={C} n={n}: value")


@pytest.mark.parametrize("C", [64, 128, 256])
def test_a_nan_weight_stays_a_nan_after_packing(C):
    """a stem weight with the bits of a negative signalling NaN whose top 7 mantissa bits are zero (0xFF800001), at the
    centre tap of the own plane, on boards full of both colours: the bf16 packing must keep it a NaN.  (Rounded by integer
    arithmetic it became -inf, and the stem's ReLU turned -inf into 0: finite logits.)"""
    P = exact_net(C, 1, 64, "bf16", SEED)
    flat = flat_params(P)
    stem = flat[:C * 18].reshape(C, 2, 3, 3)
    stem.view(np.uint32)[3, 0, 1, 1] = 0xFF800001
    from betazero_amd.net import DeviceNet
    dn = DeviceNet(C, 1, 64, flat, 8)
    full = np.uint64(0xFFFFFFFFFFFFFFFF)
    lg, v = _fwd(dn, np.array([full] * 3, np.uint64), np.array([full] * 3, np.uint64), "bf16")
    assert bool(torch.isnan(lg).all(1).any() | torch.isnan(v).any()), (lg[:, :4], v)
    assert not bool(torch.isfinite(lg).all(1).any() & torch.isfinite(v).any())


# ---------------------------------------------------------------- non-finite parameters
WHERE = ("stem_w", "tw", "tb", "pol_w", "val_w", "v1_w")
BAD = (float("nan"), -float("nan"), float("inf"), -float("inf"))


def _set_bad(P, where, val, C):
    Q = {k: t.clone() for k, t in P.items()}
    if where == "stem_w":
        Q[where][3, 0, 1, 1] = val            # (centre taps: the kernels skip products with the board's zero padding)
    elif where == "tw":
        Q[where][0, 9, 2, 1, 1] = val
    elif where == "tb":
        Q[where][0, 9] = val
    elif where in ("pol_w", "val_w"):
        Q[where].view(-1)[2] = val
    else:
        Q[where][1, 7] = val
    return Q


def _nonfinite_rows(lg, v):
    return ~(torch.isfinite(lg).all(1) & torch.isfinite(v))


@pytest.mark.parametrize("mode", ["f32", "bf16", "fp8"])
def test_non_finite_parameters_give_non_finite_outputs_where_torch_does(mode):
    C = 128
    P = exact_net(C, 1, 64, "bf16" if mode != "fp8" else "fp8", SEED)
    own, opp = boards(48, seed=12)
    import oracle.oracle as orc
    from betazero_amd.net import DeviceNet, bits_to_planes
    planes = bits_to_planes(own, opp)
    seen = 0
    for where in WHERE:
        for val in BAD:
            Q = _set_bad(P, where, val, C)
            if mode == "fp8":
                m = _fp8_module(Q)
            else:
                m = to_module(Q, torch.float32)
            with torch.no_grad():
                tl, tv = m(planes)
            want = _nonfinite_rows(tl.double(), tv.double())
            fp = m.flat_params() if mode == "fp8" else flat_params(Q)
            olg, ov = orc.Net(C, 1, 64, fp).forward(own, opp, bf16=ORACLE_MODE[mode])
            want_orc = _nonfinite_rows(torch.from_numpy(olg).double(), torch.from_numpy(ov).double())
            if mode == "fp8" and val in (float("inf"), -float("inf")):
                # e4m3fn has no infinity: the activation store saturates +inf to 448 (quant.py), where torch's fp32 net
                # carries it on -- the oracle's fp8 emulation is the yardstick here
                want = want_orc
            dn = DeviceNet(C, 1, 64, fp, 48)
            lg, v = _fwd(dn, own, opp, mode)
            got = _nonfinite_rows(lg.cpu(), v.cpu())
            for w, who in ((want, "torch"), (want_orc, "oracle")):
                miss = w & ~got
                assert not bool(miss.any()), (mode, where, val, who, int(miss.sum()), int(w.sum()))
            seen += int(want.any())
    assert seen >= 12, seen      # most of the cases really make torch's net non-finite


def test_engine_search_with_a_nan_weight_raises_eval_nonfinite():
    from betazero_amd.engine import SelfPlayEngine
    P = exact_net(128, 1, 64, "bf16", SEED)
    Q = _set_bad(P, "tw", float("nan"), 128)
    dn = _dn(Q, 64)
    own, opp = boards(20, seed=13)
    own, opp = own[-4:], opp[-4:]                # golden (legal) positions
    eng = SelfPlayEngine("reversi", 4, 8, "net_bf16", net=dn)
    eng.set_roots(own, opp, np.ones(4, np.int8))
    eng.search()
    with pytest.raises(RuntimeError, match="non-finite"):
        eng.status()
    clean = SelfPlayEngine("reversi", 4, 8, "net_bf16", net=_dn(P, 64))   # the same net without the NaN raises nothing
    clean.set_roots(own, opp, np.ones(4, np.int8))
    clean.search()
    clean.status()
