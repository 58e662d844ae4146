"""The tic-tac-toe MLP with a value head on the MI355X (csrc/bz_mlp.hip):
- the f32 forward bit for bit through the unchanged 9-output C oracle (the value is the same fmaf chain as a logit, then
  tanhf_spec), the bf16 forward bit for bit on nets whose every intermediate is exact, and within the existing bound on dense nets;
- a value head of zeros changes nothing in a search; a real one reaches the leaves exactly as an external evaluator's would;
- the PV training step one step at a time against an fp64 step from the same (p, m, v), with derived tolerances;
- its error word, the trainer's plumbing, and the self-play loop in small."""
import os

import numpy as np
import pytest
import torch

from test_gpu_mlp import _bf16_emulation
from test_gpu_mlp_numerics import U, _adam_moments, _bits, _gam, _positions, _row_weights

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _split(flat, H):
    """PV flat vector -> (the policy net's flat vector: fc4 rows 0..8; a 9-output vector whose fc4 row 0 / bias 0 are the PV
    net's row 9 / bias 9, the other rows zero: its logit 0 is the value pre-activation u, by the same chain)"""
    body = flat[:2 * H * H + 12 * H]
    w4 = flat[2 * H * H + 12 * H:2 * H * H + 22 * H].reshape(10, H)
    b4 = flat[-10:]
    pol = np.concatenate([body, w4[:9].reshape(-1), b4[:9]]).astype(np.float32)
    wv, bv = np.zeros((9, H), np.float32), np.zeros(9, np.float32)
    wv[0], bv[0] = w4[9], b4[9]
    return pol, np.concatenate([body, wv.reshape(-1), bv]).astype(np.float32)


def _tanh_oracle(u):
    from oracle import oracle as orc
    return np.array([orc.tanhf(q) for q in np.asarray(u, np.float32).reshape(-1)], np.float32)


@pytest.fixture(scope="module")
def fix():
    from betazero_amd.mlp import TicTacToeNet
    z = np.load(os.path.join(GOLD, "ttt_mlp.npz"))
    m = TicTacToeNet(9, z["fc1_w"].shape[0], 9)
    m.load_state_dict({f"fc{l}.{k}": torch.from_numpy(z[f"fc{l}_{k[0]}"]) for l in (1, 2, 3, 4) for k in ("weight", "bias")})
    return m.eval(), z


def _canon(z, idx=None):
    idx = np.arange(len(z["move"])) if idx is None else idx
    tm = z["to_move"][idx]
    own = np.where(tm == 1, z["x_bits"][idx], z["o_bits"][idx]).astype(np.uint64)
    opp = np.where(tm == 1, z["o_bits"][idx], z["x_bits"][idx]).astype(np.uint64)
    return own, opp, tm


# ---------------------------------------------------------------- 1. f32, bit for bit through the unchanged oracle
@pytest.mark.parametrize("H", [32, 288, 512])
def test_f32_forward_bitexact_through_the_policy_oracle(H):
    from betazero_amd.mlp import DeviceMLP, TicTacToePVNet
    from oracle import oracle as orc
    own, opp = _positions()
    rng = np.random.RandomState(H)
    rows = rng.choice(5478, 33, replace=False)
    own, opp = own[rows], opp[rows]
    xs = orc.ttt_states(own, opp)
    xr = rng.randn(33, 9).astype(np.float32)  # beyond {-1, 0, 1}
    torch.manual_seed(H)
    p1 = TicTacToePVNet(H).flat_params()
    for scale in (1, 8):  # x8: weights, activations and logits leave [-1, 1], and the value saturates at +-1
        p = (p1 * scale).astype(np.float32)
        pol, val = _split(p, H)
        want_lg, want_lr = orc.mlp_forward_f32(H, pol, xs), orc.mlp_forward_f32(H, pol, xr)
        want_v, want_vr = _tanh_oracle(orc.mlp_forward_f32(H, val, xs)[:, 0]), _tanh_oracle(orc.mlp_forward_f32(H, val, xr)[:, 0])
        assert np.abs(want_v).max() > 1e-3 and (scale > 1 or np.abs(want_v).max() < 1.0)
        for n in (1, 15, 16, 17, 33):
            net = DeviceMLP(H, p, max_batch=n)
            assert net.value_head
            lg, v = net.forward(own[:n], opp[:n], value=True)
            ls, vs = net.forward_states(xs[:n], value=True)
            lr, vr = net.forward_states(xr[:n], value=True)
            for got, want in ((lg, want_lg), (ls, want_lg), (lr, want_lr), (v, want_v), (vs, want_v), (vr, want_vr),
                              (net.forward(own[:n], opp[:n]), want_lg), (net.forward_states(xr[:n]), want_lr)):
                assert np.array_equal(_bits(got.cpu().numpy()), _bits(want[:n])), n  # (a row's bits: whatever the batch)
            # the last rows of the batch too: another position in the 16-row tile
            lt, vt = net.forward_states(xr[33 - n:], value=True)
            assert np.array_equal(_bits(lt.cpu().numpy()), _bits(want_lr[33 - n:]))
            assert np.array_equal(_bits(vt.cpu().numpy()), _bits(want_vr[33 - n:]))


def test_policy_only_handle_has_no_value():
    from betazero_amd import _lib
    from betazero_amd.mlp import DeviceMLP, TicTacToeNet, TicTacToePVNet
    net = DeviceMLP.from_module(TicTacToeNet(9, 32, 9), max_batch=4)
    assert not net.value_head and _lib.lib().bz_mlp_has_value(net.h) == 0
    with pytest.raises(ValueError, match="value head"):
        net.forward_states(np.zeros((1, 9), np.float32), value=True)
    lg = torch.empty((1, 9), device="cuda"); v = torch.empty(1, device="cuda"); x = torch.zeros((1, 9), device="cuda")
    assert _lib.lib().bz_mlp_forward_pv_states_f32(net.h, x.data_ptr(), 1, lg.data_ptr(), v.data_ptr(), None) == _lib.BZ_EINVAL
    assert b"no value head" in _lib.lib().bz_last_error()
    pv = DeviceMLP.from_module(TicTacToePVNet(32), max_batch=4)
    assert pv.value_head and _lib.lib().bz_mlp_has_value(pv.h) == 1
    with pytest.raises(ValueError):
        pv.update(TicTacToeNet(9, 32, 9))     # a handle keeps its kind
    with pytest.raises(ValueError):
        net.update(TicTacToePVNet(32))


# ---------------------------------------------------------------- 2. bf16, bit for bit on exact nets
def _exact_net(H, seed, scaled):
    """tests/test_gpu_mlp_numerics.py's construction with a tenth fc4 row: fc1..fc3 rows of 3 nonzero weights in {-1, +1}
    (every column of every layer used), biases in {-1, 0, 1}; fc4 dense +-1 in all 10 rows, biases in {-1, 0, 1}.  On ternary
    inputs every activation is an integer <= 40 and fc4's outputs integers <= 512 * 40 + 1.  scaled: every weight and bias x 2^-3."""
    rng = np.random.RandomState(seed)
    layers = []
    for K, N in ((9, H), (H, H), (H, H)):
        W = np.zeros((N, K))
        sigma, rho = rng.permutation(K), rng.permutation(N)
        cols = sigma[(np.arange(N)[:, None] + np.arange(3)) % K]
        W[rho[:, None], cols] = rng.choice([-1.0, 1.0], (N, 3))
        layers.append((W, rng.randint(-1, 2, N).astype(np.float64)))
    layers.append((rng.choice([-1.0, 1.0], (10, H)), rng.randint(-1, 2, 10).astype(np.float64)))
    if scaled:
        layers = [(W / 8, b / 8) for W, b in layers]
    flat64 = np.concatenate([t.reshape(-1) for W, b in layers for t in (W, b)])
    flat = flat64.astype(np.float32)
    assert np.array_equal(flat.astype(np.float64), flat64)
    return layers, flat


def _exact_forward(layers, x, scaled):
    a = x.astype(np.float64)
    for l, (W, b) in enumerate(layers):
        y = a @ W.T + b
        q = 2.0 ** (3 * (l + 1)) if scaled else 1.0
        if l < 3:
            a = np.maximum(y, 0.0)
            assert np.array_equal(a * q, np.round(a * q)) and (a * q).max() < 2 ** 8        # exact in bf16
        else:
            assert np.array_equal(y * q, np.round(y * q)) and np.abs(y * q).max() < 2 ** 24  # exact in fp32
    return y


@pytest.mark.parametrize("H", [32, 288, 512])
def test_bf16_forward_bitexact_on_exact_nets(H):
    from betazero_amd.mlp import DeviceMLP
    from oracle import oracle as orc
    own, opp = _positions()
    own, opp = own[:4520], opp[:4520]
    xs = orc.ttt_states(own, opp)
    for scaled in (False, True):
        layers, flat = _exact_net(H, 5000 + H, scaled)
        y = _exact_forward(layers, xs, scaled).astype(np.float32)
        want_lg, u = y[:, :9], y[:, 9]
        uniq, inv = np.unique(u, return_inverse=True)
        want_v = _tanh_oracle(uniq)[inv]
        assert (u != 0).mean() > 0.5 and (np.abs(want_v) < 1).any()  # the value row is alive
        rng = np.random.RandomState(H)
        for n in (1, 17, 4520):
            idx = rng.choice(4520, n, replace=False)
            net = DeviceMLP(H, flat, max_batch=n)
            for lg, v in (net.forward(own[idx], opp[idx], bf16=True, value=True), net.forward_states(xs[idx], bf16=True, value=True),
                          net.forward(own[idx], opp[idx], value=True)):
                assert np.array_equal(_bits(lg.cpu().numpy()), _bits(want_lg[idx]))
                assert np.array_equal(_bits(v.cpu().numpy()), _bits(want_v[idx]))
            assert np.array_equal(_bits(net.forward(own[idx], opp[idx], bf16=True).cpu().numpy()), _bits(want_lg[idx]))


# ---------------------------------------------------------------- 3. bf16 on dense random weights
@pytest.mark.parametrize("H", [32, 256, 512])
def test_bf16_forward_dense_within_the_logits_bound(H):
    from betazero_amd.mlp import DeviceMLP, TicTacToePVNet
    from oracle.spec_math import BOUND
    torch.manual_seed(H)
    m = TicTacToePVNet(H).eval()
    with torch.no_grad():
        m.fc4.weight[9] *= 8; m.fc4.bias[9] += 0.5   # a value that is not in tanh's linear part only
    net = DeviceMLP.from_module(m, max_batch=1000)
    x = torch.randint(-1, 2, (1000, 9)).to(torch.float32)
    em = _bf16_emulation(m, x).numpy()               # [1000, 10]: the emulation runs over fc4's ten rows as they are
    assert em.shape == (1000, 10)
    for n in (1, 37, 1000):
        lb, vb = net.forward_states(x[:n], bf16=True, value=True)
        lb, vb = lb.cpu().numpy(), vb.cpu().numpy()
        bound = 2e-2 * max(1.0, np.abs(em[:n]).max())
        err_l, err_v = np.abs(lb - em[:n, :9]).max(), np.abs(vb - np.tanh(em[:n, 9])).max()
        print(f"H={H} n={n}: logits err {err_l:.3e}, value err {err_v:.3e}, bound {bound:.3e}")
        assert err_l <= bound
        assert err_v <= bound + BOUND["tanhf_spec"]   # tanh is 1-Lipschitz
        assert np.abs(vb).max() <= 1.0


# ---------------------------------------------------------------- 4. a value head of zeros changes nothing
def test_from_policy_net_value_zero_and_the_same_search(fix):
    from betazero_amd.engine import SelfPlayEngine
    from betazero_amd.mlp import DeviceMLP, TicTacToePVNet
    m, z = fix
    pol = DeviceMLP.from_module(m, max_batch=4520)
    pv = DeviceMLP.from_module(TicTacToePVNet.from_policy_net(m), max_batch=4520)
    own, opp, _ = _canon(z)
    for bf16 in (False, True):
        lg, v = pv.forward(own, opp, bf16=bf16, value=True)
        assert np.array_equal(_bits(lg.cpu().numpy()), _bits(pol.forward(own, opp, bf16=bf16).cpu().numpy()))
        assert not _bits(v.cpu().numpy()).any()      # +0.0, every bit
    idx = np.random.RandomState(1).choice(4520, 64, replace=False)
    own, opp, tm = _canon(z, idx)
    stats = []
    for net in (pol, pv):
        e = SelfPlayEngine("ttt", 64, 50, "mlp_f32", net=net)
        e.set_roots(own, opp, tm); e.search()
        stats.append(e.root_stats())
        e.status()
    assert stats[0][0].sum() > 0
    assert np.array_equal(stats[0][0], stats[1][0]) and np.array_equal(_bits(stats[0][1]), _bits(stats[1][1]))


# ---------------------------------------------------------------- 5. the search with a value
def test_search_with_a_value_equals_external():
    from betazero_amd.engine import SelfPlayEngine
    from betazero_amd.mlp import DeviceMLP, TicTacToePVNet
    torch.manual_seed(17)
    m = TicTacToePVNet(64)
    with torch.no_grad():
        m.fc4.weight[9] *= 4
    net = DeviceMLP.from_module(m, max_batch=64)
    seen = []

    def fn(own, opp, kind):
        x = (((own[:, None] >> torch.arange(9, device=own.device)) & 1) - ((opp[:, None] >> torch.arange(9, device=own.device)) & 1))
        lg, v = net.forward_states(x.to(torch.float32), value=True)
        seen.append(bool((v[kind == 1] != 0).any()))
        return lg, v
    a = SelfPlayEngine("ttt", 64, 50, "mlp_f32", net=net, temp_moves=4, seed=9)
    b = SelfPlayEngine("ttt", 64, 50, "external", temp_moves=4, seed=9)
    a.reset_games(); b.reset_games()
    for move in range(2):
        a.search(); b.search_external(fn)
        Na, Wa, Pa = a.root_stats()
        Nb, Wb, Pb = b.root_stats()
        assert Na.sum() > 0 and np.abs(Wa).max() > 0
        assert np.array_equal(Na, Nb) and np.array_equal(_bits(Wa), _bits(Wb)) and np.array_equal(_bits(Pa), _bits(Pb)), move
        a.play(False); b.play(False)
    assert any(seen)   # leaves carried a value: on the old path (value 0) W would differ from the external engine's
    for _ in range(10):
        if a.status()[0] == 0:
            break
        a.search(); a.play(False); b.search_external(fn); b.play(False)
    ea, eb = a.examples(), b.examples()
    assert len(ea.act) == len(eb.act) > 0
    assert np.array_equal(ea.act, eb.act) and np.array_equal(_bits(ea.pi), _bits(eb.pi)) and np.array_equal(ea.z, eb.z)
    assert np.array_equal(ea.own, eb.own) and np.array_equal(ea.opp, eb.opp)


# ---------------------------------------------------------------- 6. the training step against fp64, one step at a time
TANH_BOUND = 1e-7   # oracle/spec_math.BOUND["tanhf_spec"] (asserted equal below)


def _unflat(p, H):
    shapes = [(H, 9), (H,), (H, H), (H,), (H, H), (H,), (10, H), (10,)]
    out, o = [], 0
    for s in shapes:
        k = int(np.prod(s))
        out.append(p[o:o + k].reshape(s))
        o += k
    assert o == p.size
    return out


def _ref_step(H, p0, m0, v0, x, pi, vt, w, c, hp, step):
    """One PV step in fp64 from the kernel's pre-step (p, m, v) and an elementwise bound on how far an fp32 computation in the
    kernel's operation order may lie from it: tests/test_gpu_mlp_numerics.py's gamma_k chains (forward, softmax, backward-data,
    weight gradient, Adam), extended by
    - S = sum_o pi_o, a recursive sum of 9 non-negative fp32 terms: gamma(9) S; the gradient on logit o is
      scale (S p_o - pi_o): the product and the difference round once each;
    - the row's policy loss sum_o pi_o (lse - z_o): lse moves by at most max|dz| plus the roundings of expf / the 9-term sum /
      logf, each term rounds twice, the 9-term sum adds gamma(9) sum |terms|;
    - v = tanhf_spec(u): 1-Lipschitz in u plus tanhf_spec's stated bound;
    - the u-gradient ((scale c) (2 (v - vt))) (1 - v v): three rounded products (x 2 is exact), the difference and 1 - v v
      round once each.
    No term is measured: every one is derived.  Returns (reference, bound, hyper-parameters)."""
    f64 = np.float64
    P = _unflat(p0.astype(f64), H)
    Ws, bs = P[0::2], P[1::2]
    n = x.shape[0]
    from betazero_amd.mlp import TicTacToePVNet
    mod = TicTacToePVNet(H).double()
    with torch.no_grad():
        for fc, W, b in zip((mod.fc1, mod.fc2, mod.fc3, mod.fc4), Ws, bs):
            fc.weight.copy_(torch.from_numpy(W)); fc.bias.copy_(torch.from_numpy(b))
    x, pi, vt, w = (q.astype(f64) for q in (x, pi, vt, w))
    c = float(np.float32(c))
    lg_t, v_t = mod(torch.from_numpy(x))
    rows_t = -(torch.from_numpy(pi) * torch.log_softmax(lg_t, 1)).sum(1) + c * (v_t - torch.from_numpy(vt)) ** 2
    wt = torch.from_numpy(w)
    loss_t = (wt * rows_t).sum() / wt.sum()
    loss_t.backward()
    g = torch.cat([q.grad.reshape(-1) for fc in (mod.fc1, mod.fc2, mod.fc3, mod.fc4) for q in (fc.weight, fc.bias)]).numpy()
    # the same step by hand, carrying the bounds
    a, ea, amb = [x], [np.zeros((n, 9))], []
    for l in range(4):
        W, b = Ws[l], bs[l]
        y = a[-1] @ W.T + b
        ey = _gam(W.shape[1] + 1) * (np.abs(a[-1]) @ np.abs(W).T + np.abs(b)) + ea[-1] @ np.abs(W).T
        if l < 3:
            amb.append(np.abs(y) <= ey); a.append(np.maximum(y, 0.0)); ea.append(ey)
    z, ez, u, eu = y[:, :9], ey[:, :9], y[:, 9], ey[:, 9]
    v = np.tanh(u)
    ev = eu + TANH_BOUND
    sw = w.sum()
    sc = w / sw
    esc = _gam(n) + 2 * U
    zm = z.max(1)
    ex = np.exp(z - zm[:, None]); s = ex.sum(1); pr = ex / s[:, None]
    lse = zm + np.log(s)
    S = pi.sum(1)
    Ez = ez.max(1)
    rel_p = np.expm1(2 * Ez + 2 * U * np.abs(z - zm[:, None]).max(1)) + 16 * U
    gl = sc[:, None] * (S[:, None] * pr - pi)
    egl = np.abs(sc)[:, None] * (S[:, None] * pr * (rel_p[:, None] + _gam(9) + 2 * U) + U * np.abs(S[:, None] * pr - pi)) \
        + np.abs(gl) * (esc + U)
    dv = v - vt
    edv = ev + U * np.abs(dv)
    q1 = 1 - v * v
    eq1 = 2 * np.abs(v) * ev + ev * ev + U * v * v + U * np.abs(q1)
    gu = sc * c * 2 * dv * q1
    egu = np.abs(sc * c) * (2 * edv * np.abs(q1) + 2 * np.abs(dv) * eq1 + 2 * edv * eq1) + np.abs(gu) * (esc + 3 * U)
    term = pi * (lse[:, None] - z)
    elz = (2 * Ez + 2 * (_gam(9) + 8 * U))[:, None] + 8 * U * (np.abs(zm) + np.abs(np.log(s)))[:, None] + 8 * U * np.abs(z)
    ece = (pi * elz + U * np.abs(term)).sum(1) + _gam(9) * np.abs(term).sum(1)
    rl = term.sum(1) + c * dv * dv
    erl = ece + c * (2 * np.abs(dv) * edv + edv * edv + 2 * U * dv * dv) + U * np.abs(rl)
    tl = np.abs(sc * rl)
    eloss = (np.abs(sc) * erl + tl * (esc + U)).sum() + _gam(n) * tl.sum()
    d, ed = [None] * 4, [None] * 4
    d[3], ed[3] = np.concatenate([gl, gu[:, None]], 1), np.concatenate([egl, egu[:, None]], 1)
    for l in (3, 2, 1):
        W = Ws[l]
        v_ = d[l] @ W
        ev_ = _gam(W.shape[0]) * (np.abs(d[l]) @ np.abs(W)) + ed[l] @ np.abs(W)
        mask = a[l] > 0
        d[l - 1] = v_ * mask
        ed[l - 1] = np.where(amb[l - 1], np.abs(v_) + ev_, ev_ * mask)
    gm, egm = [], []
    for l in range(4):
        A, EA, D, ED = a[l], ea[l], d[l], ed[l]
        gm += [(D.T @ A).reshape(-1), D.sum(0)]
        egm += [(_gam(n) * (np.abs(D).T @ np.abs(A)) + ED.T @ np.abs(A) + np.abs(D).T @ EA + ED.T @ EA).reshape(-1),
                _gam(n) * np.abs(D).sum(0) + ED.sum(0)]
    gm, eg = np.concatenate(gm), np.concatenate(egm)
    assert np.abs(gm - g).max() <= 1e-12 * max(np.abs(g).max(), 1e-30)  # the hand-written backward is autograd's
    assert abs(loss_t.item() - (sc * rl).sum()) <= 1e-12 * abs(loss_t.item())
    # Adam at the float32 hyper-parameters (tests/test_gpu_mlp_numerics.py's, unchanged)
    lr, b1, b2, eps = (float(np.float32(q)) for q in hp)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    ss, bc2s = lr / bc1, np.sqrt(bc2)
    m0, v0, p0 = m0.astype(f64), v0.astype(f64), p0.astype(f64)
    m1 = m0 + (1 - b1) * (g - m0)
    v1 = v0 * b2 + (1 - b2) * g * g
    den = np.sqrt(v1) / bc2s + eps
    p1 = p0 - ss * m1 / den
    em = (1 - b1) * eg + 4 * U * (np.abs(m1) + (1 - b1) * np.abs(g - m0))
    evv = (1 - b2) * (2 * np.abs(g) * eg + eg * eg) + 4 * U * v1
    lo = np.sqrt(np.maximum(v1 - evv, 0.0))
    esq = np.where(np.sqrt(v1) + lo > 0, evv / np.maximum(np.sqrt(v1) + lo, 1e-300), np.sqrt(evv))
    eden = esq / bc2s + 4 * U * den
    den_lo = np.maximum(den - eden, eps)
    upd = ss * m1 / den
    ep = ss * (em / den_lo + np.abs(m1) * eden / (den * den_lo)) + 4 * U * np.abs(upd) + U * np.abs(p1)
    ref = {"loss": loss_t.item(), "grad": g, "m": m1, "v": v1, "p": p1}
    bnd = {"loss": eloss, "grad": eg, "m": em, "v": evv, "p": ep}
    return ref, bnd, (lr, b1, b2, eps, ss, bc2s)


def _check_step(tr, x, pi, vt, w, c, p0, m0, v0, hp):
    from betazero_amd.mlp import DeviceMLP
    H, n = tr.H, x.shape[0]
    ref, bnd, hps = _ref_step(H, p0, m0, v0, x, pi, vt, w, c, hp, tr.adam.step)
    loss = float(tr.loss.cpu()[0])
    g, m, v, p = (q.cpu().numpy().astype(np.float64) for q in (tr.grad, tr.m, tr.v, tr.p))
    # the bounds are first order in u: x2 covers the second-order terms
    assert abs(loss - ref["loss"]) <= 2 * bnd["loss"], (loss, ref["loss"], bnd["loss"])
    o = 0
    for k in (9 * H, H, H * H, H, H * H, H, 10 * H, 10):  # per tensor
        s_ = slice(o, o + k); o += k
        bad = np.abs(g[s_] - ref["grad"][s_]) > 2 * bnd["grad"][s_]
        assert not bad.any(), (s_, np.flatnonzero(bad)[:5], g[s_][bad][:5], ref["grad"][s_][bad][:5], bnd["grad"][s_][bad][:5])
    for key, val in (("m", m), ("v", v), ("p", p)):
        bad = np.abs(val - ref[key]) > 2 * bnd[key]
        assert not bad.any(), (key, np.flatnonzero(bad)[:5], val[bad][:5], ref[key][bad][:5], bnd[key][bad][:5])
    # Adam on the kernel's own gradient: m, v within 4 u (one rounding per fp32 operation), p within 8 u of the update
    lr, b1, b2, eps, ss, bc2s = hps
    m1, v1 = _adam_moments(g, m0, v0, 1 - b1, b2, 1 - b2)
    assert (np.abs(m - m1) <= 4 * U * (np.abs(m1) + (1 - b1) * np.abs(g - m0))).all()
    assert (np.abs(v - v1) <= 4 * U * v1).all()
    p1 = p0.astype(np.float64) - ss * m / (np.sqrt(v) / bc2s + eps)
    assert (np.abs(p - p1) <= 8 * U * np.abs(ss * m / (np.sqrt(v) / bc2s + eps)) + U * np.abs(p1)).all()
    # the training forward is the inference forward on the pre-step parameters, bit for bit (that one: test 1)
    lg, vv = DeviceMLP(H, p0, max_batch=n).forward_states(x, value=True)
    assert np.array_equal(_bits(tr.logits[:n].cpu().numpy()), _bits(lg.cpu().numpy()))
    assert np.array_equal(_bits(tr.value[:n].cpu().numpy()), _bits(vv.cpu().numpy()))
    return g


def _pv_rows(n, rng, ternary=True):
    x = rng.randint(-1, 2, (n, 9)).astype(np.float32) if ternary else rng.randn(n, 9).astype(np.float32)
    cnt = (rng.randint(1, 50, (n, 9)) * (rng.rand(n, 9) > 0.4)).astype(np.float64)   # visit counts, with zeros
    cnt[np.arange(n), rng.randint(0, 9, n)] += 1
    pi = (cnt / cnt.sum(1, keepdims=True)).astype(np.float32)
    vt = rng.choice(np.array([-1.0, 0.0, 1.0, 0.37, -0.81], np.float32), n)
    return x, pi, vt


_DEFAULT = (1e-3, 0.9, 0.999, 1e-8)
_CUSTOM = (3e-3, 0.8, 0.95, 1e-3)
# (H, n, row weights, value_weight, Adam): every value of each axis appears at least once
_CASES = [(32, 1, "ones", 1.0, "default"), (96, 3, "frac", 0.25, "custom"), (512, 4, "zeros", 1.0, "default"),
          (32, 5, "zeros", 0.25, "custom"), (96, 128, "frac", 1.0, "default"), (512, 128, "ones", 0.25, "custom")]


@pytest.mark.parametrize("H,n,wkind,c,adam", _CASES)
def test_training_steps_match_fp64(H, n, wkind, c, adam):
    from betazero_amd.mlp import PVTrainer, TicTacToePVNet
    from oracle.spec_math import BOUND
    assert BOUND["tanhf_spec"] == TANH_BOUND
    rng = np.random.RandomState(H * 1000 + n)
    torch.manual_seed(H + n)
    hp = _DEFAULT if adam == "default" else _CUSTOM
    mod = TicTacToePVNet(H)
    with torch.no_grad():
        mod.fc4.weight[9] *= 4          # |u| up to ~1: (1 - v^2) and tanh away from their linear ends
    tr = PVTrainer(mod, lr=hp[0], betas=hp[1:3], eps=hp[3], value_weight=c, max_batch=n)
    twin = PVTrainer(mod, lr=hp[0], betas=hp[1:3], eps=hp[3], value_weight=c, max_batch=n)
    for step in range(10):
        x, pi, vt = _pv_rows(n, rng, ternary=step % 2 == 0)
        w = _row_weights(wkind, n, rng)
        p0, m0, v0 = (q.cpu().numpy().copy() for q in (tr.p, tr.m, tr.v))
        for t in (tr, twin):
            t.step(x, pi, vt, None if wkind == "ones" else w)
            assert t.error() == 0
        for a_, b_ in zip((tr.p, tr.m, tr.v, tr.grad, tr.loss), (twin.p, twin.m, twin.v, twin.grad, twin.loss)):
            assert torch.equal(a_.view(torch.int32), b_.view(torch.int32))   # the same step twice: the same bits
        _check_step(tr, x, pi, vt, w, c, p0, m0, v0, hp)
    assert not np.array_equal(p0, tr.p.cpu().numpy())


def test_zero_weight_rows_contribute_exact_zeros():
    from betazero_amd.mlp import PVTrainer, TicTacToePVNet
    torch.manual_seed(3)
    mod = TicTacToePVNet(64)
    a, b = PVTrainer(mod, max_batch=50), PVTrainer(mod, max_batch=50)
    x, pi, vt = _pv_rows(50, np.random.RandomState(3))
    w = np.ones(50, np.float32); w[49] = 0.0
    la, lb = float(a.step(x, pi, vt, w)[0]), float(b.step(x[:49], pi[:49], vt[:49])[0])
    assert a.error() == 0 and b.error() == 0
    assert la == lb and torch.equal(a.p, b.p) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v) and torch.equal(a.grad, b.grad)


# ---------------------------------------------------------------- 7. the error word
def _bad_rows(kind, x, pi, vt, row):
    x, pi, vt = x.copy(), pi.copy(), vt.copy()
    if kind == "negative pi":
        pi[row, 2] = -0.25
    elif kind == "nan pi":
        pi[row, 5] = np.nan
    elif kind == "zero pi":
        pi[row] = 0.0
    elif kind == "vt 1.5":
        vt[row] = 1.5
    else:
        assert kind == "vt nan"
        vt[row] = np.nan
    return x, pi, vt


@pytest.mark.parametrize("kind", ["negative pi", "nan pi", "zero pi", "vt 1.5", "vt nan"])
def test_error_word_bad_targets(kind):
    from betazero_amd.mlp import PVTrainer, TicTacToePVNet
    torch.manual_seed(21)
    tr = PVTrainer(TicTacToePVNet(64), max_batch=64)
    x, pi, vt = _pv_rows(64, np.random.RandomState(21))
    tr.step(x, pi, vt)
    assert tr.error() == 0
    w = np.ones(64, np.float32); w[7] = 0.0
    xb, pb, vb = _bad_rows(kind, x, pi, vt, 7)
    before = [q.clone() for q in (tr.p, tr.m, tr.v)]
    tr.step(xb, pb, vb, w)                    # on a row of weight 0: nothing is set, the step is taken
    assert tr.error() == 0 and not torch.equal(tr.p, before[0])
    assert torch.isfinite(tr.p).all() and torch.isfinite(tr.loss).all()
    before = [q.clone() for q in (tr.p, tr.m, tr.v)]
    tr.step(xb, pb, vb)                       # on a weighted row: bit 1, and nothing moves
    assert tr.error() == 1
    for a_, b_ in zip(before, (tr.p, tr.m, tr.v)):
        assert torch.equal(a_.view(torch.int32), b_.view(torch.int32))
    tr.step(x, pi, vt)                        # sticky: a good step is refused while the word is set
    assert tr.error() == 1 and torch.equal(tr.p, before[0])
    tr.clear_error()
    tr.step(x, pi, vt)
    assert tr.error() == 0 and not torch.equal(tr.p, before[0])


def test_error_word_zero_weights_and_nonfinite_loss():
    from betazero_amd.mlp import PVTrainer, TicTacToePVNet
    torch.manual_seed(22)
    hp = (3e-3, 0.8, 0.95, 1e-3)
    tr = PVTrainer(TicTacToePVNet(64), lr=hp[0], betas=hp[1:3], eps=hp[3], max_batch=64)
    x, pi, vt = _pv_rows(64, np.random.RandomState(22))
    tr.step(x, pi, vt)
    assert tr.error() == 0
    xi = x.copy(); xi[5, 4] = np.inf          # a weighted row; 1e30 could leave the logits finite
    for xx, w, bit in ((x, np.zeros(64, np.float32), 4), (xi, np.ones(64, np.float32), 2)):
        before = [q.clone() for q in (tr.p, tr.m, tr.v)]
        tr.step(xx, pi, vt, w)
        assert tr.error() & bit and not tr.error() & 1
        for a_, b_ in zip(before, (tr.p, tr.m, tr.v)):
            assert torch.equal(a_.view(torch.int32), b_.view(torch.int32))
        tr.clear_error()
        p0, m0, v0 = (q.cpu().numpy().copy() for q in (tr.p, tr.m, tr.v))
        w1 = np.ones(64, np.float32)
        tr.step(x, pi, vt, w1)
        assert tr.error() == 0 and not torch.equal(tr.p, before[0])
        _check_step(tr, x, pi, vt, w1, 1.0, p0, m0, v0, hp)


def test_supervised_and_pv_steps_refuse_the_other_net():
    from betazero_amd import _lib
    from betazero_amd.mlp import DeviceMLP, MLPTrainer, PVTrainer, TicTacToeNet, TicTacToePVNet
    sl, pv = MLPTrainer(TicTacToeNet(9, 32, 9), max_batch=4), PVTrainer(TicTacToePVNet(32), max_batch=4)
    x, pi, vt = _pv_rows(4, np.random.RandomState(0))
    sl.mlp, keep = DeviceMLP.from_module(TicTacToePVNet(32), max_batch=1024), sl.mlp
    with pytest.raises(Exception, match="value head"):
        sl.step(x, np.zeros(4, np.int32))
    sl.mlp = keep
    pv.mlp, keep = DeviceMLP.from_module(TicTacToeNet(9, 32, 9), max_batch=1024), pv.mlp
    with pytest.raises(Exception, match="no value head"):
        pv.step(x, pi, vt)
    pv.mlp = keep
    assert _lib.lib().bz_mlp_has_value(pv.mlp.h) == 1


# ---------------------------------------------------------------- 8. the trainer's plumbing
def _fwd_all(net, bf16):
    own, opp = _positions()
    lg, v = net.forward(own, opp, bf16=bf16, value=True)
    return np.concatenate([lg.cpu().numpy(), v.cpu().numpy()[:, None]], 1)


@pytest.mark.parametrize("k", [1, 5])
def test_forward_after_training_equals_fresh_upload(k):
    from betazero_amd.mlp import DeviceMLP, PVTrainer, TicTacToePVNet
    torch.manual_seed(30 + k)
    tr = PVTrainer(TicTacToePVNet(96), lr=3e-3, max_batch=128)
    assert tr.device_mlp is tr.mlp and tr.device_mlp.value_head and tr.device_mlp.max_batch >= 65536
    rng = np.random.RandomState(k)
    before = _fwd_all(tr.device_mlp, True)
    for _ in range(k):
        tr.step(*_pv_rows(128, rng))
    assert tr.error() == 0
    fresh = DeviceMLP(96, tr.params(), max_batch=5478)
    fresh_mod = DeviceMLP.from_module(tr.to_module(), max_batch=5478)
    for bf16 in (False, True):
        got = _fwd_all(tr.device_mlp, bf16)
        assert np.array_equal(_bits(got), _bits(_fwd_all(fresh, bf16))) and np.array_equal(_bits(got), _bits(_fwd_all(fresh_mod, bf16)))
    assert not np.array_equal(before, _fwd_all(tr.device_mlp, True))


def test_state_dict_resumes_bit_for_bit():
    from betazero_amd.mlp import PVTrainer, TicTacToePVNet
    torch.manual_seed(41)
    kw = dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-3, value_weight=0.5, max_batch=64)
    tr = PVTrainer(TicTacToePVNet(64), **kw)
    rng = np.random.RandomState(41)
    batches = [_pv_rows(64, rng) for _ in range(5)]
    for b in batches[:3]:
        tr.step(*b)
    sd = tr.state_dict()
    assert all(isinstance(sd[k], torch.Tensor) and sd[k].device.type == "cpu" for k in ("p", "m", "v")) and sd["steps"] == 3
    torch.manual_seed(42)
    other = PVTrainer(TicTacToePVNet(64), **kw)     # other weights: everything must come from the state
    other.load_state_dict(sd)
    assert other.steps == 3
    for b in batches[3:]:
        tr.step(*b); other.step(*b)
        for a_, b_ in zip((tr.p, tr.m, tr.v, tr.loss), (other.p, other.m, other.v, other.loss)):
            assert torch.equal(a_.view(torch.int32), b_.view(torch.int32))
        assert np.array_equal(_bits(_fwd_all(tr.device_mlp, True)), _bits(_fwd_all(other.device_mlp, True)))
    wrong = PVTrainer(TicTacToePVNet(32), **kw)
    p_before = wrong.p.clone()
    with pytest.raises(ValueError, match="hidden size"):
        wrong.load_state_dict(sd)
    assert torch.equal(wrong.p, p_before) and wrong.steps == 0


# ---------------------------------------------------------------- 9. the loop in small
def test_the_loop_in_small(fix):
    """H = 64, 3 iterations of 512 games x 32 simulations with the bf16 net in the search, each followed by 2 epochs over the
    window's augmented rows: the value's MSE against minimax over the 4,520 fixture positions must fall below the untrained
    net's (DESIGN.md 11 records both)."""
    from betazero_amd.arena import play_arena
    from betazero_amd.augment import augment_examples
    from betazero_amd.engine import PipelinedSelfPlay
    from betazero_amd.examples import concat
    from betazero_amd.mlp import PVTrainer, TicTacToePVNet
    from betazero_amd.ttt_yardstick import minimax_targets, yardstick
    _, z = fix
    own, opp, _ = _canon(z)
    targets = minimax_targets(own, opp)
    assert targets[0][0] == 0 and set(np.unique(targets[0])) == {-1.0, 0.0, 1.0} and targets[1].any(1).all()
    torch.manual_seed(64)
    tr = PVTrainer(TicTacToePVNet(64), lr=1e-3, max_batch=1024)
    before = yardstick(tr.device_mlp, own, opp, targets)
    gen = torch.Generator(device="cuda"); gen.manual_seed(64)
    window, rows = [], 0
    for it in range(3):
        sp = PipelinedSelfPlay("ttt", 512, 32, "mlp_bf16", net=tr.device_mlp, temp_moves=4, dirichlet_eps=0.25, dirichlet_alpha=1.0,
                               seed=64 + it)
        sp.run_iteration()
        ex = augment_examples(sp.device_examples())
        rows += len(ex)
        window.append(ex)
        hist = tr.fit_examples(concat(window), epochs=2, generator=gen)
        assert len(hist) == 2 and np.isfinite(hist[-1]["loss"])
    after = yardstick(tr.device_mlp, own, opp, targets)
    print(f"loop in small: rows {rows}, value MSE {before['value_mse']:.4f} -> {after['value_mse']:.4f}, "
          f"optimal top-1 {before['optimal_top1']:.3f} -> {after['optimal_top1']:.3f}")
    assert tr.error() == 0 and rows > 0 and torch.isfinite(tr.p).all()
    assert after["value_mse"] < before["value_mse"], (before, after)
    ev = tr.evaluate(window[-1])
    assert set(ev) >= {"policy_ce", "value_mse", "top1"} and np.isfinite(ev["policy_ce"]) and 0.0 <= ev["top1"] <= 1.0
    res = play_arena("ttt", 64, 50, opponent_depth=9, evaluator="mlp_bf16", net=tr.device_mlp)
    assert res.summary()["games"] == 64
