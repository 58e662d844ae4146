"""The tic-tac-toe MLP kernels (csrc/bz_mlp.hip) against plain references of the same operations, at every hidden size:
- the fp32 forward bit for bit against the C oracle (orc_mlp_forward_f32, DESIGN.md 11's operation order);
- the bf16 forward bit for bit on nets whose every intermediate value is exact in bf16 and fp32 (so the MFMA's summation
  order cannot matter and any fragment / bias mapping error is a bit difference);
- the training step one step at a time against an fp64 step from the same (p, m, v), with tolerances derived from the
  operations' rounding, not tuned;
- the error word, the forward after training steps (Adam's transposed copy, the fragment repack), and the search with
  mlp_bf16 against an external engine fed the same logits."""
import numpy as np
import pytest
import torch

from test_gpu_mlp import _augmented_csv, _external_fn

pytestmark = pytest.mark.gpu

HS = list(range(32, 513, 32))
U = 2.0 ** -24  # fp32 unit roundoff


def _gam(k):
    """gamma_k = k u / (1 - k u): the relative bound of a recursive sum (or fmaf chain) of k fp32 terms"""
    return k * U / (1 - k * U)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------- positions
_LINES = [(0, 1, 2), (3, 4, 5), (6, 7, 8), (0, 3, 6), (1, 4, 7), (2, 5, 8), (0, 4, 8), (2, 4, 6)]
_POS = None


def _positions():
    """every position reachable from the empty board (games stop at a line or a full board) as side-to-move bitboards
    (own, opp) uint64 [5478], in breadth-first order"""
    global _POS
    if _POS is None:
        masks = [sum(1 << c for c in ln) for ln in _LINES]
        seen, order, frontier = {(0, 0)}, [(0, 0)], [(0, 0)]
        while frontier:
            nxt = []
            for own, opp in frontier:
                if any(opp & m == m for m in masks) or (own | opp) == 0x1FF:
                    continue  # the player who just moved (opp) won, or the board is full
                for c in range(9):
                    if not (own | opp) >> c & 1:
                        child = (opp, own | 1 << c)
                        if child not in seen:
                            seen.add(child); order.append(child); nxt.append(child)
            frontier = nxt
        _POS = (np.array([o for o, _ in order], np.uint64), np.array([p for _, p in order], np.uint64))
    return _POS


def test_reachable_positions():
    own, opp = _positions()
    assert own.size == 5478 and not (own & opp).any()
    from oracle import oracle as orc
    x = orc.ttt_states(own, opp)
    assert np.unique(x, axis=0).shape[0] == 5478


def _oracle_rows(H):
    """the positions the C oracle recomputes at H: all of them up to H = 128, above that a seeded subset of
    400 * (512 / H)^2 (1,600 at H = 256, 400 at H = 512) -- the oracle costs ~0.7 ms per position at H = 512.  The other rows
    are pinned by the kernel's batch independence (checked below)."""
    n = min(5478, 400 * 512 * 512 // (H * H))
    if n == 5478:
        return np.arange(5478)
    return np.sort(np.random.RandomState(H).choice(5478, n, replace=False))


# ---------------------------------------------------------------- a. fp32 forward, bit for bit
@pytest.mark.parametrize("H", HS)
def test_f32_forward_bitexact_vs_oracle(H):
    from betazero_amd.mlp import DeviceMLP, TicTacToeNet
    from oracle import oracle as orc
    own, opp = _positions()
    xs = orc.ttt_states(own, opp)
    xr = np.random.RandomState(1000 + H).randn(5478, 9).astype(np.float32)  # beyond {-1, 0, 1}
    sub = _oracle_rows(H)
    torch.manual_seed(H)
    p1 = TicTacToeNet(9, H, 9).flat_params()
    ob, os_ = torch.as_tensor(own.view(np.int64)).cuda(), torch.as_tensor(opp.view(np.int64)).cuda()
    for p in (p1, (p1 * 8).astype(np.float32)):  # x8: weights, activations and logits leave [-1, 1]
        net = DeviceMLP(H, p, max_batch=5478)
        lb = net.forward(ob, os_).cpu().numpy()
        ls = net.forward_states(xs).cpu().numpy()
        lr = net.forward_states(xr).cpu().numpy()
        assert np.array_equal(_bits(lb), _bits(ls))
        assert np.array_equal(_bits(lb[sub]), _bits(orc.mlp_forward_f32(H, p, xs[sub])))
        assert np.array_equal(_bits(lr[sub]), _bits(orc.mlp_forward_f32(H, p, xr[sub])))
        rng = np.random.RandomState(H + 1)
        for n in (1, 15, 16, 17, 4520):
            idx = rng.choice(sub, n, replace=False) if n <= sub.size else rng.choice(5478, n, replace=False)
            small = DeviceMLP(H, p, max_batch=n)
            assert np.array_equal(_bits(small.forward(ob[idx], os_[idx]).cpu().numpy()), _bits(lb[idx]))
            assert np.array_equal(_bits(small.forward_states(xr[idx]).cpu().numpy()), _bits(lr[idx]))
        if H == 256:  # the default max_batch, full
            big = DeviceMLP(H, p)
            assert big.max_batch == 65536
            idx = np.resize(np.arange(5478), 65536)
            assert np.array_equal(_bits(big.forward(ob[idx], os_[idx]).cpu().numpy()), _bits(lb[idx]))
            xb = np.random.RandomState(7).randn(65536, 9).astype(np.float32)
            lbig = big.forward_states(xb).cpu().numpy()
            tail = np.arange(65536 - 300, 65536)
            assert np.array_equal(_bits(lbig[tail]), _bits(orc.mlp_forward_f32(H, p, xb[tail])))


# ---------------------------------------------------------------- b. bf16 forward, bit for bit on exact nets
def _exact_net(H, seed, scaled):
    """fc1..fc3: every output row has 3 nonzero weights in {-1, +1}; the t-th of row rho(j) sits in column
    sigma((j + t) mod K) for a seeded permutation sigma of the K inputs and rho of the N outputs, so every column of every
    layer is used; biases in {-1, 0, 1}.  fc4: dense +-1, biases in {-1, 0, 1}.  On ternary inputs the post-ReLU
    activations are integers <= 4, 13, 40 and the logits integers <= 512 * 40 + 1.  scaled: every weight and bias x 2^-3.
    Returns the fp64 [(W, b)] and the flat fp32 vector in torch's order."""
    rng = np.random.RandomState(seed)
    layers = []
    for K, N in ((9, H), (H, H), (H, H)):
        W = np.zeros((N, K))
        sigma, rho = rng.permutation(K), rng.permutation(N)
        cols = sigma[(np.arange(N)[:, None] + np.arange(3)) % K]
        W[rho[:, None], cols] = rng.choice([-1.0, 1.0], (N, 3))
        layers.append((W, rng.randint(-1, 2, N).astype(np.float64)))
    layers.append((rng.choice([-1.0, 1.0], (9, H)), rng.randint(-1, 2, 9).astype(np.float64)))
    if scaled:
        layers = [(W / 8, b / 8) for W, b in layers]
    flat = np.concatenate([t.reshape(-1) for W, b in layers for t in (W, b)]).astype(np.float32)
    assert np.array_equal(flat.astype(np.float64), np.concatenate([t.reshape(-1) for W, b in layers for t in (W, b)]))
    return layers, flat


def _exact_forward(layers, x, scaled):
    """fp64 forward; asserts that every activation is exact in bf16 (an integer multiple of 2^-3l with fewer than 8
    significant bits) and the logits exact in fp32 (a multiple of 2^-12 below 2^12, or an integer below 2^24)"""
    a = x.astype(np.float64)
    for l, (W, b) in enumerate(layers):
        y = a @ W.T + b
        q = 2.0 ** (3 * (l + 1)) if scaled else 1.0
        if l < 3:
            a = np.maximum(y, 0.0)
            assert np.array_equal(a * q, np.round(a * q)) and (a * q).max() < 2 ** 8
        else:
            assert np.array_equal(y * q, np.round(y * q)) and np.abs(y * q).max() < 2 ** 24
    return y


@pytest.mark.parametrize("H", HS)
def test_bf16_forward_bitexact_on_exact_nets(H):
    from betazero_amd.mlp import DeviceMLP
    from oracle import oracle as orc
    own, opp = _positions()
    xs = orc.ttt_states(own, opp)
    ob, os_ = torch.as_tensor(own.view(np.int64)).cuda(), torch.as_tensor(opp.view(np.int64)).cuda()
    for scaled in (False, True):
        layers, flat = _exact_net(H, 2000 + H, scaled)
        ref = _exact_forward(layers, xs, scaled).astype(np.float32)
        assert np.abs(ref).max() >= (2.0 ** -3 if scaled else 8) and (ref != 0).mean() > 0.5  # not a dead net
        net = DeviceMLP(H, flat, max_batch=5478)
        for lg in (net.forward(ob, os_, bf16=True), net.forward_states(xs, bf16=True), net.forward(ob, os_)):
            assert np.array_equal(_bits(lg.cpu().numpy()), _bits(ref))


@pytest.mark.parametrize("H", HS)
def test_bf16_rows_independent_of_batch(H):
    from betazero_amd.mlp import DeviceMLP, TicTacToeNet
    from oracle import oracle as orc
    own, opp = _positions()
    xs = orc.ttt_states(own, opp)
    torch.manual_seed(3000 + H)
    p = TicTacToeNet(9, H, 9).flat_params()
    full = DeviceMLP(H, p, max_batch=5478).forward_states(xs, bf16=True).cpu().numpy()
    rng = np.random.RandomState(H)
    for n in (1, 17, 4520):
        idx = rng.choice(5478, n, replace=False)
        net = DeviceMLP(H, p, max_batch=n)
        ob = torch.as_tensor(own[idx].view(np.int64)).cuda()
        os_ = torch.as_tensor(opp[idx].view(np.int64)).cuda()
        assert np.array_equal(_bits(net.forward(ob, os_, bf16=True).cpu().numpy()), _bits(full[idx]))
        assert np.array_equal(_bits(net.forward_states(xs[idx], bf16=True).cpu().numpy()), _bits(full[idx]))


# ---------------------------------------------------------------- c. the training step against fp64, one step at a time
def _unflat(p, H):
    shapes = [(H, 9), (H,), (H, H), (H,), (H, H), (H,), (9, H), (9,)]
    out, o = [], 0
    for s in shapes:
        k = int(np.prod(s))
        out.append(p[o:o + k].reshape(s))
        o += k
    return out


def _ref_step(H, p0, m0, v0, x, t, w, hp, step):
    """One SL step in fp64 from the kernel's pre-step (p, m, v), and an elementwise bound on how far an fp32 computation
    in the kernel's operation order may lie from it.  Every bound is the rounding of the operation that produces the value
    plus the propagation of its inputs' bounds:
    - forward: an fmaf chain of K terms from 0, then + b: gamma(K+1) (sum |w a| + |b|), plus |W| e_in (ReLU: 1-Lipschitz);
      a unit whose fp64 pre-activation lies within its bound of 0 is "ambiguous": its ReLU mask may differ;
    - softmax-CE: CE is 2-Lipschitz in max|dz|; softmax moves by a factor expm1(2 max|dz|); expf / logf / the 9-term sum /
      the divisions add a few u; w / sum w: gamma(n) + 2u;
    - backward-data: an fmaf chain of N terms: gamma(N) |d| |W|, plus |ed| |W|; on an ambiguous unit the whole value;
    - weight gradient: an fmaf chain over the n rows: gamma(n) sum |d a| + sum(ed |a| + |d| ea + ed ea); bias: gamma(n) sum |d| + sum ed;
    - Adam (torch's formula order at the float32 beta / lr / eps the ABI carries, bias corrections in double): the
      gradient's bound through m = m + (1 - b1)(g - m), v = v b2 + (1 - b2) g^2, p -= lr/bc1 m / (sqrt(v)/sqrt(bc2) + eps),
      plus 4u per result for the fp32 operations.
    Returns (reference, bound) dicts."""
    f64 = np.float64
    P = _unflat(p0.astype(f64), H)
    Ws, bs = P[0::2], P[1::2]
    n = x.shape[0]
    ar = np.arange(n)
    # gradient and loss by autograd, TicTacToeNet in double
    from betazero_amd.mlp import TicTacToeNet
    mod = TicTacToeNet(9, H, 9).double()
    with torch.no_grad():
        for fc, W, b in zip((mod.fc1, mod.fc2, mod.fc3, mod.fc4), Ws, bs):
            fc.weight.copy_(torch.from_numpy(W)); fc.bias.copy_(torch.from_numpy(b))
    xt, wt = torch.from_numpy(x.astype(f64)), torch.from_numpy(w.astype(f64))
    ce_t = torch.nn.functional.cross_entropy(mod(xt), torch.from_numpy(t.astype(np.int64)), reduction="none")
    loss_t = (wt * ce_t).sum() / wt.sum()
    loss_t.backward()
    g = torch.cat([q.grad.reshape(-1) for fc in (mod.fc1, mod.fc2, mod.fc3, mod.fc4) for q in (fc.weight, fc.bias)]).numpy()
    # the same step by hand, carrying the bounds
    a, ea, amb = [x.astype(f64)], [np.zeros((n, 9))], []
    for l in range(4):
        W, b = Ws[l], bs[l]
        y = a[-1] @ W.T + b
        ey = _gam(W.shape[1] + 1) * (np.abs(a[-1]) @ np.abs(W).T + np.abs(b)) + ea[-1] @ np.abs(W).T
        if l < 3:
            amb.append(np.abs(y) <= ey); a.append(np.maximum(y, 0.0)); ea.append(ey)
        else:
            z, ez = y, ey
    sw = w.astype(f64).sum()
    sc = w.astype(f64) / sw
    zm = z.max(1)
    ex = np.exp(z - zm[:, None]); s = ex.sum(1); pr = ex / s[:, None]
    ce = zm + np.log(s) - z[ar, t]
    oh = np.zeros_like(z); oh[ar, t] = 1.0
    Ez = ez.max(1)
    esc = _gam(n) + 2 * U
    rel_p = np.expm1(2 * Ez + 2 * U * np.abs(z - zm[:, None]).max(1)) + 16 * U
    g4 = sc[:, None] * (pr - oh)
    eg4 = np.abs(sc)[:, None] * (rel_p[:, None] * pr + U * np.abs(pr - oh)) + np.abs(g4) * (esc + U)
    ece = 2 * Ez + 8 * U * (np.abs(zm) + np.abs(np.log(s)) + np.abs(z[ar, t])) + 2 * (_gam(9) + 8 * U)
    tl = np.abs(sc * ce)
    eloss = (np.abs(sc) * ece + tl * (esc + U)).sum() + _gam(n) * tl.sum()
    d, ed = [None] * 4, [None] * 4
    d[3], ed[3] = g4, eg4
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
    assert abs(loss_t.item() - (sc * ce).sum()) <= 1e-12 * abs(loss_t.item())
    # Adam at the float32 hyper-parameters
    lr, b1, b2, eps = (float(np.float32(q)) for q in hp)
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    ss, bc2s = lr / bc1, np.sqrt(bc2)
    m0, v0, p0 = m0.astype(f64), v0.astype(f64), p0.astype(f64)
    m1 = m0 + (1 - b1) * (g - m0)
    v1 = v0 * b2 + (1 - b2) * g * g
    den = np.sqrt(v1) / bc2s + eps
    p1 = p0 - ss * m1 / den
    em = (1 - b1) * eg + 4 * U * (np.abs(m1) + (1 - b1) * np.abs(g - m0))
    ev = (1 - b2) * (2 * np.abs(g) * eg + eg * eg) + 4 * U * v1
    lo = np.sqrt(np.maximum(v1 - ev, 0.0))
    esq = np.where(np.sqrt(v1) + lo > 0, ev / np.maximum(np.sqrt(v1) + lo, 1e-300), np.sqrt(ev))
    eden = esq / bc2s + 4 * U * den
    den_lo = np.maximum(den - eden, eps)
    upd = ss * m1 / den
    ep = ss * (em / den_lo + np.abs(m1) * eden / (den * den_lo)) + 4 * U * np.abs(upd) + U * np.abs(p1)
    ref = {"loss": loss_t.item(), "grad": g, "m": m1, "v": v1, "p": p1, "z": z}
    bnd = {"loss": eloss, "grad": eg, "m": em, "v": ev, "p": ep}
    return ref, bnd, (lr, b1, b2, eps, ss, bc2s)


def _adam_moments(g, m0, v0, c1, b2, c2):
    """Adam's moments in fp64 on the kernel's own gradient, with (1 - beta1, beta2, 1 - beta2) = (c1, b2, c2): isolates the
    update's arithmetic (and its beta convention) from the gradient's"""
    g, m0, v0 = (q.astype(np.float64) for q in (g, m0, v0))
    return m0 + c1 * (g - m0), v0 * b2 + c2 * g * g


# (H, n, row weights, Adam, rows); every value of each axis appears at least once, H = 512 with n = 1,000 once
_DEFAULT = (1e-4, 0.9, 0.999, 1e-8)
_CUSTOM = (3e-3, 0.8, 0.95, 1e-3)
_CASES = [(32, 1, "ones", "default", "csv"), (96, 3, "frac", "custom", "ternary"), (256, 4, "zeros", "default", "ternary"),
          (32, 5, "zeros", "custom", "csv"), (96, 127, "frac", "default", "csv"), (256, 128, "ones", "custom", "csv"),
          (512, 1000, "frac", "custom", "ternary")]


def _row_weights(kind, n, rng):
    if kind == "ones":
        return np.ones(n, np.float32)
    if kind == "frac":
        return rng.uniform(0.1, 2.0, n).astype(np.float32)
    w = (rng.rand(n) > 0.3).astype(np.float32)
    w[0], w[-1] = 1.0, 0.0  # at least one row of each
    return w


def _check_step(tr, x, t, w, p0, m0, v0, hp):
    """compare what the step left in tr with the fp64 step from (p0, m0, v0)"""
    from oracle import oracle as orc
    H, n = tr.H, x.shape[0]
    ref, bnd, hps = _ref_step(H, p0, m0, v0, x, t, w, hp, tr.adam.step)
    loss = float(tr.loss.cpu()[0])
    g, m, v, p = (q.cpu().numpy().astype(np.float64) for q in (tr.grad, tr.m, tr.v, tr.p))
    # the bounds are first order in u: x2 covers the second-order terms
    assert abs(loss - ref["loss"]) <= 2 * bnd["loss"], (loss, ref["loss"], bnd["loss"])
    o = 0
    for k in (9 * H, H, H * H, H, H * H, H, 9 * H, 9):  # per tensor
        s_ = slice(o, o + k); o += k
        bad = np.abs(g[s_] - ref["grad"][s_]) > 2 * bnd["grad"][s_]
        assert not bad.any(), (s_, np.flatnonzero(bad)[:5], g[s_][bad][:5], ref["grad"][s_][bad][:5])
    for key, val in (("m", m), ("v", v), ("p", p)):
        bad = np.abs(val - ref[key]) > 2 * bnd[key]
        assert not bad.any(), (key, np.flatnonzero(bad)[:5], val[bad][:5], ref[key][bad][:5], bnd[key][bad][:5])
    # Adam on the kernel's own gradient: m, v within 4 u (one rounding per fp32 operation), p within 8 u of the update
    lr, b1, b2, eps, ss, bc2s = hps
    m1, v1 = _adam_moments(g, m0, v0, 1 - b1, b2, 1 - b2)  # the float32 betas: 1 - b is exact in fp32
    assert (np.abs(m - m1) <= 4 * U * (np.abs(m1) + (1 - b1) * np.abs(g - m0))).all()
    assert (np.abs(v - v1) <= 4 * U * v1).all()
    p1 = p0.astype(np.float64) - ss * m / (np.sqrt(v) / bc2s + eps)
    assert (np.abs(p - p1) <= 8 * U * np.abs(ss * m / (np.sqrt(v) / bc2s + eps)) + U * np.abs(p1)).all()
    # the training forward's logits: f32_layer, bit for bit with the oracle on the pre-step parameters
    r = min(n, 128)
    assert np.array_equal(_bits(tr.logits[:r].cpu().numpy()), _bits(orc.mlp_forward_f32(H, p0, x[:r])))
    return g, v, v1


@pytest.mark.parametrize("H,n,wkind,adam,rows", _CASES)
def test_training_steps_match_fp64(H, n, wkind, adam, rows):
    from betazero_amd.mlp import MLPTrainer, TicTacToeNet
    rng = np.random.RandomState(H * 1000 + n)
    torch.manual_seed(H + n)
    hp = _DEFAULT if adam == "default" else _CUSTOM
    tr = MLPTrainer(TicTacToeNet(9, H, 9), lr=hp[0], betas=hp[1:3], eps=hp[3], max_batch=n)
    S, T = _augmented_csv()
    for step in range(30):
        if rows == "csv":
            idx = rng.choice(len(S), n, replace=False)
            x, t = S[idx], T[idx].astype(np.int32)
        else:
            x = rng.randint(-1, 2, (n, 9)).astype(np.float32)
            t = rng.randint(0, 9, n).astype(np.int32)
        w = _row_weights(wkind, n, rng)
        p0, m0, v0 = (q.cpu().numpy().copy() for q in (tr.p, tr.m, tr.v))
        tr.step(x, t, None if wkind == "ones" else w)
        assert tr.error() == 0
        g, v, v1 = _check_step(tr, x, t, w, p0, m0, v0, hp)
        if step == 0 and hp[2] == 0.999:
            # v follows the float32-beta convention: 1 - beta2 in fp32 from the float beta2.  Torch's double
            # 1 - beta2 (cast to fp32) differs by 1.3e-5 relative at beta2 = 0.999 -- far outside 4 u.  (At 0.95 the two
            # differ by 2.4e-7, about 4 u: not told apart.)
            b2f = float(np.float32(hp[2]))
            _, vd = _adam_moments(g, m0, v0, 0.0, b2f, float(np.float32(1 - hp[2])))
            nz = g != 0
            assert nz.mean() > 0.1
            assert (np.abs(vd - v1)[nz] > 4 * U * v1[nz]).mean() > 0.99


# ---------------------------------------------------------------- d. the error word
def test_error_word_zero_weights_and_nonfinite_loss():
    from betazero_amd.mlp import MLPTrainer, TicTacToeNet
    S, T = _augmented_csv()
    torch.manual_seed(21)
    tr = MLPTrainer(TicTacToeNet(9, 64, 9), lr=3e-3, betas=(0.8, 0.95), eps=1e-3, max_batch=64)
    x, t = S[:64].copy(), T[:64].astype(np.int32)
    tr.step(x, t)
    assert tr.error() == 0
    for make, bit in ((lambda: (x, np.zeros(64, np.float32)), 4), (lambda: (_with_inf(x), np.ones(64, np.float32)), 2)):
        xx, w = make()
        before = [q.clone() for q in (tr.p, tr.m, tr.v)]
        tr.step(xx, t, w)
        assert tr.error() & bit
        if bit == 2:
            lg = tr.logits[:64].cpu().numpy()
            assert not np.isfinite(lg[5]).all()
        for a_, b_ in zip(before, (tr.p, tr.m, tr.v)):
            assert torch.equal(a_.view(torch.int32), b_.view(torch.int32))
        tr.clear_error()
        p0, m0, v0 = (q.cpu().numpy().copy() for q in (tr.p, tr.m, tr.v))
        w1 = np.ones(64, np.float32)
        tr.step(x, t, w1)
        assert tr.error() == 0
        assert not torch.equal(tr.p, before[0])
        _check_step(tr, x, t, w1, p0, m0, v0, (3e-3, 0.8, 0.95, 1e-3))


def _with_inf(x):
    y = x.copy()
    y[5, 4] = np.inf  # a weighted row; 1e30 could leave the logits finite
    return y


# ---------------------------------------------------------------- e. training, then forward
def _fwd_all(net, bf16, states=False):
    from oracle import oracle as orc
    own, opp = _positions()
    out = []
    for i in range(0, 5478, 1024):  # MLPTrainer's DeviceMLP holds max_batch 1024
        if states:
            out.append(net.forward_states(orc.ttt_states(own[i:i + 1024], opp[i:i + 1024]), bf16=bf16).cpu().numpy())
        else:
            out.append(net.forward(own[i:i + 1024], opp[i:i + 1024], bf16=bf16).cpu().numpy())
    return np.concatenate(out)


@pytest.mark.parametrize("k", [1, 7])
def test_forward_after_training_equals_fresh_upload(k):
    from betazero_amd.mlp import DeviceMLP, MLPTrainer, TicTacToeNet
    S, T = _augmented_csv()
    torch.manual_seed(30 + k)
    tr = MLPTrainer(TicTacToeNet(9, 96, 9), lr=3e-3)
    rng = np.random.RandomState(k)
    for _ in range(k):
        idx = rng.choice(len(S), 128, replace=False)
        tr.step(S[idx], T[idx])
    assert tr.error() == 0
    fresh = DeviceMLP.from_module(tr.to_module(), max_batch=1024)
    for bf16 in (False, True):
        for states in (False, True):
            assert np.array_equal(_bits(_fwd_all(tr.mlp, bf16, states)), _bits(_fwd_all(fresh, bf16, states)))


def test_bf16_forward_sees_every_step():
    from betazero_amd.mlp import DeviceMLP, MLPTrainer, TicTacToeNet
    S, T = _augmented_csv()
    torch.manual_seed(40)
    tr = MLPTrainer(TicTacToeNet(9, 160, 9), lr=3e-3)
    prev = None
    for i in range(3):
        got = _fwd_all(tr.mlp, True)
        want = _fwd_all(DeviceMLP(160, tr.params(), max_batch=1024), True)
        assert np.array_equal(_bits(got), _bits(want)), i
        assert prev is None or not np.array_equal(got, prev)
        prev = got
        if i < 2:
            tr.step(S[64 * i:64 * i + 128], T[64 * i:64 * i + 128])
    assert tr.error() == 0


# ---------------------------------------------------------------- f. the search with mlp_bf16
def _external_bf16(net):
    def fn(own, opp, kind):
        return net.forward(own, opp, bf16=True), torch.zeros(own.numel(), dtype=torch.float32, device=own.device)
    return fn


def test_search_mlp_bf16_equals_external(fix):
    from betazero_amd.engine import SelfPlayEngine
    from betazero_amd.mlp import DeviceMLP
    m, z = fix
    net = DeviceMLP.from_module(m, max_batch=256)
    rng = np.random.RandomState(2)
    idx = rng.choice(len(z["move"]), 64, replace=False)
    tm = z["to_move"][idx]
    own = np.where(tm == 1, z["x_bits"][idx], z["o_bits"][idx]).astype(np.uint64)
    opp = np.where(tm == 1, z["o_bits"][idx], z["x_bits"][idx]).astype(np.uint64)
    a = SelfPlayEngine("ttt", 64, 100, "mlp_bf16", net=net)
    b = SelfPlayEngine("ttt", 64, 100, "external")
    a.set_roots(own, opp, tm); a.search()
    b.set_roots(own, opp, tm); b.search_external(_external_bf16(net))
    Na, Wa, Pa = a.root_stats()
    Nb, Wb, Pb = b.root_stats()
    assert Na.sum() > 0
    assert np.array_equal(Na, Nb) and np.array_equal(Wa.view(np.uint32), Wb.view(np.uint32))
    assert np.array_equal(Pa.view(np.uint32), Pb.view(np.uint32))
    # and the bf16 priors are not the f32 ones (the test would not tell the evaluators apart otherwise)
    c = SelfPlayEngine("ttt", 64, 100, "external")
    c.set_roots(own, opp, tm); c.search_external(_external_fn(net))
    assert not np.array_equal(Pa.view(np.uint32), c.root_stats()[2].view(np.uint32))


def test_self_play_mlp_bf16_equals_external(fix):
    from betazero_amd.engine import SelfPlayEngine, self_play
    from betazero_amd.mlp import DeviceMLP
    m, _ = fix
    net = DeviceMLP.from_module(m, max_batch=256)
    _, _, _, ex = self_play("ttt", 64, 100, net=net, evaluator="mlp_bf16", temp_moves=4, seed=5, pipelines=1)
    b = SelfPlayEngine("ttt", 64, 100, "external", temp_moves=4, seed=5)
    b.reset_games()
    for _ in range(12):
        b.search_external(_external_bf16(net))
        b.play(False)
        if b.status()[0] == 0:
            break
    eb = b.examples()
    assert len(ex.act) == len(eb.act) > 0
    assert np.unique(np.bincount(ex.game.astype(np.int64))).size > 1  # the games end at different plies
    assert np.array_equal(ex.act, eb.act) and np.array_equal(ex.pi.view(np.uint32), eb.pi.view(np.uint32))
    assert np.array_equal(ex.z, eb.z)


@pytest.fixture(scope="module")
def fix():
    import os
    from betazero_amd.mlp import TicTacToeNet
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ttt_mlp.npz"))
    m = TicTacToeNet(9, z["fc1_w"].shape[0], 9)
    m.load_state_dict({f"fc{l}.{k}": torch.from_numpy(z[f"fc{l}_{k[0]}"]) for l in (1, 2, 3, 4) for k in ("weight", "bias")})
    return m.eval(), z
