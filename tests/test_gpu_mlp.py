"""The tic-tac-toe MLP on the MI355X: forward against the reference's logits and moves (ttt_mlp.npz), the training step
against torch fp32 autograd + torch.optim.Adam, and the MLP evaluators in the search against an external engine fed the
same logits."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def fix():
    from betazero_amd.mlp import TicTacToeNet
    z = np.load(os.path.join(GOLD, "ttt_mlp.npz"))
    m = TicTacToeNet(9, z["fc1_w"].shape[0], 9)
    m.load_state_dict({f"fc{l}.{k}": torch.from_numpy(z[f"fc{l}_{k[0]}"]) for l in (1, 2, 3, 4) for k in ("weight", "bias")})
    return m.eval(), z


def _legal_best(logits, states):
    masked = np.where(states == 0, logits, -np.inf)
    return masked.argmax(1), np.sort(masked, 1)

def _canon(z):
    """side-to-move bitboards (own, opp) of the fixture positions"""
    x, o, tm = z["x_bits"], z["o_bits"], z["to_move"]
    own = np.where(tm == 1, x, o)
    opp = np.where(tm == 1, o, x)
    return torch.as_tensor(own).cuda(), torch.as_tensor(opp).cuda()

def test_forward_f32_matches_reference(fix):
    from betazero_amd.mlp import DeviceMLP
    m, z = fix
    net = DeviceMLP.from_module(m, max_batch=4520)
    own, opp = _canon(z)
    lg = net.forward(own, opp).cpu().numpy()
    ls = net.forward_states(torch.as_tensor(z["states"])).cpu().numpy()
    assert np.array_equal(lg.view(np.uint32), ls.view(np.uint32))  # both entry points: the same x, the same bits
    assert np.abs(lg - z["logits"]).max() <= 1e-4
    best, srt = _legal_best(lg, z["states"])
    _, rsrt = _legal_best(z["logits"], z["states"])
    clear = rsrt[:, -1] - rsrt[:, -2] > 1e-4
    assert np.array_equal(best[clear], z["move"][clear])
    # a row's result does not depend on its batch: n = 1 and a batch that is not a multiple of the tile
    for idx in ([0], [4519], list(range(7, 44)), list(range(100, 117))):
        sub = net.forward(own[idx], opp[idx]).cpu().numpy()
        assert np.array_equal(sub.view(np.uint32), lg[idx].view(np.uint32))
    again = net.forward(own, opp).cpu().numpy()
    assert np.array_equal(again.view(np.uint32), lg.view(np.uint32))

def test_forward_bf16_matches_reference(fix):
    from betazero_amd.mlp import DeviceMLP
    m, z = fix
    net = DeviceMLP.from_module(m, max_batch=4520)
    own, opp = _canon(z)
    lg = net.forward(own, opp, bf16=True).cpu().numpy()
    ls = net.forward_states(torch.as_tensor(z["states"]), bf16=True).cpu().numpy()
    assert np.array_equal(lg.view(np.uint32), ls.view(np.uint32))
    err = np.abs(lg - z["logits"])
    assert err.max() <= 0.05
    assert (err.max(1) / np.abs(z["logits"]).max(1)).max() <= 0.01
    best, _ = _legal_best(lg, z["states"])
    assert (best == z["move"]).mean() >= 0.995
    for idx in ([3], list(range(0, 37))):
        sub = net.forward(own[idx], opp[idx], bf16=True).cpu().numpy()
        assert np.array_equal(sub.view(np.uint32), lg[idx].view(np.uint32))

def _bf16_emulation(m, x):
    """bf16 weights and activations, fp32 accumulation (torch CPU, fp64 sums rounded once: the order differs from the
    MFMA's, the tolerance below covers that)"""
    def r(t):
        return t.to(torch.bfloat16).to(torch.float64)
    a = r(x.to(torch.float64))
    for i, fc in enumerate((m.fc1, m.fc2, m.fc3, m.fc4)):
        y = a @ r(fc.weight.detach()).T + fc.bias.detach().to(torch.float64)
        a = r(torch.relu(y)) if i < 3 else y
    return a

@pytest.mark.parametrize("H", list(range(32, 513, 32)))
def test_forward_hidden_sizes(H):
    from betazero_amd.mlp import DeviceMLP, TicTacToeNet
    torch.manual_seed(H)
    m = TicTacToeNet(9, H, 9).eval()
    net = DeviceMLP.from_module(m, max_batch=1000)
    x = torch.randint(-1, 2, (1000, 9)).to(torch.float32)
    with torch.no_grad():
        ref = m.double()(x.double()).float().numpy()
    m.float()
    for n in (1, 37, 1000):
        lg = net.forward_states(x[:n]).cpu().numpy()
        assert np.abs(lg - ref[:n]).max() <= 1e-5 * max(1.0, np.abs(ref).max())
        lb = net.forward_states(x[:n], bf16=True).cpu().numpy()
        em = _bf16_emulation(m, x[:n]).float().numpy()
        assert np.abs(lb - em).max() <= 2e-2 * max(1.0, np.abs(em).max())

# ---------------------------------------------------------------- training
def _augmented_csv():
    """ttt_csv.npz rows through SL/train.py's 8 transforms with its (state, action) dedupe, in its order"""
    z = np.load(os.path.join(GOLD, "ttt_csv.npz"))
    fns = [lambda a: a, lambda a: a[::-1, :], lambda a: a[:, ::-1], lambda a: np.rot90(a, 1), lambda a: np.rot90(a, 2),
           lambda a: np.rot90(a, 3), lambda a: a.T, lambda a: a[::-1, :].T]
    seen, S, A = set(), [], []
    for s, a in zip(z["states"], z["actions"]):
        for f in fns:
            ts, ta = np.ascontiguousarray(f(s.reshape(3, 3))), np.ascontiguousarray(f(a.reshape(3, 3)))
            key = (ts.tobytes(), ta.tobytes())
            if key not in seen:
                seen.add(key)
                S.append(ts.reshape(9)); A.append(ta.reshape(9))
    return np.array(S, np.float32), np.array(A, np.float32).argmax(1).astype(np.int64)

def _torch_steps(m, batches, lr=1e-4):
    m = m.cuda()
    opt = torch.optim.Adam(m.parameters(), lr=lr)
    crit = torch.nn.CrossEntropyLoss()
    losses = []
    for x, t in batches:
        opt.zero_grad()
        loss = crit(m(x.cuda()), t.cuda())
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return m.cpu(), losses

def test_one_training_step_matches_torch_adam():
    from betazero_amd.mlp import MLPTrainer, TicTacToeNet
    S, T = _augmented_csv()
    torch.manual_seed(5)
    m0 = TicTacToeNet(9, 256, 9)
    tr = MLPTrainer(m0)
    x, t = torch.from_numpy(S[:128]), torch.from_numpy(T[:128])
    loss = float(tr.step(x, t)[0])
    assert tr.error() == 0
    ref = TicTacToeNet(9, 256, 9).cuda()
    ref.load_state_dict(m0.state_dict())
    opt = torch.optim.Adam(ref.parameters(), lr=1e-4)
    rl = torch.nn.CrossEntropyLoss()(ref(x.cuda()), t.cuda())
    rl.backward()
    g_ref = torch.cat([q.grad.reshape(-1) for q in ref.parameters()]).cpu()
    opt.step()
    p_ref = torch.cat([q.detach().reshape(-1) for q in ref.parameters()]).cpu()
    assert abs(loss - rl.item()) <= 1e-6 * abs(rl.item())
    g, p = tr.grad.cpu(), tr.p.cpu()
    o = 0
    for q in ref.parameters():  # the batch gradient, per tensor
        s_ = slice(o, o + q.numel()); o += q.numel()
        assert (g[s_] - g_ref[s_]).abs().max() <= 1e-5 * g_ref[s_].abs().max()
    # Adam's first step is lr * g / (|g| + eps): where |g| >> eps every parameter is within 1e-6 relative; where |g| is
    # near eps = 1e-8 the step amplifies the last bits of g (summation order) -- there it is still a fraction of lr
    big = g_ref.abs() > 1e-6
    assert big.float().mean() > 0.5
    assert ((p - p_ref).abs()[big] <= 1e-6 * torch.maximum(p_ref.abs(), torch.tensor(1e-4))[big]).all()
    assert (p - p_ref).abs().max() <= 1e-4 * 0.1


def test_200_training_steps_match_torch_adam():
    from betazero_amd.mlp import MLPTrainer, TicTacToeNet
    S, T = _augmented_csv()
    rng = np.random.RandomState(0)
    batches = []
    while len(batches) < 200:
        perm = rng.permutation(len(S))
        for i in range(0, len(S), 128):  # the last batch of every pass is short
            idx = perm[i:i + 128]
            batches.append((torch.from_numpy(S[idx]), torch.from_numpy(T[idx])))
    batches = batches[:200]
    assert any(b[0].shape[0] < 128 for b in batches)
    torch.manual_seed(6)
    m0 = TicTacToeNet(9, 256, 9)
    tr = MLPTrainer(m0)
    losses = [float(tr.step(x, t)[0]) for x, t in batches]
    assert tr.error() == 0
    ref = TicTacToeNet(9, 256, 9); ref.load_state_dict(m0.state_dict())
    ref, rl = _torch_steps(ref, batches)
    assert np.abs(np.array(losses) - np.array(rl)).max() <= 1e-4 * np.abs(rl).max()
    assert losses[-1] < losses[0]
    for a_, b_ in zip(tr.to_module().parameters(), ref.parameters()):
        assert (a_.detach() - b_.detach()).abs().max() <= 1e-4

def test_zero_weight_row_and_bad_target():
    from betazero_amd.mlp import MLPTrainer, TicTacToeNet
    S, T = _augmented_csv()
    torch.manual_seed(7)
    m0 = TicTacToeNet(9, 64, 9)
    a, b = MLPTrainer(m0), MLPTrainer(m0)
    x, t = torch.from_numpy(S[:50]), torch.from_numpy(T[:50])
    w = torch.ones(50); w[49] = 0.0
    la = float(a.step(x, t, w)[0])
    lb = float(b.step(x[:49], t[:49])[0])
    assert a.error() == 0 and b.error() == 0
    assert la == lb and torch.equal(a.p, b.p) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)
    # a bad target on a zero-weight row is ignored; on a weighted row it sets the error word and changes nothing
    t2 = t.clone(); t2[49] = 9
    a.step(x, t2, w)
    assert a.error() == 0
    before = a.p.clone()
    a.step(x, t2)
    assert a.error() & 1 and torch.equal(a.p, before)
    a.clear_error()
    t2[0] = -1
    b.step(x[:49], t2[:49])
    assert b.error() & 1

def test_fit_reports_reference_metrics():
    from betazero_amd.mlp import MLPTrainer, TicTacToeNet
    S, A = _augmented_csv()
    onehot = np.eye(9, dtype=np.float32)[A]
    torch.manual_seed(8)
    tr = MLPTrainer(TicTacToeNet(9, 64, 9), lr=1e-3)  # (lr 1e-4 needs hundreds of epochs to move these numbers)
    hist = tr.fit(S, onehot, epochs=10)
    assert len(hist) == 10 and all(set(h) >= {"train_loss", "val_loss", "train_acc", "val_acc"} for h in hist)
    assert hist[-1]["train_loss"] < hist[0]["train_loss"] and 0.0 <= hist[-1]["val_acc"] <= 1.0
    assert tr.steps == 10 * -(-(len(S) - int(len(S) * 0.2)) // 128)

# ---------------------------------------------------------------- search
def _external_fn(net):
    def fn(own, opp, kind):
        return net.forward(own, opp), torch.zeros(own.numel(), dtype=torch.float32, device=own.device)
    return fn

def test_search_mlp_f32_equals_external(fix):
    from betazero_amd.engine import SelfPlayEngine
    from betazero_amd.mlp import DeviceMLP
    m, z = fix
    net = DeviceMLP.from_module(m, max_batch=256)
    rng = np.random.RandomState(1)
    idx = rng.choice(len(z["move"]), 64, replace=False)
    tm = z["to_move"][idx]
    own = np.where(tm == 1, z["x_bits"][idx], z["o_bits"][idx]).astype(np.uint64)
    opp = np.where(tm == 1, z["o_bits"][idx], z["x_bits"][idx]).astype(np.uint64)
    a = SelfPlayEngine("ttt", 64, 100, "mlp_f32", net=net)
    b = SelfPlayEngine("ttt", 64, 100, "external")
    a.set_roots(own, opp, tm); a.search()
    b.set_roots(own, opp, tm); b.search_external(_external_fn(net))
    Na, Wa, Pa = a.root_stats()
    Nb, Wb, Pb = b.root_stats()
    assert Na.sum() > 0
    assert np.array_equal(Na, Nb) and np.array_equal(Wa.view(np.uint32), Wb.view(np.uint32))
    assert np.array_equal(Pa.view(np.uint32), Pb.view(np.uint32))
    a.status(); b.status()

def test_self_play_mlp_f32_equals_external(fix):
    from betazero_amd.engine import SelfPlayEngine, self_play
    from betazero_amd.mlp import DeviceMLP
    m, _ = fix
    net = DeviceMLP.from_module(m, max_batch=256)
    _, _, _, ex = self_play("ttt", 32, 50, net=net, evaluator="mlp_f32", temp_moves=4, seed=3, pipelines=1)
    b = SelfPlayEngine("ttt", 32, 50, "external", temp_moves=4, seed=3)
    b.reset_games()
    for _ in range(12):
        b.search_external(_external_fn(net))
        b.play(False)
        if b.status()[0] == 0:
            break
    eb = b.examples()
    assert len(ex.act) == len(eb.act) > 0
    assert np.array_equal(ex.act, eb.act) and np.array_equal(ex.pi.view(np.uint32), eb.pi.view(np.uint32))
    assert np.array_equal(ex.z, eb.z)
    # bf16 in the loop runs whole games too
    _, _, _, ex2 = self_play("ttt", 32, 50, net=net, temp_moves=4, seed=3)
    assert len(ex2.act) > 0

def test_players_complete_games(fix):
    import betazero_amd as bz
    m, _ = fix
    net = bz.DeviceMLP.from_module(m, max_batch=16)
    random.seed(0)
    for make in (lambda s: bz.AIPlayer(net, s), lambda s: bz.AIPlayer(m, s, precision="bf16"),
                 lambda s: bz.MCTSPlayer(s, sims=64, net=net), lambda s: bz.MCTSPlayer(s, sims=64, net=net, evaluator="mlp_bf16")):
        for opp in (bz.OptimalPlayer, lambda s: bz.RandomPlayer()):
            for me in (1, -1):
                p1, p2 = (make(1), opp(-1)) if me == 1 else (opp(1), make(-1))
                positions, winner = bz.TicTacToeHeadless(p1, p2).play()  # raises on an illegal move
                assert len(positions) >= 6 and winner in (-1, 0, 1, None)

def test_mlp_refuses_reversi_and_conv_net_refuses_ttt(fix):
    import betazero_amd as bz
    from betazero_amd.net import DeviceNet, PolicyValueNet
    m, _ = fix
    net = bz.DeviceMLP.from_module(m, max_batch=16)
    with pytest.raises(ValueError, match="tic-tac-toe"):
        bz.MCTSPlayer(1, sims=8, net=net).get_move(bz.ReversiBoard())
    conv = DeviceNet.from_module(PolicyValueNet(64, 1, 16), 4)
    with pytest.raises(ValueError, match="Reversi boards"):
        bz.MCTSPlayer(1, sims=8, net=conv).get_move(bz.TicTacToeBoard())

def test_update_between_searches_takes_effect(fix):
    from betazero_amd.engine import SelfPlayEngine
    from betazero_amd.mlp import DeviceMLP, TicTacToeNet
    m, _ = fix
    net = DeviceMLP.from_module(m, max_batch=16)
    e = SelfPlayEngine("ttt", 1, 64, "mlp_f32", net=net)
    e.set_roots([0], [0], [1]); e.search()
    n1, _, p1 = e.root_stats()
    torch.manual_seed(11)
    other = TicTacToeNet(9, m.hidden_size, 9)
    net.update(other)
    e.set_roots([0], [0], [1]); e.search()
    n2, _, p2 = e.root_stats()
    fresh = DeviceMLP.from_module(other, max_batch=16)
    f = SelfPlayEngine("ttt", 1, 64, "mlp_f32", net=fresh)
    f.set_roots([0], [0], [1]); f.search()
    n3, _, p3 = f.root_stats()
    assert not np.array_equal(p1, p2)
    assert np.array_equal(n2, n3) and np.array_equal(p2.view(np.uint32), p3.view(np.uint32))
