"""The tic-tac-toe MLP with a value head without a GPU: TicTacToePVNet's parameter order and its two conversions to and from
the reference's policy net, the PV step's loss and gradients restated in fp64 against torch.autograd (the formulas that
tests/test_gpu_mlp_pv.py holds the kernel to), and the new bz_mlp entry points refusing bad arguments before anything launches."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from betazero_amd import _lib
from betazero_amd.mlp import DeviceMLP, TicTacToeNet, TicTacToePVNet

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "ttt_mlp.npz")


def _fixture_module():
    z = np.load(FIX)
    m = TicTacToeNet(9, z["fc1_w"].shape[0], 9)
    m.load_state_dict({f"fc{l}.{k}": torch.from_numpy(z[f"fc{l}_{k[0]}"]) for l in (1, 2, 3, 4) for k in ("weight", "bias")})
    return m.eval(), z


@pytest.mark.parametrize("H", [32, 256, 512])
def test_parameter_count_and_flat_order(H):
    torch.manual_seed(H)
    m = TicTacToePVNet(H)
    flat = m.flat_params()
    assert flat.dtype == np.float32 and flat.size == 2 * H * H + 22 * H + 10 == _lib.lib().bz_mlp_pv_param_count(H)
    assert flat.size == _lib.lib().bz_mlp_param_count(H) + H + 1
    want = np.concatenate([t.detach().numpy().reshape(-1) for t in (m.fc1.weight, m.fc1.bias, m.fc2.weight, m.fc2.bias,
                                                                     m.fc3.weight, m.fc3.bias, m.fc4.weight, m.fc4.bias)])
    assert np.array_equal(flat, want) and m.fc4.weight.shape == (10, H)
    # the value row is the last H weights of fc4.w and the last bias
    assert np.array_equal(flat[-10 - H:-10], m.fc4.weight[9].detach().numpy()) and flat[-1] == m.fc4.bias[9].item()
    m2 = TicTacToePVNet(H).load_flat_params_(flat)
    assert np.array_equal(m2.flat_params(), flat)
    x = torch.randint(-1, 2, (7, 9)).float()
    with torch.no_grad():
        lg, v = m(x)
        y = m.fc4(torch.relu(m.fc3(torch.relu(m.fc2(torch.relu(m.fc1(x)))))))
    assert lg.shape == (7, 9) and v.shape == (7,)
    assert torch.equal(lg, y[:, :9]) and torch.equal(v, torch.tanh(y[:, 9]))


def test_from_policy_net_keeps_the_logits_and_has_value_zero():
    m, z = _fixture_module()
    pv = TicTacToePVNet.from_policy_net(m)
    assert pv.hidden_size == m.hidden_size and not pv.training
    with torch.no_grad():
        lg, v = pv(torch.from_numpy(z["states"]))
    # one more output row changes the GEMM's shape: the logits agree to rounding, the value is exactly 0
    assert np.abs(lg.numpy() - z["logits"]).max() <= 1e-5 * np.abs(z["logits"]).max()
    assert v.shape == (4520,) and not v.numpy().any()
    assert not pv.fc4.weight[9].any() and pv.fc4.bias[9] == 0
    assert np.array_equal(pv.flat_params()[:-10 - 10 * m.hidden_size], m.flat_params()[:-9 - 9 * m.hidden_size])
    with pytest.raises(ValueError):
        TicTacToePVNet.from_policy_net(TicTacToeNet(9, 32, 8))


class _RefShaped(nn.Module):  # the reference's attribute layout, independent of betazero_amd.mlp
    def __init__(self, h):
        super().__init__()
        self.fc1, self.relu1 = nn.Linear(9, h), nn.ReLU()
        self.fc2, self.relu2 = nn.Linear(h, h), nn.ReLU()
        self.fc3, self.relu3 = nn.Linear(h, h), nn.ReLU()
        self.fc4 = nn.Linear(h, 9)


def test_policy_net_round_trip():
    torch.manual_seed(2)
    pv = TicTacToePVNet(64)
    pol = pv.policy_net()
    assert isinstance(pol, TicTacToeNet) and pol.fc4.out_features == 9
    ref = _RefShaped(64)
    ref.load_state_dict(pol.state_dict())            # what the reference's AIPlayer would load
    assert list(ref.state_dict()) == list(pol.state_dict())
    x = torch.randint(-1, 2, (50, 9)).float()
    with torch.no_grad():
        assert np.abs(pol(x).numpy() - pv(x)[0].numpy()).max() <= 1e-6
    back = TicTacToePVNet.from_policy_net(pol)
    for name in ("fc1", "fc2", "fc3"):
        for k, t in getattr(pv, name).state_dict().items():
            assert torch.equal(getattr(back, name).state_dict()[k], t)
    assert torch.equal(back.fc4.weight[:9], pv.fc4.weight[:9]) and torch.equal(back.fc4.bias[:9], pv.fc4.bias[:9])


def pv_step_fp64(layers, x, pi, vt, w, c):
    """The PV step's loss and gradients by hand in fp64, in the kernel's formulas: loss = sum_r (w_r / sum w) [ sum_o pi_o
    (lse(z) - z_o) + c (v - vt)^2 ]; on logit o: scale (S p_o - pi_o) with S = sum_o pi_o; on u: scale c 2 (v - vt) (1 - v^2);
    backward-data through fc4 over its 10 rows.  layers: [(W, b)] x 4 in fp64.  Returns (loss, [(dW, db)] x 4, z, v)."""
    a = [x]
    for l, (W, b) in enumerate(layers):
        y = a[-1] @ W.T + b
        if l < 3:
            a.append(np.maximum(y, 0.0))
    z, u = y[:, :9], y[:, 9]
    v = np.tanh(u)
    scale = w / w.sum()
    zm = z.max(1, keepdims=True)
    lse = zm[:, 0] + np.log(np.exp(z - zm).sum(1))
    p = np.exp(z - lse[:, None])
    S = pi.sum(1)
    loss = (scale * ((pi * (lse[:, None] - z)).sum(1) + c * (v - vt) ** 2)).sum()
    d = np.concatenate([scale[:, None] * (S[:, None] * p - pi), (scale * c * 2 * (v - vt) * (1 - v * v))[:, None]], 1)
    grads = [None] * 4
    for l in (3, 2, 1, 0):
        grads[l] = (d.T @ a[l], d.sum(0))
        if l:
            d = (d @ layers[l][0]) * (a[l] > 0)
    return loss, grads, z, v


@pytest.mark.parametrize("H,n,c", [(32, 1, 1.0), (64, 5, 0.25), (96, 40, 1.0)])
def test_fp64_restatement_of_the_step_is_autograd(H, n, c):
    rng = np.random.RandomState(H + n)
    torch.manual_seed(H + n)
    mod = TicTacToePVNet(H).double()
    layers = [(fc.weight.detach().numpy().copy(), fc.bias.detach().numpy().copy()) for fc in (mod.fc1, mod.fc2, mod.fc3, mod.fc4)]
    x = rng.randint(-1, 2, (n, 9)).astype(np.float64)
    cnt = rng.randint(0, 20, (n, 9)) * (rng.rand(n, 9) > 0.4)
    cnt[:, 0] += 1
    pi = cnt / cnt.sum(1, keepdims=True)
    if n > 1:
        pi[1] *= 0.5                                 # a row that does not sum to 1: S p - pi, not p - pi
    vt = rng.choice([-1.0, 0.0, 1.0, 0.37], n)
    w = rng.uniform(0.1, 2.0, n)
    if n > 2:
        w[2] = 0.0
    loss, grads, z, v = pv_step_fp64(layers, x, pi, vt, w, c)
    lg, vv = mod(torch.from_numpy(x))
    assert np.abs(lg.detach().numpy() - z).max() <= 1e-12 and np.abs(vv.detach().numpy() - v).max() <= 1e-12
    rows = -(torch.from_numpy(pi) * torch.log_softmax(lg, 1)).sum(1) + c * (vv - torch.from_numpy(vt)) ** 2
    wt = torch.from_numpy(w)
    # sum_o pi_o (lse - z_o) is -sum_o pi_o log_softmax(z)_o whatever pi sums to
    lt = (wt * rows).sum() / wt.sum()
    lt.backward()
    assert abs(lt.item() - loss) <= 1e-12 * abs(loss)
    for fc, (dW, db) in zip((mod.fc1, mod.fc2, mod.fc3, mod.fc4), grads):
        scale = max(fc.weight.grad.abs().max().item(), 1e-30)
        assert np.abs(fc.weight.grad.numpy() - dW).max() <= 1e-12 * scale
        assert np.abs(fc.bias.grad.numpy() - db).max() <= 1e-12 * max(scale, fc.bias.grad.abs().max().item())
    if n > 2:  # a row of weight 0 contributes exact zeros: without it, the same numbers
        keep = np.arange(n) != 2
        l2, g2, _, _ = pv_step_fp64(layers, x[keep], pi[keep], vt[keep], w[keep], c)
        assert l2 == pytest.approx(loss, rel=1e-14)
        assert np.abs(g2[0][0] - grads[0][0]).max() <= 1e-14 * np.abs(grads[0][0]).max()


_PV_SYMBOLS = {"bz_mlp_pv_param_count": 1, "bz_mlp_pv_workspace_bytes": 2, "bz_mlp_create_pv": 7, "bz_mlp_has_value": 1,
               "bz_mlp_forward_pv_f32": 7, "bz_mlp_forward_pv_bf16": 7, "bz_mlp_forward_pv_states_f32": 6,
               "bz_mlp_forward_pv_states_bf16": 6, "bz_mlp_train_pv_workspace_bytes": 2, "bz_mlp_train_step_pv": 19}


def test_pv_symbols_declared_exported_bound():
    hdr = open(os.path.join(ROOT, "include", "bz_abi.h")).read()
    L = _lib.lib()
    for name, nargs in _PV_SYMBOLS.items():
        assert f" {name}(" in hdr and name in _lib.ABI_SYMBOLS and len(getattr(L, name).argtypes) == nargs, name
    import betazero_amd as bz
    assert bz.TicTacToePVNet is TicTacToePVNet and bz.PVTrainer.__name__ == "PVTrainer"
    assert {"TicTacToePVNet", "PVTrainer"} <= set(bz.__all__)


def test_pv_entry_points_answer_without_a_gpu_and_refuse_bad_arguments():
    L = _lib.lib()
    for h in (0, 16, 33, 544, -32):
        assert L.bz_mlp_pv_param_count(h) == -1 and b"multiple of 32" in L.bz_last_error()
        assert L.bz_mlp_pv_workspace_bytes(h, 8) == -1 and L.bz_mlp_train_pv_workspace_bytes(h, 8) == -1
    assert L.bz_mlp_pv_param_count(256) == 136457 + 257 == 2 * 256 * 256 + 22 * 256 + 10
    assert L.bz_mlp_pv_workspace_bytes(256, 0) == -1 and L.bz_mlp_train_pv_workspace_bytes(256, 0) == -1
    assert L.bz_mlp_pv_workspace_bytes(256, 1) > L.bz_mlp_pv_param_count(256) * 4
    assert L.bz_mlp_pv_workspace_bytes(256, 1) >= L.bz_mlp_workspace_bytes(256, 1)
    # the step's workspace: six [B][H] arrays, g4 [B][10] and the rows' loss, each rounded up to 256 bytes
    r = lambda b: (b + 255) & ~255  # noqa: E731
    assert L.bz_mlp_train_pv_workspace_bytes(96, 5) == 6 * r(5 * 96 * 4) + r(5 * 10 * 4) + r(5 * 4)
    assert L.bz_mlp_train_workspace_bytes(96, 5) == 6 * r(5 * 96 * 4) + r(5 * 9 * 4) + r(5 * 4)
    assert L.bz_mlp_train_pv_workspace_bytes(96, 128) - L.bz_mlp_train_workspace_bytes(96, 128) == 128 * 4
    out = C.c_void_p()
    p = np.zeros(136457 + 257, np.float32)
    ws = C.c_void_p(256)
    assert L.bz_mlp_create_pv(48, 8, p.ctypes.data, ws, 1 << 30, None, C.byref(out)) == _lib.BZ_EINVAL
    assert L.bz_mlp_create_pv(256, 8, None, ws, 1 << 30, None, C.byref(out)) == _lib.BZ_EINVAL
    assert L.bz_mlp_create_pv(256, 8, p.ctypes.data, None, 1 << 30, None, C.byref(out)) == _lib.BZ_EINVAL
    assert L.bz_mlp_create_pv(256, 8, p.ctypes.data, ws, 16, None, C.byref(out)) == _lib.BZ_ENOMEM
    assert b"bz_mlp_create_pv" in L.bz_last_error()
    assert L.bz_mlp_has_value(None) == 0
    assert L.bz_mlp_forward_pv_f32(None, None, None, 1, None, None, None) == _lib.BZ_EINVAL
    assert L.bz_mlp_forward_pv_bf16(None, None, None, 1, None, None, None) == _lib.BZ_EINVAL
    assert L.bz_mlp_forward_pv_states_f32(None, None, 1, None, None, None) == _lib.BZ_EINVAL
    assert L.bz_mlp_forward_pv_states_bf16(None, None, 1, None, None, None) == _lib.BZ_EINVAL
    adam = _lib.MlpAdam(1e-3, 0.9, 0.999, 1e-8, 1)
    assert L.bz_mlp_train_step_pv(None, None, None, None, None, None, None, None, None, 1, 1.0, C.byref(adam), None, 0, None,
                                  None, None, None, None) == _lib.BZ_EINVAL


def test_value_of_a_policy_only_net_is_refused():
    net = DeviceMLP.__new__(DeviceMLP)       # (no GPU here: the refusal comes before anything touches the device)
    net.value_head, net.h = False, None
    with pytest.raises(ValueError, match="value head"):
        net.forward(np.zeros(1, np.uint64), np.zeros(1, np.uint64), value=True)
    with pytest.raises(ValueError, match="value head"):
        net.forward_states(np.zeros((1, 9), np.float32), bf16=True, value=True)


def test_yardstick_targets_are_minimax():
    """the loop's yard-stick (betazero_amd/ttt_yardstick.py) over the fixture's 4,520 positions: values and optimal moves from
    bz_ttt_minimax agree with a plain negamax written here"""
    from functools import lru_cache
    from betazero_amd.ttt_yardstick import minimax_targets
    lines = [sum(1 << c for c in ln) for ln in ((0, 1, 2), (3, 4, 5), (6, 7, 8), (0, 3, 6), (1, 4, 7), (2, 5, 8), (0, 4, 8), (2, 4, 6))]

    @lru_cache(maxsize=None)
    def negamax(own, opp):  # own to move
        if any(opp & m == m for m in lines):
            return -1
        if (own | opp) == 0x1FF:
            return 0
        return max(-negamax(opp, own | 1 << c) for c in range(9) if not (own | opp) >> c & 1)
    _, z = _fixture_module()
    own = np.where(z["to_move"] == 1, z["x_bits"], z["o_bits"]).astype(np.uint64)
    opp = np.where(z["to_move"] == 1, z["o_bits"], z["x_bits"]).astype(np.uint64)
    value, optimal = minimax_targets(own, opp)
    assert value.shape == (4520,) and optimal.shape == (4520, 9)
    for i in range(0, 4520, 7):
        a, b = int(own[i]), int(opp[i])
        assert value[i] == negamax(a, b), i
        want = [c for c in range(9) if not (a | b) >> c & 1 and -negamax(b, a | 1 << c) == value[i]]
        assert list(np.flatnonzero(optimal[i])) == want, i
    assert value[0] == 0 and optimal[0].all()      # the empty board: a draw, by any opening
