"""The reference's tic-tac-toe MLP without a GPU: the torch module against the reference's own logits (fixture
ttt_mlp.npz, tools/gen_mlp_golden.py), checkpoint loading with weights_only=True, state_dict interchange, and the
bz_mlp C ABI refusing bad arguments before anything launches."""
import ctypes as C
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from betazero_amd import _lib
from betazero_amd.mlp import TicTacToeNet, load_reference_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "ttt_mlp.npz")


def _fixture_module():
    z = np.load(FIX)
    m = TicTacToeNet(9, z["fc1_w"].shape[0], 9)
    m.load_state_dict({f"fc{l}.{k}": torch.from_numpy(z[f"fc{l}_{k[0]}"]) for l in (1, 2, 3, 4) for k in ("weight", "bias")})
    return m.eval(), z


def test_module_reproduces_reference_logits_bit_for_bit():
    m, z = _fixture_module()
    with torch.no_grad():
        lg = m(torch.from_numpy(z["states"])).numpy()
    assert lg.shape == (4520, 9) and lg.dtype == np.float32
    assert np.array_equal(lg.view(np.uint32), z["logits"].view(np.uint32))


def test_fixture_is_consistent():
    _, z = _fixture_module()
    cells = np.arange(9)
    board = ((z["x_bits"][:, None] >> cells) & 1) - ((z["o_bits"][:, None] >> cells) & 1)
    assert np.array_equal(z["states"], (z["to_move"][:, None] * board).astype(np.float32))
    # the reference AIPlayer's move is legal and is the best legal logit wherever that is unambiguous
    legal = board == 0
    assert legal[np.arange(len(board)), z["move"]].all()
    masked = np.where(legal, z["logits"], -np.inf)
    srt = np.sort(masked, 1)
    clear = srt[:, -1] - srt[:, -2] > 1e-4
    assert clear.mean() > 0.99
    assert np.array_equal(masked.argmax(1)[clear], z["move"][clear])


# the reference's train.py saves torch.save(model, path) from a script whose class lives in __main__; this writes such a
# file with a class of the same shape (attribute names fc1..fc4, relu1..3), defined here from scratch
_SAVE_SCRIPT = r'''
import sys, torch, torch.nn as nn
class TicTacToeNet(nn.Module):
    def __init__(self, input_size, hidden_size, output_size):
        super().__init__()
        self.fc1 = nn.Linear(input_size, hidden_size); self.relu1 = nn.ReLU()
        self.fc2 = nn.Linear(hidden_size, hidden_size); self.relu2 = nn.ReLU()
        self.fc3 = nn.Linear(hidden_size, hidden_size); self.relu3 = nn.ReLU()
        self.fc4 = nn.Linear(hidden_size, output_size)
    def forward(self, x):
        return self.fc4(self.relu3(self.fc3(self.relu2(self.fc2(self.relu1(self.fc1(x)))))))
torch.manual_seed(3)
m = TicTacToeNet(9, 64, 9)
torch.save(m, sys.argv[1])
torch.save(m.state_dict(), sys.argv[2])
'''


def test_whole_module_pickle_loads_with_weights_only(tmp_path):
    whole, sd = str(tmp_path / "model.pth"), str(tmp_path / "sd.pth")
    script = tmp_path / "save.py"
    script.write_text(_SAVE_SCRIPT)
    subprocess.check_call([sys.executable, str(script), whole, sd])
    ref_sd = torch.load(sd, weights_only=True)
    for path in (whole, sd):
        m = load_reference_model(path)
        assert isinstance(m, TicTacToeNet) and m.hidden_size == 64
        for k, v in m.state_dict().items():
            assert torch.equal(v, ref_sd[k]), k


def test_pickle_with_foreign_code_is_refused(tmp_path):
    class Evil:
        def __reduce__(self):
            return (os.system, ("true",))
    p = tmp_path / "evil.pth"
    with open(p, "wb") as f:
        pickle.dump(Evil(), f)
    with pytest.raises(pickle.UnpicklingError):
        load_reference_model(str(p))


class _RefShaped(nn.Module):  # the reference's attribute layout, independent of betazero_amd.mlp
    def __init__(self, h):
        super().__init__()
        self.fc1, self.relu1 = nn.Linear(9, h), nn.ReLU()
        self.fc2, self.relu2 = nn.Linear(h, h), nn.ReLU()
        self.fc3, self.relu3 = nn.Linear(h, h), nn.ReLU()
        self.fc4 = nn.Linear(h, 9)


def test_state_dict_round_trip():
    torch.manual_seed(1)
    ref = _RefShaped(32)
    m = TicTacToeNet(9, 32, 9)
    m.load_state_dict(ref.state_dict())
    back = _RefShaped(32)
    back.load_state_dict(m.state_dict())
    for k, v in ref.state_dict().items():
        assert torch.equal(back.state_dict()[k], v)
    assert list(m.state_dict()) == list(ref.state_dict())
    flat = m.flat_params()
    assert flat.size == _lib.lib().bz_mlp_param_count(32) == 2 * 32 * 32 + 21 * 32 + 9
    m2 = TicTacToeNet(9, 32, 9).load_flat_params_(flat)
    assert np.array_equal(m2.flat_params(), flat)


_MLP_SYMBOLS = ("bz_mlp_param_count", "bz_mlp_workspace_bytes", "bz_mlp_create", "bz_mlp_update", "bz_mlp_destroy",
                "bz_mlp_forward_f32", "bz_mlp_forward_bf16", "bz_mlp_forward_states_f32", "bz_mlp_forward_states_bf16",
                "bz_mlp_train_workspace_bytes", "bz_mlp_train_step", "bz_engine_set_mlp")


def test_mlp_symbols_declared_exported_bound():
    hdr = open(os.path.join(ROOT, "include", "bz_abi.h")).read()
    L = _lib.lib()
    assert _lib.ABI_VERSION == 7 and L.bz_abi_version() == 7
    for n in _MLP_SYMBOLS:
        assert f"{n}(" in hdr and hasattr(L, n) and n in _lib.ABI_SYMBOLS, n
    assert (_lib.EVAL_MLP_F32, _lib.EVAL_MLP_BF16) == (6, 7)
    assert "BZ_EVAL_MLP_F32 = 6, BZ_EVAL_MLP_BF16 = 7" in hdr
    assert C.sizeof(_lib.EngineCfg) == 80


def test_mlp_entry_points_refuse_bad_arguments():
    L = _lib.lib()
    for h in (0, 16, 33, 544, -32):
        assert L.bz_mlp_param_count(h) == -1 and L.bz_mlp_workspace_bytes(h, 8) == -1
        assert L.bz_mlp_train_workspace_bytes(h, 8) == -1
    assert L.bz_mlp_param_count(256) == 136457
    assert L.bz_mlp_workspace_bytes(256, 0) == -1 and L.bz_mlp_workspace_bytes(256, 1) > 136457 * 4
    assert L.bz_mlp_train_workspace_bytes(256, 128) >= 6 * 128 * 256 * 4
    out = C.c_void_p()
    p = np.zeros(136457, np.float32)
    ws = C.c_void_p(256)
    assert L.bz_mlp_create(48, 8, p.ctypes.data, ws, 1 << 30, None, C.byref(out)) == _lib.BZ_EINVAL
    assert L.bz_mlp_create(256, 8, None, ws, 1 << 30, None, C.byref(out)) == _lib.BZ_EINVAL
    assert L.bz_mlp_create(256, 8, p.ctypes.data, None, 1 << 30, None, C.byref(out)) == _lib.BZ_EINVAL
    assert L.bz_mlp_create(256, 8, p.ctypes.data, ws, 16, None, C.byref(out)) == _lib.BZ_ENOMEM
    assert L.bz_mlp_forward_f32(None, None, None, 1, None, None) == _lib.BZ_EINVAL
    assert L.bz_mlp_forward_bf16(None, None, None, 1, None, None) == _lib.BZ_EINVAL
    assert L.bz_mlp_forward_states_f32(None, None, 1, None, None) == _lib.BZ_EINVAL
    assert L.bz_mlp_forward_states_bf16(None, None, 1, None, None) == _lib.BZ_EINVAL
    assert L.bz_mlp_update(None, None, None) == _lib.BZ_EINVAL
    adam = _lib.MlpAdam(1e-4, 0.9, 0.999, 1e-8, 1)
    assert L.bz_mlp_train_step(None, None, None, None, None, None, None, None, 1, C.byref(adam), None, 0, None, None,
                               None, None) == _lib.BZ_EINVAL
    assert L.bz_engine_set_mlp(None, None) == _lib.BZ_EINVAL


@pytest.mark.parametrize("game,kind,ok", [(0, 6, True), (0, 7, True), (1, 6, False), (1, 7, False), (2, 6, False),
                                          (3, 7, False), (0, 8, False)])
def test_engine_mlp_evaluators_need_tic_tac_toe(game, kind, ok):
    L = _lib.lib()
    cfg = _lib.EngineCfg(game, 4, 8, kind, 1.5, 0, 0, 1, 9 if game == 0 else 64, 0, 0, 0, 4, 0, 0.0, 0.0, 0)
    assert (L.bz_engine_workspace_bytes(C.byref(cfg)) > 0) == ok
    out = C.c_void_p()
    if not ok:
        assert L.bz_engine_create(C.byref(cfg), C.c_void_p(256), 1 << 30, C.byref(out)) == _lib.BZ_EINVAL


def test_python_refuses_mlp_evaluator_on_reversi():
    from betazero_amd.engine import SelfPlayEngine
    with pytest.raises(ValueError, match="tic-tac-toe"):
        SelfPlayEngine("reversi", 4, 8, "mlp_f32")


# ---------------------------------------------------------------- the C oracle's MLP (tests/test_gpu_mlp_numerics.py's yardstick)
def test_oracle_mlp_forward_matches_reference_logits():
    from oracle import oracle as orc
    m, z = _fixture_module()
    lg = orc.mlp_forward_f32(256, m.flat_params(), z["states"])
    assert lg.shape == (4520, 9) and lg.dtype == np.float32
    assert np.abs(lg - z["logits"]).max() <= 1e-5
    # the bitboard helper gives the same inputs as the reference's symbol * board
    tm = z["to_move"]
    own = np.where(tm == 1, z["x_bits"], z["o_bits"]).astype(np.uint64)
    opp = np.where(tm == 1, z["o_bits"], z["x_bits"]).astype(np.uint64)
    assert np.array_equal(orc.ttt_states(own, opp), z["states"])


@pytest.mark.parametrize("H", [32, 96, 512])
def test_oracle_mlp_forward_matches_fp64_torch(H):
    from oracle import oracle as orc
    torch.manual_seed(100 + H)
    m = TicTacToeNet(9, H, 9).eval()
    g = torch.Generator().manual_seed(H)
    x = torch.cat([torch.randint(-1, 2, (150, 9), generator=g).float(), torch.randn(50, 9, generator=g)])
    with torch.no_grad():
        ref = m.double()(x.double()).numpy()
    lg = orc.mlp_forward_f32(H, m.float().flat_params(), x.numpy())
    assert np.abs(lg - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())
