"""A board symmetry per row of a training batch, the parts that need no GPU: bz_train_sym_row -- the code
k_train_sym_batch runs per row -- against a numpy twin built from symmetry.sym_board / sym_action_map; the policy row as a
permutation of bit patterns; the group laws; the legal-move check on Reversi positions of the golden fixtures, which is what tells
tau from its inverse on the two 90-degree rotations; and every refusal, raised before a device is touched."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from betazero_amd import _lib
from betazero_amd.symmetry import SYM_INVERSE, sym_action_map, sym_board
from betazero_amd.train_symmetry import check_size, check_sym, sym_row, transform_rows

G = os.path.join(os.path.dirname(__file__), "golden")
SIZES = (4, 6, 8)
M64 = (1 << 64) - 1


def twin_row(own, opp, pi, size, s, fown=0, fopp=0):
    """the definition: boards through sym_board, pi'[tau_s(j)] = pi[j] (moved as bit patterns)"""
    tau = sym_action_map(size, s)
    out = np.empty(65, np.uint32)
    out[tau] = np.asarray(pi, np.float32).view(np.uint32)
    return sym_board(own, size, s), sym_board(opp, size, s), out.view(np.float32), sym_board(fown, size, s), sym_board(fopp, size, s)


def corner(size):
    return sum(1 << (8 * r + c) for r in range(size) for c in range(size))


def same(a, b):
    assert a[0] == b[0] and a[1] == b[1] and a[3] == b[3] and a[4] == b[4], (a, b)
    assert np.array_equal(a[2].view(np.int32), b[2].view(np.int32))


def random_row(rng, size, pass_mass=False):
    own = int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)) & corner(size)
    opp = int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)) & corner(size) & ~own
    fown = int(rng.integers(0, 1 << 63)) * 2 + 1 & corner(size)
    fopp = corner(size) & ~fown
    pi = rng.random(65).astype(np.float32)
    if not pass_mass:
        pi[64] = 0.0
    pi /= pi.sum()
    return own, opp, pi, fown, fopp


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("s", range(8))
def test_row_matches_the_twin(size, s):
    rng = np.random.default_rng(100 * size + s)
    for k in range(24):
        own, opp, pi, fown, fopp = random_row(rng, size, pass_mass=k % 2 == 0)
        same(sym_row(own, opp, pi, size, s, fown, fopp), twin_row(own, opp, pi, size, s, fown, fopp))
    own, opp, pi, fown, fopp = random_row(rng, size, pass_mass=True)
    same(sym_row(0, 0, pi, size, s, 0, 0), twin_row(0, 0, pi, size, s, 0, 0))                  # empty boards
    same(sym_row(own, opp, pi, size, s, fown, 0), twin_row(own, opp, pi, size, s, fown, 0))    # an all-zero fopp
    only_pass = np.zeros(65, np.float32)
    only_pass[64] = 1.0
    got = sym_row(own, opp, only_pass, size, s)
    assert got[2][64] == 1.0 and got[2][:64].sum() == 0.0
    # bits outside the size x size corner stay where they are
    junk = ~corner(size) & M64
    assert sym_row(own | junk, opp, pi, size, s)[0] == sym_board(own, size, s) | junk


@pytest.mark.parametrize("size", SIZES)
def test_policy_row_is_a_permutation_of_the_source_bits(size):
    rng = np.random.default_rng(size)
    bits = rng.integers(0, 1 << 32, 65, dtype=np.uint64).astype(np.uint32)
    bits[3], bits[17], bits[64] = 0x7FC01234, 0xFFA00001, 0x80000000   # two NaN payloads, -0 on pass
    bits[5] = 0x80000000
    pi = bits.view(np.float32)
    for s in range(8):
        out = sym_row(1, 2, pi, size, s)[2].view(np.uint32)
        assert np.array_equal(np.sort(out), np.sort(bits)) and out[64] == bits[64]
        assert int(out.view(np.int32).sum(dtype=np.int64)) == int(bits.view(np.int32).sum(dtype=np.int64))
        assert np.array_equal(out[sym_action_map(size, s)].view(np.int32), bits.view(np.int32))


@pytest.mark.parametrize("size", SIZES)
def test_group_laws(size):
    rng = np.random.default_rng(7 + size)
    own, opp, pi, fown, fopp = random_row(rng, size, pass_mass=True)
    for s in range(8):
        a = sym_row(own, opp, pi, size, s, fown, fopp)
        back = sym_row(a[0], a[1], a[2], size, SYM_INVERSE[s], a[3], a[4])
        same(back, (own, opp, pi, fown, fopp))
    asym = 0b1 | 0b11 << 8 | 0b1 << 17   # no symmetry of the square maps it to itself (size >= 4)
    images = {sym_row(asym, 0, pi, size, s)[0] for s in range(8)}
    assert len(images) == 8
    assert len({sym_row(0, 0, np.arange(65, dtype=np.float32), size, s)[2].tobytes() for s in range(8)}) == 8


def legal(own, opp, size):
    out = C.c_uint64()
    assert _lib.lib().bz_reversi_legal(own, opp, size, C.byref(out)) == _lib.BZ_OK
    return int(out.value)


def golden_positions():
    pos = np.load(os.path.join(G, "reversi_positions.npz"))["pos"].tolist()[::40]
    pos += np.load(os.path.join(G, "reversi_other_sizes.npz"))["pos"].tolist()[::24]
    return [(int(p[0]), int(p[1]), int(p[2])) for p in pos]


def test_legal_moves_move_with_the_board():
    rows = golden_positions()
    assert {r[0] for r in rows} >= {4, 6, 8}
    seen = 0
    for size, x, o in rows:
        for own, opp in ((x, o), (o, x)):
            lg = legal(own, opp, size)
            cells = [j for j in range(64) if lg >> j & 1]
            if not cells:
                continue
            seen += 1
            pi = np.zeros(65, np.float32)
            pi[cells] = np.arange(1, len(cells) + 1, dtype=np.float32)
            pi /= pi.sum()
            for s in range(8):
                own2, opp2, pi2, _, _ = sym_row(own, opp, pi, size, s)
                lg2 = legal(own2, opp2, size)
                tau = sym_action_map(size, s)
                assert lg2 == sum(1 << int(tau[j]) for j in cells), (size, s)          # legal(board') is the tau-image of legal(board)
                support = [a for a in range(65) if pi2[a] != 0.0]
                assert all(lg2 >> a & 1 for a in support) and len(support) == len(cells), (size, s)
    assert seen >= 60


def test_row_entry_point_refuses_bad_arguments():
    L = _lib.lib()
    pi, out = np.zeros(65, np.float32), np.zeros(65, np.float32)
    a, b = C.c_uint64(), C.c_uint64()
    ok = lambda size, s, src=pi, dst=out: L.bz_train_sym_row(1, 2, src.ctypes.data, 0, 0, size, s, C.byref(a), C.byref(b), dst.ctypes.data, None, None)  # noqa: E731
    assert ok(8, 7) == _lib.BZ_OK and ok(1, 0) == _lib.BZ_OK
    for size, s in ((0, 0), (9, 0), (8, 8), (8, -1)):
        assert ok(size, s) == _lib.BZ_EINVAL
    assert ok(8, 0, dst=pi) == _lib.BZ_EINVAL                # not in place
    assert L.bz_train_sym_row(1, 2, None, 0, 0, 8, 0, C.byref(a), C.byref(b), out.ctypes.data, None, None) == _lib.BZ_EINVAL
    assert L.bz_train_sym_batch(None, None, 4, 8, None, None, None) == _lib.BZ_EINVAL
    assert L.bz_train_sym_rows_per_workgroup() == 64
    hdr = open(os.path.join(os.path.dirname(G), "..", "include", "bz_abi.h")).read()
    for name in ("bz_train_sym_batch", "bz_train_sym_row", "bz_train_sym_rows_per_workgroup"):
        assert f" {name}(" in hdr and name in _lib.ABI_SYMBOLS
    assert C.sizeof(_lib.TrainSymCols) == 32 and C.sizeof(_lib.TrainSymStage) == 56 and C.sizeof(_lib.TrainBatch) == 48


def host_examples(n=6, size=8):
    from betazero_amd.examples import DeviceExamples
    z64 = torch.zeros(n, dtype=torch.int64)
    return DeviceExamples(own=z64, opp=z64.clone(), pi=torch.full((n, 65), 1 / 65), z=torch.zeros(n, dtype=torch.int8),
                          mover=torch.ones(n, dtype=torch.int8), act=torch.zeros(n, dtype=torch.uint8), game=z64.clone(),
                          ply=torch.zeros(n, dtype=torch.int32), size=size)


def test_refusals_without_a_device():
    from betazero_amd.net import PolicyValueNet
    from betazero_amd.train import GraphedTrainStep, train_step
    from betazero_amd.train_kernels import StepPlan
    for bad in (0, 9, -1, 8.0, True, None, "8"):
        with pytest.raises(ValueError, match="size"):
            check_size(bad)
    assert [check_size(k) for k in range(1, 9)] == list(range(1, 9))
    ok = torch.zeros(8, dtype=torch.uint8)
    assert check_sym(ok, 8, "cpu") is ok
    for bad in (None, [0] * 8, torch.zeros(8, dtype=torch.int64), torch.zeros(8, dtype=torch.int8), torch.zeros(7, dtype=torch.uint8),
                torch.zeros((8, 1), dtype=torch.uint8), torch.zeros(16, dtype=torch.uint8)[::2]):
        with pytest.raises(ValueError, match="sym"):
            check_sym(bad, 8, "cpu")
    fused = PolicyValueNet(64, 1, 24, fused_tower=True)
    # the plan: like ownership=, the all-kernel step only; a size outside 1..8
    with pytest.raises(ValueError, match="fused_tower"):
        StepPlan(PolicyValueNet(64, 1, 24), 8, symmetry=True)
    for size in (0, 9, 8.5):
        with pytest.raises(ValueError, match="size"):
            StepPlan(fused, 8, symmetry=True, size=size)
    # the graphed step: every form that is not the all-kernel step
    for kw in (dict(step_kernels=False), dict(autocast=False), dict(na=9)):
        with pytest.raises(ValueError, match="symmetry=True needs the all-kernel step"):
            GraphedTrainStep(fused, batch=8, device="cpu", symmetry=True, **kw)
    with pytest.raises(ValueError, match="symmetry=True needs the all-kernel step"):
        GraphedTrainStep(PolicyValueNet(64, 1, 24), batch=8, device="cpu", symmetry=True)
    with pytest.raises(ValueError, match="symmetry=True needs the all-kernel step"):
        GraphedTrainStep(PolicyValueNet(64, 1, 65, fused_tower=True), batch=8, device="cpu", symmetry=True)
    # the kernel on its own
    ex, idx = host_examples(), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="needs sym"):
        transform_rows(ex, idx, None)
    with pytest.raises(ValueError, match="sym must be"):
        transform_rows(ex, idx, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="sym must be"):
        transform_rows(ex, idx, torch.zeros(5, dtype=torch.uint8))
    with pytest.raises(ValueError, match="idx"):
        transform_rows(ex, idx.to(torch.int32), torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="size"):
        transform_rows(host_examples(size=9), idx, torch.zeros(4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="DeviceExamples"):
        transform_rows(None, idx, torch.zeros(4, dtype=torch.uint8))
    # the torch path
    with pytest.raises(ValueError, match="size"):
        train_step(fused, None, host_examples(size=0), sym=torch.zeros(6, dtype=torch.uint8))
    import betazero_amd
    assert betazero_amd.transform_rows is transform_rows and "transform_rows" in betazero_amd.__all__
