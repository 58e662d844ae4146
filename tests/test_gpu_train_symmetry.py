"""A board symmetry per row inside the fused training step on the GPU.  Every comparison but the torch path's is
bit for bit: the staging kernel alone (transform_rows) against a numpy twin built from symmetry.sym_board / sym_action_map and
against the augmentation kernel; StepPlan(symmetry=True) against the plain plan run on the twin's pre-transformed rows; the
graphed step against eager steps across new symmetries and a new data set; bad input; and the loop tool.

k_train_sym_batch stages 64 rows per workgroup (16 per wave): n = 60 / 64 / 68 sit below, on and past a workgroup's edge, 4 fills a
quarter of one wave, 260 and 1028 end four rows into a workgroup (and into a wave's 16) after 4 and 16 full ones."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from betazero_amd.examples import DeviceExamples, Examples, columns
from betazero_amd.symmetry import sym_action_map, sym_board

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _corner(size):
    return np.uint64(sum(1 << (8 * r + c) for r in range(size) for c in range(size)))


def _examples(rows, size, seed, vt=False, own=False, payloads=True):
    """host Examples: random boards on the size x size corner (an empty and a full one among them), pi with and without mass on
    pass, every column the rows can carry besides count; payloads: a NaN payload and a -0 in row 0's pi (for the kernel alone: a
    step's loss would be NaN)"""
    rng = np.random.default_rng(seed)
    u64 = lambda: rng.integers(0, 2**63, rows, dtype=np.int64).astype(np.uint64) | (rng.integers(0, 2, rows).astype(np.uint64) << np.uint64(63))  # noqa: E731
    m = _corner(size)
    a = u64() & m
    b = u64() & m & ~a
    a[0], b[0] = 0, 0
    a[1], b[1] = m, 0
    pi = rng.random((rows, 65)).astype(np.float32) ** 3
    pi[::2, 64] = 0.0
    pi /= pi.sum(1, keepdims=True)
    pi[2] = 0.0
    pi[2, 64] = 1.0
    if payloads:
        pi.view(np.uint32)[0, 5], pi.view(np.uint32)[0, 9] = 0x7FC01234, 0x80000000
    fa = u64() & m
    return Examples(own=a, opp=b, pi=pi, z=rng.integers(-1, 2, rows).astype(np.int8), mover=(rng.integers(0, 2, rows) * 2 - 1).astype(np.int8),
                    act=rng.integers(0, 65, rows).astype(np.uint8), game=np.arange(rows, dtype=np.int64) // 7, ply=(np.arange(rows) % 7).astype(np.int32),
                    size=size, kl=rng.random(rows).astype(np.float32), q=(rng.random(rows) * 2 - 1).astype(np.float32),
                    vt=(rng.random(rows) * 2 - 1).astype(np.float32) if vt else None, fown=fa if own else None,
                    fopp=(m & ~fa) if own else None)


def _draw(rows, n, seed, shift=0):
    """row numbers with repeats and the batch's symmetries, all eight present: in the first eight positions, or for n < 8 over
    the calls with shift = 0, 1, .."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, rows, n).astype(np.int64)
    sym = rng.integers(0, 8, n).astype(np.uint8)
    sym[:min(n, 8)] = (np.arange(min(n, 8)) + shift * n) % 8
    return idx, sym


def _twin(ex, idx, sym):
    """host Examples of the transformed rows, from the definition"""
    maps = [sym_action_map(ex.size, s) for s in range(8)]
    n = len(idx)
    board = lambda col: np.array([sym_board(int(col[idx[p]]), ex.size, int(sym[p])) for p in range(n)], dtype=np.uint64)  # noqa: E731
    pi = np.empty((n, 65), np.uint32)
    for p in range(n):
        pi[p, maps[sym[p]]] = ex.pi[idx[p]].view(np.uint32)
    moved = dict(own=board(ex.own), opp=board(ex.opp), pi=pi.view(np.float32), act=np.array([maps[sym[p]][ex.act[idx[p]]] for p in range(n)], np.uint8))
    if ex.fown is not None:
        moved.update(fown=board(ex.fown), fopp=board(ex.fopp))
    return Examples(size=ex.size, **{k: moved[k] if k in moved else a[idx] for k, a in columns(ex).items()})


def _same_rows(got, want):
    """DeviceExamples against host Examples, every column, as bytes"""
    g, w = columns(got), columns(DeviceExamples.from_host(want, "cpu"))
    assert set(g) == set(w) and got.size == want.size
    for k in w:
        assert g[k].dtype == w[k].dtype and g[k].cpu().numpy().tobytes() == w[k].numpy().tobytes(), k


def _dev(a):
    return torch.as_tensor(a).to(DEV)


# ---------------------------------------------------------------- the kernel alone
@pytest.mark.parametrize("size", [4, 6, 8])
@pytest.mark.parametrize("n", [4, 60, 64, 68, 260, 1028])
def test_transform_rows_equals_the_twin_in_every_column(n, size):
    from betazero_amd import transform_rows
    for k, (vt, own) in enumerate(((False, False), (True, True), (True, False), (False, True))):
        ex = _examples(97, size, 1000 * n + size, vt=vt, own=own)
        idx, sym = _draw(97, n, n + size, shift=k)
        got = transform_rows(DeviceExamples.from_host(ex, DEV), _dev(idx), _dev(sym))
        assert len(got) == n and (got.vt is not None) == vt and (got.fown is not None) == own
        _same_rows(got, _twin(ex, idx, sym))


def test_transform_rows_of_a_three_row_data_set_with_repeats():
    from betazero_amd import transform_rows
    ex = _examples(3, 8, 5, vt=True, own=True)
    idx = np.array([2, 2, 0, 1, 1, 2, 0, 0, 1, 2, 2, 2], np.int64)
    sym = np.array([0, 1, 2, 3, 4, 5, 6, 7, 3, 5, 7, 7], np.uint8)
    _same_rows(transform_rows(DeviceExamples.from_host(ex, DEV), _dev(idx), _dev(sym)), _twin(ex, idx, sym))


def test_staged_rows_equal_the_augmentation_kernels(size=8):
    """for s <= 6 the staged own / opp / pi / fown / fopp are rows 8 i + s of augment_examples(dedupe=False), which is pinned to
    the reference (the augmentation kernel serves the 8 x 8 board, and tic-tac-toe's 3 x 3 in another bit layout)"""
    from betazero_amd import transform_rows
    from betazero_amd.augment import augment_examples
    n = 68
    ex = _examples(n, size, 40 + size, own=True)
    ex.pi.view(np.uint32)[0, 5] = 0   # (the eightfold copy is compared as bits as well; the NaN stays out of augment's key)
    dex = DeviceExamples.from_host(ex, DEV)
    aug = augment_examples(dex, dedupe=False)
    assert len(aug) == 8 * n
    rows = torch.arange(n, device=DEV)
    for s in range(7):
        got = transform_rows(dex, rows, torch.full((n,), s, dtype=torch.uint8, device=DEV))
        for k in ("own", "opp", "fown", "fopp", "act"):
            assert torch.equal(getattr(got, k), getattr(aug, k)[s::8]), (k, s)
        assert torch.equal(got.pi.view(torch.int32), aug.pi[s::8].contiguous().view(torch.int32)), s


# ---------------------------------------------------------------- the step
def _net(C, NB, VH, seed):
    from betazero_amd.net import PolicyValueNet
    torch.manual_seed(seed)
    m = PolicyValueNet(C, NB, VH, fused_tower=True).cuda()
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.normal_(0.0, 0.2)
        m.pol.weight.mul_(3.0); m.val.weight.mul_(3.0); m.polfc.weight.mul_(2.0)
    return m


OPTIONS = {"plain": {}, "value_targets": dict(value_targets=True), "ownership": dict(ownership=True), "fp8_qat": dict(fp8_qat=True),
           "extended": {}}
# (C, conv layers, n, VH).  The smallest batch a plan takes at 64 channels is 8 (a workgroup of the tower kernels holds 8 positions
# there, 4 at 128 channels), so the first shape runs at n = 8: below one wave's 16 staged rows, like 4
SHAPES = [(64, 2, 8, 24), (64, 2, 72, 64), (128, 2, 8, 64)]
CASES = [(*shape, o) for shape in SHAPES for o in OPTIONS if o != "fp8_qat" or shape[0] == 128]


def _plans(C, layers, n, VH, option, seed):
    """(symmetric plan, plain plan) on two copies of one net (and of one ownership head)"""
    from betazero_amd.net import OwnershipHead
    from betazero_amd.train_kernels import StepPlan
    kw = dict(OPTIONS[option])
    m1 = _net(C, layers // 2, VH, seed)
    m2 = copy.deepcopy(m1)
    kw1, kw2 = dict(kw), dict(kw)
    if kw.get("ownership"):
        h1 = OwnershipHead(C).cuda()
        with torch.no_grad():
            h1.conv.weight.mul_(3.0)
        kw1["ownership"], kw2["ownership"] = h1, copy.deepcopy(h1)
    return StepPlan(m1, n, symmetry=True, size=8, **kw1), StepPlan(m2, n, **kw2)


def _batch_kw(ex, option):
    kw = {}
    if option == "value_targets":
        kw["vt"] = ex.vt
    if option == "ownership":
        kw.update(fown=ex.fown, fopp=ex.fopp)
    return kw


def _equal_plans(a, b, what):
    for k in a.NAMES:
        assert torch.equal(a.params[k].grad, b.params[k].grad), (what, "grad", k)
        assert torch.equal(a.params[k].detach(), b.params[k].detach()), (what, "param", k)
        if a.adam_m is not None:
            assert torch.equal(a.adam_m[k], b.adam_m[k]) and torch.equal(a.adam_v[k], b.adam_v[k]), (what, "moments", k)
    if a.ownership is not None:
        for k in ("w", "b"):
            assert torch.equal(a.own_params[k].grad, b.own_params[k].grad) and torch.equal(a.own_params[k].detach(), b.own_params[k].detach()), (what, k)
        assert torch.equal(a.own_loss, b.own_loss)
    if a.ema is not None:
        assert all(torch.equal(a.ema[k], b.ema[k]) for k in a.NAMES), what


@pytest.mark.parametrize("C,layers,n,VH,option", CASES)
def test_step_under_symmetries_is_the_plain_step_on_the_twins_rows(C, layers, n, VH, option):
    """grads and step with (idx, sym) against the same plan type without symmetry=, run with idx=None on the rows the twin
    transformed on the host: four losses, fourteen gradients, parameters and moments after Adam -- the same bits"""
    rows = 3 * n + 5
    ex = _examples(rows, 8, 7 * n + C, vt=option == "value_targets", own=option == "ownership", payloads=False)
    idx, sym = _draw(rows, n, n + C)
    dex, tw = DeviceExamples.from_host(ex, DEV), DeviceExamples.from_host(_twin(ex, idx, sym), DEV)
    a, b = _plans(C, layers, n, VH, option, 11)
    la = a.grads(dex.own, dex.opp, dex.pi, dex.z, _dev(idx), sym=_dev(sym), **_batch_kw(dex, option)).clone()
    lb = b.grads(tw.own, tw.opp, tw.pi, tw.z, None, **_batch_kw(tw, option)).clone()
    assert torch.equal(la, lb) and float(la[3]) == 0.0 and bool(torch.isfinite(la).all()) and float(la[1]) > 0, (la, lb)
    _equal_plans(a, b, "grads")
    ext = dict(weight_decay=1e-2, clip_norm=0.5, ema_decay=0.9) if option == "extended" else {}
    for p in (a, b):
        p.enable_adam(1e-3, warmup_steps=2, **ext)
    for t in range(2):
        la, lb = a.step().clone(), b.step().clone()
        assert torch.equal(la, lb), (t, la, lb)
        _equal_plans(a, b, f"step {t}")
    assert a.bad_rows() == 0 and b.bad_rows() == 0
    if option == "extended":
        assert a.optim_stats() == b.optim_stats()


@pytest.mark.parametrize("C,layers,n,VH", SHAPES)
def test_identity_symmetry_and_arange_equal_the_plain_plan(C, layers, n, VH):
    """sym all zero and idx = arange: every bit of the plain plan on the same data"""
    ex = DeviceExamples.from_host(_examples(n, 8, 3 * n, payloads=False), DEV)
    a, b = _plans(C, layers, n, VH, "plain", 12)
    la = a.grads(ex.own, ex.opp, ex.pi, ex.z, torch.arange(n, device=DEV), sym=torch.zeros(n, dtype=torch.uint8, device=DEV)).clone()
    lb = b.grads(ex.own, ex.opp, ex.pi, ex.z, torch.arange(n, device=DEV)).clone()
    assert torch.equal(la, lb) and float(la[1]) > 0
    _equal_plans(a, b, "identity")
    g = a.sym_stage
    assert torch.equal(g.own, ex.own) and torch.equal(g.opp, ex.opp) and torch.equal(g.z, ex.z)
    assert torch.equal(g.pi.view(torch.int32), ex.pi.view(torch.int32))


def test_state_moves_between_steps_with_and_without_symmetry():
    a, b = _plans(64, 2, 8, 24, "plain", 13)
    for p in (a, b):
        p.enable_adam(1e-3)
    ex = DeviceExamples.from_host(_examples(8, 8, 1, payloads=False), DEV)
    a.set_batch(ex.own, ex.opp, ex.pi, ex.z, sym=torch.full((8,), 3, dtype=torch.uint8, device=DEV))
    a.step()
    same_state = lambda: all(torch.equal(t, b._state_tensors()[k]) for k, t in a._state_tensors().items())  # noqa: E731
    assert not same_state()
    b.load_state_dict(a.state_dict())
    assert same_state() and set(a.state_dict()) == set(b.state_dict())
    b.set_batch(ex.own, ex.opp, ex.pi, ex.z)
    b.step()
    assert not same_state()
    a.load_state_dict(b.state_dict())
    assert same_state()
    with pytest.raises(ValueError, match="needs sym"):
        a.set_batch(ex.own, ex.opp, ex.pi, ex.z)
    with pytest.raises(ValueError, match="without symmetry"):
        b.set_batch(ex.own, ex.opp, ex.pi, ex.z, sym=torch.zeros(8, dtype=torch.uint8, device=DEV))


def test_graphed_step_replays_new_symmetries_and_a_new_data_set():
    """batch 64 on a 64 x 2 net: five replays of ONE graph against eager StepPlan steps on a deep copy, a new sym every replay and
    a new data set at the fourth: losses and every parameter, the same bits"""
    from betazero_amd.train import GraphedTrainStep
    from betazero_amd.train_kernels import StepPlan
    m1 = _net(64, 2, 64, 14)
    m2 = copy.deepcopy(m1)
    g = GraphedTrainStep(m1, lr=1e-3, batch=64, lr_warmup_steps=3, symmetry=True)
    eager = StepPlan(m2, 64, symmetry=True, size=8)
    eager.enable_adam(1e-3, warmup_steps=3)
    sets = [DeviceExamples.from_host(_examples(300, 8, 20, payloads=False), DEV), DeviceExamples.from_host(_examples(150, 8, 21, payloads=False), DEV)]
    graph = None
    for t in range(5):
        ex = sets[t >= 3]
        idx, sym = _draw(len(ex), 64, 100 + t)
        idx, sym = _dev(idx), _dev(sym)
        got = g.step(ex, idx, sym)
        eager.set_batch(ex.own, ex.opp, ex.pi, ex.z, idx, sym=sym)
        want = eager.step()
        assert torch.equal(got, want[:3]) and float(got[1]) > 0, (t, got, want)
        for (k, p), q in zip(m1.named_parameters(), m2.parameters()):
            assert torch.equal(p.detach(), q.detach()), (t, k)
        graph = graph or g.graph
        assert g.graph is graph and graph is not None
    g.check()
    with pytest.raises(ValueError, match="needs sym"):
        g.step(sets[0], idx)
    ex6 = copy.copy(sets[0])
    ex6.size = 6
    with pytest.raises(ValueError, match="captured for 8 x 8"):
        g.step(ex6, idx, sym)


def test_graphed_step_tracks_the_torch_path():
    """GraphedTrainStep(symmetry=True) against train_step(sym=) through stock autograd from the same weights on the same batches
    and symmetries, at the tolerances tests/test_gpu_train_kernels.py holds the plain graphed step to against the plain torch
    path (test_graphed_train_step_on_the_tower_kernels_tracks_the_autograd_step): the losses within 3e-2 step by step, the
    cosine of the tower's weight updates after 8 steps > 0.9, of the ends' weights > 0.999"""
    from betazero_amd.train import GraphedTrainStep, make_optimizer, train_step
    ex = DeviceExamples.from_host(_examples(1024, 8, 30, payloads=False), DEV)
    torch.manual_seed(5)
    from betazero_amd.net import PolicyValueNet
    m1 = PolicyValueNet(64, 2, 64, fused_tower=True).cuda()
    m2 = copy.deepcopy(m1)
    w0 = m1.tower_w.detach().clone()
    g = GraphedTrainStep(m1, lr=1e-3, batch=128, symmetry=True)
    opt = make_optimizer(m2, lr=1e-3)
    for step in range(8):
        idx, sym = _draw(1024, 128, 200 + step)
        idx, sym = _dev(idx), _dev(sym)
        l1 = g(ex, idx, sym).cpu().numpy()
        l2 = torch.stack(train_step(m2, opt, ex, idx, sym=sym)).cpu().numpy()
        print("losses kernel / torch:", l1, l2)
        assert np.isfinite(l1).all() and np.abs(l1 - l2).max() < 3e-2 * max(1.0, np.abs(l2).max()), (step, l1, l2)
    d1, d2 = (m1.tower_w.detach() - w0).flatten(), (m2.tower_w.detach() - w0).flatten()
    cos = float(torch.nn.functional.cosine_similarity(d1, d2, dim=0))
    print("cosine of the tower's weight updates:", cos)
    assert float(d1.abs().max()) > 0 and cos > 0.9
    for name in ("stem", "pol", "polfc", "val", "v1", "v2"):
        a, b = getattr(m1, name).weight.detach().flatten(), getattr(m2, name).weight.detach().flatten()
        assert float(torch.nn.functional.cosine_similarity(a, b, dim=0)) > 0.999, name


def test_bad_index_and_bad_symmetry_are_clamped_counted_and_raised():
    from betazero_amd.train import GraphedTrainStep
    rows, n = 40, 64
    ex = DeviceExamples.from_host(_examples(rows, 8, 50, payloads=False), DEV)
    idx, sym = _draw(rows, n, 51)
    a, b = _plans(64, 2, n, 24, "plain", 15)
    bad_idx, bad_sym = idx.copy(), sym.copy()
    bad_idx[5], bad_idx[63] = rows, -3       # clamped to the last / the first row
    bad_sym[17] = 9                          # taken & 7 = 1
    idx[5], idx[63], sym[17] = rows - 1, 0, 1
    la = a.grads(ex.own, ex.opp, ex.pi, ex.z, _dev(bad_idx), sym=_dev(bad_sym)).clone()
    tw = DeviceExamples.from_host(_twin(ex.cpu(), idx, sym), DEV)
    lb = b.grads(tw.own, tw.opp, tw.pi, tw.z).clone()
    assert torch.equal(la[:3], lb[:3])       # the step ran, on the clamped rows
    _equal_plans(a, b, "clamped")
    assert a.bad_rows(reset=False) == 3
    with pytest.raises(IndexError, match="symmetry outside 0..7"):
        a.check_rows()
    a.check_rows()                           # reset with the error word
    g = GraphedTrainStep(_net(64, 2, 24, 16), lr=1e-3, batch=n, symmetry=True)
    g.step(ex, _dev(idx), _dev(sym))
    g.check()
    bad_idx[63] = 0
    g.step(ex, _dev(bad_idx), _dev(sym))     # an index >= rows
    with pytest.raises(IndexError):
        g.check()
    g.step(ex, _dev(idx), _dev(bad_sym))     # a symmetry of 9
    with pytest.raises(IndexError):
        g.check()
    g.step(ex, _dev(idx), _dev(sym))
    g.check()


# ---------------------------------------------------------------- the loop tool (tests/test_gpu_checkpoint.py's smallest configuration)
SMALL = ["--games", "64", "--sims", "16", "--channels", "64", "--blocks", "1", "--arena-games", "16", "--arena-sims", "8", "--depth", "1",
         "--final-depths", "", "--batch", "64"]
TIMING = ("seconds", "self_play_s", "games_per_s", "train_s", "reanalyse_s")


def _loop(*flags):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "az_loop.py"), *SMALL, *flags], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    return [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]


def _untimed(d):
    if isinstance(d, dict):
        return {k: _untimed(v) for k, v in d.items() if k not in TIMING}
    return [_untimed(v) for v in d] if isinstance(d, list) else d


def test_az_loop_train_symmetry_runs_and_resumes_bit_for_bit(tmp_path):
    """three iterations in one process against two, a checkpoint, and one more in a second process: the window holds the rows as
    played (no eightfold copy), an epoch is 8 rows / batch steps, and the resumed run is the uninterrupted one -- the same
    lines, the same weights_hash, the same bytes in the saved net"""
    flags = ["--train-symmetry", "--reanalyse-frac", "0.25"]
    a, b = tmp_path / "a", tmp_path / "b"
    a.mkdir(), b.mkdir()
    whole = _loop(*flags, "--iters", "3", "--checkpoint", str(a / "run.ckpt"), "--save-net", str(a / "net.pt"))
    its = lambda lines: [d for d in lines if d.get("what") == "iteration"]  # noqa: E731
    two = its(whole)[:2]
    for d in two:
        assert d["train_symmetry"] is True and d["augmented_rows"] <= d["examples"] and np.isfinite(d["loss_last_tenth"]).all()
        assert d["steps"] == max(1, 8 * d["train_rows"] // 64)
    assert two[1]["train_rows"] == two[0]["augmented_rows"] + two[1]["augmented_rows"] and two[1]["reanalysed_rows"] > 0
    first = _loop(*flags, "--iters", "2", "--checkpoint", str(b / "run.ckpt"))
    second = _loop(*flags, "--iters", "3", "--resume", str(b / "run.ckpt"), "--checkpoint", str(b / "run.ckpt"), "--save-net", str(b / "net.pt"))
    assert [d["iter"] for d in its(whole)] == [1, 2, 3] and [d["iter"] for d in its(first)] == [1, 2] and [d["iter"] for d in its(second)] == [3]
    for x, y in zip(its(whole), its(first) + its(second)):
        assert x["weights_hash"] == y["weights_hash"], (x["iter"], x["weights_hash"], y["weights_hash"])
        assert _untimed(x) == _untimed(y), x["iter"]
    assert len({d["weights_hash"] for d in its(whole)}) == 3
    assert open(a / "net.pt", "rb").read() == open(b / "net.pt", "rb").read()
