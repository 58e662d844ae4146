"""Checkpoints without a GPU: every column of the example rows through the .npz format, the checkpoint file
(atomic write, safe load, version) and tools/az_loop.py's refusal of a checkpoint that does not fit.  "Equal" = bit for bit."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTIONAL = ("kl", "q", "vt", "fown", "fopp", "count")
INT_VIEW = {4: np.uint32, 8: np.uint64, 1: np.uint8}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(INT_VIEW[a.dtype.itemsize])


def _rows(n=37, seed=5, without=()):
    """rows with every optional column (NaNs with distinct payloads, infinities, -0.0 in the float ones; bit 63 in the boards)"""
    from betazero_amd.engine import Examples
    rng = np.random.default_rng(seed)
    u64 = lambda: rng.integers(0, 2**63, n, dtype=np.int64).astype(np.uint64) | (rng.integers(0, 2, n).astype(np.uint64) << np.uint64(63))  # noqa: E731

    def f32():
        a = rng.standard_normal(n).astype(np.float32)
        a.view(np.uint32)[:5] = [0x7FC00001, 0xFFC12345, 0x7F800000, 0x80000000, 0x7F800001]   # NaN payloads, +inf, -0.0, sNaN
        return a
    opt = dict(kl=f32(), q=f32(), vt=f32(), fown=u64(), fopp=u64(), count=rng.integers(1, 2**31 - 1, n).astype(np.int32))
    pi = rng.random((n, 65)).astype(np.float32)
    pi.view(np.uint32)[0, :2] = [0x7FC0BEEF, 0x80000000]
    return Examples(u64(), u64(), pi, rng.integers(-1, 2, n).astype(np.int8), rng.choice([-1, 1], n).astype(np.int8),
                    rng.integers(0, 65, n).astype(np.uint8), rng.integers(0, 10**12, n), rng.integers(0, 60, n).astype(np.int32), 8,
                    **{k: v for k, v in opt.items() if k not in without})


# ---------------------------------------------------------------- the rows on disk
@pytest.mark.parametrize("without", [()] + [(k,) for k in OPTIONAL] + [OPTIONAL])
def test_npz_round_trip_carries_every_column_the_rows_have(tmp_path, without):
    from betazero_amd.examples_io import load_examples_npz, save_examples_npz
    ex = _rows(without=without)
    p = str(tmp_path / "rows.npz")
    save_examples_npz(ex, p)
    back = load_examples_npz(p)
    assert back.size == ex.size and len(back) == len(ex)
    for k in ("own", "opp", "pi", "z", "mover", "act", "game", "ply") + OPTIONAL:
        a, b = getattr(ex, k), getattr(back, k)
        if k in without:
            assert b is None, k
            continue
        assert b.dtype == a.dtype and b.shape == a.shape and np.array_equal(_bits(a), _bits(b)), k
    with np.load(p) as d:
        assert sorted(d.files) == sorted(("size", "own", "opp", "pi", "z", "mover", "act", "game", "ply") + tuple(k for k in OPTIONAL if k not in without))


def test_npz_file_with_the_eight_columns_of_before_loads_as_before(tmp_path):
    from betazero_amd.examples_io import load_examples_npz
    ex = _rows(without=OPTIONAL)
    p = str(tmp_path / "old.npz")
    keys = ("own", "opp", "pi", "z", "mover", "act", "game", "ply")
    np.savez_compressed(p, size=np.int64(8), **{k: getattr(ex, k) for k in keys})   # what the writer wrote before the optional columns
    back = load_examples_npz(p)
    assert back.size == 8 and all(getattr(back, k) is None for k in OPTIONAL)
    for k in keys:
        assert getattr(back, k).dtype == getattr(ex, k).dtype and np.array_equal(_bits(getattr(back, k)), _bits(getattr(ex, k))), k


# ---------------------------------------------------------------- the checkpoint file
def _state():
    import torch
    return {"iter": 3, "args": {"channels": 64, "lr": 2e-3, "out": None, "final_depths": "1,3"}, "lines": [{"what": "x", "l": [1.5, None]}],
            "step": {"param.stem_w": torch.arange(6, dtype=torch.float32).view(2, 3), "hyper": torch.tensor([1e-3, 5.0, 300.0, 0.0]),
                     "extended": False, "C": 64},
            "optimizer": {"state": {0: {"step": torch.tensor(3.0)}}, "param_groups": [{"betas": [0.9, 0.999], "params": [0]}]},
            "generator": torch.Generator().manual_seed(4).get_state(), "window": None}


def _same(a, b):
    import torch
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and a.device.type == "cpu" == b.device.type and \
            torch.equal(a.reshape(-1).contiguous().view(torch.uint8), b.reshape(-1).contiguous().view(torch.uint8))
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def test_checkpoint_round_trip_reads_under_weights_only(tmp_path, monkeypatch):
    import torch
    from betazero_amd import checkpoint
    p = str(tmp_path / "run.ckpt")
    checkpoint.save_checkpoint(p, _state())
    assert os.listdir(tmp_path) == ["run.ckpt"]
    calls = []
    real = torch.load
    monkeypatch.setattr(torch, "load", lambda *a, **k: (calls.append(k), real(*a, **k))[1])
    assert _same(_state(), checkpoint.load_checkpoint(p))
    assert len(calls) == 1 and calls[0].get("weights_only") is True
    monkeypatch.undo()
    assert _same(_state()["step"], torch.load(p, weights_only=True)["state"]["step"])   # and by hand, with no allowlist


class _Unsavable:
    pass


def _raise_halfway(obj, f, *a, **k):
    f.write(b"half a checkpoint")
    f.flush()
    raise OSError("no space left on device")


@pytest.mark.parametrize("how", ["object_in_state", "unpicklable_in_state", "writer_fails_halfway", "replace_fails"])
def test_failed_write_leaves_the_previous_checkpoint_and_nothing_else(tmp_path, monkeypatch, how):
    import torch
    from betazero_amd import checkpoint
    p = str(tmp_path / "run.ckpt")
    checkpoint.save_checkpoint(p, _state())
    before = open(p, "rb").read()
    bad = _state()
    if how == "object_in_state":          # refused by the writer's own check of the types
        bad["lines"].append({"x": _Unsavable()})
        err = TypeError
    elif how == "unpicklable_in_state":   # past that check, refused by torch.save itself after the file was opened
        monkeypatch.setattr(checkpoint, "_check_plain", lambda *a: None)
        bad["lines"].append(lambda: 0)
        err = Exception
    elif how == "writer_fails_halfway":
        monkeypatch.setattr(torch, "save", _raise_halfway)
        err = OSError
    else:
        def boom(*a):
            raise OSError("replace failed")
        monkeypatch.setattr(os, "replace", boom)
        err = OSError
    with pytest.raises(err):
        checkpoint.save_checkpoint(p, bad)
    monkeypatch.undo()
    assert os.listdir(tmp_path) == ["run.ckpt"] and open(p, "rb").read() == before
    assert _same(_state(), checkpoint.load_checkpoint(p))


def test_first_write_that_fails_leaves_an_empty_directory(tmp_path):
    from betazero_amd import checkpoint
    with pytest.raises(TypeError, match=r"state\['step'\]\['bad'\]"):
        checkpoint.save_checkpoint(str(tmp_path / "run.ckpt"), {"step": {"bad": {1, 2}}})
    assert os.listdir(tmp_path) == []


def test_unknown_version_and_foreign_files_are_refused(tmp_path):
    import torch
    from betazero_amd import checkpoint
    p = str(tmp_path / "run.ckpt")
    torch.save({"format": checkpoint.FORMAT, "version": checkpoint.VERSION + 1, "state": {}}, p)
    with pytest.raises(ValueError, match=f"version {checkpoint.VERSION + 1}"):
        checkpoint.load_checkpoint(p)
    torch.save({"stem.weight": torch.zeros(2)}, p)   # a --save-net file is not a checkpoint
    with pytest.raises(ValueError, match="not a"):
        checkpoint.load_checkpoint(p)


# ---------------------------------------------------------------- the loop's refusals
def _az_loop():
    spec = importlib.util.spec_from_file_location("az_loop_tool", os.path.join(ROOT, "tools", "az_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


SMALL = ["--games", "64", "--sims", "16", "--channels", "64", "--blocks", "1", "--arena-games", "16", "--arena-sims", "8", "--depth", "1",
         "--final-depths", "", "--batch", "64"]


@pytest.mark.parametrize("flags,words", [(["--channels", "128"], ("--channels", "64", "128")),
                                         (["--seed", "1"], ("--seed",)),
                                         (["--weight-decay", "1e-4"], ("--weight-decay",)),
                                         (["--ownership"], ("--ownership",)),
                                         (["--init-net", "x.pt"], ("--init-net", "--resume"))])
def test_az_loop_refuses_a_checkpoint_that_does_not_fit_before_a_device_is_touched(tmp_path, flags, words):
    from betazero_amd.checkpoint import save_checkpoint
    args = vars(_az_loop().build_parser().parse_args(SMALL + ["--iters", "2", "--checkpoint", "elsewhere.ckpt"]))
    p = str(tmp_path / "run.ckpt")
    save_checkpoint(p, {"iter": 2, "args": args, "lines": []})   # the host-side check needs no more than this
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "az_loop.py"), *SMALL, "--iters", "4", "--resume", p, *flags],   # (a repeated flag: the last one holds)
                         capture_output=True, text=True, timeout=300,   # (an argument error: no device is visible, and none is asked for)
                         env={**os.environ, "HIP_VISIBLE_DEVICES": "", "CUDA_VISIBLE_DEVICES": ""})
    assert out.returncode == 2 and all(w in out.stderr for w in words), out.stderr[-500:]
    assert "Traceback" not in out.stderr


def test_az_loop_refuses_a_file_that_is_no_checkpoint(tmp_path):
    import torch
    p = str(tmp_path / "net.pt")
    torch.save({"stem.weight": torch.zeros(2)}, p)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "az_loop.py"), *SMALL, "--resume", p], capture_output=True, text=True,
                         timeout=300, env={**os.environ, "HIP_VISIBLE_DEVICES": "", "CUDA_VISIBLE_DEVICES": ""})
    assert out.returncode == 2 and "--resume" in out.stderr and "Traceback" not in out.stderr, out.stderr[-500:]
