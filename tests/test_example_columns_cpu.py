"""The column table of betazero_amd/examples.py without a GPU (DeviceExamples on device="cpu"): COLUMNS against the two
dataclasses, the host <-> device round trip, and rows with EVERY column through every carrier of rows -- take / select_rows,
the concat functions, the .npz format, az_loop's window_rows / rows_to_device.  The loops run over COLUMNS, not over a list of
this file's: a column that is added to the table and dropped by a carrier fails here.  "Equal" = bit for bit."""
import dataclasses
import importlib.util
import os

import numpy as np
import pytest
import torch

from betazero_amd.examples import COLUMNS, DeviceExamples, Examples, columns, concat_device_examples, concat_examples, take

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTIONAL = [c.name for c in COLUMNS if c.optional]
INT_VIEW = {1: np.uint8, 4: np.uint32, 8: np.uint64}


def _bits(a):
    a = np.ascontiguousarray(a.numpy() if torch.is_tensor(a) else a)
    return a.view(INT_VIEW[a.dtype.itemsize])


def _rows(n=7, first=0, without=()):
    """n tic-tac-toe rows, every column filled from the table with values that tell the column and the row: value first + i
    + 1000 * (the column's index) in the column's dtype; the uint64 columns with bit 63 set, pi[., 0] a NaN with the row in
    its payload"""
    cols = {}
    for j, c in enumerate(COLUMNS):
        v = np.arange(first, first + n, dtype=np.int64) + 1000 * j
        if c.host is np.uint64:
            a = v.astype(np.uint64) | np.uint64(1 << 63)
        elif c.na:
            a = (v[:, None] + np.arange(9) / 16).astype(c.host)
            a.view(np.uint32)[:, 0] = 0x7FC00000 + np.arange(first, first + n) + 1
        else:
            a = (v % 100 if np.dtype(c.host).itemsize == 1 else v).astype(c.host)
        cols[c.name] = a
    return Examples(size=3, **{k: a for k, a in cols.items() if k not in without})


def _same(got, want, where):
    """got (Examples or DeviceExamples) carries every column of the table and each equals want's (host Examples)"""
    host = isinstance(got, Examples)
    assert got.size == want.size, where
    for c in COLUMNS:
        a, b = getattr(got, c.name), getattr(want, c.name)
        assert a is not None, (where, c.name)
        assert (a.dtype == c.host) if host else (a.dtype == c.device), (where, c.name, a.dtype)
        assert tuple(a.shape) == b.shape and np.array_equal(_bits(a), _bits(b)), (where, c.name)


def _az_loop():
    spec = importlib.util.spec_from_file_location("az_loop_tool", os.path.join(ROOT, "tools", "az_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------- 1. the table and the dataclasses
@pytest.mark.parametrize("cls", [Examples, DeviceExamples])
def test_the_dataclass_fields_are_the_tables_columns_in_order(cls):
    fields = [f for f in dataclasses.fields(cls) if f.name != "size"]
    assert [f.name for f in fields] == [c.name for c in COLUMNS]
    assert [f.default is None for f in fields] == [c.optional for c in COLUMNS]   # (a required field's default is MISSING)
    assert [f.name for f in dataclasses.fields(cls)].index("size") == 8            # the tools construct the rows positionally
    assert all(c.label for c in COLUMNS if c.optional) and all(c.meaning for c in COLUMNS)
    assert [c.name for c in COLUMNS if c.na] == ["pi"]


# ---------------------------------------------------------------- 2. host <-> device
@pytest.mark.parametrize("without", [None] + OPTIONAL)
def test_from_host_and_cpu_round_trip_every_column_bit_for_bit(without):
    ex = _rows(without=(without,))
    dev = DeviceExamples.from_host(ex, "cpu")
    back = dev.cpu()
    assert isinstance(back, Examples) and back.size == ex.size == dev.size and len(back) == len(dev) == len(ex)
    for c in COLUMNS:
        a, d, b = getattr(ex, c.name), getattr(dev, c.name), getattr(back, c.name)
        if c.name == without:
            assert d is None and b is None, c.name
            continue
        assert d.dtype == c.device and b.dtype == c.host and b.shape == a.shape, c.name
        assert np.array_equal(_bits(d), _bits(a)) and np.array_equal(_bits(b), _bits(a)), c.name
    assert [k for k in OPTIONAL if getattr(back, k) is None] == ([without] if without else [])


def test_from_host_casts_to_the_tables_dtypes_and_cpu_makes_ply_int32():
    ex = _rows()
    ex.ply, ex.game, ex.z = np.arange(len(ex), dtype=np.int64), ex.game.astype(np.int32), ex.z.astype(np.int64)
    dev = DeviceExamples.from_host(ex, "cpu")
    assert all(getattr(dev, c.name).dtype == c.device for c in COLUMNS)
    dev.ply = dev.ply.to(torch.uint8)   # (what a packed block holds)
    assert dev.cpu().ply.dtype == np.int32 and np.array_equal(dev.cpu().ply, ex.ply)


# ---------------------------------------------------------------- 3. every carrier carries every column
@pytest.mark.parametrize("idx", [[5, 0, 5, 2], []])
def test_take_and_select_rows_carry_every_column(idx):
    from betazero_amd.train import select_rows
    ex = _rows()
    want = Examples(size=3, **{k: a[np.asarray(idx, np.int64)] for k, a in columns(ex).items()})
    assert len(columns(want)) == len(COLUMNS)
    got = take(ex, np.asarray(idx, np.int64))
    assert isinstance(got, Examples)
    _same(got, want, "take, host")
    dev = DeviceExamples.from_host(ex, "cpu")
    for fn in (take, select_rows):
        got = fn(dev, torch.tensor(idx, dtype=torch.int64))
        assert isinstance(got, DeviceExamples) and len(got) == len(idx)
        _same(got, want, fn.__name__)


def test_take_leaves_absent_columns_absent():
    got = take(DeviceExamples.from_host(_rows(without=("q", "count")), "cpu"), torch.tensor([1, 1]))
    assert [k for k in OPTIONAL if getattr(got, k) is None] == ["q", "count"]


def test_concat_carries_every_column():
    a, b = _rows(4), _rows(3, first=4)
    want = _rows(7)
    got = concat_examples([a, b])
    assert isinstance(got, Examples)
    _same(got, want, "concat_examples")
    got = concat_device_examples([DeviceExamples.from_host(a, "cpu"), DeviceExamples.from_host(b, "cpu")])
    assert isinstance(got, DeviceExamples)
    _same(got, want, "concat_device_examples")


def test_npz_carries_every_column(tmp_path):
    from betazero_amd.examples_io import load_examples_npz, save_examples_npz
    ex = _rows()
    for what, rows in (("host", ex), ("device", DeviceExamples.from_host(ex, "cpu"))):
        p = str(tmp_path / f"{what}.npz")
        save_examples_npz(rows, p)
        _same(load_examples_npz(p), ex, f"npz, {what}")
        with np.load(p) as d:
            assert sorted(d.files) == sorted(["size"] + [c.name for c in COLUMNS])


def test_window_rows_and_rows_to_device_carry_every_column():
    tool = _az_loop()
    ex = _rows()
    rows = tool.window_rows(DeviceExamples.from_host(ex, "cpu"))
    assert sorted(rows) == sorted(["size"] + [c.name for c in COLUMNS]) and rows["size"] == 3
    got = tool.rows_to_device(rows, "cpu")
    assert isinstance(got, DeviceExamples)
    _same(got, ex, "window_rows -> rows_to_device")


# ---------------------------------------------------------------- 4. all-or-none
@pytest.mark.parametrize("name", OPTIONAL)
def test_concat_refuses_a_column_that_only_some_parts_carry(name):
    a, b = _rows(4), _rows(3, first=4, without=(name,))
    for parts in ([a, b], [b, a]):
        with pytest.raises(ValueError, match=f"every part must carry {name} "):
            concat_examples(parts)
        with pytest.raises(ValueError, match=f"every part must carry {name} "):
            concat_device_examples([DeviceExamples.from_host(p, "cpu") for p in parts])
    both = concat_examples([b, b])   # none carries it: fine, and it stays absent
    assert [k for k in OPTIONAL if getattr(both, k) is None] == [name]


def test_the_all_or_none_message_is_the_one_of_before():
    a, b = _rows(2), _rows(2, without=("kl",))
    with pytest.raises(ValueError) as e:
        concat_examples([a, b])
    assert str(e.value) == "concatenating examples: every part must carry kl (policy surprise), or none"
    with pytest.raises(ValueError, match=r"every part must carry fopp \(ownership target\), or none"):
        concat_examples([a, _rows(2, without=("fopp",))])


# ---------------------------------------------------------------- 5. merged rows stay refused by reanalysis
def test_check_reanalyse_still_refuses_merged_rows_after_a_selection_or_a_concat():
    from betazero_amd.reanalyse import check_reanalyse
    from betazero_amd.train import select_rows
    merged = DeviceExamples.from_host(_rows(without=("vt", "fown", "fopp")), "cpu")
    assert merged.count is not None
    for what, ex in (("as they are", merged), ("select_rows", select_rows(merged, torch.tensor([0, 3, 3]))),
                     ("concat", concat_device_examples([merged, merged])), ("host concat", concat_examples([merged.cpu(), merged.cpu()]))):
        with pytest.raises(ValueError, match="merged positions"):
            check_reanalyse(ex, None, True, 3)
    plain = DeviceExamples.from_host(_rows(without=("vt", "fown", "fopp", "count")), "cpu")
    assert check_reanalyse(select_rows(plain, torch.tensor([0, 3, 3])), None, True, 3) == 3
