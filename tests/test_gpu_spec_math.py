"""The float primitives of csrc/bz_math.h as the gfx950 build computes them (bz_spec_probe, where = device) against the host
build: every bit-exact claim of the project assumes the two return the same bits.  "Equal" = the same bits,
every NaN counted as one value.  Differences allowed: 0."""
import os

import numpy as np
import pytest
import torch

from betazero_amd import _lib
from oracle import spec_math as sm
from test_spec_math_cpu import EDGES, NANS, counter_u64, fdiv_pairs, first_difference, gamma_inputs, sqrt_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = os.path.join(os.path.dirname(__file__), "golden")
f32, u64 = np.float32, np.uint64


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x).view(np.int32 if x.dtype == f32 else np.int64)).to(DEV)


def device_map(op, a, b=None):
    ta, tb = _dev(a), _dev(b)
    out = torch.empty(a.shape[0], dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().bz_spec_probe(sm.OP[op], _lib.PROBE_DEVICE, _lib.PROBE_MAP, ta.data_ptr(), tb.data_ptr() if tb is not None else None,
                                        a.shape[0], 0, 0, out.data_ptr(), torch.cuda.current_stream().cuda_stream))
    return out.cpu().numpy().view(f32)


def device_sweep(op, lo, hi):
    out = torch.empty(((hi - 1) >> 24) - (lo >> 24) + 1, dtype=torch.int64, device=DEV)
    _lib.check(_lib.lib().bz_spec_probe(sm.OP[op], _lib.PROBE_DEVICE, _lib.PROBE_SWEEP, None, None, 0, lo, hi, out.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream))
    return out.cpu().numpy().view(u64)


def _map_inputs(op):
    if op == "expf_spec":   # its domain: x <= 0 and NaN; a dense run of arguments of the softmax and of tanh besides the edges
        return (np.concatenate([EDGES[(EDGES <= 0) | np.isnan(EDGES)], -(counter_u64(1 << 20, 7) >> u64(40)).astype(f32) * f32(88.0 / (1 << 24))]),)
    if op == "tanhf_spec":
        return (np.concatenate([EDGES, ((counter_u64(1 << 20, 8) >> u64(40)).astype(f32) - f32(1 << 23)) * f32(12.0 / (1 << 23))]),)
    if op == "fsqrt":
        return (sqrt_inputs(),)
    if op == "logf_spec":   # all 2^23 mantissas at the exponents -126, -1, 0, 1, 127
        m = np.arange(1 << 23, dtype=np.uint32)
        return (np.concatenate([EDGES] + [(m | np.uint32((e + 127) << 23)).view(f32) for e in (-126, -1, 0, 1, 127)]),)
    if op == "fdiv":
        return fdiv_pairs()
    if op == "u01_spec":    # all 2^23 values of bits >> 41, under varying low bits
        return ((np.arange(1 << 23, dtype=u64) << u64(41)) | (counter_u64(1 << 23, 9) >> u64(23)),)
    if op == "hash_logit":
        return counter_u64(1 << 20, 10), np.arange(1 << 20, dtype=u64) % u64(65)
    if op == "hash_value":
        return (counter_u64(1 << 20, 11),)
    assert op == "gamma_spec"
    return gamma_inputs()


def test_device_sweep_equals_fixture():
    """every chunk checksum of every sweep op -- expf_spec on -0 .. -inf and +0, logf_spec on every positive finite pattern,
    tanhf_spec and fsqrt on all 2^32 -- equals what the host build recorded in tests/golden/spec_math.npz: host == device on
    ~1.5e10 evaluations.  Chunks allowed to differ: 0."""
    d = np.load(os.path.join(G, "spec_math.npz"))
    bad = {}
    for op, ranges in sm.SWEEPS.items():
        got = np.concatenate([device_sweep(op, lo, hi) for lo, hi in ranges])
        ch = sm.chunks(ranges)
        assert got.shape == d[op + "_sum"].shape == (len(ch),)
        diff = np.nonzero(got != d[op + "_sum"])[0]
        print(op, len(ch), "chunks,", diff.size, "differ")
        if diff.size:
            bad[op] = ["0x%08X..0x%08X" % (ch[i][0], ch[i][1] - 1) for i in diff[:8]] + [f"{diff.size} of {len(ch)} chunks"]
    assert not bad, bad


@pytest.mark.parametrize("op", _lib.PROBE_OPS)
def test_device_map_equals_host_map(op):
    """the same input arrays through both builds, outputs compared bit for bit; names the first differing input.  fsqrt: the
    integers 1 .. 8189 (sq of the PUCT selection and the LDS table of k_tree_step) and 2^20 arguments of forced_nf; logf_spec:
    all 2^23 mantissas at five exponents; fdiv: the edge list squared, the denormal / overflow quotients and 2^20 pattern
    pairs; u01_spec: all 2^23 inputs; the hash ops: 2^20 words; gamma_spec: 4 alphas x 64 edges x 4096 (game, ply) pairs."""
    args = _map_inputs(op)
    host, dev = sm.host_map(op, *args), device_map(op, *args)
    x = args[0] if len(args) == 1 else np.stack([args[0], args[1][:, -1] if args[1].ndim == 2 else args[1]], 1)
    assert first_difference(x, dev, host) is None, f"{op}: (n differing, first index, input, device bits, host bits)"


def test_sqrt_table_inputs():
    """the 128 entries k_tree_step keeps in LDS are fsqrt(max(i, 1)), i = 0 .. 127: fsqrt of the integers 1 .. 127.  That range
    is part of test_device_map_equals_host_map[fsqrt] (1 .. 8189), so there is no hook into the engine for it; here the same
    range is held to IEEE directly: the device's fsqrt is numpy's correctly rounded float32 sqrt.  (The probe compiles its
    own copy of fsqrt: the table as the engine fills it stays covered by the engine-level parity tests.)"""
    x = np.arange(128, dtype=f32)
    assert first_difference(x, device_map("fsqrt", x), np.sqrt(x)) is None


def test_device_nan_in_nan_out():
    for op in ("expf_spec", "tanhf_spec", "fsqrt"):
        assert np.isnan(device_map(op, NANS)).all(), op
