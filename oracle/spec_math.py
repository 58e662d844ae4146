"""The float primitives of csrc/bz_math.h through bz_spec_probe  -- TEST INFRASTRUCTURE ONLY.

Shared by oracle/gen_golden.py (fixture tests/golden/spec_math.npz, written from the HOST build) and by
tests/test_spec_math_cpu.py / tests/test_gpu_spec_math.py: the sweep domains, the chunking, the host calls and the error of
each function against float64 numpy."""
import ctypes as C

import numpy as np

from betazero_amd import _lib

OP = {name: i for i, name in enumerate(_lib.PROBE_OPS)}
CHUNK = 1 << 24
# the 32-bit patterns every sweep op is pinned over, host == device: [lo, hi) ranges
SWEEPS = {
    "expf_spec": ((0x80000000, 0xFF800001), (0, 1)),   # -0 .. -inf, and +0
    "logf_spec": ((0x00000001, 0x7F800000),),          # every positive finite value, denormals included
    "tanhf_spec": ((0, 1 << 32),),
    "fsqrt": ((0, 1 << 32),),
}
# where the accuracy bound of each function holds: exp on [-87, 0], ln on positive normals, tanh on every finite input
ACCURACY = {
    "expf_spec": ((0x80000000, 0xC2AE0001), (0, 1)),
    "logf_spec": ((0x00800000, 0x7F800000),),
    "tanhf_spec": ((0, 0x7F800000), (0x80000000, 0xFF800000)),
}
BOUND = {"expf_spec": 1e-7, "logf_spec": 1e-7, "tanhf_spec": 1e-7}


def chunks(ranges):
    """the ranges cut at multiples of 2^24, in order: one (lo, hi) per checksum bz_spec_probe returns"""
    out = []
    for lo, hi in ranges:
        p = lo
        while p < hi:
            q = min(hi, (p // CHUNK + 1) * CHUNK)
            out.append((p, q))
            p = q
    return out


def spread(ranges, n=16):
    """n of the chunks, evenly spread from the first to the last"""
    ch = chunks(ranges)
    return [ch[i] for i in sorted(set(np.linspace(0, len(ch) - 1, n).round().astype(int).tolist()))]


def canon(bits):
    """every NaN pattern -> 0x7FC00000"""
    bits = np.asarray(bits).view(np.uint32)
    return np.where((bits & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), np.uint32(0x7FC00000), bits)


def patterns(lo, hi):
    return np.arange(lo, hi, dtype=np.uint64).astype(np.uint32).view(np.float32)


def _ptr(x):
    return None if x is None else x.ctypes.data


def host_map(op, a, b=None):
    """op over host arrays (float32 or uint64, see include/bz_abi.h) -> float32 [n], bits untouched"""
    a = np.ascontiguousarray(a)
    b = None if b is None else np.ascontiguousarray(b)
    assert a.dtype in (np.float32, np.uint64) and (b is None or b.dtype in (np.float32, np.uint64))
    out = np.empty(a.shape[0], np.float32)
    _lib.check(_lib.lib().bz_spec_probe(OP[op], _lib.PROBE_HOST, _lib.PROBE_MAP, _ptr(a), _ptr(b), a.shape[0], 0, 0, _ptr(out), None))
    return out


def host_sweep(op, lo, hi):
    """-> uint64 checksums, one per 2^24-pattern chunk of [lo, hi)"""
    out = np.zeros(((hi - 1) >> 24) - (lo >> 24) + 1, np.uint64)
    _lib.check(_lib.lib().bz_spec_probe(OP[op], _lib.PROBE_HOST, _lib.PROBE_SWEEP, None, None, 0, lo, hi, _ptr(out), None))
    return out


def error(op, x, y):
    """the error of y = op(x) (float32 arrays) in the measure of BOUND[op], against float64 numpy"""
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    with np.errstate(all="ignore"):
        if op == "expf_spec":
            ref = np.exp(x64)
            return np.abs(y64 - ref) / ref
        if op == "logf_spec":
            ref = np.log(x64)
            return np.abs(y64 - ref) / np.maximum(1.0, np.abs(ref))
        assert op == "tanhf_spec"
        return np.abs(y64 - np.tanh(x64))


def chunk_max_error(op, lo, hi):
    """(max error, the pattern it is at) of the host build over the patterns [lo, hi)"""
    x = patterns(lo, hi)
    err = error(op, x, host_map(op, x))
    i = int(np.argmax(err))
    return float(err[i]), lo + i
