"""A board symmetry per row inside the training step: batch position p trains on row idx[p] of the data set
under the element sym[p] of the evaluation symmetries (symmetry.SYM_NAMES: 0..6 are the augmentation's transforms 0..6, 7 is the
anti-transpose).  AlphaGo Zero's trainers keep the self-play rows as they were played and draw a rotation or reflection per
sampled position when the minibatch is formed; augment_examples' eightfold copy of the data set (the reference's supervised
recipe, SL/train.py:24-52) stays available and stays the default.

The work is ONE staging kernel, k_train_sym_batch (csrc/bz_train_sym.hip), in front of the step's stem: it gathers the batch's
rows, transforms each by its own symmetry and writes them into a staging batch (SymStaging) that the step's own descriptor
points at.  StepPlan(symmetry=True) / GraphedTrainStep(symmetry=True) own one; transform_rows() is the kernel on its own."""
import ctypes as ct

import numpy as np
import torch

from . import _lib
from .examples import DeviceExamples, columns
from .symmetry import N_SYM, sym_action_map


def check_size(size):
    """the board size the symmetries act on: an int in 1..8 (ValueError before any device is touched)"""
    if isinstance(size, bool) or not isinstance(size, (int, np.integer)) or not 1 <= int(size) <= 8:
        raise ValueError(f"symmetry: size must be an int in 1..8 (got {size!r})")
    return int(size)


def check_sym(sym, n, device):
    """the batch's symmetries: a contiguous uint8 tensor [n] on `device` (ValueError for anything else, None included)"""
    if sym is None:
        raise ValueError(f"symmetry=True needs sym: a uint8 tensor of {n} board symmetries 0..7, one per batch position")
    if not (torch.is_tensor(sym) and sym.dtype == torch.uint8 and sym.shape == (n,) and sym.is_contiguous() and sym.device == torch.device(device)):
        got = f"{sym.dtype} {tuple(sym.shape)} on {sym.device}" if torch.is_tensor(sym) else type(sym).__name__
        raise ValueError(f"sym must be a contiguous uint8 tensor of {n} board symmetries on {device} (got {got})")
    return sym


def sym_row(own, opp, pi, size, s, fown=0, fopp=0):
    """one row through the code the kernel runs (bz_train_sym_row; host, needs no GPU): ints own / opp / fown / fopp, pi a
    float32 array [65] -> (own', opp', pi', fown', fopp')"""
    pi = np.ascontiguousarray(pi, np.float32)
    if pi.shape != (65,):
        raise ValueError("sym_row: pi must hold 65 floats")
    out = np.empty(65, np.float32)
    o = [ct.c_uint64() for _ in range(4)]
    _lib.check(_lib.lib().bz_train_sym_row(int(own), int(opp), pi.ctypes.data, int(fown), int(fopp), int(size), int(s), ct.byref(o[0]),
                                           ct.byref(o[1]), out.ctypes.data, ct.byref(o[2]), ct.byref(o[3])))
    return int(o[0].value), int(o[1].value), out, int(o[2].value), int(o[3].value)


def torch_sym_rows(own, opp, pi, sym, size, fown=None, fopp=None):
    """the same transform in torch ops, where the tensors live (train_step's path, the GPU tests' reference): the cell
    permutation tau_s of symmetry.sym_action_map -- the one symmetry.sym_board moves the stones by -- applied to the boards' bits
    and to the policy's entries, pi'[tau_s(j)] = pi[j].  sym is taken & 7.  Returns (own', opp', pi', fown', fopp')."""
    size, dev = check_size(size), own.device
    maps = torch.as_tensor(np.stack([sym_action_map(size, s) for s in range(N_SYM)]).astype(np.int64), device=dev)   # [8, 65]
    t = maps[sym.to(torch.int64) & 7]                                                                                # [n, 65]
    sh = torch.arange(64, dtype=torch.int64, device=dev)

    def board(b):
        bits = (b[:, None] >> sh) & 1
        return (torch.zeros_like(bits).scatter_(1, t[:, :64], bits) << sh).sum(1)   # (int64 wraps: bit 63 is the sign)
    moved = torch.empty_like(pi).scatter_(1, t, pi)
    return (board(own), board(opp), moved, board(fown) if fown is not None else None, board(fopp) if fopp is not None else None)


class SymStaging:
    """the staging batch of n rows and the two device blocks k_train_sym_batch reads the data set through: `src`, a
    bz_train_batch (own / opp / pi / z / idx / n_rows), and `cols`, a bz_train_sym_cols (vt / fown / fopp / sym).  set_source()
    rewrites the blocks, launch() is the kernel -- nothing else: a captured launch keeps working on a new data set.
    own / opp / pi / z (and vt, fown / fopp when asked for) are the staged rows; `bad` holds one error word per workgroup."""

    def __init__(self, n, size, device, vt=False, ownership=False):
        self.size = check_size(size)
        _lib.require_gpu()
        L, dev = _lib.lib(), torch.device(device)
        self.n, self.device = int(n), dev
        z64 = lambda: torch.zeros(self.n, dtype=torch.int64, device=dev)  # noqa: E731
        self.own, self.opp = z64(), z64()
        self.pi = torch.zeros((self.n, 65), dtype=torch.float32, device=dev)
        self.z = torch.zeros(self.n, dtype=torch.int8, device=dev)
        self.vt = torch.zeros(self.n, dtype=torch.float32, device=dev) if vt else None
        self.fown, self.fopp = (z64(), z64()) if ownership else (None, None)
        rpw = L.bz_train_sym_rows_per_workgroup()
        self.bad = torch.zeros((self.n + rpw - 1) // rpw, dtype=torch.int32, device=dev)
        self.src = torch.zeros(ct.sizeof(_lib.TrainBatch), dtype=torch.uint8, device=dev)
        self.cols = torch.zeros(ct.sizeof(_lib.TrainSymCols), dtype=torch.uint8, device=dev)
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        self._stage = _lib.TrainSymStage(own=self.own.data_ptr(), opp=self.opp.data_ptr(), pi=self.pi.data_ptr(), z=self.z.data_ptr(),
                                         vt=ptr(self.vt), fown=ptr(self.fown), fopp=ptr(self.fopp))
        self._refs = None

    def set_source(self, own, opp, pi, z, idx, sym, vt=None, fown=None, fopp=None):
        """point the kernel at rows idx (None: rows 0..n-1) of the data set and at the batch's symmetries.  The tensors have
        been checked by the caller (StepPlan.set_batch's rules); they are kept alive until the next call.  Asynchronous on the
        current stream."""
        ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
        a = bytes(_lib.TrainBatch(own=own.data_ptr(), opp=opp.data_ptr(), pi=pi.data_ptr(), z=z.data_ptr(), idx=ptr(idx), n_rows=int(own.shape[0])))
        b = bytes(_lib.TrainSymCols(vt=ptr(vt) if self.vt is not None else None, fown=ptr(fown) if self.fown is not None else None,
                                    fopp=ptr(fopp) if self.fopp is not None else None, sym=sym.data_ptr()))
        with torch.cuda.device(self.device):   # (pageable host copies: ordered on the current stream, done on return)
            if self._refs is None or self._refs[0] != a:
                self.src.copy_(torch.frombuffer(bytearray(a), dtype=torch.uint8))
            if self._refs is None or self._refs[1] != b:
                self.cols.copy_(torch.frombuffer(bytearray(b), dtype=torch.uint8))
        self._refs = (a, b, own, opp, pi, z, idx, sym, vt, fown, fopp)

    def launch(self):
        if self._refs is None:
            raise RuntimeError("SymStaging: set_source() first")
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().bz_train_sym_batch(self.src.data_ptr(), self.cols.data_ptr(), self.n, self.size, ct.byref(self._stage),
                                                     self.bad.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream))

    def bad_rows(self, reset=True):
        """batch positions since the last reset whose row index was outside the data set or whose symmetry was outside 0..7
        (synchronises)"""
        n = int(self.bad.sum().item())
        if n and reset:
            self.bad.zero_()
        return n


def transform_rows(ex, idx, sym, check=True):
    """the staging kernel on its own: DeviceExamples of the len(idx) rows idx of ex, row p under the symmetry sym[p] -- own, opp,
    pi, z and, where ex carries them, vt, fown and fopp as the kernel staged them; `act` goes through the same cell permutation
    (a table look-up in torch), every other column is the source row's.  idx: int64 [n], sym: uint8 [n], both on ex's device.
    check: raise IndexError when an index was outside ex or a symmetry outside 0..7 (synchronises); without it such a position
    holds the clamped row under sym & 7."""
    if not isinstance(ex, DeviceExamples):
        raise ValueError("transform_rows: ex must be DeviceExamples (DeviceExamples.from_host uploads host rows)")
    size, dev = check_size(ex.size), ex.own.device
    if not (torch.is_tensor(idx) and idx.dtype == torch.int64 and idx.dim() == 1 and idx.numel() >= 1 and idx.is_contiguous() and idx.device == dev):
        raise ValueError(f"transform_rows: idx must be a contiguous int64 tensor of at least one row number on {dev}")
    n = int(idx.numel())
    check_sym(sym, n, dev)
    if len(ex) < 1:
        raise ValueError("transform_rows: the data set is empty")
    if ex.pi.shape != (len(ex), 65):
        raise ValueError("transform_rows: the symmetries act on the Reversi boards' 65 actions")
    if (ex.fown is None) != (ex.fopp is None):
        raise ValueError("transform_rows: the examples must carry both fown and fopp (ownership target), or neither")
    st = SymStaging(n, size, dev, vt=ex.vt is not None, ownership=ex.fown is not None)
    c = lambda t: t.contiguous() if t is not None else None  # noqa: E731
    st.set_source(c(ex.own), c(ex.opp), c(ex.pi), c(ex.z), idx, sym, vt=c(ex.vt), fown=c(ex.fown), fopp=c(ex.fopp))
    st.launch()
    if check:
        bad = st.bad_rows()
        if bad:
            raise IndexError(f"transform_rows: {bad} position(s) had a row index outside the data set or a symmetry outside 0..7")
    staged = {k: getattr(st, k) for k in ("own", "opp", "pi", "z", "vt", "fown", "fopp") if getattr(st, k) is not None}
    rows = idx.clamp(0, len(ex) - 1)
    maps = torch.as_tensor(np.stack([sym_action_map(size, s) for s in range(N_SYM)]), device=dev)   # uint8 [8, 65]
    staged["act"] = maps[sym.to(torch.int64) & 7, ex.act[rows].to(torch.int64)]
    return DeviceExamples(size=size, **{k: staged[k] if k in staged else t[rows] for k, t in columns(ex).items()})
