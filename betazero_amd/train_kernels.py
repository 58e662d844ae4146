"""The residual tower's training step on the hand-written HIP kernels of csrc/bz_train.hip (bz_train_* in
include/bz_abi.h): forward with saved activations, backward-data, backward-weights -- as ONE torch.autograd.Function,
so that stem, heads, losses and the optimiser stay plain torch (the loop shape of src/tic_tac_toe/SL/train.py:85-136).

    plan = TowerPlan(C, n_layers, batch)                    # every device buffer of one training shape, allocated once
    y = tower_apply(x0, W, b, plan)                         # x0 [n, C, 8, 8] = relu(stem(planes)); W [L, C, C, 3, 3]; b [L, C]
    loss(y).backward()                                      # d/dx0, d/dW, d/db through the kernels

bf16 activations and gradients, fp32 accumulation, fp32 master weights (the kernels repack W into their bf16 fragment
streams every step -- 2 x 147 k values per layer at C = 128).  There is no CPU path: without the HIP library or a GPU
this raises.  PolicyValueNet uses these kernels when its forward() is handed a TowerPlan (fused_tower form); its plain
forward() is the torch definition of the same net (CPU tests, the fp32 reference of the GPU tests).

StepPlan goes one further: the WHOLE step's forward, losses and backward on kernels (csrc/bz_train_ends.hip adds the stem,
the heads with their losses, the reduction of every partial sum into the parameters' .grad tensors, and Adam) -- 9
launches for the gradients, a tenth for the update, no autograd, no torch kernel; the batch's rows are gathered by the
kernels themselves.  That is what GraphedTrainStep captures by default."""
import ctypes as ct

import torch

from . import _lib


class TowerPlan:
    """device buffers of one (channels, conv layers, batch) training shape:
    acts / gs [L + 1, n, 64, C] bf16 (act[a], g[a] of bz_abi.h), the ReLU bit masks, the two weight-fragment streams,
    the weight-gradient partials and C zeros.  Static addresses: a step can be captured into a HIP graph."""

    def __init__(self, channels, n_layers, batch, device="cuda:0"):
        _lib.require_gpu()
        L = _lib.lib()
        self.C, self.L, self.n, self.device = channels, n_layers, batch, torch.device(device)
        P = L.bz_train_positions_per_workgroup(channels)
        if P <= 0 or n_layers < 2 or n_layers % 2:
            raise ValueError("the training kernels are built for 64 or 128 channels and an even number of conv layers")
        if batch % P:
            raise ValueError(f"batch must be a multiple of {P} at {channels} channels (positions resident per workgroup)")
        dev = self.device
        self.acts = torch.zeros((n_layers + 1, batch, 64, channels), dtype=torch.bfloat16, device=dev)
        self.gs = torch.zeros((n_layers + 1, batch, 64, channels), dtype=torch.bfloat16, device=dev)
        self.masks = torch.zeros(L.bz_train_mask_bytes(channels, n_layers, batch), dtype=torch.uint8, device=dev)
        nb = L.bz_train_wf_bytes(channels, n_layers)
        self.wf_fwd = torch.zeros(nb, dtype=torch.uint8, device=dev)   # (the 2 taps of padding behind the stream stay zero)
        self.wf_bwd = torch.zeros(nb, dtype=torch.uint8, device=dev)
        self.splits = L.bz_train_wgrad_splits(channels, n_layers, batch)
        self.partial = torch.zeros((n_layers, self.splits, 9, channels, channels), dtype=torch.float32, device=dev)
        self.db_partial = torch.zeros((n_layers, L.bz_train_wgrad_bias_rows(channels, self.splits), channels), dtype=torch.float32, device=dev)
        self.zeros_c = torch.zeros(channels, dtype=torch.float32, device=dev)

    def _stream(self):
        return torch.cuda.current_stream(self.device).cuda_stream


class _TowerFn(torch.autograd.Function):
    """x0 / the result / their gradients are [n, C, 8, 8] (nhwc=False: what a torch conv net passes around) or
    [n, 64, C] (nhwc=True: the kernels' own layout -- no permute copies at either end)"""

    @staticmethod
    def forward(ctx, x0, W, b, plan, nhwc):
        L, p = _lib.lib(), plan
        n, C, Ly = p.n, p.C, p.L
        assert x0.shape == ((n, 64, C) if nhwc else (n, C, 8, 8)), "input shape does not match the plan"
        assert W.shape == (Ly, C, C, 3, 3) and b.shape == (Ly, C), "weight shapes do not match the plan"
        Wc, bc = W.detach().contiguous().float(), b.detach().contiguous().float()
        with torch.cuda.device(p.device):
            p.acts[0].copy_(x0.detach() if nhwc else x0.detach().permute(0, 2, 3, 1).reshape(n, 64, C))
            _lib.check(L.bz_train_pack_weights(Wc.data_ptr(), C, Ly, p.wf_fwd.data_ptr(), p.wf_bwd.data_ptr(), p._stream()))
            _lib.check(L.bz_train_tower_fwd(p.acts[0].data_ptr(), p.wf_fwd.data_ptr(), bc.data_ptr(), C, Ly, n,
                                            p.acts[1].data_ptr(), p.masks.data_ptr(), p._stream()))
        ctx.plan, ctx.nhwc, ctx.in_dtype = p, nhwc, x0.dtype
        y = p.acts[Ly]
        return y.to(x0.dtype, copy=True) if nhwc else y.view(n, 8, 8, C).permute(0, 3, 1, 2).to(x0.dtype, copy=True)

    @staticmethod
    def backward(ctx, gy):
        L, p = _lib.lib(), ctx.plan
        n, C, Ly = p.n, p.C, p.L
        with torch.cuda.device(p.device):
            # g[L] = d loss / d (pre-activation of act[L]): the incoming gradient times the last layer's ReLU pattern
            gyn = gy if ctx.nhwc else gy.permute(0, 2, 3, 1).reshape(n, 64, C)
            torch.mul(gyn, p.acts[Ly] > 0, out=p.gs[Ly])
            _lib.check(L.bz_train_tower_bwd(p.gs[Ly].data_ptr(), p.wf_bwd.data_ptr(), p.zeros_c.data_ptr(), p.masks.data_ptr(),
                                            C, Ly, n, p.gs[0].data_ptr(), p._stream()))
            _lib.check(L.bz_train_wgrad(p.acts[0].data_ptr(), p.gs[1].data_ptr(), C, Ly, n, p.splits, p.partial.data_ptr(),
                                        p.db_partial.data_ptr(), p._stream()))
        # sum over the batch slices, then [L, tap, ci, co] -> torch's [L, co, ci, 3, 3]
        dW = p.partial.sum(1).view(Ly, 3, 3, C, C).permute(0, 4, 3, 1, 2).contiguous()
        db = p.db_partial.sum(1)
        g0 = p.gs[0]
        gx0 = g0.to(ctx.in_dtype, copy=True) if ctx.nhwc else g0.view(n, 8, 8, C).permute(0, 3, 1, 2).to(ctx.in_dtype, copy=True)
        return gx0, dW, db, None, None


class _RowsLinear(torch.autograd.Function):
    """y = x @ W.T + b for x [rows, K] with MANY rows (batch x 64 cells) and small K / N (the stem: K = 32, the head
    convolutions: N = 32).  The forward and d/dx are ordinary GEMMs; d/dW = dy.T @ x is a [N x rows] x [rows x K]
    product whose long axis is the reduction: the BLAS picks a kernel without a K split for it (measured 174-239 us for
    a 3 x 64 result), so it is done as a batched GEMM over 64 row chunks plus a sum (~10 us)."""

    @staticmethod
    def forward(ctx, x, W, b):
        # under autocast the product runs in bf16 (this Function is opaque to autocast, so it casts itself)
        dt = torch.bfloat16 if (x.is_cuda and torch.is_autocast_enabled()) else x.dtype
        xb, Wb = x.to(dt), W.to(dt)
        ctx.save_for_backward(xb, Wb)
        ctx.dts = (x.dtype, W.dtype, b.dtype)
        with torch.autocast("cuda", enabled=False):
            return torch.addmm(b.to(dt), xb, Wb.t())

    @staticmethod
    def backward(ctx, gy):
        x, W = ctx.saved_tensors
        gy = gy.to(x.dtype)
        gx = (gy @ W).to(ctx.dts[0]) if ctx.needs_input_grad[0] else None
        rows = x.shape[0]
        ch = 64 if rows % 64 == 0 else 1
        gyc = gy.view(ch, rows // ch, -1).transpose(1, 2)
        gW = torch.bmm(gyc, x.view(ch, rows // ch, -1)).sum(0, dtype=torch.float32)
        # the bias gradient the same way (x a column of ones) rather than as gy.sum(0): a 65,536-row column sum is a
        # multi-block torch reduction, and inside replayed HIP graphs such sums came back wrong once in a few hundred
        # steps on this stack (all zeros here; 6e32 in the stock channels-last path -- profiles/r04_channels_last_cause.txt)
        # (the cause, found in round 5: that reduction zeroes its semaphores with a captured cudaMemsetAsync, and captured memset
        # nodes do not reliably execute on replay on this stack -- profiles/r05_graph_memset_node.txt; GraphedTrainStep no
        # longer captures the autograd forms of the step unless asked to, train.py)
        gb = torch.bmm(gyc, gy.new_ones((ch, rows // ch, 1))).sum(0, dtype=torch.float32).squeeze(1)
        return gx, gW.to(ctx.dts[1]), gb.to(ctx.dts[2])


def check_own_weight(own_weight):
    """the ownership loss's weight: a finite number >= 0, anything else is refused (ValueError, before any
    device is touched)"""
    w = own_weight
    if isinstance(w, bool) or not isinstance(w, (int, float)) or not 0.0 <= w < float("inf"):   # (NaN fails)
        raise ValueError(f"own_weight must be a finite number >= 0 (got {w!r})")
    return float(w)


def check_fp8_qat(fp8_qat, module):
    """fp8 quantisation-aware training exists where the fp8 tower does: 128 channels; anything else is refused
    (ValueError, before any device is touched)"""
    if fp8_qat and getattr(module, "C", None) != 128:
        raise ValueError(f"fp8_qat: the fp8 tower is built for 128 channels (got {getattr(module, 'C', None)}); "
                         "quantisation-aware training is offered for that net only")
    return bool(fp8_qat)


class StepPlan(TowerPlan):
    """forward + losses + backward (+ Adam) of one training step of `module` (PolicyValueNet(fused_tower=True), on the
    device) at a fixed batch size, entirely on the HIP kernels:

        plan = StepPlan(module, batch)
        plan.set_batch(own, opp, pi, z, idx)     # the data set's tensors and the batch's row indices (idx None: rows 0..batch-1)
        losses = plan.grads()                    # [loss, policy CE, value MSE, error word] (device, static); every p.grad is set
        optimizer.step()                         # torch's -- or instead of the two lines above:
        plan.enable_adam(lr); losses = plan.step()    # + the Adam update as a tenth launch (torch.optim.Adam's arithmetic)

    own / opp: int64 tensors holding the uint64 bitboards [rows]; pi fp32 [rows, 65]; z int8 [rows]; idx int64 [batch].
    The kernels read the batch through a 48-byte descriptor in device memory (bz_train_batch) and gather the rows
    themselves: a captured step keeps working when set_batch() points it at new tensors -- nothing is copied.  The
    gradient tensors are allocated once and installed as the parameters' .grad (static addresses: the step can be
    captured into a HIP graph; do not call zero_grad(set_to_none=True) in between -- every launch overwrites them)."""

    NAMES = ("stem_w", "stem_b", "tower_w", "tower_b", "pol_w", "pol_b", "polfc_w", "polfc_b", "val_w", "val_b", "v1_w", "v1_b", "v2_w", "v2_b")

    @staticmethod
    def _named(module):
        return {"stem_w": module.stem.weight, "stem_b": module.stem.bias, "tower_w": module.tower_w, "tower_b": module.tower_b,
                "pol_w": module.pol.weight, "pol_b": module.pol.bias, "polfc_w": module.polfc.weight, "polfc_b": module.polfc.bias,
                "val_w": module.val.weight, "val_b": module.val.bias, "v1_w": module.v1.weight, "v1_b": module.v1.bias,
                "v2_w": module.v2.weight, "v2_b": module.v2.bias}

    def __init__(self, module, batch, device="cuda:0", value_targets=False, ownership=None, own_weight=1.0, fp8_qat=False,
                 symmetry=False, size=8):
        """symmetry: batch position p trains on row idx[p] under the board symmetry sym[p] (set_batch(..., sym=),
        uint8 0..7, symmetry.SYM_NAMES) of the size x size board -- one launch more, k_train_sym_batch, in front of the stem: it
        gathers and transforms the batch's rows into a staging batch this plan owns (train_symmetry.SymStaging), and the step's own
        descriptor, its vt slot and its ownership slot point at the staged columns for good.  Every other kernel runs as it is, so the
        option composes with all of the below; off (the default), the step is launch for launch the one it was.

        fp8_qat: quantisation-aware training for the fp8 net -- the step's forward is bz_net_forward_fp8's
        arithmetic (k_qat_stem, k_qat_scales, k_qat_pack, k_qat_fwd in place of the stem, the weight packing and the tower
        forward: one launch more), the backward the straight-through estimator: the gradients with respect to the quantised
        weights land in the fp32 masters' .grad.  128 channels only (the fp8 tower's); composes with every option below.

        value_targets: the head kernel reads a float value target per row (set_batch(..., vt=...)) in place
        of z, through k_train_heads_vt; everything else of the step is the same.

        ownership: an OwnershipHead(C) -- the head kernel becomes k_train_heads_own (or its _vt form), which
        also computes the head on act[L], its loss L_own against the rows' ownership targets (set_batch(..., fown=, fopp=)) and
        its gradients; the step's loss is CE + MSE + own_weight * L_own, and one more small launch (k_train_own_finish) ends the
        step: the head's .grad, own_loss[0] = L_own and, with enable_adam(), plain Adam on the head's own C + 1 parameters."""
        own_weight = check_own_weight(own_weight)
        if ownership is not None:
            from .net import OwnershipHead
            if not isinstance(ownership, OwnershipHead) or ownership.C != getattr(module, "C", None):
                raise ValueError("StepPlan: ownership must be an OwnershipHead of the module's channel count")
        if not getattr(module, "fused_tower", False):
            raise ValueError("StepPlan needs PolicyValueNet(..., fused_tower=True)")
        if module.VH > 64:
            raise ValueError("the head kernels hold the value head's hidden layer in one wavefront: value_hidden <= 64")
        check_fp8_qat(fp8_qat, module)
        self.symmetry = bool(symmetry)
        if self.symmetry:
            from .train_symmetry import check_size
            size = check_size(size)
        super().__init__(module.C, 2 * module.NB, batch, device)
        L, dev = _lib.lib(), self.device
        self.module, self.VH = module, module.VH
        named = self._named(module)
        for k, p in named.items():
            if p.device != dev or p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError(f"StepPlan: parameter {k} must be a contiguous fp32 tensor on {dev}")
            p.grad = torch.zeros_like(p)
        self.params = named
        sizes = (ct.c_int32 * 6)()
        _lib.check(L.bz_train_ends_sizes(self.C, batch, sizes))
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
        self.stem_partial, self.heads_partial, self.heads_w_partial = f32(sizes[0], sizes[1]), f32(sizes[2], sizes[3]), f32(sizes[4], sizes[5])
        self.hv, self.dl, self.dv1 = f32(batch, 192), f32(batch, 65), f32(batch, 64)
        self.losses = f32(4)   # loss, CE, MSE and the error word: batch positions whose row index was out of range, summed over steps
        self._head = _lib.TrainHeadParams(**{k: named[k].data_ptr() for k, _ in _lib.TrainHeadParams._fields_})
        # fp8_qat: the per-output-channel scales (tower, then the 3 head rows) and the fake-quantised shadow of the head conv1x1
        # rows, which the head kernels read in place of the masters (their gradients still go to the masters' .grad)
        self.fp8_qat = bool(fp8_qat)
        if self.fp8_qat:
            self.qat_scales, self.qat_head = f32(self.L * self.C + 3), f32(3, self.C)
            self._head.pol_w, self._head.val_w = self.qat_head.data_ptr(), self.qat_head[2].data_ptr()
        self._grads = _lib.TrainTensors(**{k: named[k].grad.data_ptr() for k in self.NAMES})
        self._partials = _lib.TrainPartials(tower=self.partial.data_ptr(), tower_b=self.db_partial.data_ptr(), stem=self.stem_partial.data_ptr(),
                                            heads=self.heads_partial.data_ptr(), heads_w=self.heads_w_partial.data_ptr(), splits=self.splits)
        self.batch_desc = torch.zeros(ct.sizeof(_lib.TrainBatch), dtype=torch.uint8, device=dev)
        self._batch_refs = None
        # the address of the data set's fp32 value targets: one device word, rewritten by set_batch like the descriptor
        self.value_targets = bool(value_targets)
        self.vt_slot = torch.zeros(1, dtype=torch.int64, device=dev)
        self._vt_ref = None
        self._adam, self.adam_m, self.adam_v, self.hyper = None, None, None, None
        # the ownership head: its parameters (outside `params`: no bz_train_tensors has them), its partial sums, the device slot
        # with the addresses of the data set's two target arrays, and L_own
        self.ownership, self.own_weight = ownership, own_weight
        self._own, self._own_adam, self._own_ref = None, None, None
        if ownership is not None:
            self.own_params = {"w": ownership.conv.weight, "b": ownership.conv.bias}
            for k, t in self.own_params.items():
                if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
                    raise ValueError(f"StepPlan: the ownership head's parameter {k} must be a contiguous fp32 tensor on {dev}")
                t.grad = torch.zeros_like(t)
            self.own_partial, self.own_loss = f32(sizes[2], self.C + 2), f32(1)
            self.own_slot = torch.zeros(2, dtype=torch.int64, device=dev)
            self._own = _lib.TrainOwn(w=self.own_params["w"].data_ptr(), b=self.own_params["b"].data_ptr(), targets=self.own_slot.data_ptr(),
                                      weight=own_weight, partial=self.own_partial.data_ptr())
        self._optim, self.ema, self.stats, self.optim_partials = None, None, None, None   # the extended optimiser (enable_adam)
        # symmetry: the staging batch, and the step's descriptor and slots pointed at it once (rows 0..batch-1 of the staged rows)
        self.sym_stage = None
        if self.symmetry:
            from .train_symmetry import SymStaging
            g = self.sym_stage = SymStaging(batch, size, dev, vt=self.value_targets, ownership=ownership is not None)
            d = _lib.TrainBatch(own=g.own.data_ptr(), opp=g.opp.data_ptr(), pi=g.pi.data_ptr(), z=g.z.data_ptr(), idx=None, n_rows=batch)
            with torch.cuda.device(dev):
                self.batch_desc.copy_(torch.frombuffer(bytearray(bytes(d)), dtype=torch.uint8))
                if self.value_targets:
                    self.vt_slot.copy_(torch.tensor([g.vt.data_ptr()], dtype=torch.int64))
                if ownership is not None:
                    self.own_slot.copy_(torch.tensor([g.fown.data_ptr(), g.fopp.data_ptr()], dtype=torch.int64))

    # ---- the batch
    def set_batch(self, own, opp, pi, z, idx=None, vt=None, fown=None, fopp=None, sym=None):
        """point the step at rows `idx` (int64 [batch], on the device; None: rows 0..batch-1) of the data set (own, opp, pi,
        z).  Asynchronous on the current stream; the tensors are kept alive until the next call.  vt: the data set's value
        targets, fp32 [rows] (a plan built with value_targets=True needs them; they are gathered by the same idx).  fown /
        fopp: the data set's ownership targets, int64 [rows] (a plan built with ownership= needs them; gathered by idx too).
        sym: the batch positions' board symmetries, uint8 [batch] on the device (a plan built with symmetry=True needs them)."""
        n, dev = self.n, self.device
        rows = int(own.shape[0])
        if rows < 1:
            raise ValueError("set_batch: the data set is empty")
        ok = (own.dtype == torch.int64 and opp.dtype == torch.int64 and own.shape == (rows,) and opp.shape == (rows,) and
              pi.dtype == torch.float32 and pi.shape == (rows, 65) and z.dtype == torch.int8 and z.shape == (rows,) and
              all(t.is_contiguous() and t.device == dev for t in (own, opp, pi, z)))
        if not ok:
            raise ValueError("set_batch: own / opp int64 [rows], pi fp32 [rows, 65], z int8 [rows], contiguous, on the plan's device")
        if self.value_targets:
            if vt is None or not (vt.dtype == torch.float32 and vt.shape == (rows,) and vt.is_contiguous() and vt.device == dev):
                raise ValueError("set_batch: a plan with value_targets=True needs vt fp32 [rows], contiguous, on the plan's device")
        elif vt is not None:
            raise ValueError("set_batch: vt given, but the plan was built without value_targets=True")
        if self._own is not None:
            if fown is None or fopp is None or not all(t.dtype == torch.int64 and t.shape == (rows,) and t.is_contiguous() and t.device == dev
                                                       for t in (fown, fopp)):
                raise ValueError("set_batch: a plan with ownership= needs fown / fopp int64 [rows], contiguous, on the plan's device")
        elif fown is not None or fopp is not None:
            raise ValueError("set_batch: fown / fopp given, but the plan was built without ownership=")
        if idx is None:
            if rows < n:
                raise ValueError(f"set_batch: the data set has {rows} rows, the batch needs {n}")
        elif not (idx.dtype == torch.int64 and idx.shape == (n,) and idx.is_contiguous() and idx.device == dev):
            raise ValueError(f"set_batch: idx must be a contiguous int64 tensor of {n} row numbers on the plan's device")
        if self.symmetry:   # the staging kernel reads the data set; the step's own descriptor and slots stay on the staged rows
            from .train_symmetry import check_sym
            self.sym_stage.set_source(own, opp, pi, z, idx, check_sym(sym, n, dev), vt=vt, fown=fown, fopp=fopp)
            self._batch_refs, self._vt_ref, self._own_ref = ("staged",), vt, ((fown, fopp) if self._own is not None else None)
            return
        if sym is not None:
            raise ValueError("set_batch: sym given, but the plan was built without symmetry=True")
        d = _lib.TrainBatch(own=own.data_ptr(), opp=opp.data_ptr(), pi=pi.data_ptr(), z=z.data_ptr(),
                            idx=idx.data_ptr() if idx is not None else None, n_rows=rows)
        key = bytes(d)
        if self._batch_refs is None or self._batch_refs[0] != key:   # (a pageable host copy: ordered on the current stream, done on return)
            with torch.cuda.device(dev):
                self.batch_desc.copy_(torch.frombuffer(bytearray(key), dtype=torch.uint8))
        self._batch_refs = (key, own, opp, pi, z, idx)
        if self.value_targets:
            if self._vt_ref is None or self._vt_ref.data_ptr() != vt.data_ptr():
                with torch.cuda.device(dev):
                    self.vt_slot.copy_(torch.tensor([vt.data_ptr()], dtype=torch.int64))
            self._vt_ref = vt
        if self._own is not None:
            if self._own_ref is None or (self._own_ref[0].data_ptr(), self._own_ref[1].data_ptr()) != (fown.data_ptr(), fopp.data_ptr()):
                with torch.cuda.device(dev):
                    self.own_slot.copy_(torch.tensor([fown.data_ptr(), fopp.data_ptr()], dtype=torch.int64))
            self._own_ref = (fown, fopp)

    # ---- the optimiser as the step's tenth launch
    def enable_adam(self, lr, betas=(0.9, 0.999), eps=1e-8, warmup_steps=0, weight_decay=0.0, clip_norm=0.0, ema_decay=None,
                    decay_biases=False, extended=None):
        """Adam (torch.optim.Adam's arithmetic, no weight decay / amsgrad: what the reference constructs, train.py:87) applied
        by k_train_adam right behind k_train_finish (one coalesced pass over all 14 tensors).  State: adam_m / adam_v (dicts of tensors like the parameters) and
        the device block `hyper` = {lr, steps done, warm-up steps, 0}: the kernel advances the step count itself and ramps
        the rate over the first warmup_steps steps (lr * min(1, t / warmup_steps)), so consecutive steps need no host write.

        weight_decay / clip_norm / ema_decay / decay_biases, or extended=True, select the extended optimiser instead
        (bz_train_optim_step, bz_abi.h: AdamW's decoupled decay -- of the weights, and of the biases only with decay_biases --, a
        clip of the global gradient norm at clip_norm, a step with a non-finite norm skipped as a whole, and with ema_decay an
        averaged copy of the parameters in `ema`): two launches behind k_train_finish, eleven in all.  `hyper` is then the
        32-byte block {lr, steps attempted, warm-up, weight decay, max norm, EMA decay, 0, 0}, `stats` the kernels' 16 bytes
        (optim_stats()).  With every option off the extended step leaves the bits of the plain one."""
        if extended is None:
            extended = bool(weight_decay) or bool(clip_norm) or ema_decay is not None or bool(decay_biases)
        elif not extended and (weight_decay or clip_norm or ema_decay is not None or decay_biases):
            raise ValueError("enable_adam: weight_decay / clip_norm / ema_decay / decay_biases need the extended optimiser")
        self.adam_m = {k: torch.zeros_like(p) for k, p in self.params.items()}
        self.adam_v = {k: torch.zeros_like(p) for k, p in self.params.items()}
        T = _lib.TrainTensors
        tensors = lambda d: T(**{k: d[k].data_ptr() for k in self.NAMES})  # noqa: E731
        self._adam, self._optim, self.ema, self.stats, self.optim_partials = None, None, None, None, None
        if not extended:
            self.hyper = torch.zeros(4, dtype=torch.float32, device=self.device)
            self._adam = _lib.TrainAdam(hyper=self.hyper.data_ptr(), beta1=betas[0], beta2=betas[1], eps=eps,
                                        p=tensors(self.params), m=tensors(self.adam_m), v=tensors(self.adam_v))
        else:
            self.weight_decay, self.clip_norm = float(weight_decay), float(clip_norm)
            self.ema_decay = 0.0 if ema_decay is None else float(ema_decay)
            self.lr, self.warmup = float(lr), int(warmup_steps)
            self._hyper_block()   # (refuses a bad value before anything is allocated)
            self.hyper = torch.zeros(8, dtype=torch.float32, device=self.device)
            self.stats = torch.zeros(4, dtype=torch.float32, device=self.device)
            self.optim_partials = torch.zeros(_lib.lib().bz_train_optim_partials(), dtype=torch.float32, device=self.device)
            if ema_decay is not None:
                self.ema = {k: p.detach().clone() for k, p in self.params.items()}
                self._ema_set = tensors(self.ema)
            self._optim = _lib.TrainOptim(hyper=self.hyper.data_ptr(), stats=self.stats.data_ptr(), partials=self.optim_partials.data_ptr(),
                                          beta1=betas[0], beta2=betas[1], eps=eps, decay_biases=int(bool(decay_biases)),
                                          p=tensors(self.params), m=tensors(self.adam_m), v=tensors(self.adam_v),
                                          ema=ct.pointer(self._ema_set) if self.ema is not None else None)
        if self._own is not None:   # the head's own Adam state; it reads the rate, the step count and the warm-up of `hyper`
            self.own_m = {k: torch.zeros_like(t) for k, t in self.own_params.items()}
            self.own_v = {k: torch.zeros_like(t) for k, t in self.own_params.items()}
            self._own_adam = _lib.TrainOwnAdam(hyper=self.hyper.data_ptr(), beta1=betas[0], beta2=betas[1], eps=eps,
                                               pw=self.own_params["w"].data_ptr(), pb=self.own_params["b"].data_ptr(),
                                               mw=self.own_m["w"].data_ptr(), mb=self.own_m["b"].data_ptr(),
                                               vw=self.own_v["w"].data_ptr(), vb=self.own_v["b"].data_ptr())
        self.reset_adam(lr, warmup_steps)

    def _hyper_block(self, steps_done=0):
        """the extended optimiser's hyper block as a host tensor, laid out and checked by the library"""
        blk = (ct.c_float * 8)()
        _lib.check(_lib.lib().bz_train_optim_hyper(self.lr, float(steps_done), float(self.warmup), self.weight_decay, self.clip_norm,
                                                   self.ema_decay, blk))
        return torch.tensor(list(blk), dtype=torch.float32)

    def reset_adam(self, lr=None, warmup_steps=None, steps_done=0):
        """zero moments, step count `steps_done`, (new) rate / warm-up; the extended optimiser's EMA becomes a copy of the
        parameters again and its statistics are zeroed"""
        if lr is not None:
            self.lr = float(lr)
        if warmup_steps is not None:
            self.warmup = int(warmup_steps)
        for d in (self.adam_m, self.adam_v) + ((self.own_m, self.own_v) if self._own_adam is not None else ()):
            for t in d.values():
                t.zero_()
        with torch.cuda.device(self.device):
            if self._optim is None:
                self.hyper.copy_(torch.tensor([self.lr, float(steps_done), float(self.warmup), 0.0], dtype=torch.float32))
                return
            self.hyper.copy_(self._hyper_block(steps_done))
            self.stats.zero_()
            if self.ema is not None:
                for k, t in self.ema.items():
                    t.copy_(self.params[k].detach())

    def set_lr(self, lr):
        """change the (peak) learning rate; moments and step count stay"""
        self.lr = float(lr)
        with torch.cuda.device(self.device):
            self.hyper[0:1].copy_(torch.tensor([self.lr], dtype=torch.float32))

    def optim_step(self):
        """the extended optimiser's two launches alone (k_train_gnorm, k_train_optim) on whatever the .grad tensors hold"""
        if self._optim is None:
            raise RuntimeError("StepPlan: enable_adam(..., extended=True) (or one of its options) first")
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().bz_train_optim_step(ct.byref(self._grads), ct.byref(self._optim), self.C, self.L, self.VH, self._stream()))

    def optim_stats(self, reset=True):
        """{grad_norm, scale, skipped, clipped} of the extended optimiser: the last step's gradient norm before the clip and the
        scale it applied (0.0: the step was skipped), and how many steps since the last reset were skipped (non-finite norm)
        / clipped.  One read of the device (synchronises); call it where the losses are looked at."""
        if self._optim is None:
            raise RuntimeError("StepPlan: enable_adam(..., extended=True) (or one of its options) first")
        norm, scale, skipped, clipped = self.stats.tolist()
        if reset and (skipped or clipped):
            self.stats[2:4].zero_()
        return {"grad_norm": norm, "scale": scale, "skipped": int(skipped), "clipped": int(clipped)}

    def ema_module(self):
        """a deep copy of the module holding the averaged weights (enable_adam(..., ema_decay=...))"""
        import copy
        if self.ema is None:
            raise RuntimeError("StepPlan: enable_adam(..., ema_decay=...) first")
        m = copy.deepcopy(self.module)
        with torch.no_grad():
            for k, p in self._named(m).items():
                p.copy_(self.ema[k])
                p.grad = None
        return m

    @property
    def adam_t(self):
        """steps done so far (reads the device counter: synchronises)"""
        return int(self.hyper[1].item()) if self.hyper is not None else 0

    # ---- the step's state, to carry a run across processes
    def _describe(self):
        """what a saved state must agree on with the step it is loaded into, in the order a mismatch is reported"""
        return {"C": self.C, "blocks": self.L // 2, "VH": self.VH, "extended": self._optim is not None, "has_ema": self.ema is not None,
                "has_ownership": self._own is not None, "fp8_qat": self.fp8_qat}

    def _state_tensors(self):
        """{key: device tensor} of everything a step reads and writes from one replay to the next"""
        if self.adam_m is None:
            raise RuntimeError("StepPlan: enable_adam() first (the state is the optimiser's as much as the net's)")
        t = {f"param.{k}": self.params[k].detach() for k in self.NAMES}
        t.update({f"adam_m.{k}": self.adam_m[k] for k in self.NAMES})
        t.update({f"adam_v.{k}": self.adam_v[k] for k in self.NAMES})
        t["hyper"] = self.hyper
        if self.stats is not None:
            t["stats"] = self.stats
        if self.ema is not None:
            t.update({f"ema.{k}": self.ema[k] for k in self.NAMES})
        if self._own is not None:
            for k in ("w", "b"):
                t[f"own.{k}"], t[f"own_m.{k}"], t[f"own_v.{k}"] = self.own_params[k].detach(), self.own_m[k], self.own_v[k]
        return t

    def state_dict(self):
        """a flat dict of CPU tensors and plain numbers, enough to continue bit for bit: the fp32 parameters ("param." + NAMES),
        adam_m / adam_v, the whole hyper block as stored (the device step counter included), stats, ema and the ownership head's
        w, b and moments where they exist, the host-side lr and warm-up -- and C, blocks, VH, batch and which optional parts
        exist, for load_state_dict's check.  Synchronises."""
        sd = {k: t.cpu().clone() for k, t in self._state_tensors().items()}
        sd.update(self._describe())
        sd.update(batch=self.n, value_targets=self.value_targets, lr=self.lr, warmup=self.warmup)
        if self._optim is not None:
            sd.update(weight_decay=self.weight_decay, clip_norm=self.clip_norm, ema_decay=self.ema_decay)
        return sd

    def _check_state(self, sd):
        """ValueError naming the first difference between `sd` and this step; nothing is written"""
        for k, mine in self._describe().items():
            if k not in sd:
                raise ValueError(f"load_state_dict: the state has no {k!r}: not a StepPlan state")
            if sd[k] != mine:
                raise ValueError(f"load_state_dict: {k} differs: the state was saved with {k} = {sd[k]!r}, this step has {mine!r}")
        for k, t in self._state_tensors().items():
            s = sd.get(k)
            if not torch.is_tensor(s) or s.shape != t.shape or s.dtype != t.dtype:
                got = f"{s.dtype} {tuple(s.shape)}" if torch.is_tensor(s) else repr(type(s).__name__)
                raise ValueError(f"load_state_dict: tensor {k} differs: the state has {got}, this step {t.dtype} {tuple(t.shape)}")
        for k in ("lr", "warmup"):
            if not isinstance(sd.get(k), (int, float)) or isinstance(sd.get(k), bool):
                raise ValueError(f"load_state_dict: the state's {k} is not a number")

    def load_state_dict(self, sd):
        """copy a state_dict() into the step's own tensors, in place and on the current stream: the addresses a captured graph
        holds stay valid, so the next launch (or replay) continues from the loaded state.  C / blocks / VH, plain against
        extended optimiser, an EMA or an ownership head on one side only, or fp8_qat differing raise ValueError naming the first
        difference BEFORE anything is written.  (batch and value_targets shape no state and may differ.)"""
        self._check_state(sd)
        with torch.cuda.device(self.device), torch.no_grad():
            for k, t in self._state_tensors().items():
                t.copy_(sd[k])
        self.lr, self.warmup = float(sd["lr"]), int(sd["warmup"])
        if self._optim is not None and "weight_decay" in sd:
            self.weight_decay, self.clip_norm, self.ema_decay = float(sd["weight_decay"]), float(sd["clip_norm"]), float(sd["ema_decay"])

    # ---- the launches
    def launch(self, adam=False):
        """the 9 (adam: 10, or 11 with the extended optimiser) launches of one step on the current stream (no host work besides:
        this is what a HIP graph captures); with the ownership head one more, k_train_own_finish, at the end; with fp8_qat one
        more, k_qat_scales, in front of the weight packing; with symmetry one more, k_train_sym_batch, in front of everything"""
        L, p, n, Cc, Ly = _lib.lib(), self.params, self.n, self.C, self.L
        if self._batch_refs is None:
            raise RuntimeError("StepPlan: set_batch() first")
        if adam and self._adam is None and self._optim is None:
            raise RuntimeError("StepPlan: enable_adam() first")
        for k, t in p.items():   # (an optimiser that swapped a gradient tensor out would leave the kernels writing into a dead one)
            assert t.grad is not None and t.grad.data_ptr() == getattr(self._grads, k), f"the .grad of {k} was replaced"
        with torch.cuda.device(self.device):
            st, bd = self._stream(), self.batch_desc.data_ptr()
            chk = _lib.check
            if self.symmetry:
                self.sym_stage.launch()
            if self.fp8_qat:
                chk(L.bz_train_qat_stem_fwd(bd, n, p["stem_w"].data_ptr(), p["stem_b"].data_ptr(), Cc, self.acts[0].data_ptr(), st))
                chk(L.bz_train_qat_scales(p["tower_w"].data_ptr(), p["pol_w"].data_ptr(), p["val_w"].data_ptr(), Cc, Ly,
                                          self.qat_scales.data_ptr(), self.qat_head.data_ptr(), st))
                chk(L.bz_train_qat_pack_weights(p["tower_w"].data_ptr(), self.qat_scales.data_ptr(), Cc, Ly, self.wf_fwd.data_ptr(),
                                                self.wf_bwd.data_ptr(), st))
                chk(L.bz_train_qat_tower_fwd(self.acts[0].data_ptr(), self.wf_fwd.data_ptr(), p["tower_b"].data_ptr(), Cc, Ly, n,
                                             self.acts[1].data_ptr(), self.masks.data_ptr(), st))
            else:
                chk(L.bz_train_stem_fwd(bd, n, p["stem_w"].data_ptr(), p["stem_b"].data_ptr(), Cc, self.acts[0].data_ptr(), st))
                chk(L.bz_train_pack_weights(p["tower_w"].data_ptr(), Cc, Ly, self.wf_fwd.data_ptr(), self.wf_bwd.data_ptr(), st))
                chk(L.bz_train_tower_fwd(self.acts[0].data_ptr(), self.wf_fwd.data_ptr(), p["tower_b"].data_ptr(), Cc, Ly, n,
                                         self.acts[1].data_ptr(), self.masks.data_ptr(), st))
            if self._own is not None and self._own_ref is None:
                raise RuntimeError("StepPlan: set_batch(..., fown=..., fopp=...) first")
            if self.value_targets and self._vt_ref is None:
                raise RuntimeError("StepPlan: set_batch(..., vt=...) first")
            if self._own is not None:
                for k, t in self.own_params.items():
                    assert t.grad is not None, f"the .grad of the ownership head's {k} was replaced"
                if self.value_targets:
                    chk(L.bz_train_heads_own_vt(self.acts[Ly].data_ptr(), bd, self.vt_slot.data_ptr(), ct.byref(self._own), n, Cc, self.VH,
                                                ct.byref(self._head), self.gs[Ly].data_ptr(), self.hv.data_ptr(), self.dl.data_ptr(),
                                                self.dv1.data_ptr(), self.heads_partial.data_ptr(), st))
                else:
                    chk(L.bz_train_heads_own(self.acts[Ly].data_ptr(), bd, ct.byref(self._own), n, Cc, self.VH, ct.byref(self._head),
                                             self.gs[Ly].data_ptr(), self.hv.data_ptr(), self.dl.data_ptr(), self.dv1.data_ptr(),
                                             self.heads_partial.data_ptr(), st))
            elif self.value_targets:
                chk(L.bz_train_heads_vt(self.acts[Ly].data_ptr(), bd, self.vt_slot.data_ptr(), n, Cc, self.VH, ct.byref(self._head),
                                        self.gs[Ly].data_ptr(), self.hv.data_ptr(), self.dl.data_ptr(), self.dv1.data_ptr(),
                                        self.heads_partial.data_ptr(), st))
            else:
                chk(L.bz_train_heads(self.acts[Ly].data_ptr(), bd, n, Cc, self.VH, ct.byref(self._head), self.gs[Ly].data_ptr(),
                                     self.hv.data_ptr(), self.dl.data_ptr(), self.dv1.data_ptr(), self.heads_partial.data_ptr(), st))
            chk(L.bz_train_tower_bwd(self.gs[Ly].data_ptr(), self.wf_bwd.data_ptr(), self.zeros_c.data_ptr(), self.masks.data_ptr(), Cc, Ly, n,
                                     self.gs[0].data_ptr(), st))
            chk(L.bz_train_wgrad(self.acts[0].data_ptr(), self.gs[1].data_ptr(), Cc, Ly, n, self.splits, self.partial.data_ptr(),
                                 self.db_partial.data_ptr(), st))
            chk(L.bz_train_stem_wgrad(bd, self.acts[0].data_ptr(), self.gs[0].data_ptr(), n, Cc, self.stem_partial.data_ptr(), st))
            chk(L.bz_train_heads_wgrad(self.hv.data_ptr(), self.dl.data_ptr(), self.dv1.data_ptr(), n, self.VH, self.heads_w_partial.data_ptr(), st))
            chk(L.bz_train_finish(ct.byref(self._partials), ct.byref(self._grads), Cc, Ly, self.VH, n, self.losses.data_ptr(),
                                  ct.byref(self._adam) if adam and self._optim is None else None, st))
        if adam and self._optim is not None:
            self.optim_step()
        if self._own is not None:   # behind the launch that advanced the step counter
            with torch.cuda.device(self.device):
                w, b = self.own_params["w"], self.own_params["b"]
                _lib.check(L.bz_train_own_finish(ct.byref(self._own), Cc, n, w.grad.data_ptr(), b.grad.data_ptr(), self.own_loss.data_ptr(),
                                                 self.losses.data_ptr(), ct.byref(self._own_adam) if adam else None, self._stream()))
        return self.losses

    def bad_rows(self, reset=True):
        """the step's error word (bz_abi.h, bz_train_finish): how many batch positions since the last reset had a row index
        outside the data set -- the kernels clamped them, i.e. trained on row 0 / the last row instead.  With symmetry=True the
        staged step sees no index any more: the staging kernel's own count (an index outside the data set, or a symmetry outside
        0..7, which it takes & 7) is added here and reset along.  Reads the device (synchronises); call it where the losses are
        looked at."""
        n = int(self.losses[3].item())
        if n and reset:
            self.losses[3:4].zero_()
        if self.symmetry:
            n += self.sym_stage.bad_rows(reset=reset)
        return n

    def check_rows(self):
        """raise IndexError if any step since the last check gathered a row outside the data set (what torch.index_select,
        the loop shape of SL/train.py:102-108, would have raised at once)"""
        n = self.bad_rows()
        if n:
            raise IndexError(f"StepPlan: {n} batch position(s) had a row index outside the data set"
                             f"{' or a symmetry outside 0..7' if self.symmetry else ''} since the last check; "
                             "the kernels clamp instead of faulting, so those steps trained on the wrong rows")

    def grads(self, own=None, opp=None, pi=None, z=None, idx=None, vt=None, fown=None, fopp=None, sym=None):
        """forward, losses, backward: every parameter's .grad is set; returns the static [loss, CE, MSE, error word] tensor.
        (own, opp, pi, z[, idx][, vt][, fown, fopp]) given: set_batch() first.  With the ownership head the loss includes
        own_weight * L_own, and own_loss[0] is L_own."""
        if own is not None:
            self.set_batch(own, opp, pi, z, idx, vt=vt, fown=fown, fopp=fopp, sym=sym)
        return self.launch(adam=False)

    def step(self):
        """grads() and the Adam update: 10 launches, 11 with the extended optimiser (enable_adam() first)"""
        return self.launch(adam=True)


def rows_linear(x, W, b):
    return _RowsLinear.apply(x, W, b)


def tower_apply(x0, W, b, plan):
    """x0 [n, C, 8, 8] (the stem's output after its ReLU) -> the tower's output [n, C, 8, 8]; differentiable in x0, W, b"""
    return _TowerFn.apply(x0, W, b, plan, False)


def tower_apply_nhwc(x0, W, b, plan):
    """the same on [n, 64 cells, C] tensors -- the kernels' own layout (what PolicyValueNet's fused path passes)"""
    return _TowerFn.apply(x0, W, b, plan, True)
