"""Closing the AlphaZero loop: one optimisation step on (s, pi, z)
with stock PyTorch-ROCm autograd.  Loop shape after src/tic_tac_toe/SL/train.py:85-136
(cross-entropy on the policy, Adam lr 1e-4), plus the value MSE the reference lacks.

The data path is device-resident: DeviceExamples in (from gather_examples_device / augment_examples), batches are
index-selected on the GPU, the two input planes are expanded from the bitboards by torch ops on the GPU, forward and
backward run under bf16 autocast (fp32 master weights, fp32 losses).  Nothing is copied to the host; the three loss
values come back as device scalars (call .item() when you want to look at them, not every step)."""
import torch
import torch.nn.functional as F

from .examples import DeviceExamples, Examples, take

_SHIFTS = {}


def planes_from_bits(own, opp):
    """int64 tensors holding uint64 bitboards [n] -> float planes [n, 2, 8, 8] (bit 8*r+c), on their device.
    (>> on int64 is arithmetic, which still leaves bit s of the pattern at bit 0 for every s <= 63.)"""
    dev = own.device
    sh = _SHIFTS.get(dev)
    if sh is None:
        sh = _SHIFTS[dev] = torch.arange(64, dtype=torch.int64, device=dev)
    a = ((own[:, None] >> sh) & 1).to(torch.float32).view(-1, 8, 8)
    b = ((opp[:, None] >> sh) & 1).to(torch.float32).view(-1, 8, 8)
    return torch.stack([a, b], dim=1)


def make_optimizer(module, lr=1e-4):
    return torch.optim.Adam(module.parameters(), lr=lr)  # train.py:87,192


def ownership_targets(fown, fopp):
    """int64 tensors holding the uint64 target boards [n] -> the cells' targets, float [n, 64] in {+1, 0, -1}:
    bit_i(fown) - bit_i(fopp)"""
    dev = fown.device
    sh = _SHIFTS.get(dev)
    if sh is None:
        sh = _SHIFTS[dev] = torch.arange(64, dtype=torch.int64, device=dev)
    return (((fown[:, None] >> sh) & 1) - ((fopp[:, None] >> sh) & 1)).to(torch.float32)


def train_step(module, optimizer, ex, idx=None, device="cuda:0", autocast=True, value_targets=False, ownership=None, own_weight=1.0,
               fp8_qat=False, sym=None):
    """one Adam step on the rows `idx` of ex (Reversi 8x8 net).  ex: DeviceExamples (stays on the GPU; idx a device
    index tensor or None = all rows) or host Examples (uploaded first).  Returns (loss, policy CE, value MSE) as
    detached device scalars.  value_targets: the value MSE is against ex.vt (fp32) instead of z.
    ownership: an OwnershipHead on the trunk's output, trained on ex.fown / ex.fopp -- the loss gains
    own_weight * L_own, L_own = the mean over positions and all 64 cells of (o - t)^2, and a fourth value, L_own, is returned.
    The optimizer must then hold the head's parameters too.
    fp8_qat: the forward is quant.qat_forward -- the fp8 net's arithmetic in fp32 torch, straight-through
    gradients -- instead of the module's under autocast (128 channels only).
    sym: a uint8 tensor of board symmetries 0..7, one per trained row -- row p is trained under sym[p]: boards,
    pi and the ownership targets go through train_symmetry.torch_sym_rows (symmetry.sym_action_map's cell permutation, the one
    symmetry.sym_board moves the stones by) in front of the code below; what StepPlan(symmetry=True) does in its staging kernel."""
    from .train_kernels import check_fp8_qat, check_own_weight
    own_weight = check_own_weight(own_weight)
    check_fp8_qat(fp8_qat, module)
    if sym is not None:
        from .train_symmetry import check_size
        check_size(ex.size)
    if isinstance(ex, Examples):
        ex = DeviceExamples.from_host(ex, device)
    if value_targets and ex.vt is None:
        raise ValueError("train_step: value_targets=True needs examples with vt (betazero_amd.value_targets.value_targets)")
    if ownership is not None and (ex.fown is None or ex.fopp is None):
        raise ValueError("train_step: ownership= needs examples with fown / fopp (self-play with ownership=True records them)")
    dev = ex.own.device
    if next(module.parameters()).device != dev:
        module.to(dev)
    module.train()
    if idx is None:
        own, opp, pi, z = ex.own, ex.opp, ex.pi, ex.vt if value_targets else ex.z
    else:
        idx = torch.as_tensor(idx, device=dev)
        own, opp, pi, z = ex.own[idx], ex.opp[idx], ex.pi[idx], (ex.vt if value_targets else ex.z)[idx]
    fown, fopp = (None, None) if ownership is None else (ex.fown, ex.fopp) if idx is None else (ex.fown[idx], ex.fopp[idx])
    if sym is not None:
        from .train_symmetry import check_sym, torch_sym_rows
        own, opp, pi, fown, fopp = torch_sym_rows(own, opp, pi, check_sym(sym, int(own.shape[0]), dev), ex.size, fown, fopp)
    if fp8_qat:
        from .quant import qat_forward
        logits, v, saved = qat_forward(module, own, opp, acts=True)
        if ownership is not None:
            o = ownership.to(dev)(saved[-1])
    else:
        x = planes_from_bits(own, opp)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            if ownership is None:
                logits, v = module(x)
            else:
                logits, v, trunk = module(x, trunk=True)
                o = ownership.to(dev)(trunk)
    logits, v = logits.float(), v.float()
    ce = -(pi * F.log_softmax(logits, dim=1)).sum(1).mean()
    mse = F.mse_loss(v, z.to(torch.float32))
    loss = ce + mse
    if ownership is not None:
        t = ownership_targets(fown, fopp)
        l_own = F.mse_loss(o.float(), t)
        loss = loss + own_weight * l_own
    optimizer.zero_grad(set_to_none=True)
    loss.backward()
    optimizer.step()
    if ownership is not None:
        return loss.detach(), ce.detach(), mse.detach(), l_own.detach()
    return loss.detach(), ce.detach(), mse.detach()


def holdout_split(n_rows, val_fraction=0.2, generator=None, device="cuda:0"):
    """the reference's train / validation split (SL/train.py:66-76: val_size = int(total_size * validation_split), a
    random split of the ROWS) as two device index tensors (train_idx, val_idx) into a data set of n_rows rows"""
    perm = torch.randperm(int(n_rows), generator=generator, device=device)
    n_val = int(int(n_rows) * val_fraction)
    return perm[n_val:], perm[:n_val]


def select_rows(ex, idx):
    """DeviceExamples holding the rows `idx` (a device index tensor) of ex: every column ex carries"""
    return take(ex, idx)


@torch.no_grad()
def validate(device_net, ex, idx=None, symmetry=None, fp8=False):
    """The validation line of the reference's training loop (SL/train.py:121-146: loss and accuracy on the held-out rows
    after every epoch) for (s, pi, z) examples, on the net the SEARCH uses -- the engine's bf16 MFMA forward
    (DeviceNet.forward), i.e. on the weights as they will play: mean policy cross-entropy against pi, value MSE against z,
    and top-1 agreement (argmax of the logits == argmax of pi; the reference's accuracy is `predicted == actions.argmax`,
    :139-142).  Everything stays on the GPU; returns a dict of Python floats (one synchronisation).
    symmetry: passed to DeviceNet.forward with the examples' board size -- e.g. "mean" validates the
    symmetrised net; None (the default) is the plain forward.  fp8: the engine's fp8 forward instead (what net_fp8 searches use)."""
    own, opp, pi, z = (ex.own, ex.opp, ex.pi, ex.z) if idx is None else (ex.own[idx], ex.opp[idx], ex.pi[idx], ex.z[idx])
    n = int(own.shape[0])
    if n == 0:
        return {"rows": 0, "policy_ce": None, "value_mse": None, "top1": None}
    ce = torch.zeros((), dtype=torch.float64, device=own.device)
    se, hit = torch.zeros_like(ce), torch.zeros_like(ce)
    for a in range(0, n, device_net.max_batch):
        b = min(n, a + device_net.max_batch)
        if symmetry is None:
            logits, v = device_net.forward(own[a:b].contiguous(), opp[a:b].contiguous(), fp8=fp8)
        else:
            logits, v = device_net.forward(own[a:b].contiguous(), opp[a:b].contiguous(), symmetry=symmetry, size=ex.size, fp8=fp8)
        ce += -(pi[a:b] * F.log_softmax(logits, dim=1)).sum()
        se += ((v - z[a:b].to(torch.float32)) ** 2).sum()
        hit += (logits.argmax(1) == pi[a:b].argmax(1)).sum()
    ce, se, hit = (float(t) / n for t in (ce, se, hit))
    return {"rows": n, "loss": ce + se, "policy_ce": ce, "value_mse": se, "top1": hit}


class GraphedTrainStep:
    """train_step() with every buffer static and, for the all-kernel step, captured ONCE into a HIP graph and replayed (ten
    launches back to back instead of ten host calls).  Same arithmetic as train_step (same module, Adam, bf16 autocast),
    fixed batch size.

        step = GraphedTrainStep(module, lr=2e-3, batch=1024, na=65)
        loss, ce, mse = step(examples, idx)      # idx: device index tensor of exactly `batch` rows
        step.check()                             # where the losses are read: raises if an index was out of range

    The optimiser lives inside (the Adam kernel, or torch's Adam with capturable=True: its step counter is a device tensor).
    The forms of the step that go through torch autograd run eagerly unless capture_autograd=True (see __init__)."""

    def __init__(self, module, lr=1e-4, batch=1024, na=65, device="cuda:0", autocast=True, tower_kernels=None, lr_warmup_steps=0,
                 step_kernels=None, fused_adam=None, capture_autograd=False, value_targets=False, weight_decay=0.0, clip_norm=0.0,
                 ema_decay=None, decay_biases=False, ownership=None, own_weight=1.0, fp8_qat=False, symmetry=False):
        # symmetry: every batch position is trained under a board symmetry of its own, step(ex, idx, sym) -- inside
        # the all-kernel step (StepPlan(symmetry=True): one launch more, k_train_sym_batch, in the same graph; the board size is
        # the examples').  Any other form of the step refuses it.
        self.symmetry = bool(symmetry)
        if self.symmetry and (step_kernels is False or not getattr(module, "fused_tower", False) or not autocast or na != 65 or
                              getattr(module, "VH", 65) > 64):
            raise ValueError("symmetry=True needs the all-kernel step (PolicyValueNet(fused_tower=True), step_kernels)")
        # fp8_qat: quantisation-aware training for the fp8 net, inside the all-kernel step (StepPlan(fp8_qat=True):
        # the four k_qat_* kernels in place of stem / pack / tower forward, one launch more in the same graph).  128 channels
        # only, and any other form of the step refuses it.
        from .train_kernels import check_fp8_qat
        self.fp8_qat = check_fp8_qat(fp8_qat, module)
        if self.fp8_qat and (step_kernels is False or not getattr(module, "fused_tower", False) or not autocast or na != 65):
            raise ValueError("fp8_qat=True needs the all-kernel step (PolicyValueNet(fused_tower=True), step_kernels)")
        # ownership: an OwnershipHead trained next to the net on the examples' fown / fopp, inside the all-kernel
        # step (StepPlan(ownership=...): k_train_heads_own and one more launch, k_train_own_finish, in the same graph); the loss
        # is CE + MSE + own_weight * L_own and __call__ returns L_own as a fourth value.  Any other form of the step refuses it.
        from .train_kernels import check_own_weight
        self.ownership, self.own_weight = ownership, check_own_weight(own_weight)
        if ownership is not None and (step_kernels is False or fused_adam is False or not getattr(module, "fused_tower", False)):
            raise ValueError("ownership= needs the all-kernel step (PolicyValueNet(fused_tower=True), step_kernels, fused_adam)")
        # weight_decay / clip_norm / ema_decay / decay_biases: the extended optimiser of the all-kernel step (StepPlan.enable_adam:
        # AdamW's decoupled decay, a clip of the global gradient norm, non-finite steps skipped, an averaged copy of the weights
        # for ema_module()).  It exists only as kernels: any other form of the step refuses the options, before a device is touched.
        self._optim_opts = dict(weight_decay=weight_decay, clip_norm=clip_norm, ema_decay=ema_decay, decay_biases=decay_biases)
        self.extended = bool(weight_decay) or bool(clip_norm) or ema_decay is not None or bool(decay_biases)
        if self.extended and (fused_adam is False or step_kernels is False or not getattr(module, "fused_tower", False)):
            raise ValueError("weight_decay / clip_norm / ema_decay / decay_biases need fused_adam (the all-kernel step)")
        # value_targets: the value loss is against the examples' fp32 `vt` instead of z -- on the all-kernel
        # step through k_train_heads_vt (the graph is captured once with that kernel), on the autograd forms as the MSE target
        self.value_targets = bool(value_targets)
        # (NCHW on purpose: channels-last convolutions measured ~20 % faster per step in tools/bench_train.py, but the
        # closed loop then failed to learn the value head in one run and produced non-finite weights in two others --
        # profiles/r03_az_loop_channels_last_failure.txt -- so that layout is not offered)
        self.module, self.batch, self.dev, self.autocast = module.to(device), batch, torch.device(device), autocast
        # tower_kernels: run the residual tower's forward / backward on the hand-written HIP kernels (csrc/bz_train.hip)
        # instead of MIOpen; default: whenever the module keeps its tower stacked (PolicyValueNet(fused_tower=True))
        if tower_kernels is None:
            tower_kernels = bool(getattr(module, "fused_tower", False))
        # step_kernels: the WHOLE forward / losses / backward on the HIP kernels (train_kernels.StepPlan: 9 launches + Adam's, no
        # autograd -- stem, heads and losses too); default: whenever the tower kernels are on and the step runs in bf16.
        # step_kernels=False keeps stem / heads / losses in torch autograd around the tower kernels (the round-4 form).
        if step_kernels is None:
            step_kernels = tower_kernels and autocast and na == 65 and getattr(module, "VH", 65) <= 64
        self.plan, self.step_plan = None, None
        if tower_kernels or step_kernels:
            from .train_kernels import StepPlan, TowerPlan
            if not getattr(module, "fused_tower", False):
                raise ValueError("tower_kernels / step_kernels need PolicyValueNet(..., fused_tower=True)")
            if step_kernels:
                if ownership is not None:
                    ownership.to(device)
                self.step_plan = self.plan = StepPlan(self.module, batch, device, value_targets=self.value_targets, ownership=ownership,
                                                      own_weight=self.own_weight, fp8_qat=self.fp8_qat, symmetry=self.symmetry)
                self.idx = torch.zeros(batch, dtype=torch.int64, device=self.dev)   # the batch's rows: the kernels gather them themselves
                self.sym = torch.zeros(batch, dtype=torch.uint8, device=self.dev) if self.symmetry else None   # and their symmetries
            else:
                self.plan = TowerPlan(module.C, 2 * module.NB, batch, device)
        if ownership is not None and self.step_plan is None:
            raise ValueError("ownership= needs the all-kernel step (PolicyValueNet(fused_tower=True), step_kernels, fused_adam)")
        if self.fp8_qat and self.step_plan is None:
            raise ValueError("fp8_qat=True needs the all-kernel step (PolicyValueNet(fused_tower=True), step_kernels)")
        if self.symmetry and self.step_plan is None:
            raise ValueError("symmetry=True needs the all-kernel step (PolicyValueNet(fused_tower=True), step_kernels)")
        # lr_warmup_steps > 0: the learning rate ramps linearly from lr / warmup to lr over the first steps.  Adam's first
        # updates move every weight by ~lr whatever the gradient's size; at the loop demo's lr = 2e-3 that kills the
        # single-channel value head's ReLU (and in 2 of 4 seeds every head ReLU, i.e. the whole net) within the first
        # 1-40 steps, in either memory layout -- profiles/r04_channels_last_cause.txt.  The rate lives in a device
        # scalar (capturable Adam reads it inside the graph) that __call__ sets before each replay.
        self.lr, self.warmup, self.steps_done = float(lr), int(lr_warmup_steps), 0
        self.lr_t = torch.tensor(self._lr_at(0), dtype=torch.float32, device=self.dev)
        # fused_adam (default with step_kernels): the Adam update as the step's tenth kernel (StepPlan.enable_adam: step count
        # and warm-up live on the device; a step is then ONE graph launch and a copy of the batch's row numbers).  Otherwise torch's:
        # (fused: the whole Adam update of all parameter tensors is one kernel instead of ~10 multi-tensor ones)
        self.fused_adam = bool(self.step_plan is not None) if fused_adam is None else bool(fused_adam)
        if self.fused_adam:
            if self.step_plan is None:
                raise ValueError("fused_adam needs step_kernels")
            self.step_plan.enable_adam(self.lr, warmup_steps=self.warmup, **(self._optim_opts if self.extended else {}))
            self.optimizer = None
        else:
            if self.extended:
                raise ValueError("weight_decay / clip_norm / ema_decay / decay_biases need fused_adam (the all-kernel step)")
            self.optimizer = torch.optim.Adam(module.parameters(), lr=self.lr_t, capturable=True, fused=True)
        # capture_autograd: a step that goes through torch autograd (step_kernels=False, or a module without the fused tower) is
        # NOT captured into a HIP graph unless asked for -- it runs eagerly, same arithmetic.  Captured autograd steps returned
        # wrong gradients once in a few hundred replays on this stack (a bias gradient of 6e32 at replay 305 / 306, an all-zero
        # one at replay 702 / 703: profiles/r04_channels_last_cause.txt).  Cause (profiles/r05_graph_memset_node.txt,
        # tools/exp_graph_reduction.py): torch's multi-block reductions zero their semaphores with cudaMemsetAsync on the launch
        # stream -- a memset NODE under capture -- and a captured memset node does not reliably zero its buffer on replay here
        # (reproduced with the memset alone).  The all-kernel step (step_kernels) contains no memset node and no torch kernel
        # and is captured as before.
        self.capture = self.step_plan is not None or bool(capture_autograd)
        self.own = torch.zeros(batch, dtype=torch.int64, device=self.dev)
        self.opp = torch.zeros(batch, dtype=torch.int64, device=self.dev)
        self.pi = torch.full((batch, na), 1.0 / na, dtype=torch.float32, device=self.dev)
        self.z = torch.zeros(batch, dtype=torch.float32 if self.value_targets else torch.int8, device=self.dev)
        self.graph, self.out = None, None
        self._restore = None   # a state_dict loaded before the graph exists (load_state_dict)

    def _lr_at(self, k):
        return self.lr * min(1.0, (k + 1) / self.warmup) if self.warmup > 0 else self.lr

    def _step(self):
        if self.step_plan is not None:
            if self.fused_adam:
                return self.step_plan.step()           # 10 launches: gradients and the Adam update
            losses = self.step_plan.grads()            # sets every parameter's .grad
            self.optimizer.step()
            return losses
        x = planes_from_bits(self.own, self.opp)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=self.autocast):
            logits, v = self.module(x, plan=self.plan) if self.plan is not None else self.module(x)
        logits, v = logits.float(), v.float()
        ce = -(self.pi * F.log_softmax(logits, dim=1)).sum(1).mean()
        mse = F.mse_loss(v, self.z.to(torch.float32))
        loss = ce + mse
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        self.optimizer.step()
        return torch.stack([loss.detach(), ce.detach(), mse.detach()])

    def _capture(self):
        """3 eager steps on a side stream (library handles, autotuning, optimiser state) on the batch __call__ has just
        placed in the static buffers, with lr scaled to 0 so that the weights do not move and the optimiser state zeroed
        afterwards; then the capture (which launches nothing: the first real step is the first replay)"""
        self.module.train()
        self.lr_t.zero_()
        if self.fused_adam:
            self.step_plan.set_lr(0.0)
        side = torch.cuda.Stream(device=self.dev)
        side.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(side):
            for _ in range(3):
                self._step()
        torch.cuda.current_stream(self.dev).wait_stream(side)
        if self.fused_adam:   # the warm-up must not count as steps / leave moments behind
            self.step_plan.reset_adam(self.lr, self.warmup, steps_done=self.steps_done)
        else:
            for st in self.optimizer.state.values():
                for k, v in st.items():
                    if torch.is_tensor(v):
                        v.zero_()
        if self._restore is not None:   # a state loaded before the first call: the warm-up above ran over it
            self._apply_state(self._restore)
            self._restore = None
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = self._step()

    def step(self, ex, idx, sym=None):
        """__call__ under its name: one step on rows idx of ex; with symmetry=True, row p under the board symmetry sym[p]"""
        return self(ex, idx, sym)

    def __call__(self, ex, idx, sym=None):
        assert idx.numel() == self.batch, "GraphedTrainStep replays a fixed batch size"
        if self.symmetry:   # (refused before anything is written)
            from .train_symmetry import check_size, check_sym
            check_sym(sym, self.batch, self.dev)
            stage = self.step_plan.sym_stage
            if check_size(ex.size) != stage.size:
                if self.graph is not None:
                    raise ValueError(f"GraphedTrainStep(symmetry=True): the graph was captured for {stage.size} x {stage.size} boards, "
                                     f"these examples are {ex.size} x {ex.size}")
                stage.size = int(ex.size)
        elif sym is not None:
            raise ValueError("GraphedTrainStep: sym given, but the step was built without symmetry=True")
        if self.value_targets and ex.vt is None:
            raise ValueError("GraphedTrainStep(value_targets=True) needs examples with vt (betazero_amd.value_targets.value_targets)")
        if self.ownership is not None and (ex.fown is None or ex.fopp is None):
            raise ValueError("GraphedTrainStep(ownership=...) needs examples with fown / fopp (self-play with ownership=True)")
        if self.step_plan is not None:   # the kernels read rows idx of the data set themselves: one 8-byte-per-row copy, no gathers
            self.idx.copy_(idx)
            own_kw = dict(fown=ex.fown, fopp=ex.fopp) if self.ownership is not None else {}
            if self.symmetry:
                self.sym.copy_(sym)
                own_kw["sym"] = self.sym
            self.step_plan.set_batch(ex.own, ex.opp, ex.pi, ex.z, self.idx, vt=ex.vt if self.value_targets else None, **own_kw)
        else:
            torch.index_select(ex.own, 0, idx, out=self.own)
            torch.index_select(ex.opp, 0, idx, out=self.opp)
            torch.index_select(ex.pi, 0, idx, out=self.pi)
            torch.index_select(ex.vt if self.value_targets else ex.z, 0, idx, out=self.z)
        if not self.capture:   # an autograd form of the step: eager (see capture_autograd in __init__)
            self.module.train()
            self.lr_t.fill_(self._lr_at(self.steps_done))
            out = self._step()
            self.steps_done += 1
            return out[:3].clone()
        if self.graph is None:
            self._capture()
        if not self.fused_adam:
            self.lr_t.fill_(self._lr_at(self.steps_done))
        self.graph.replay()
        self.steps_done += 1
        if self.ownership is not None:   # loss (with own_weight * L_own), CE, MSE, L_own
            return torch.cat([self.out[:3], self.step_plan.own_loss])
        return self.out[:3].clone()

    def set_lr(self, lr):
        """change the (peak) learning rate from the next step on; the fused optimiser reads it from device memory, so the
        captured graph is not recaptured (moments, step count and warm-up stay)"""
        self.lr = float(lr)
        if self.fused_adam:
            self.step_plan.set_lr(self.lr)

    def optim_stats(self, reset=True):
        """{grad_norm, scale, skipped, clipped} of the extended optimiser (StepPlan.optim_stats; synchronises)"""
        if not self.extended:
            raise RuntimeError("GraphedTrainStep: optim_stats() needs weight_decay / clip_norm / ema_decay")
        return self.step_plan.optim_stats(reset=reset)

    def ema_module(self):
        """a deep copy of the module holding the EMA weights (ema_decay=...): what refresh_device_net takes in place of the
        module, and its non-finite check then covers the averaged net"""
        if not self.extended or self.step_plan.ema is None:
            raise RuntimeError("GraphedTrainStep: ema_module() needs ema_decay")
        return self.step_plan.ema_module()

    # ---- the step's state, to carry a run across processes
    def state_dict(self):
        """StepPlan.state_dict() of the all-kernel step -- enough to continue bit for bit -- plus the host-side fields this
        class keeps (the replay counter behind _lr_at, lr, warm-up).  The forms of the step that go through torch's optimiser
        (no fused Adam) save the module's parameters and torch's optimiser state_dict instead, under "module." keys and
        "optimizer"; nothing is claimed about their bits.  CPU tensors and plain numbers only; synchronises."""
        host = dict(steps_done=self.steps_done, lr=self.lr, warmup=self.warmup, fused_adam=self.fused_adam)
        if self.fused_adam:
            return {**self.step_plan.state_dict(), **host}
        cpu = lambda x: x.detach().cpu().clone() if torch.is_tensor(x) else x  # noqa: E731
        opt = self.optimizer.state_dict()
        opt = {"state": {i: {k: cpu(v) for k, v in st.items()} for i, st in opt["state"].items()},
               "param_groups": [{k: (list(v) if isinstance(v, tuple) else cpu(v)) for k, v in g.items()} for g in opt["param_groups"]]}
        return {**{f"module.{k}": cpu(p) for k, p in self.module.named_parameters()}, "optimizer": opt,
                "C": getattr(self.module, "C", None), "blocks": getattr(self.module, "NB", None), "VH": getattr(self.module, "VH", None),
                "batch": self.batch, **host}

    def load_state_dict(self, sd):
        """continue from a state_dict(): copied into the existing tensors (StepPlan.load_state_dict), so a step that has captured
        its graph keeps that graph and the next replay continues from the loaded state; before the first call the state is
        put in place again behind the capture's warm-up steps, which would otherwise zero the moments.  A state that does not
        fit raises ValueError naming the first difference before anything is written."""
        if bool(sd.get("fused_adam")) != self.fused_adam:
            raise ValueError(f"load_state_dict: fused_adam differs: the state was saved with fused_adam = {sd.get('fused_adam')!r}, "
                             f"this step has {self.fused_adam!r}")
        for k in ("steps_done", "lr", "warmup"):
            if not isinstance(sd.get(k), (int, float)) or isinstance(sd.get(k), bool):
                raise ValueError(f"load_state_dict: the state's {k} is not a number")
        if self.fused_adam:
            self.step_plan._check_state(sd)
        else:
            for k, p in self.module.named_parameters():
                s = sd.get(f"module.{k}")
                if not torch.is_tensor(s) or s.shape != p.shape or s.dtype != p.dtype:
                    raise ValueError(f"load_state_dict: tensor module.{k} differs from this step's module")
            if not isinstance(sd.get("optimizer"), dict):
                raise ValueError("load_state_dict: the state has no torch optimiser state")
        self._apply_state(sd)
        self._restore = sd if (self.capture and self.graph is None) else None   # _capture() puts it back behind its warm-up

    def _apply_state(self, sd):
        """the writing half of load_state_dict (the state has been checked)"""
        if self.fused_adam:
            self.step_plan.load_state_dict(sd)
        else:
            with torch.no_grad():
                for k, p in self.module.named_parameters():
                    p.copy_(sd[f"module.{k}"])
            self._load_torch_optimizer(sd["optimizer"])
        self.steps_done, self.lr, self.warmup = int(sd["steps_done"]), float(sd["lr"]), int(sd["warmup"])

    def _load_torch_optimizer(self, opt):
        """torch's optimiser state: in place where the tensors exist (a captured graph holds their addresses), through
        torch's own load_state_dict otherwise; the rate stays the device scalar lr_t"""
        groups = [{**g, "lr": self.lr_t, "betas": tuple(g["betas"])} for g in opt["param_groups"]]
        ps = [p for g in self.optimizer.param_groups for p in g["params"]]
        if self.graph is not None and all(p in self.optimizer.state for p in ps):
            with torch.no_grad():
                for i, p in enumerate(ps):
                    for k, v in opt["state"][i].items():
                        self.optimizer.state[p][k].copy_(v)
        else:
            self.optimizer.load_state_dict({"state": opt["state"], "param_groups": groups})
            for g in self.optimizer.param_groups:
                g["lr"] = self.lr_t

    def check(self):
        """raise IndexError if a step since the last check was handed a row index outside the data set (the all-kernel step
        clamps instead of faulting and counts the event in its error word; the autograd forms raise inside index_select).
        Synchronises: call it where the losses are read, not every step."""
        if self.step_plan is not None:
            self.step_plan.check_rows()


def refresh_device_net(device_net, module):
    """push the trained weights into the HIP engine's net (bf16-rounded copy for the MFMA path).  Raises
    FloatingPointError when a parameter is not finite (one isfinite reduction per refresh): the losses of a step are
    computed BEFORE its optimiser update, so a last step that overflows is invisible in them.  A net with such weights
    gives non-finite logits or values (the inference ReLUs pass a NaN), and the engine would then raise
    ERR_EVAL_NONFINITE in the next search, far from the cause."""
    import copy
    bad = [n for n, p in module.named_parameters() if not bool(torch.isfinite(p.detach()).all())]
    if bad:
        raise FloatingPointError(f"refresh_device_net: non-finite values in {len(bad)} parameter tensor(s), first: {bad[0]}; "
                                 "the engine's net was NOT updated")
    m = copy.deepcopy(module).cpu()
    m.round_to_bf16_()
    flat = m.flat_params()
    device_net.update(flat)
    return flat
