"""The reference's tic-tac-toe policy MLP (src/tic_tac_toe/SL/neural_networks.py): the torch module, a loader for the
reference's checkpoints, the device handle around bz_mlp (forward in fp32 parity or bf16 MFMA mode) and the supervised
trainer of SL/train.py on the bz_mlp training step (include/bz_abi.h).  And the same net with a value head
(TicTacToePVNet: fc4 has a tenth row, v = tanh of it), which the same handle serves and PVTrainer trains on what self-play
produces, a visit distribution pi and a value target per row (bz_mlp_train_step_pv)."""
import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from . import _lib


class TicTacToeNet(nn.Module):
    """Linear(in, H) - ReLU - Linear(H, H) - ReLU - Linear(H, H) - ReLU - Linear(H, out), policy logits only.  Constructor
    and attribute names are the reference's, so state_dicts interchange both ways."""

    def __init__(self, input_size, hidden_size, output_size):
        super().__init__()
        self.fc1 = nn.Linear(input_size, hidden_size)
        self.relu1 = nn.ReLU()
        self.fc2 = nn.Linear(hidden_size, hidden_size)
        self.relu2 = nn.ReLU()
        self.fc3 = nn.Linear(hidden_size, hidden_size)
        self.relu3 = nn.ReLU()
        self.fc4 = nn.Linear(hidden_size, output_size)

    def forward(self, x):
        x = self.relu1(self.fc1(x))
        x = self.relu2(self.fc2(x))
        x = self.relu3(self.fc3(x))
        return self.fc4(x)

    @property
    def hidden_size(self):
        return self.fc1.out_features

    def flat_params(self):
        """fp32 vector in bz_mlp's order (torch layouts): fc1.w fc1.b fc2.w fc2.b fc3.w fc3.b fc4.w fc4.b"""
        return torch.cat([t.detach().reshape(-1) for m in (self.fc1, self.fc2, self.fc3, self.fc4)
                          for t in (m.weight, m.bias)]).to(torch.float32).cpu().numpy().copy()

    @torch.no_grad()
    def load_flat_params_(self, flat):
        flat = torch.as_tensor(np.asarray(flat, dtype=np.float32))
        o = 0
        for m in (self.fc1, self.fc2, self.fc3, self.fc4):
            for t in (m.weight, m.bias):
                t.copy_(flat[o:o + t.numel()].view_as(t))
                o += t.numel()
        assert o == flat.numel()
        return self


class TicTacToePVNet(nn.Module):
    """TicTacToeNet with a value head: fc1..fc3 are the reference's, fc4 = Linear(H, 10) whose rows 0..8 are the policy
    logits and whose row 9 is the value pre-activation u, v = tanh(u).  forward(x) -> (logits [n, 9], v [n])."""

    def __init__(self, hidden_size):
        super().__init__()
        self.fc1 = nn.Linear(9, hidden_size)
        self.relu1 = nn.ReLU()
        self.fc2 = nn.Linear(hidden_size, hidden_size)
        self.relu2 = nn.ReLU()
        self.fc3 = nn.Linear(hidden_size, hidden_size)
        self.relu3 = nn.ReLU()
        self.fc4 = nn.Linear(hidden_size, 10)

    def forward(self, x):
        x = self.relu1(self.fc1(x))
        x = self.relu2(self.fc2(x))
        x = self.relu3(self.fc3(x))
        y = self.fc4(x)
        return y[..., :9], torch.tanh(y[..., 9])

    @property
    def hidden_size(self):
        return self.fc1.out_features

    def flat_params(self):
        """fp32 vector in bz_mlp's order, fc4.w [10][H] and fc4.b [10]: 2 H^2 + 22 H + 10 floats"""
        return TicTacToeNet.flat_params(self)

    def load_flat_params_(self, flat):
        return TicTacToeNet.load_flat_params_(self, flat)

    @classmethod
    @torch.no_grad()
    def from_policy_net(cls, m):
        """a TicTacToeNet (e.g. one from load_reference_model) with a value head of zeros: the same logits, v = 0 exactly"""
        if m.fc1.in_features != 9 or m.fc4.out_features != 9:
            raise ValueError("TicTacToePVNet.from_policy_net: the net must map 9 cells to 9 logits")
        pv = cls(m.hidden_size)
        for name in ("fc1", "fc2", "fc3"):
            getattr(pv, name).load_state_dict({k: v.to(torch.float32) for k, v in getattr(m, name).state_dict().items()})
        pv.fc4.weight.zero_(); pv.fc4.bias.zero_()
        pv.fc4.weight[:9].copy_(m.fc4.weight); pv.fc4.bias[:9].copy_(m.fc4.bias)
        return pv.train(m.training)

    @torch.no_grad()
    def policy_net(self):
        """the TicTacToeNet of rows 0..8: its state_dict is what the reference's AIPlayer loads"""
        m = TicTacToeNet(9, self.hidden_size, 9)
        for name in ("fc1", "fc2", "fc3"):
            getattr(m, name).load_state_dict(getattr(self, name).state_dict())
        m.fc4.weight.copy_(self.fc4.weight[:9]); m.fc4.bias.copy_(self.fc4.bias[:9])
        return m.train(self.training)


def _module_from_state_dict(sd):
    H, n_in = sd["fc1.weight"].shape
    m = TicTacToeNet(int(n_in), int(H), int(sd["fc4.weight"].shape[0]))
    m.load_state_dict({k: v.to(torch.float32) for k, v in sd.items()})
    return m


def load_reference_model(path):
    """A TicTacToeNet from either a state_dict file or the reference's whole-module checkpoint (SL/train.py saves
    torch.save(model, ...) with the class bound to __main__.TicTacToeNet).  Only ever torch.load(weights_only=True): the
    whole-module form is read with an allowlist of exactly this class (under the reference's name), nn.Linear and nn.ReLU,
    so no code from the file runs."""
    with torch.serialization.safe_globals([(TicTacToeNet, "__main__.TicTacToeNet"), (TicTacToeNet, "neural_networks.TicTacToeNet"),
                                           nn.Linear, nn.ReLU]):
        obj = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(obj, nn.Module):
        obj = obj.state_dict()
    if not isinstance(obj, dict) or "fc1.weight" not in obj:
        raise ValueError(f"{path}: neither a TicTacToeNet nor its state_dict")
    return _module_from_state_dict(obj).eval()


def _bits(t, device):
    if isinstance(t, torch.Tensor):
        return t.to(device=device, dtype=torch.int64).contiguous()
    return torch.as_tensor(np.asarray(t, dtype=np.uint64).view(np.int64)).to(device)


class DeviceMLP:
    """bz_mlp handle: the weights repacked for the HIP kernels in a torch-owned workspace.  The parameter count says which
    net it is: TicTacToeNet's (policy only) or TicTacToePVNet's (.value_head: the forwards can return v, and the MLP evaluators
    of the search put it on the leaves)."""

    def __init__(self, hidden_size, params, max_batch=65536, device="cuda:0"):
        _lib.require_gpu()
        L = _lib.lib()
        params = np.ascontiguousarray(params, dtype=np.float32)
        self.value_head = params.size == L.bz_mlp_pv_param_count(hidden_size)
        if not self.value_head and L.bz_mlp_param_count(hidden_size) != params.size:
            raise ValueError(f"DeviceMLP: {params.size} parameters do not make a 9-{hidden_size}-{hidden_size}-{hidden_size}-9 net "
                             f"or one with a value head (H: a multiple of 32 in 32..512) {_lib.last_error()}")
        nbytes = (L.bz_mlp_pv_workspace_bytes if self.value_head else L.bz_mlp_workspace_bytes)(hidden_size, max_batch)
        if nbytes < 0:
            raise ValueError(_lib.last_error())
        self.device = torch.device(device)
        self.ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        self._base = (self.ws.data_ptr() + 255) & ~255
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check((L.bz_mlp_create_pv if self.value_head else L.bz_mlp_create)(
                hidden_size, max_batch, params.ctypes.data, self._base, nbytes, torch.cuda.current_stream().cuda_stream, C.byref(h)))
        self.h = h
        self.H, self.max_batch = hidden_size, max_batch

    @classmethod
    def from_module(cls, module, max_batch=65536, device="cuda:0"):
        """a TicTacToeNet or a TicTacToePVNet"""
        if module.fc1.in_features != 9 or module.fc4.out_features != (10 if isinstance(module, TicTacToePVNet) else 9):
            raise ValueError("DeviceMLP: the net must map 9 cells to 9 logits (TicTacToePVNet: and a value)")
        return cls(module.hidden_size, module.flat_params(), max_batch, device)

    @property
    def param_count(self):
        L = _lib.lib()
        return (L.bz_mlp_pv_param_count if self.value_head else L.bz_mlp_param_count)(self.H)

    def _call(self, fn, *args):
        with torch.cuda.device(self.device):
            _lib.check(fn(self.h, *args, torch.cuda.current_stream().cuda_stream))

    def _check_value(self, value):
        if value and not self.value_head:
            raise ValueError("DeviceMLP: value=True needs a net with a value head (TicTacToePVNet); this one is policy only")

    def _forward(self, name, value, n, *inputs):
        logits = torch.empty((n, 9), dtype=torch.float32, device=self.device)
        L = _lib.lib()
        if not value:
            self._call(getattr(L, "bz_mlp_forward_" + name), *inputs, n, logits.data_ptr())
            return logits
        v = torch.empty(n, dtype=torch.float32, device=self.device)
        self._call(getattr(L, "bz_mlp_forward_pv_" + name), *inputs, n, logits.data_ptr(), v.data_ptr())
        return logits, v

    def forward(self, own, opp, bf16=False, value=False):
        """own/opp: side-to-move bitboards (cell i = bit i), uint64-as-int64 tensors or arrays [n] -> logits [n, 9] f32;
        value=True (a net with a value head): (logits, v [n] f32)"""
        self._check_value(value)
        own, opp = _bits(own, self.device), _bits(opp, self.device)
        return self._forward("bf16" if bf16 else "f32", value, own.numel(), own.data_ptr(), opp.data_ptr())

    def forward_states(self, x, bf16=False, value=False):
        """x: the reference's input (symbol * board), [n, 9] or [n, 3, 3] -> logits [n, 9] f32; value=True: (logits, v [n])"""
        self._check_value(value)
        x = torch.as_tensor(x).to(device=self.device, dtype=torch.float32).reshape(-1, 9).contiguous()
        return self._forward("states_bf16" if bf16 else "states_f32", value, x.shape[0], x.data_ptr())

    def update(self, module_or_params):
        """replace the weights in place (same H, same kind of net): a module or a flat parameter vector"""
        p = module_or_params.flat_params() if isinstance(module_or_params, nn.Module) else module_or_params
        if isinstance(p, torch.Tensor):
            p = p.detach().cpu().numpy()
        p = np.ascontiguousarray(p, dtype=np.float32)
        if p.size != self.param_count:
            raise ValueError("DeviceMLP.update: parameter count does not match H (and the net's kind: with or without a value head)")
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().bz_mlp_update(self.h, p.ctypes.data, torch.cuda.current_stream().cuda_stream))

    def __del__(self):
        try:
            _lib.lib().bz_mlp_destroy(self.h)
        except Exception:
            pass


def _targets(actions):
    a = torch.as_tensor(actions)
    return a.reshape(a.shape[0], -1).argmax(1).to(torch.int32)


class MLPTrainer:
    """SL/train.py's training on the device: CrossEntropyLoss(logits, action.argmax(1)) averaged over the batch, then
    torch.optim.Adam (lr 1e-4, betas (0.9, 0.999), eps 1e-8, no weight decay).  One step = two kernel launches
    (bz_mlp_train_step); parameters, moments and gradients are fp32 device tensors in torch's flat order."""

    def __init__(self, module, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, max_batch=128, device="cuda:0"):
        _lib.require_gpu()
        L = _lib.lib()
        self.device = torch.device(device)
        self.H, self.max_batch = module.hidden_size, max_batch
        self.adam = _lib.MlpAdam(lr, betas[0], betas[1], eps, 0)
        flat = module.flat_params()
        self.mlp = DeviceMLP(self.H, flat, max(max_batch, 1024), device)
        self.p = torch.as_tensor(flat).to(self.device)
        self.m = torch.zeros_like(self.p)
        self.v = torch.zeros_like(self.p)
        self.grad = torch.zeros_like(self.p)
        nbytes = L.bz_mlp_train_workspace_bytes(self.H, max_batch)
        if nbytes < 0:
            raise ValueError(_lib.last_error())
        self._ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        self._ws_base, self._ws_bytes = (self._ws.data_ptr() + 255) & ~255, nbytes
        self.err = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.logits = torch.empty((max_batch, 9), dtype=torch.float32, device=self.device)
        self.steps = 0

    def step(self, states, targets, row_weight=None):
        """one Adam step on a batch: states [n, 9] (symbol * board), targets [n] (0..8) or one-hot actions [n, 9].  Returns
        the batch loss as a device tensor [1] (not synchronised).  The error word (self.err) is checked by error()."""
        x = torch.as_tensor(states).to(device=self.device, dtype=torch.float32).reshape(-1, 9).contiguous()
        t = torch.as_tensor(targets)
        t = (_targets(t) if t.dim() > 1 else t).to(device=self.device, dtype=torch.int32).contiguous()
        n = x.shape[0]
        if t.numel() != n or not 1 <= n <= self.max_batch:
            raise ValueError(f"MLPTrainer.step: need 1 <= n <= {self.max_batch} rows and one target per row")
        w = None if row_weight is None else torch.as_tensor(row_weight).to(device=self.device, dtype=torch.float32).contiguous()
        self.adam.step = self.steps + 1
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().bz_mlp_train_step(
                self.mlp.h, self.p.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.grad.data_ptr(), x.data_ptr(),
                t.data_ptr(), None if w is None else w.data_ptr(), n, C.byref(self.adam), self._ws_base, self._ws_bytes,
                self.loss.data_ptr(), self.logits.data_ptr(), self.err.data_ptr(), torch.cuda.current_stream().cuda_stream))
        self.steps += 1
        self._keep = (x, t, w)  # alive until the stream has consumed them
        return self.loss

    def error(self):
        """the sticky error word (bz_abi.h): 0 = fine, 1 = bad target, 2 = non-finite loss, 4 = row weights sum <= 0"""
        return int(self.err.item())

    def clear_error(self):
        self.err.zero_()

    def _eval(self, x, t, batch):
        """(summed per-batch mean loss, batches, correct) of the f32 forward over x, in batches of `batch`"""
        loss, nb, correct = torch.zeros((), device=self.device), 0, torch.zeros((), dtype=torch.int64, device=self.device)
        for i in range(0, x.shape[0], batch):
            lg = self.mlp.forward_states(x[i:i + batch])
            tt = t[i:i + batch].to(torch.int64)
            loss = loss + torch.nn.functional.cross_entropy(lg, tt)
            correct = correct + (lg.argmax(1) == tt).sum()
            nb += 1
        return loss, nb, correct

    def fit(self, states, actions, epochs, batch=128, val_fraction=0.2, generator=None, val_batch=1000, log=None):
        """SL/train.py's loop: random split (val = int(n * val_fraction) rows), per epoch a fresh shuffle of the training
        rows in batches of `batch` (the last one short: its missing rows carry weight 0), then the validation rows.  Data
        stays on the device; the shuffle and split draw from `generator` (a torch.Generator on this device; default seed
        0).  Returns a list of per-epoch dicts: train_loss / val_loss (means of the per-batch means, as the reference's
        progress bar) and train_acc / val_acc."""
        if batch > self.max_batch:
            raise ValueError("MLPTrainer.fit: batch > max_batch")
        x = torch.as_tensor(states).to(device=self.device, dtype=torch.float32).reshape(-1, 9)
        t = _targets(actions).to(self.device)
        if generator is None:
            generator = torch.Generator(device=self.device)
            generator.manual_seed(0)
        n = x.shape[0]
        n_val = int(n * val_fraction)
        perm = torch.randperm(n, generator=generator, device=self.device)
        tr, va = perm[:n - n_val], perm[n - n_val:]
        xv, tv = x[va].contiguous(), t[va].contiguous()
        n_tr = tr.numel()
        n_batches = (n_tr + batch - 1) // batch
        pad = n_batches * batch - n_tr
        wfull = torch.ones(n_batches * batch, dtype=torch.float32, device=self.device)
        if pad:
            wfull[n_tr:] = 0.0
        hist = []
        for ep in range(epochs):
            order = tr[torch.randperm(n_tr, generator=generator, device=self.device)]
            if pad:
                order = torch.cat([order, order[:pad]])
            xb, tb = x[order].contiguous(), t[order].contiguous()
            tl = torch.zeros((), device=self.device)
            correct = torch.zeros((), dtype=torch.int64, device=self.device)
            for b in range(n_batches):
                s = slice(b * batch, (b + 1) * batch)
                nb = batch if b < n_batches - 1 or not pad else batch - pad
                # a short last batch: the same shape, the padding rows weigh 0 (they neither move the loss nor the step)
                loss = self.step(xb[s], tb[s], wfull[s] if nb < batch else None)
                tl = tl + loss[0]
                correct = correct + (self.logits[:nb].argmax(1) == tb[s][:nb]).sum()
            vl, vnb, vc = self._eval(xv, tv, val_batch) if n_val else (torch.zeros(()), 1, torch.zeros(()))
            rec = {"epoch": ep + 1, "train_loss": float(tl) / n_batches, "train_acc": int(correct) / n_tr,
                   "val_loss": float(vl) / vnb, "val_acc": (int(vc) / n_val) if n_val else float("nan")}
            if self.error():
                raise RuntimeError(f"MLPTrainer.fit: training error word {self.error()} in epoch {ep + 1}")
            hist.append(rec)
            if log:
                log(rec)
        return hist

    def params(self):
        return self.p.detach().cpu().numpy().copy()

    def to_module(self):
        """a plain TicTacToeNet holding the trained weights"""
        return TicTacToeNet(9, self.H, 9).load_flat_params_(self.params()).eval()


class PVTrainer:
    """AlphaZero's training on the device for TicTacToePVNet: per row the policy cross-entropy against the search's visit
    distribution pi plus value_weight times the squared error of v = tanh(u) against a value target, averaged over the batch
    with optional row weights, then torch.optim.Adam's formula (bz_mlp_train_step_pv: two kernel launches).
    `module` is a TicTacToePVNet, or a TicTacToeNet, which gets a value head of zeros (TicTacToePVNet.from_policy_net).
    lr's default is untuned: nobody has searched it for this net and this loop."""

    def __init__(self, module, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, value_weight=1.0, max_batch=1024, device="cuda:0"):
        _lib.require_gpu()
        L = _lib.lib()
        if not isinstance(module, TicTacToePVNet):
            module = TicTacToePVNet.from_policy_net(module)
        self.device = torch.device(device)
        self.H, self.max_batch, self.value_weight = module.hidden_size, max_batch, float(value_weight)
        self.adam = _lib.MlpAdam(lr, betas[0], betas[1], eps, 0)
        flat = module.flat_params()
        self.mlp = DeviceMLP(self.H, flat, max(max_batch, 65536), device)   # what the engines hold: any n_games they run
        self.p = torch.as_tensor(flat).to(self.device)
        self.m = torch.zeros_like(self.p)
        self.v = torch.zeros_like(self.p)
        self.grad = torch.zeros_like(self.p)
        nbytes = L.bz_mlp_train_pv_workspace_bytes(self.H, max_batch)
        if nbytes < 0:
            raise ValueError(_lib.last_error())
        self._ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        self._ws_base, self._ws_bytes = (self._ws.data_ptr() + 255) & ~255, nbytes
        self.err = torch.zeros(1, dtype=torch.int32, device=self.device)
        self.loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.logits = torch.empty((max_batch, 9), dtype=torch.float32, device=self.device)
        self.value = torch.empty(max_batch, dtype=torch.float32, device=self.device)
        self.steps = 0

    @property
    def device_mlp(self):
        """the handle the engines search with; every step leaves it current"""
        return self.mlp

    def step(self, states, pi, vt, row_weight=None):
        """one Adam step on a batch: states [n, 9] (symbol * board), pi [n, 9] >= 0, vt [n] in [-1, 1].  Returns the batch loss
        as a device tensor [1] (not synchronised).  The error word (self.err) is checked by error()."""
        def f32(t, shape):
            return torch.as_tensor(t).to(device=self.device, dtype=torch.float32).reshape(shape).contiguous()
        x, pi, vt = f32(states, (-1, 9)), f32(pi, (-1, 9)), f32(vt, (-1,))
        n = x.shape[0]
        if pi.shape[0] != n or vt.numel() != n or not 1 <= n <= self.max_batch:
            raise ValueError(f"PVTrainer.step: need 1 <= n <= {self.max_batch} rows, and a pi row and a value target per row")
        w = None if row_weight is None else f32(row_weight, (-1,))
        if w is not None and w.numel() != n:
            raise ValueError("PVTrainer.step: one row weight per row")
        self.adam.step = self.steps + 1
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().bz_mlp_train_step_pv(
                self.mlp.h, self.p.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.grad.data_ptr(), x.data_ptr(),
                pi.data_ptr(), vt.data_ptr(), None if w is None else w.data_ptr(), n, self.value_weight, C.byref(self.adam),
                self._ws_base, self._ws_bytes, self.loss.data_ptr(), self.logits.data_ptr(), self.value.data_ptr(),
                self.err.data_ptr(), torch.cuda.current_stream().cuda_stream))
        self.steps += 1
        self._keep = (x, pi, vt, w)  # alive until the stream has consumed them
        return self.loss

    def error(self):
        """the sticky error word (bz_abi.h): 0 = fine, 1 = a bad pi row or value target, 2 = non-finite loss, 4 = row weights
        sum <= 0"""
        return int(self.err.item())

    def clear_error(self):
        self.err.zero_()

    @staticmethod
    def _rows(ex, idx):
        """(states [n, 9] f32, pi, value target, act) of a DeviceExamples of size 3, all rows or the rows idx"""
        if ex.size != 3 or ex.pi.shape[1] != 9:
            raise ValueError("PVTrainer: the examples must be tic-tac-toe rows (size 3, 9 actions)")
        x = ex.states().reshape(-1, 9).to(torch.float32)
        vt = (ex.vt if ex.vt is not None else ex.z).to(torch.float32)
        pi, act = ex.pi, ex.act.to(torch.int64)
        if idx is not None:
            idx = torch.as_tensor(idx).to(device=x.device, dtype=torch.int64)
            x, pi, vt, act = x[idx], pi[idx], vt[idx], act[idx]
        return x, pi, vt, act

    def fit_examples(self, ex, epochs, batch=None, generator=None, idx=None):
        """`epochs` passes over a DeviceExamples of tic-tac-toe rows (all of them, or the rows `idx`: an index list, with
        repeats if it has them, e.g. from surprise_resample / merged_repeats): states from own / opp on the device, the value
        target ex.vt where the rows carry one, else ex.z.  Per epoch a fresh shuffle in batches of `batch` (default: max_batch);
        a short last batch keeps the shape, its padding rows weigh 0.  The shuffle draws from `generator` (a torch.Generator
        on this device; default seed 0).  Returns a list of per-epoch dicts: epoch, loss (mean of the batch losses), rows."""
        batch = self.max_batch if batch is None else batch
        if not 1 <= batch <= self.max_batch:
            raise ValueError("PVTrainer.fit_examples: need 1 <= batch <= max_batch")
        x, pi, vt, _ = self._rows(ex, idx)
        n = x.shape[0]
        if n == 0:
            raise ValueError("PVTrainer.fit_examples: no rows")
        if generator is None:
            generator = torch.Generator(device=self.device)
            generator.manual_seed(0)
        n_batches = (n + batch - 1) // batch
        pad = n_batches * batch - n
        wlast = torch.ones(batch, dtype=torch.float32, device=self.device)
        if pad:
            wlast[batch - pad:] = 0.0
        hist = []
        for ep in range(epochs):
            order = torch.randperm(n, generator=generator, device=self.device)
            if pad:
                order = torch.cat([order, order[:1].expand(pad)])
            xb, pb, vb = x[order].contiguous(), pi[order].contiguous(), vt[order].contiguous()
            tl = torch.zeros((), device=self.device)
            for b in range(n_batches):
                s = slice(b * batch, (b + 1) * batch)
                tl = tl + self.step(xb[s], pb[s], vb[s], wlast if pad and b == n_batches - 1 else None)[0]
            if self.error():
                raise RuntimeError(f"PVTrainer.fit_examples: training error word {self.error()} in epoch {ep + 1}")
            hist.append({"epoch": ep + 1, "loss": float(tl) / n_batches, "rows": n})
        return hist

    def evaluate(self, ex, idx=None):
        """the f32 forward over the rows: {"policy_ce": mean of sum_o pi_o (lse(z) - z_o), "value_mse": mean (v - target)^2,
        "top1": the share of rows whose top logit is ex.act, "rows"}"""
        x, pi, vt, act = self._rows(ex, idx)
        n = x.shape[0]
        ce = torch.zeros((), dtype=torch.float64, device=self.device)
        se = torch.zeros((), dtype=torch.float64, device=self.device)
        hit = torch.zeros((), dtype=torch.int64, device=self.device)
        for i in range(0, n, self.mlp.max_batch):
            s = slice(i, i + self.mlp.max_batch)
            lg, v = self.mlp.forward_states(x[s], value=True)
            lse = torch.logsumexp(lg.double(), 1, keepdim=True)
            ce = ce + (pi[s].double() * (lse - lg.double())).sum()
            se = se + ((v.double() - vt[s].double()) ** 2).sum()
            hit = hit + (lg.argmax(1) == act[s]).sum()
        return {"policy_ce": float(ce) / max(n, 1), "value_mse": float(se) / max(n, 1), "top1": int(hit) / max(n, 1), "rows": n}

    def params(self):
        return self.p.detach().cpu().numpy().copy()

    def to_module(self):
        """a plain TicTacToePVNet holding the trained weights"""
        return TicTacToePVNet(self.H).load_flat_params_(self.params()).eval()

    def state_dict(self):
        """parameters, Adam's moments and the step count, as CPU tensors: what load_state_dict needs to go on bit for bit"""
        return {"hidden_size": self.H, "p": self.p.cpu().clone(), "m": self.m.cpu().clone(), "v": self.v.cpu().clone(),
                "steps": self.steps}

    def load_state_dict(self, sd):
        """resume from state_dict(): a state of another H is refused (ValueError) before anything is written; the
        hyper-parameters are this trainer's own"""
        n = self.p.numel()
        if int(sd["hidden_size"]) != self.H or any(torch.as_tensor(sd[k]).numel() != n for k in ("p", "m", "v")):
            raise ValueError(f"PVTrainer.load_state_dict: the state is of hidden size {int(sd['hidden_size'])}, this trainer of {self.H}")
        if int(sd["steps"]) < 0:
            raise ValueError("PVTrainer.load_state_dict: negative step count")
        p = torch.as_tensor(sd["p"]).to(torch.float32).reshape(-1)
        self.mlp.update(p)   # drains the device first: no search sees half-replaced weights
        self.p.copy_(p)
        self.m.copy_(torch.as_tensor(sd["m"]).to(torch.float32).reshape(-1))
        self.v.copy_(torch.as_tensor(sd["v"]).to(torch.float32).reshape(-1))
        self.steps = int(sd["steps"])
