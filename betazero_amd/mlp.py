"""The reference's tic-tac-toe policy MLP (src/tic_tac_toe/SL/neural_networks.py): the torch module, a loader for the
reference's checkpoints, the device handle around bz_mlp (forward in fp32 parity or bf16 MFMA mode) and the supervised
trainer of SL/train.py on the bz_mlp training step (include/bz_abi.h)."""
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
    """bz_mlp handle: the weights repacked for the HIP kernels in a torch-owned workspace."""

    def __init__(self, hidden_size, params, max_batch=65536, device="cuda:0"):
        _lib.require_gpu()
        L = _lib.lib()
        params = np.ascontiguousarray(params, dtype=np.float32)
        if L.bz_mlp_param_count(hidden_size) != params.size:
            raise ValueError(f"DeviceMLP: {params.size} parameters do not make a 9-{hidden_size}-{hidden_size}-{hidden_size}-9 net "
                             f"(H: a multiple of 32 in 32..512) {_lib.last_error()}")
        nbytes = L.bz_mlp_workspace_bytes(hidden_size, max_batch)
        if nbytes < 0:
            raise ValueError(_lib.last_error())
        self.device = torch.device(device)
        self.ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=self.device)
        self._base = (self.ws.data_ptr() + 255) & ~255
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(L.bz_mlp_create(hidden_size, max_batch, params.ctypes.data, self._base, nbytes,
                                       torch.cuda.current_stream().cuda_stream, C.byref(h)))
        self.h = h
        self.H, self.max_batch = hidden_size, max_batch

    @classmethod
    def from_module(cls, module, max_batch=65536, device="cuda:0"):
        if module.fc1.in_features != 9 or module.fc4.out_features != 9:
            raise ValueError("DeviceMLP: the net must map 9 cells to 9 logits")
        return cls(module.hidden_size, module.flat_params(), max_batch, device)

    def _call(self, fn, *args):
        with torch.cuda.device(self.device):
            _lib.check(fn(self.h, *args, torch.cuda.current_stream().cuda_stream))

    def forward(self, own, opp, bf16=False):
        """own/opp: side-to-move bitboards (cell i = bit i), uint64-as-int64 tensors or arrays [n] -> logits [n, 9] f32"""
        own, opp = _bits(own, self.device), _bits(opp, self.device)
        n = own.numel()
        logits = torch.empty((n, 9), dtype=torch.float32, device=self.device)
        L = _lib.lib()
        self._call(L.bz_mlp_forward_bf16 if bf16 else L.bz_mlp_forward_f32, own.data_ptr(), opp.data_ptr(), n, logits.data_ptr())
        return logits

    def forward_states(self, x, bf16=False):
        """x: the reference's input (symbol * board), [n, 9] or [n, 3, 3] -> logits [n, 9] f32"""
        x = torch.as_tensor(x).to(device=self.device, dtype=torch.float32).reshape(-1, 9).contiguous()
        n = x.shape[0]
        logits = torch.empty((n, 9), dtype=torch.float32, device=self.device)
        L = _lib.lib()
        self._call(L.bz_mlp_forward_states_bf16 if bf16 else L.bz_mlp_forward_states_f32, x.data_ptr(), n, logits.data_ptr())
        return logits

    def update(self, module_or_params):
        """replace the weights in place (same H): a TicTacToeNet or a flat parameter vector"""
        p = module_or_params.flat_params() if isinstance(module_or_params, nn.Module) else module_or_params
        if isinstance(p, torch.Tensor):
            p = p.detach().cpu().numpy()
        p = np.ascontiguousarray(p, dtype=np.float32)
        if p.size != _lib.lib().bz_mlp_param_count(self.H):
            raise ValueError("DeviceMLP.update: parameter count does not match H")
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
