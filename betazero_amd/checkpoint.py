"""One file that carries a training run across processes.

    save_checkpoint(path, state)       # state: a dict of tensors, numbers, strings, lists and dicts, nothing else
    state = load_checkpoint(path)      # the same dict, tensors on the CPU

The file is torch.save's zip of {"format": ..., "version": ..., "state": state} and is only ever read with
torch.load(weights_only=True): no code from the file runs, and a state holding anything but the plain types above is refused
when it is WRITTEN, not when it is read.  The write is atomic: a temporary file in the target's directory, flushed, then
os.replace -- whatever fails, the previous checkpoint stays byte for byte and no temporary file is left behind.

What goes into `state` is the caller's business (tools/az_loop.py: GraphedTrainStep.state_dict(), the nets, the window, the
generator); StepPlan.state_dict / load_state_dict (train_kernels.py) are the part that is specified to the bit."""
import os
import tempfile

import torch

FORMAT = "betazero_amd checkpoint"
VERSION = 1

_PLAIN = (bool, int, float, str, type(None))


def _check_plain(x, where):
    """refuse, with the place it sits at, anything torch.load(weights_only=True) would not hand back"""
    if isinstance(x, _PLAIN) or torch.is_tensor(x):
        return
    if isinstance(x, dict):
        for k, v in x.items():
            if not isinstance(k, (str, int)) or isinstance(k, bool):
                raise TypeError(f"save_checkpoint: {where} has the key {k!r}; keys are strings or ints")
            _check_plain(v, f"{where}[{k!r}]")
        return
    if isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            _check_plain(v, f"{where}[{i}]")
        return
    raise TypeError(f"save_checkpoint: {where} is a {type(x).__name__}; a checkpoint holds tensors, numbers, strings, lists "
                    "and dicts only")


def save_checkpoint(path, state):
    """write `state` to `path` atomically (see the module's text); tensors are stored as they are, so hand over CPU tensors"""
    if not isinstance(state, dict):
        raise TypeError("save_checkpoint: state must be a dict")
    path = os.fspath(path)
    fd, tmp = tempfile.mkstemp(prefix=os.path.basename(path) + ".", suffix=".tmp", dir=os.path.dirname(os.path.abspath(path)))
    try:
        with os.fdopen(fd, "wb") as f:
            _check_plain(state, "state")
            torch.save({"format": FORMAT, "version": VERSION, "state": state}, f)
            f.flush()
            os.fsync(f.fileno())
        umask = os.umask(0)   # (mkstemp creates the file for its owner alone; a checkpoint gets the mode any new file gets)
        os.umask(umask)
        os.chmod(tmp, 0o666 & ~umask)
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except FileNotFoundError:
            pass
        raise


def load_checkpoint(path):
    """-> the state dict save_checkpoint was given, tensors on the CPU.  ValueError for a file that is no checkpoint of this
    package or whose format version this code does not know"""
    obj = torch.load(os.fspath(path), map_location="cpu", weights_only=True)
    if not isinstance(obj, dict) or obj.get("format") != FORMAT or "state" not in obj:
        raise ValueError(f"load_checkpoint: {path} is not a {FORMAT} file")
    if obj.get("version") != VERSION:
        raise ValueError(f"load_checkpoint: {path} has format version {obj.get('version')!r}; this code reads version {VERSION}")
    return obj["state"]
