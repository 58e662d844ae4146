"""Checkpoints on the GPU: the fused step's state_dict / load_state_dict continue a run bit for bit and keep a
captured graph, a state that does not fit is refused with every tensor untouched, tools/az_loop.py resumed from a checkpoint is
the uninterrupted run, and --init-net plays the saved net.  "Equal" = bit for bit."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, BATCH = 320, 64
NAMES = ("stem_w", "stem_b", "tower_w", "tower_b", "pol_w", "pol_b", "polfc_w", "polfc_b", "val_w", "val_b", "v1_w", "v1_b", "v2_w", "v2_b")
# the extended optimiser with everything on: decay, a clip far below the gradient norm of a fresh net (so that it fires), EMA
EXTENDED = dict(weight_decay=1e-2, clip_norm=0.05, ema_decay=0.9)


def _bits(t):
    return t.detach().reshape(-1).contiguous().view(torch.int32).cpu()


@pytest.fixture(scope="module")
def data():
    """a fixed synthetic data set with every column a step may read, and the row numbers of six batches"""
    rng = np.random.default_rng(11)
    u64 = lambda: rng.integers(0, 2**63, ROWS, dtype=np.int64).astype(np.uint64) | (rng.integers(0, 2, ROWS).astype(np.uint64) << np.uint64(63))  # noqa: E731
    own = u64()
    opp = u64() & ~own
    fown = u64()
    fopp = u64() & ~fown
    pi = rng.random((ROWS, 65)).astype(np.float32) ** 4
    pi /= pi.sum(1, keepdims=True)
    t = lambda a: torch.as_tensor(a).to(DEV)  # noqa: E731
    ex = types.SimpleNamespace(own=t(own.view(np.int64)), opp=t(opp.view(np.int64)), pi=t(pi), z=t(rng.integers(-1, 2, ROWS).astype(np.int8)),
                               vt=t((rng.random(ROWS) * 2 - 1).astype(np.float32)), fown=t(fown.view(np.int64)), fopp=t(fopp.view(np.int64)))
    idxs = [t(rng.integers(0, ROWS, BATCH).astype(np.int64)) for _ in range(6)]
    return ex, idxs


def _step(seed, C=64, NB=1, VH=24, extended=False, ema=True, ownership=False, value_targets=False, fp8_qat=False):
    from betazero_amd.net import OwnershipHead, PolicyValueNet
    from betazero_amd.train import GraphedTrainStep
    torch.manual_seed(seed)
    module = PolicyValueNet(C, NB, VH, fused_tower=True)
    head = OwnershipHead(C) if ownership else None
    opts = {**EXTENDED, **({} if ema else {"ema_decay": None})} if extended else {}
    return GraphedTrainStep(module, lr=2e-3, batch=BATCH, lr_warmup_steps=4, value_targets=value_targets, ownership=head,
                            fp8_qat=fp8_qat, **opts)


def _tensors(step):
    """every tensor of the step that lives from one replay to the next, named here and not by the code under test"""
    sp = step.step_plan
    out = {f"p.{k}": sp.params[k] for k in NAMES}
    out.update({f"m.{k}": sp.adam_m[k] for k in NAMES})
    out.update({f"v.{k}": sp.adam_v[k] for k in NAMES})
    out["hyper"] = sp.hyper
    if sp.stats is not None:
        out["stats"] = sp.stats
    if sp.ema is not None:
        out.update({f"ema.{k}": sp.ema[k] for k in NAMES})
    if step.ownership is not None:
        for k in ("w", "b"):
            out[f"own.{k}"], out[f"own_m.{k}"], out[f"own_v.{k}"] = sp.own_params[k], sp.own_m[k], sp.own_v[k]
    return out


def _snapshot(step):
    torch.cuda.synchronize()
    return {k: _bits(t) for k, t in _tensors(step).items()}


def _run(step, ex, idxs):
    return torch.stack([step(ex, i) for i in idxs]).cpu()


CONFIGS = {"plain": dict(), "extended_ownership_vt": dict(extended=True, ownership=True, value_targets=True)}


# ---------------------------------------------------------------- (a) the step's state
@pytest.fixture(scope="module", params=list(CONFIGS))
def continued(request, data, tmp_path_factory):
    """three replays, the state, then two more: (config, the state as it comes back from a checkpoint FILE, the two replays' losses,
    every state tensor's bits after them, the step's host-side lr)"""
    from betazero_amd.checkpoint import load_checkpoint, save_checkpoint
    ex, idxs = data
    cfg = CONFIGS[request.param]
    step = _step(1, **cfg)
    _run(step, ex, idxs[:2])
    step.set_lr(1.5e-3)            # a decayed rate: lives in the hyper block and on the host
    _run(step, ex, idxs[2:3])
    sd = step.state_dict()
    for k, v in sd.items():
        assert (torch.is_tensor(v) and v.device.type == "cpu") or isinstance(v, (bool, int, float)), k
    assert (sd["C"], sd["blocks"], sd["VH"], sd["batch"], sd["steps_done"], sd["lr"], sd["warmup"]) == (64, 1, 24, BATCH, 3, 1.5e-3, 4)
    assert sd["extended"] == sd["has_ema"] == sd["has_ownership"] == bool(cfg) and sd["fp8_qat"] is False
    assert sd["hyper"].numel() == (8 if cfg else 4) and float(sd["hyper"][1]) == 3.0    # the device step counter
    if cfg:
        assert float(sd["stats"][3]) > 0    # the clip fired
    path = str(tmp_path_factory.mktemp("state") / "step.ckpt")
    save_checkpoint(path, {"step": sd})
    before = _snapshot(step)
    losses = _run(step, ex, idxs[3:5])
    after = _snapshot(step)
    assert all(not torch.equal(before[k], after[k]) for k in ("p.tower_w", "m.tower_w", "v.tower_w", "hyper"))   # it does train
    return cfg, load_checkpoint(path)["step"], losses, after, step.lr


@pytest.mark.parametrize("captured", [True, False])
def test_loaded_state_continues_bit_for_bit_and_keeps_the_graph(continued, data, captured):
    """a second step from a differently seeded module -- with its graph captured and its state dirty, or before its first call --
    loads the state and replays the same two batches: losses and every state tensor equal the first step's, and the graph is
    the one it captured before the load"""
    ex, idxs = data
    cfg, sd, losses, after, lr = continued
    step = _step(2, **cfg)
    graph = None
    if captured:
        _run(step, ex, idxs[5:6])
        graph = step.graph
        assert graph is not None
    step.load_state_dict(sd)
    got = _run(step, ex, idxs[3:5])
    assert step.graph is graph or not captured
    assert step.steps_done == 5 and step.lr == lr == step.step_plan.lr
    assert torch.equal(_bits(got), _bits(losses))
    snap = _snapshot(step)
    assert sorted(snap) == sorted(after)
    for k in after:
        assert torch.equal(snap[k], after[k]), k
    assert step.step_plan.adam_t == 5


# ---------------------------------------------------------------- (b) refused loads
MISMATCHES = {   # name: (the saved step, the loading step, the word the error names)
    "C": (dict(C=128), dict(), "C differs"),
    "blocks": (dict(NB=2), dict(), "blocks differs"),
    "VH": (dict(VH=32), dict(), "VH differs"),
    "plain_into_extended": (dict(), dict(extended=True), "extended differs"),
    "extended_into_plain": (dict(extended=True), dict(), "extended differs"),
    "ema_saved_only": (dict(extended=True), dict(extended=True, ema=False), "has_ema differs"),
    "ema_loading_only": (dict(extended=True, ema=False), dict(extended=True), "has_ema differs"),
    "ownership_saved_only": (dict(ownership=True), dict(), "has_ownership differs"),
    "ownership_loading_only": (dict(), dict(ownership=True), "has_ownership differs"),
    "fp8_qat": (dict(C=128), dict(C=128, fp8_qat=True), "fp8_qat differs"),
}


@pytest.mark.parametrize("name", list(MISMATCHES))
def test_state_that_does_not_fit_is_refused_and_nothing_is_written(data, name):
    ex, idxs = data
    saved, loading, words = MISMATCHES[name]
    sd = _step(3, **saved).state_dict()
    step = _step(4, **loading)
    _run(step, ex, idxs[:1])    # captured and dirty
    graph, before, done = step.graph, _snapshot(step), step.steps_done
    with pytest.raises(ValueError, match=words):
        step.load_state_dict(sd)
    with pytest.raises(ValueError, match=words):
        step.step_plan.load_state_dict(sd)
    after = _snapshot(step)
    assert step.graph is graph and step.steps_done == done and all(torch.equal(before[k], after[k]) for k in before)


def test_state_with_a_tensor_of_another_shape_is_refused_before_any_write(data):
    """the description agrees but a late tensor does not (a truncated file, say): nothing before it was written either"""
    ex, idxs = data
    sd = _step(3).state_dict()
    sd["adam_v.v2_b"] = torch.zeros(2)
    step = _step(4)
    _run(step, ex, idxs[:1])
    before = _snapshot(step)
    with pytest.raises(ValueError, match="adam_v.v2_b"):
        step.load_state_dict(sd)
    after = _snapshot(step)
    assert all(torch.equal(before[k], after[k]) for k in before)


# ---------------------------------------------------------------- (c), (d) the loop
SMALL = ["--games", "64", "--sims", "16", "--channels", "64", "--blocks", "1", "--arena-games", "16", "--arena-sims", "8", "--depth", "1",
         "--final-depths", "", "--batch", "64"]
TIMING = ("seconds", "self_play_s", "games_per_s", "train_s")


def _loop(*flags):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "az_loop.py"), *SMALL, *flags], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    return [json.loads(line) for line in out.stdout.splitlines() if line.startswith("{")]


def _untimed(d):
    if isinstance(d, dict):
        return {k: _untimed(v) for k, v in d.items() if k not in TIMING}
    return [_untimed(v) for v in d] if isinstance(d, list) else d


EVERYTHING = ["--ema-decay", "0.99", "--weight-decay", "1e-4", "--clip-norm", "1", "--lr-decay", "0.9", "--ownership",
              "--value-lambda", "0.9", "--surprise", "--gate-games", "16"]
# name: (flags, iterations before the checkpoint, iterations in all).  The third case stops where the gate has just REJECTED the
# candidate (iteration 1 of this configuration scores 0.19), so the net self-play resumes with is not the trained one
OPTIONS = {"defaults": ([], 2, 4), "everything": (EVERYTHING, 2, 4), "everything_after_a_rejection": (EVERYTHING, 1, 3)}


@pytest.mark.parametrize("options", list(OPTIONS))
def test_az_loop_resumed_from_a_checkpoint_is_the_uninterrupted_run(tmp_path, options):
    """four iterations in one process against two, a checkpoint, and two more in a second process: the same lines (timings
    apart), the same weights_hash per iteration, the same bytes in the saved net"""
    flags, split, total = OPTIONS[options]
    split, total = str(split), str(total)
    a, b = tmp_path / "a", tmp_path / "b"   # (the saved nets share their file name: torch.save writes it into the archive)
    a.mkdir(), b.mkdir()
    whole = _loop(*flags, "--iters", total, "--checkpoint", str(a / "run.ckpt"), "--save-net", str(a / "net.pt"))
    first = _loop(*flags, "--iters", split, "--checkpoint", str(b / "run.ckpt"))
    second = _loop(*flags, "--iters", total, "--resume", str(b / "run.ckpt"), "--checkpoint", str(b / "run.ckpt"), "--save-net", str(b / "net.pt"),
                   "--out", str(b / "out.json"))
    its = lambda lines: [d for d in lines if d.get("what") == "iteration"]  # noqa: E731
    n, k = int(total), int(split)
    assert [d["iter"] for d in its(whole)] == list(range(1, n + 1)) and [d["iter"] for d in its(first)] == list(range(1, k + 1))
    assert [d["iter"] for d in its(second)] == list(range(k + 1, n + 1))
    if options == "everything_after_a_rejection":
        assert its(first)[-1]["gate"]["promoted"] is False
    for x, y in zip(its(whole), its(first) + its(second)):
        assert x["weights_hash"] == y["weights_hash"] and len(x["weights_hash"]) == 16, (x["iter"], x["weights_hash"], y["weights_hash"])
        assert _untimed(x) == _untimed(y), x["iter"]
    assert len({d["weights_hash"] for d in its(whole)}) == n
    assert _untimed(whole) == _untimed(first + its(second))
    assert _untimed(json.load(open(b / "out.json"))["lines"]) == _untimed(whole)   # the resumed run's record is the whole run's
    assert open(a / "net.pt", "rb").read() == open(b / "net.pt", "rb").read()
    assert sorted(os.listdir(a)) == ["net.pt", "run.ckpt"] and sorted(os.listdir(b)) == ["net.pt", "out.json", "run.ckpt"]


def test_az_loop_init_net_plays_the_saved_net(tmp_path):
    """a run's saved net, loaded by a second run of the same seed with no iteration: its "untrained net" arena is the first
    run's last arena, game for game in the counts"""
    net = str(tmp_path / "net.pt")
    last = [d for d in _loop("--iters", "1", "--save-net", net) if d.get("what") == "iteration"][-1]["arena"]
    line = [d for d in _loop("--iters", "0", "--init-net", net) if d.get("what") == "arena, untrained net"]
    assert len(line) == 1
    assert {k: line[0][k] for k in ("games", "wins", "draws", "losses")} == {k: last[k] for k in ("games", "wins", "draws", "losses")}
