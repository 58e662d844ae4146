"""The training step's five options in combination, the parts that need no GPU: the enumeration of the option
lattice that tests/test_gpu_step_options.py walks, and the torch statement of the all-on step -- train_step(value_targets=,
ownership=, fp8_qat=, sym=), the GPU file's reference -- held to the same lattice on the CPU: with one option neutralised it is
the step without that option.  A reference that broke one of these relations could hide a kernel that broke it the same way.

    V  value_targets=True           neutral input: vt = z as floats
    O  ownership=OwnershipHead      neutral input: own_weight = 0
    Q  fp8_qat=True                 no neutral input (128 channels only)
    S  symmetry=True / sym=         neutral input: the rows transformed beforehand (the twin), every symmetry 0
    X  the extended optimiser       neutral input: every optimiser option off (the optimiser is outside train_step)"""
import copy
import itertools

import numpy as np
import torch

OPTIONS = "VOQSX"
NEUTRAL = "VOSX"                                    # the options an edge can switch off through their input
SHAPES = {128: (128, 1, 64, 8), 64: (64, 1, 24, 8)}   # C: (C, blocks, VH, batch) -- the smallest batch a plan takes at either width


def subsets(C):
    """every subset of the options a plan of C channels can be built with, as strings in OPTIONS' order ('' is the plain step)"""
    pool = OPTIONS if C == 128 else OPTIONS.replace("Q", "")
    return ["".join(c) for k in range(len(pool) + 1) for c in itertools.combinations(pool, k)]


def edges(C):
    """(T, o): a subset and one of its options that has a neutral input -- plan(T) fed that input is plan(T minus o)"""
    return [(T, o) for T in subsets(C) for o in T if o in NEUTRAL]


def without(T, o):
    return T.replace(o, "")


# ---------------------------------------------------------------- the enumeration
def test_the_lattice_has_32_and_16_subsets_and_64_and_32_edges():
    for C, n_sub, n_edge in ((128, 32, 64), (64, 16, 32)):
        S, E = subsets(C), edges(C)
        assert len(S) == len(set(S)) == n_sub and len(E) == len(set(E)) == n_edge
        assert all("".join(sorted(T, key=OPTIONS.index)) == T and set(T) <= set(OPTIONS) for T in S)
        assert all(o in T and o != "Q" and without(T, o) in S for T, o in E)
        assert {without(T, o) for T, o in E} | {T for T, _ in E} == set(S)
        # every subset is joined to '' or 'Q' by a chain of edges: the two plans the single-option suites hold to references
        reach = {"", "Q"} & set(S)
        for _ in range(len(OPTIONS)):
            reach |= {T for T, o in E if without(T, o) in reach}
        assert reach == set(S)
    assert not any("Q" in T for T in subsets(64)) and sum("Q" in T for T in subsets(128)) == 16
    assert OPTIONS in subsets(128) and "" in subsets(64)
    assert all(sum(o == x for _, o in edges(C)) == n for C, n in ((128, 16), (64, 8)) for x in NEUTRAL)


# ---------------------------------------------------------------- the torch reference obeys the lattice
def _case():
    """a 128 x 1 net, an ownership head and 3 n + 5 rows with every column, all on the CPU; row numbers with repeats and all
    eight symmetries; the twin: the same rows transformed on the host"""
    from betazero_amd.examples import DeviceExamples
    from betazero_amd.net import OwnershipHead, PolicyValueNet
    from test_gpu_train_symmetry import _draw, _examples, _twin
    C, NB, VH, n = SHAPES[128]
    torch.manual_seed(3)
    net, head = PolicyValueNet(C, NB, VH, fused_tower=True), OwnershipHead(C)
    with torch.no_grad():
        for p in net.parameters():
            if p.dim() == 1:
                p.normal_(0.0, 0.2)
        head.conv.weight.mul_(3.0)
    ex = _examples(3 * n + 5, 8, 77, vt=True, own=True, payloads=False)
    idx, sym = _draw(len(ex), n, 78)
    host = lambda e: DeviceExamples.from_host(e, "cpu")  # noqa: E731
    return net, head, host(ex), host(_twin(ex, idx, sym)), torch.as_tensor(idx), torch.as_tensor(sym)


def _run(net, head, ex, idx=None, sym=None, value_targets=True, own_weight=0.5):
    """train_step with an optimiser that moves nothing, on copies: (losses, {name: gradient}) of the net and of the head"""
    from betazero_amd.train import train_step
    net, head = copy.deepcopy(net), copy.deepcopy(head) if head is not None else None
    params = list(net.parameters()) + (list(head.parameters()) if head is not None else [])
    kw = dict(ownership=head, own_weight=own_weight) if head is not None else {}
    losses = train_step(net, torch.optim.SGD(params, lr=0.0), ex, idx, value_targets=value_targets, fp8_qat=True, sym=sym, **kw)
    grads = {k: p.grad.clone() for k, p in net.named_parameters()}
    if head is not None:
        grads.update({"own." + k: p.grad.clone() for k, p in head.named_parameters()})
    assert all(bool(torch.isfinite(g).all()) for g in grads.values()) and float(grads["tower_w"].abs().max()) > 0
    return torch.stack(losses), grads


def _close(a, b, names, what):
    assert torch.allclose(a[0][:3], b[0][:3]), (what, a[0], b[0])
    for k in names:
        assert torch.allclose(a[1][k], b[1][k]), (what, k, float((a[1][k] - b[1][k]).abs().max()))


def test_the_all_on_torch_step_with_one_option_neutralised_is_the_step_without_it():
    """all four options train_step knows (V, O, Q, S) on, each of V, O, S neutralised in turn: losses and gradients equal those of
    the call without that option, to torch.allclose's default tolerances.  fp8_qat's forward uses no autocast, so this runs where
    train_step does -- on the CPU"""
    net, head, ex, tw, idx, sym = _case()
    trunk = [k for k, _ in net.named_parameters()]
    everything = trunk + ["own.conv.weight", "own.conv.bias"]
    all_on = _run(net, head, ex, idx, sym)
    assert all_on[0].shape == (4,) and float(all_on[0][3]) > 0.1
    assert abs(float(all_on[0][0]) - float(all_on[0][1] + all_on[0][2] + 0.5 * all_on[0][3])) < 1e-5
    # S: (idx, sym) on the data set against no symmetry on the rows the twin transformed on the host
    on_twin = _run(net, head, tw)
    _close(all_on, on_twin, everything, "S")
    assert torch.allclose(all_on[0][3], on_twin[0][3])
    plain_rows = _run(net, head, ex, idx)          # (the symmetries are not all the identity: the untransformed rows differ)
    assert not torch.allclose(all_on[1]["tower_w"], plain_rows[1]["tower_w"])
    # V: vt = z as floats against the outcome itself
    z_as_vt = copy.copy(ex)
    z_as_vt.vt = ex.z.to(torch.float32)
    _close(_run(net, head, z_as_vt, idx, sym), _run(net, head, ex, idx, sym, value_targets=False), everything, "V")
    assert not torch.allclose(all_on[0][2], _run(net, head, ex, idx, sym, value_targets=False)[0][2])
    # O: own_weight = 0 against no head at all -- everything the net owns; the head receives no gradient
    zero = _run(net, head, ex, idx, sym, own_weight=0.0)
    _close(zero, _run(net, None, ex, idx, sym), trunk, "O")
    assert not zero[1]["own.conv.weight"].any() and not zero[1]["own.conv.bias"].any()
    assert torch.allclose(zero[0][3], all_on[0][3]) and not torch.allclose(zero[1]["tower_w"], all_on[1]["tower_w"])


def test_the_twin_holds_the_rows_the_torch_path_transforms():
    """torch_sym_rows on the gathered rows (train_step's path) gives the twin's boards, policies and ownership targets, bit for bit"""
    from betazero_amd.train_symmetry import torch_sym_rows
    _, _, ex, tw, idx, sym = _case()
    got = torch_sym_rows(ex.own[idx], ex.opp[idx], ex.pi[idx], sym, 8, ex.fown[idx], ex.fopp[idx])
    for g, w in zip(got, (tw.own, tw.opp, tw.pi, tw.fown, tw.fopp)):
        assert np.array_equal(g.numpy().view(np.uint8), w.numpy().view(np.uint8))
    assert torch.equal(ex.vt[idx], tw.vt) and torch.equal(ex.z[idx], tw.z) and len(set(sym.tolist())) == 8
