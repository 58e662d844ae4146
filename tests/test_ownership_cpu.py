"""Ownership targets without a GPU: bz_ownership_row -- the function k_pack_own runs -- against a numpy
restatement, the ownership twins (the existing feature twins, keeping the final board of the game they play), the buffer layout,
and the ABI / Python validation and carrying of the two fields.  tests/test_gpu_ownership.py pins the engine to these twins."""
import ctypes as C

import numpy as np
import pytest

from betazero_amd import _lib
from oracle.py_twin import Twin
from test_forced_playouts_cpu import ForcedTwin
from test_fpu_cpu import FpuTwin
from test_gumbel_cpu import GumbelTwin
from test_gumbel_interior_cpu import GumbelFullTwin
from test_leaf_parallel_cpu import KTwin
from test_playout_cap_cpu import CapTwin, _cfg, boards

M64 = (1 << 64) - 1


# ---------------------------------------------------------------- restatements
def ownership_row(fin_x, fin_o, mover):
    """the final board in the mover's frame, arrays at once"""
    fin_x, fin_o, mover = np.asarray(fin_x, np.uint64), np.asarray(fin_o, np.uint64), np.asarray(mover)
    return np.where(mover == 1, fin_x, fin_o), np.where(mover == 1, fin_o, fin_x)


def cell_targets(t_own, t_opp):
    """the 64 cell targets of a row, int8 [n, 64]: bit_i(t_own) - bit_i(t_opp)"""
    sh = np.arange(64, dtype=np.uint64)
    a = ((np.asarray(t_own, np.uint64)[:, None] >> sh) & np.uint64(1)).astype(np.int8)
    b = ((np.asarray(t_opp, np.uint64)[:, None] >> sh) & np.uint64(1)).astype(np.int8)
    return a - b


def board_from_bits(game, fin_x, fin_o):
    """a board object of the twins' board classes holding the absolute position (fin_x, fin_o)"""
    Rev, Ttt = boards()
    if game == "ttt":
        cells = np.array([[(1 if fin_x >> (3 * r + c) & 1 else 0) - (1 if fin_o >> (3 * r + c) & 1 else 0) for c in range(3)]
                          for r in range(3)])
        return Ttt(cells)
    return Rev.from_bits(int(fin_x), int(fin_o), size={"reversi6": 6, "reversi4": 4}.get(game, 8))


def winner_of(game, fin_x, fin_o):
    """(over, winner) of the absolute position by the board classes, through the twin's own terminal()"""
    return Twin(game, "hash", boards=boards()).terminal(board_from_bits(game, fin_x, fin_o))


# ---------------------------------------------------------------- the ownership twins
class _Own:
    """mixin over a feature twin: keeps the final board of the game selfplay() plays.  Every twin's selfplay() asks
    terminal(b) about the position a move produced and returns at once when it is over; the tree's own terminal tests (new_node)
    all lie before that, so the last position terminal() found over is the game's final one."""

    def terminal(self, b):
        over, w = super().terminal(b)
        if over:
            self.final = b
        return over, w

    def final_bits(self):
        """(fin_x, fin_o): the final board in absolute colours, in the engine's bit layout"""
        return self.bits(self.final, 1)


def OwnTwin(base):
    return type("Own" + base.__name__, (_Own, base), {})


def _selfplay(kind, game, g, sims, temp_moves, openings, seed, base, noise, cap, reuse, stagger=0):
    kw = dict(boards=boards(), **(dict(dir_alpha=0.3, dir_eps=0.25) if noise else {}))
    if kind == "plain" and stagger == 0:
        tw = OwnTwin(Twin)(game, "hash", reuse=reuse, **kw)
        return tw, tw.selfplay(base + g, sims, temp_moves, openings, seed)
    if kind == "plain":  # (KTwin at K = 1 is Twin with the bench's stagger)
        tw = OwnTwin(KTwin)(game, "hash", leaves=1, reuse=reuse, **kw)
    elif kind == "k8":
        tw = OwnTwin(KTwin)(game, "hash", leaves=8, reuse=reuse, **kw)
    elif kind == "cap":
        tw = OwnTwin(CapTwin)(game, "hash", cap[0], cap[1], **kw)
    elif kind == "forced":
        tw = OwnTwin(ForcedTwin)(game, "hash", 2.0, prune=True, cap=cap, **kw)
    elif kind == "fpu":
        tw = OwnTwin(FpuTwin)(game, "hash", fpu=(0.2, 0.1), cap=cap, **kw)
    elif kind == "gfull":
        tw = OwnTwin(GumbelFullTwin)(game, "hash", interior="gumbel", **kw)
    else:
        assert kind == "gumbel", kind
        tw = OwnTwin(GumbelTwin)(game, "hash", **kw)
    return tw, tw.selfplay(base + g, sims, temp_moves, openings, seed, slot=g, stagger=stagger)


def own_games(kind, game, n, sims, temp_moves=0, openings=0, seed=0, base=0, noise=False, cap=None, reuse=False, stagger=0):
    """n games of an ownership twin: [(rows, (fin_x, fin_o), winner)].  kind: "plain" | "k8" | "cap" | "forced" | "fpu" |
    "gumbel" | "gfull"."""
    out = []
    for g in range(n):
        tw, (rows, w, _) = _selfplay(kind, game, g, sims, temp_moves, openings, seed, base, noise, cap, reuse, stagger)
        out.append((rows, tw.final_bits(), w))
    return out


def after_last_row(game, row):
    """apply(last row's own, opp, act) in absolute colours, through the board classes"""
    own, opp, _, mover, act = row
    tw = Twin(game, "hash", boards=boards())
    x, o = (own, opp) if mover == 1 else (opp, own)
    return tw.bits(tw.play(board_from_bits(game, x, o), mover, act), 1)


# ---------------------------------------------------------------- bz_ownership_row
def _c_row(fin_x, fin_o, mover):
    a, b = C.c_uint64(7), C.c_uint64(7)
    assert _lib.lib().bz_ownership_row(int(fin_x), int(fin_o), int(mover), C.addressof(a), C.addressof(b)) == 0, _lib.lib().bz_last_error()
    return a.value, b.value


def test_ownership_row_equals_the_restatement_on_random_boards_both_movers_and_empty_boards():
    rng = np.random.default_rng(0)
    x = rng.integers(0, 1 << 63, 2000, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 2000, dtype=np.uint64)
    o = (rng.integers(0, 1 << 63, 2000, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 2000, dtype=np.uint64)) & ~x
    x[:8] = [0, 0, M64, 0, 1, 1 << 63, 0x0F0F0F0F, 0]
    o[:8] = [0, M64, 0, 1, 0, 0, 0xF0F0F0F0, 1 << 63]
    mover = np.where(rng.random(2000) < 0.5, 1, -1)
    want_own, want_opp = ownership_row(x, o, mover)
    for i in range(2000):
        assert _c_row(x[i], o[i], mover[i]) == (int(want_own[i]), int(want_opp[i])), i
        assert _c_row(x[i], o[i], -mover[i]) == (int(want_opp[i]), int(want_own[i])), i  # the other mover: the boards swap
    t = cell_targets(want_own, want_opp)
    assert set(np.unique(t)) == {-1, 0, 1}
    assert (t[0] == 0).all() and (t[1] == -mover[1]).all() and (t[2] == mover[2]).all()  # empty board: every cell 0
    assert np.array_equal(t.sum(1), [bin(int(a)).count("1") - bin(int(b)).count("1") for a, b in zip(want_own, want_opp)])
    # a 4x4 corner position: the cells outside the board are 0
    corner = cell_targets(*ownership_row([0x0F0F0000], [0x00000F0F], [-1]))[0]
    assert (corner[[8 * r + c for r in range(8) for c in range(8) if r >= 4 or c >= 4]] == 0).all() and (corner[:4] == 1).all()


def test_ownership_row_refuses_bad_arguments_with_a_message():
    L = _lib.lib()
    a, b = C.c_uint64(), C.c_uint64()
    for args in ((1, 2, 1, None, C.addressof(b)), (1, 2, 1, C.addressof(a), None), (1, 2, 0, C.addressof(a), C.addressof(b)),
                 (1, 2, 2, C.addressof(a), C.addressof(b))):
        assert L.bz_ownership_row(*args) == _lib.BZ_EINVAL and b"bz_ownership_row" in L.bz_last_error()


# ---------------------------------------------------------------- the twins
CASES = [("plain", {}), ("plain", dict(noise=True, reuse=True)), ("cap", dict(noise=True, cap=(4, 32768))),
         ("forced", dict(noise=True, cap=(4, 32768))), ("forced", dict(noise=True)), ("gumbel", dict(temp_moves=3)),
         ("gfull", dict(temp_moves=3)), ("fpu", dict(noise=True)), ("k8", dict(noise=True)), ("plain", dict(stagger=3))]


@pytest.mark.parametrize("kind,kw", CASES)
@pytest.mark.parametrize("game", ["ttt", "reversi4"])
def test_twin_final_boards_give_the_twins_winner_and_follow_the_last_row(game, kind, kw):
    sims = 24 if game == "ttt" else 16
    games = own_games(kind, game, 6, sims, seed=3, base=2, **dict(dict(temp_moves=2), **kw))
    capped = kw.get("cap") is not None
    followed = 0
    for rows, (fx, fo), w in games:
        assert fx & fo == 0 and (fx | fo) != 0
        over, won = winner_of(game, fx, fo)
        assert over and won == w, (game, kind, fx, fo, won, w)
        if game != "ttt":
            d = bin(fx).count("1") - bin(fo).count("1")
            assert w == (d > 0) - (d < 0) and (fx | fo) & ~0x0F0F0F0F == 0
        if not capped:
            assert after_last_row(game, rows[-1]) == (fx, fo)
            followed += 1
        elif rows and after_last_row(game, rows[-1]) == (fx, fo):
            followed += 1
    # under the cap the last move is often not recorded: the final board cannot be rebuilt from the rows
    assert followed == 6 or (capped and followed < 6), (kind, followed)


def test_twin_final_board_of_a_game_without_rows_and_of_reversi6():
    rows, (fx, fo), w = own_games("cap", "reversi4", 1, 16, seed=1, cap=(4, 0))[0]  # every search fast: no row at all
    assert rows == [] and winner_of("reversi4", fx, fo) == (True, w)
    rows, (fx, fo), w = own_games("plain", "reversi6", 1, 8, seed=1)[0]
    assert winner_of("reversi6", fx, fo) == (True, w) and after_last_row("reversi6", rows[-1]) == (fx, fo)
    assert (fx | fo) & ~0x00003F3F3F3F3F3F == 0


# ---------------------------------------------------------------- buffer size, ABI and Python validation
def test_ownership_bytes_is_the_stated_layout_and_the_abi_refuses_bad_arguments():
    L = _lib.lib()
    al = lambda x: (x + 255) // 256 * 256  # noqa: E731
    for game in (0, 1, 2, 3):
        na = 9 if game == 0 else 65
        for B in (1, 4, 33, 64, 4096):
            for rounds in (1, 3):
                cfg = _cfg(game, B, 8)
                cfg.rounds, cfg.t_max = rounds, 9 if game == 0 else 64
                want = 2 * al(rounds * B * 8) + al(B * na * 4) + al(B * 4)  # fin_x, fin_o, the scratch pi and act
                assert L.bz_engine_ownership_bytes(C.byref(cfg)) == want, (game, B, rounds)
    # nothing the engine accepts is refused: subtree reuse, K > 1, the caches
    for cfg in (_cfg(flags=_lib.ENGINE_REUSE_SUBTREE), _cfg(K=8), _cfg(flags=_lib.ENGINE_EVAL_CACHE | _lib.ENGINE_EVAL_CACHE_CARRY)):
        assert L.bz_engine_ownership_bytes(C.byref(cfg)) > 0
    assert L.bz_engine_ownership_bytes(None) == -1 and b"bz_engine_ownership_bytes" in L.bz_last_error()
    assert L.bz_engine_ownership_bytes(C.byref(_cfg(sims=9000))) == -1
    assert L.bz_engine_set_ownership(None, None, 0, None) == _lib.BZ_EINVAL and b"bz_engine_set_ownership" in L.bz_last_error()
    assert L.bz_engine_pack_ownership(None, None, None, 1, 0, None) == _lib.BZ_EINVAL and b"bz_engine_pack_ownership" in L.bz_last_error()
    assert L.bz_abi_version() == 7


def _examples(n, seed=0, own=False, **have):
    from betazero_amd.engine import Examples
    g = np.random.default_rng(seed)
    extra = {f: g.random(n).astype(np.float32) for f in ("kl", "q", "vt") if have.get(f)}
    if own:
        extra["fown"] = g.integers(0, 1 << 63, n, dtype=np.uint64) | np.uint64(1 << 63)  # (bit 63 set: the sign bit of the int64 view)
        extra["fopp"] = g.integers(0, 1 << 63, n, dtype=np.uint64) & ~extra["fown"]
    return Examples(g.integers(0, 2 ** 62, n).astype(np.uint64), g.integers(0, 2 ** 62, n).astype(np.uint64),
                    g.random((n, 65)).astype(np.float32), g.integers(-1, 2, n).astype(np.int8), np.ones(n, np.int8),
                    np.zeros(n, np.uint8), np.arange(n), np.zeros(n, np.int32), 8, **extra)


def test_examples_carry_the_ownership_fields_through_concat_select_and_the_host_round_trip():
    import torch
    from betazero_amd.engine import DeviceExamples, Examples, concat_device_examples, concat_examples
    from betazero_amd.train import select_rows
    a, b, bare, with_vt = _examples(5, 1, own=True), _examples(3, 2, own=True), _examples(4, 3), _examples(4, 4, own=True, q=True, vt=True)
    # the two fields are the last ones, after vt, and default to None: positional constructions keep working
    first = ("own", "opp", "pi", "z", "mover", "act", "game", "ply", "size")
    pos = Examples(*[getattr(bare, f) for f in first])
    assert pos.vt is None and pos.fown is None and pos.fopp is None
    pos = Examples(*[getattr(with_vt, f) for f in first + ("kl", "q", "vt", "fown", "fopp")])
    assert pos.vt is with_vt.vt and pos.fown is with_vt.fown and pos.fopp is with_vt.fopp
    ab = concat_examples([a, b])
    assert np.array_equal(ab.fown, np.concatenate([a.fown, b.fown])) and np.array_equal(ab.fopp, np.concatenate([a.fopp, b.fopp]))
    assert ab.fown.dtype == np.uint64 and ab.q is None and concat_examples([bare, bare]).fown is None
    half = _examples(4, 5, own=True)
    half.fopp = None
    for parts, field in (([a, bare], "fown"), ([bare, a], "fown"), ([a, half], "fopp")):  # a mixture raises, per field
        with pytest.raises(ValueError, match=rf"carry {field} "):
            concat_examples(parts)
    da, db, dbare = (DeviceExamples.from_host(x, "cpu") for x in (a, b, bare))
    assert da.fown.dtype == torch.int64 and da.fopp.dtype == torch.int64 and dbare.fown is None and dbare.fopp is None
    assert np.array_equal(da.fown.numpy().view(np.uint64), a.fown) and (da.fown < 0).all()  # the bit patterns, bit 63 included
    dab = concat_device_examples([da, db])
    assert np.array_equal(dab.fown.numpy().view(np.uint64), ab.fown) and np.array_equal(dab.fopp.numpy().view(np.uint64), ab.fopp)
    with pytest.raises(ValueError, match=r"carry fown "):
        concat_device_examples([dbare, da])
    idx = torch.tensor([7, 0, 0, 3])
    sel = select_rows(dab, idx)
    assert np.array_equal(sel.fown.numpy().view(np.uint64), ab.fown[[7, 0, 0, 3]])
    assert np.array_equal(sel.fopp.numpy().view(np.uint64), ab.fopp[[7, 0, 0, 3]]) and sel.q is None
    assert select_rows(dbare, torch.tensor([1])).fown is None
    back = dab.cpu()
    assert back.fown.dtype == np.uint64 and np.array_equal(back.fown, ab.fown) and np.array_equal(back.fopp, ab.fopp)
    assert dbare.cpu().fown is None and DeviceExamples.from_host(with_vt, "cpu").cpu().vt is not None


def test_python_refuses_an_ownership_that_is_no_bool_before_touching_a_device(monkeypatch):
    from betazero_amd import engine

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(_lib, "require_gpu", no_device)
    monkeypatch.setattr(_lib, "lib", no_device)
    for bad in (1, "yes", None, 0.5):
        with pytest.raises(ValueError, match="ownership"):
            engine.SelfPlayEngine("reversi", 4, 8, ownership=bad)
        with pytest.raises(ValueError, match="ownership"):
            engine.PipelinedSelfPlay("reversi", 4, 8, pipelines=1, streams=[None], ownership=bad)
        with pytest.raises(ValueError, match="ownership"):
            engine.self_play("reversi", 4, 8, ownership=bad)
    assert engine.check_ownership(True) is True and engine.check_ownership(np.bool_(False)) is False


def test_the_training_entry_points_refuse_a_bad_own_weight_and_missing_fields_before_touching_a_device(monkeypatch):
    import ctypes
    from betazero_amd.engine import DeviceExamples
    from betazero_amd.net import OwnershipHead, PolicyValueNet
    from betazero_amd.train import GraphedTrainStep, train_step
    from betazero_amd.train_kernels import StepPlan, check_own_weight
    L = _lib.lib()
    # the ABI's own refusals come before a launch (this host has no GPU to launch on)
    assert L.bz_train_heads_own(None, None, None, 64, 64, 64, None, None, None, None, None, None, None) == _lib.BZ_EINVAL
    assert b"bz_train_heads_own" in L.bz_last_error()
    assert L.bz_train_heads_own_vt(None, None, None, None, 64, 64, 64, None, None, None, None, None, None, None) == _lib.BZ_EINVAL
    assert b"bz_train_heads_own_vt" in L.bz_last_error()
    a = np.zeros(4, np.int64)
    p = a.ctypes.data
    hp = _lib.TrainHeadParams(*([p] * 10))
    for own in (None, _lib.TrainOwn(w=p, b=p, targets=None, weight=1.0, partial=p), _lib.TrainOwn(w=p, b=p, targets=p, weight=-1.0, partial=p),
                _lib.TrainOwn(w=p, b=p, targets=p, weight=float("nan"), partial=p), _lib.TrainOwn(w=p, b=p, targets=p, weight=float("inf"), partial=p)):
        ref = ctypes.byref(own) if own is not None else None
        assert L.bz_train_heads_own(p, p, ref, 64, 64, 64, ctypes.byref(hp), p, p, p, p, p, None) == _lib.BZ_EINVAL
        assert b"own" in L.bz_last_error()
    assert L.bz_train_own_finish(None, 64, 64, p, p, p, None, None, None) == _lib.BZ_EINVAL and b"bz_train_own_finish" in L.bz_last_error()
    ok = _lib.TrainOwn(w=p, b=p, targets=p, weight=1.0, partial=p)
    assert L.bz_train_own_finish(ctypes.byref(ok), 96, 64, p, p, p, None, None, None) == _lib.BZ_EINVAL     # width
    bad = _lib.TrainOwnAdam(hyper=p, beta1=0.9, beta2=0.999, eps=0.0, pw=p, pb=p, mw=p, mb=p, vw=p, vb=p)
    assert L.bz_train_own_finish(ctypes.byref(ok), 64, 64, p, p, p, None, ctypes.byref(bad), None) == _lib.BZ_EINVAL and b"eps" in L.bz_last_error()
    assert ctypes.sizeof(_lib.TrainBatch) == 48 and L.bz_abi_version() == 7

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(_lib, "require_gpu", no_device)
    monkeypatch.setattr(_lib, "lib", no_device)
    for bad in (-0.5, float("nan"), float("inf"), "1", None, True):
        with pytest.raises(ValueError, match="own_weight"):
            check_own_weight(bad)
        with pytest.raises(ValueError, match="own_weight"):
            StepPlan(None, 8, own_weight=bad)
        with pytest.raises(ValueError, match="own_weight"):
            GraphedTrainStep(None, batch=8, own_weight=bad)
        with pytest.raises(ValueError, match="own_weight"):
            train_step(None, None, None, own_weight=bad)
    assert check_own_weight(0) == 0.0 and check_own_weight(2.5) == 2.5
    head = OwnershipHead(64)
    ex = DeviceExamples.from_host(_examples(4), "cpu")
    with pytest.raises(ValueError, match="fown"):
        train_step(None, None, ex, ownership=head)
    with pytest.raises(ValueError, match="all-kernel step"):
        GraphedTrainStep(PolicyValueNet(64, 1, 64), batch=8, ownership=head)
    with pytest.raises(ValueError, match="OwnershipHead"):
        StepPlan(PolicyValueNet(64, 1, 64, fused_tower=True), 8, ownership=OwnershipHead(128))
    # the head is a module of its own: C + 1 parameters, none of them in the net's flat parameter block
    assert sum(p.numel() for p in head.parameters()) == 65 and not any("own" in k for k in PolicyValueNet(64, 1, 64).state_dict())
    import torch
    x = torch.randn(3, 64, 8, 8)
    o = head(x)
    assert o.shape == (3, 64) and float(o.abs().max()) < 1 and torch.allclose(o, torch.tanh(head.conv(x)).flatten(1))
    m = PolicyValueNet(64, 1, 64)
    planes = torch.zeros(2, 2, 8, 8)
    lg, v, trunk = m(planes, trunk=True)
    lg2, v2 = m(planes)
    assert trunk.shape == (2, 64, 8, 8) and torch.equal(lg, lg2) and torch.equal(v, v2)
