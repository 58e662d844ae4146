"""The example pack kernels on the GPU -- k_pack_scan, k_pack_rows, k_pack_f32 (csrc/bz_mcts.hip) -- against pack_twin
of tests/test_pack_cpu.py, byte for byte over the WHOLE block: the header, every row, every byte the kernels must leave alone,
the pack_off they leave in the engine and the kl / q vectors.  Most blocks are synthetic: an engine that never plays, whose
example buffers (writable views) are filled from a seeded generator, at every games-per-block count around the scan's
1024-game chunk.  A few played runs close the loop with the raw unpackers."""
import numpy as np
import pytest
import torch

from betazero_amd import _lib
from betazero_amd.engine import (PipelinedSelfPlay, PlayoutCap, SelfPlayEngine, alloc_packed_block, concat_examples,
                                 packed_block_header, unpack_example_block, unpack_packed_block)
from test_pack_cpu import (FIELDS, NEVER, PACKED_MAGIC, ROW_FIELDS, direct_rows, header_words, pack_twin, poisoned, random_arrays,
                           same_rows, twin_layout)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GAMES = {"ttt": (_lib.GAME_TTT, 9, 9), "reversi": (_lib.GAME_REVERSI, 65, 64)}  # id, na, t_max
SENTINEL = 0x7FA5A5A5  # what the kl / q vectors hold before a pack (a NaN payload: compared as bits)
OFF_POISON = 0x5A5A5A5A


def _off_view(eng):
    """the engine's pack_off [rounds][B] int32.  It is engine scratch, not in bz_engine_layout: with a synthetic evaluator (no
    evaluation cache) it is the workspace's last array (carve() in csrc/bz_mcts.hip).  The tests poison this view before every
    pack, so the guess is proved first, reading only: the engine's games are packed into a scratch block and appended to it
    once more, which must leave total + (rows before each finished game) there, -1 for the unfinished ones"""
    assert eng.cfg.eval_kind in (_lib.EVAL_UNIFORM, _lib.EVAL_HASH), "pack_off is the last array only without the evaluation cache"
    n = eng.rounds * eng.B * 4
    o = eng._pad + (eng.ws.numel() - 256) - (-(-n // 256) * 256)
    view = eng.ws[o:o + n].view(torch.int32)
    lens = eng.example_tensors()["len"].cpu().numpy().reshape(-1).astype(np.int64)
    rows = np.maximum(lens, 0)
    tot = int(rows.sum())
    assert tot > 0, "the probe needs a finished game with rows"
    scratch = alloc_packed_block(eng.na, 2 * tot, eng.device)
    eng.pack_examples(scratch, 2 * tot)
    eng.pack_examples(scratch, 2 * tot, append=True)
    torch.cuda.synchronize()
    want = np.where(lens >= 0, tot + np.cumsum(rows) - rows, -1)
    assert np.array_equal(view.cpu().numpy(), want), "pack_off is not where this test expects it: the workspace layout changed"
    return view


class Played:
    """an engine after its games, with the host copies of its buffers that the twin reads"""

    def __init__(self, eng, base, stride):
        self.eng, self.base, self.stride, self.B, self.R = eng, base, stride, eng.B, eng.rounds
        self.gid, self.na, self.T, self.off_view = eng.game, eng.na, eng.t_max, _off_view(eng)
        t = {k: v.cpu().numpy() for k, v in eng.example_tensors().items()}
        self.lens, self.arrays = t["len"], {f: t[f] for f in ROW_FIELDS}
        self.arrays["kl"], self.arrays["q"] = eng.surprise_rows().cpu().numpy(), eng.search_value_rows().cpu().numpy()


class Synth:
    """an engine that is never searched or played: its example buffers are filled by the test"""

    def __init__(self, game, B, R=1, base=0, stride=None, seed=0):
        self.gid, self.na, self.T = GAMES[game]
        self.B, self.R, self.base, self.stride = B, R, base, B if stride is None else stride
        self.eng = SelfPlayEngine(game, B, 1, "hash", rounds=R, game_id_base=base, game_id_stride=stride, surprise=True,
                                  search_value=True)
        assert (self.eng.na, self.eng.t_max) == (self.na, self.T)
        self.eng.example_tensors()["len"].fill_(1)  # (one row a game for the probe of _off_view; fill() below sets the real ones)
        self.off_view = _off_view(self.eng)
        self.rng = np.random.default_rng([seed, B, R, self.na])
        self.rows = random_arrays(self.rng, R, B, self.T, self.na)
        self.fill(np.full((R, B), -1))

    def fill(self, lens):
        """these lens (never above t_max: the kernels trust them), the random rows below them, poison at and above them"""
        lens = np.asarray(lens, np.int32).reshape(self.R, self.B)
        assert lens.min() >= -1 and lens.max() <= self.T
        self.lens, self.arrays = lens, poisoned(self.rows, lens)
        t = self.eng.example_tensors()
        for f in ROW_FIELDS:
            t[f].copy_(torch.from_numpy(self.arrays[f]))
        t["len"].copy_(torch.from_numpy(lens))
        self.eng.surprise_rows().copy_(torch.from_numpy(self.arrays["kl"]))
        self.eng.search_value_rows().copy_(torch.from_numpy(self.arrays["q"]))
        return self

    def total(self, upto=None):
        return int(np.maximum(self.lens.reshape(-1)[:upto], 0).sum())


class Block:
    """a packed block on the device with its kl / q vectors, and the twin's copy of all three on the host"""

    def __init__(self, na, cap, fill=0xA5):
        self.dev = alloc_packed_block(na, cap, DEV)
        self.dev.fill_(fill)
        self.host = np.full(self.dev.numel(), fill, np.uint8)
        self.kl = torch.full((cap + 64,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
        self.q = self.kl.clone()
        self.hkl = np.full(cap + 64, SENTINEL, np.uint32).view(np.float32)
        self.hq = self.hkl.copy()

    def pack(self, s, cap, append=False):
        """the three pack calls of engine `s` behind each other, the twin on the host copy, and everything compared"""
        s.off_view.fill_(OFF_POISON)
        s.eng.pack_examples(self.dev, cap, append=append)
        s.eng.pack_surprise(self.kl, cap, append=append)
        s.eng.pack_search_value(self.q, cap, append=append)
        torch.cuda.synchronize()
        p = pack_twin(self.host, s.arrays, s.lens, s.base, s.stride, s.na, s.gid, cap, append,
                      kl=(s.arrays["kl"], self.hkl), q=(s.arrays["q"], self.hq))
        what = (s.R, s.B, cap, append)
        got = self.dev.cpu().numpy()
        assert header_words(got)[:16] == header_words(p.block)[:16], (what, header_words(got)[:8], header_words(p.block)[:8])
        if not np.array_equal(got, p.block):
            k = int(np.flatnonzero(got != p.block)[0])
            offs = twin_layout(s.na, cap)[0]
            a = max(i for i, o in enumerate([0] + offs) if o <= k)
            raise AssertionError(f"{what}: byte {k} (in {(['header'] + list(FIELDS))[a]}, {k - ([0] + offs)[a]} bytes in) is "
                                 f"{got[k]:#x}, the twin has {p.block[k]:#x}; {int((got != p.block).sum())} bytes differ")
        off = s.off_view.cpu().numpy()
        assert np.array_equal(off, p.pack_off), (what, np.flatnonzero(off != p.pack_off)[:8], off[off != p.pack_off][:8],
                                                 p.pack_off[off != p.pack_off][:8])
        for name, dev, want in (("kl", self.kl, p.kl), ("q", self.q, p.q)):
            g = dev.cpu().numpy().view(np.uint32)
            assert np.array_equal(g, want.view(np.uint32)), (what, name, np.flatnonzero(g != want.view(np.uint32))[:8])
        self.host, self.hkl, self.hq = p.block, p.kl, p.q
        return p


def _fresh(s, cap, append=False):
    return Block(s.na, cap).pack(s, cap, append)


# ---------------------------------------------------------------- synthetic blocks: every games-per-block count
def _shape(n):
    """(rounds, B) with rounds * B == n, as many rounds (<= 3) as divide it"""
    for r in (3, 2, 1):
        if n % r == 0:
            return r, n // r
    raise AssertionError(n)


def _patterns(s, n):
    """(name, lens [n], capacities): the length patterns of one size and the cuts each is packed with"""
    rng, T = s.rng, s.T
    mix = rng.integers(-1, T + 1, size=n)
    out = [("none", np.full(n, -1), [1, 7]), ("zero", np.zeros(n, int), [1, 5]), ("full", np.full(n, T), [n * T, n * T - 1, 1])]
    rows = np.cumsum(np.maximum(mix, 0))
    tot = int(rows[-1])
    caps = [tot, tot - 1, 1, int(rows[min(n, 1024) // 2]) + 1]     # the total, one short, one row, a cut inside chunk 0
    if n > 1024:
        caps += [int(rows[1023]) - 1, int(rows[1023]), int(rows[1023]) + 1]   # on and next to the first chunk's row count
    if n > 2048:
        caps += [int(rows[2047]), int(rows[2048 + (n - 2048) // 2]) + 1]       # the second edge, a cut inside chunk 2
    out.append(("mix", mix, caps))
    # a cut followed only by games without rows and unfinished games
    tail = np.concatenate([rng.integers(1, T + 1, size=(n + 1) // 2), rng.choice([0, -1], size=n // 2)])
    ttot = int(np.maximum(tail, 0).sum())
    out.append(("tail", tail, [ttot, ttot - 1]))
    for k in sorted({0, 1023, 1024, n - 1}):   # exactly one finished game
        if k < n:
            one = np.full(n, -1)
            one[k] = T if k % 2 else max(1, T - 2)
            out.append((f"one@{k}", one, [int(one[k]), int(one[k]) - 1] if k in (0, 1024) else [int(one[k])]))
    return [(name, lens, sorted({c for c in caps if c >= 1})) for name, lens, caps in out]


def _every_pattern(game, n):
    R, B = _shape(n)
    s = Synth(game, B, R, base=2 ** 40 + 11 * n, stride=B + 3)
    seen = 0
    for name, lens, caps in _patterns(s, n):
        s.fill(lens)
        for cap in caps:
            p = _fresh(s, cap)
            tot = s.total()
            if name == "none":
                assert (p.n_rows, p.n_games, p.dropped) == (0, 0, 0) and header_words(p.block)[0] == PACKED_MAGIC
            if name == "zero":
                assert (p.n_rows, p.n_games, p.dropped) == (0, n, 0)
            if cap >= tot:
                assert (p.n_rows, p.dropped, p.n_games) == (tot, 0, int((s.lens >= 0).sum())), (name, cap)
            else:
                assert p.dropped == tot - p.n_rows > 0, (name, cap)
            seen += 1
    return seen


@pytest.mark.parametrize("n", [1, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 2047, 2049, 3073])
def test_tic_tac_toe_blocks_equal_the_twin(n):
    assert _every_pattern("ttt", n) >= 10


@pytest.mark.parametrize("n", [5, 65, 1025])
def test_reversi_blocks_equal_the_twin(n):
    """na 65, t_max 64: the len * na copy loop runs more than once per lane and a game has as many rows as a wave has lanes"""
    assert _every_pattern("reversi", n) >= 10


def test_capacity_equal_to_the_row_count_drops_nothing_and_one_less_drops_the_last_game():
    s = Synth("ttt", 5).fill([3, 9, 0, 1, 4])
    p = _fresh(s, 17)
    assert (p.n_rows, p.n_games, p.dropped, p.pack_off.tolist()) == (17, 5, 0, [0, 3, 12, 12, 13])
    p = _fresh(s, 16)
    assert (p.n_rows, p.n_games, p.dropped, p.pack_off.tolist()) == (13, 4, 4, [0, 3, 12, 12, -1])
    p = _fresh(s.fill([3, 9, 1, 4, 0]), 17)  # a game without rows right at the capacity still counts
    assert (p.n_rows, p.n_games, p.dropped, p.pack_off.tolist()) == (17, 5, 0, [0, 3, 12, 13, 17])
    p = _fresh(s, 16)                          # ... and behind a dropped game it is dropped too
    assert (p.n_rows, p.n_games, p.dropped, p.pack_off.tolist()) == (13, 3, 4, [0, 3, 12, -1, -1])


# ---------------------------------------------------------------- append chains
def _chain(k):
    shapes = [(1, 40), (2, 600), (3, 7), (1, 65)][:k]  # different B, one engine with more than 1024 games
    base, out = 1000, []
    for R, B in shapes:
        s = Synth("ttt", B, R, base=base, stride=5000)
        out.append(s.fill(s.rng.integers(-1, 10, size=R * B)))
        base += B
    return out


@pytest.mark.parametrize("k", [3, 4])
def test_append_chains_equal_the_twin_applied_in_sequence(k):
    engs = _chain(k)
    tot = [s.total() for s in engs]
    # everything fits exactly
    blk = Block(9, sum(tot))
    for i, s in enumerate(engs):
        p = blk.pack(s, sum(tot), append=i > 0)
        assert (p.n_rows, p.dropped) == (sum(tot[:i + 1]), 0)
    assert p.n_games == sum(int((s.lens >= 0).sum()) for s in engs)
    h = packed_block_header(blk.dev)
    assert (h["n_rows"], h["n_games"], h["dropped_rows"]) == (p.n_rows, p.n_games, 0)
    # the second engine overflows, the third again: dropped_rows adds up over the chain
    cap = tot[0] + tot[1] // 2
    blk, ps = Block(9, cap), []
    for i, s in enumerate(engs):
        ps.append(blk.pack(s, cap, append=i > 0))
    assert ps[0].dropped == 0 < ps[1].dropped < ps[2].dropped <= ps[-1].dropped
    assert ps[-1].dropped == sum(tot) - ps[-1].n_rows and ps[-1].n_rows <= cap
    with pytest.raises(RuntimeError, match="did not fit"):
        packed_block_header(blk.dev)
    assert packed_block_header(blk.dev, strict=False)["dropped_rows"] == ps[-1].dropped


# ---------------------------------------------------------------- geometry mismatches
def _refused(blk, s, cap, before_hdr):
    """engine `s` appended to a block it does not belong to: the sentinel, nothing but header words written"""
    arrays_before, kl_before, q_before = blk.dev[256:].clone(), blk.kl.clone(), blk.q.clone()
    p = blk.pack(s, cap, append=True)
    assert p.bad and p.dropped == NEVER and (p.pack_off == -1).all()
    h = header_words(blk.dev.cpu().numpy())
    assert h[6] == NEVER and h[1] == before_hdr[1] and h[2] == before_hdr[2] and h[16:] == before_hdr[16:]
    assert torch.equal(blk.dev[256:], arrays_before)
    assert torch.equal(blk.kl.view(torch.int32), kl_before.view(torch.int32))
    assert torch.equal(blk.q.view(torch.int32), q_before.view(torch.int32))
    with pytest.raises(RuntimeError, match="another geometry"):
        packed_block_header(blk.dev)
    return p


def test_an_engine_of_another_game_is_refused_by_the_block():
    rev, ttt = Synth("reversi", 3), Synth("ttt", 6)
    rev.fill([64, 5, 0]); ttt.fill([9, 1, -1, 0, 4, 9])
    blk = Block(65, 100)  # (a Reversi block of 100 rows is larger than a tic-tac-toe block of 100 rows: the host check passes)
    first = blk.pack(rev, 100)
    _refused(blk, ttt, 100, header_words(first.block))
    assert header_words(blk.host)[3:6] == [100, 9, _lib.GAME_TTT]  # the header now describes the newcomer: hence the sentinel


def test_an_engine_with_another_capacity_is_refused_by_the_block():
    a, b = Synth("ttt", 6).fill([9, 1, -1, 0, 4, 9]), Synth("ttt", 4, base=6).fill([2, 2, 2, 2])
    blk = Block(9, 100)
    first = blk.pack(a, 100)
    _refused(blk, b, 90, header_words(first.block))


@pytest.mark.parametrize("whole", [True, False])
def test_a_block_with_a_poison_magic_is_refused(whole):
    a, b = Synth("ttt", 6).fill([9, 1, -1, 0, 4, 9]), Synth("ttt", 4, base=6).fill([2, 2, 2, 2])
    blk = Block(9, 100)
    if not whole:  # a healthy block whose magic alone is overwritten
        blk.pack(a, 100)
        blk.dev[:8] = 0xA5
        blk.host[:8] = 0xA5
    before = header_words(blk.host)
    assert before[0] != PACKED_MAGIC
    _refused(blk, b, 100, before)


def test_the_sentinel_is_final_for_a_block():
    """A with cap 100, B appended with cap 90 (bad), C appended with cap 90: C matches the header B rewrote, and exactly one of
    its rows does not fit -- 2^64 - 1 plus that one row would read as dropped_rows = 0, a healthy block holding two layouts"""
    a, b = Synth("ttt", 4).fill([9] * 4), Synth("ttt", 2, base=4).fill([9, 9])
    c = Synth("ttt", 7, base=6).fill([9] * 6 + [1])
    blk = Block(9, 100)
    pa = blk.pack(a, 100)
    assert (pa.n_rows, pa.n_games) == (36, 4)
    _refused(blk, b, 90, header_words(pa.block))
    rows_after_a = blk.dev[256:].clone()
    assert pa.n_rows + c.total() == 91
    pc = _refused(blk, c, 90, header_words(pa.block))
    assert (pc.n_rows, pc.n_games) == (36, 4)
    assert torch.equal(blk.dev[256:], rows_after_a) and (c.off_view == -1).all()
    assert header_words(blk.dev.cpu().numpy())[6] == NEVER


# ---------------------------------------------------------------- host refusals: a status code, nothing launched
def test_the_host_refuses_blocks_it_cannot_fill():
    L = _lib.lib()
    rev = Synth("reversi", 2).fill([64, 3])
    cap = 2 * 64
    blk = alloc_packed_block(9, cap, DEV)  # sized for tic-tac-toe
    blk.fill_(0xA5)
    rev.off_view.fill_(OFF_POISON)
    st = torch.cuda.current_stream().cuda_stream
    assert blk.numel() < twin_layout(65, cap)[1]
    assert L.bz_engine_pack_examples(rev.eng.h, blk.data_ptr(), blk.numel(), cap, 0, st) == _lib.BZ_ENOMEM
    big = alloc_packed_block(65, cap, DEV)
    big.fill_(0xA5)
    assert L.bz_engine_pack_examples(rev.eng.h, big.data_ptr(), big.numel(), 0, 0, st) == _lib.BZ_EINVAL
    assert L.bz_engine_pack_examples(rev.eng.h, big.data_ptr() + 8, big.numel() - 8, cap - 1, 0, st) == _lib.BZ_EINVAL
    assert L.bz_engine_pack_examples(rev.eng.h, None, big.numel(), cap, 0, st) == _lib.BZ_EINVAL
    torch.cuda.synchronize()
    assert (blk == 0xA5).all() and (big == 0xA5).all() and (rev.off_view == OFF_POISON).all()
    with pytest.raises(RuntimeError, match=f"libbz_hip error {_lib.BZ_ENOMEM}: .*block too small"):  # the wrapper raises
        rev.eng.pack_examples(blk, cap)
    _fresh(rev, cap)  # the engine is none the worse for it


# ---------------------------------------------------------------- played games
def _kl_q(engines):
    out = []
    for rows in ("surprise_rows", "search_value_rows"):
        parts = [np.zeros(0, np.float32)]
        for e in engines:
            _, lens = e.winners()
            v = getattr(e, rows)().cpu().numpy()
            parts += [v[r, b, :max(0, lens[r, b])] for r in range(lens.shape[0]) for b in range(lens.shape[1])]
        out.append(np.concatenate(parts))
    return out


def _same_examples(a, b):
    assert len(a) == len(b)
    for f in FIELDS:
        x, y = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), f


def test_two_rounds_with_restart_partly_finished():
    """tic-tac-toe, two rounds, a staggered pool, 12 moves with restart: the first round is over, the second partly -- its
    unfinished games (ex_len = -1, rows half written) are in neither the packed block nor the raw unpack"""
    B, cap = 24, 2 * 24 * 9
    eng = SelfPlayEngine("ttt", B, 16, "hash", rounds=2, stagger=3, temp_moves=4, seed=5, game_id_base=300, surprise=True,
                         search_value=True)
    eng.reset_games()
    for _ in range(12):
        eng.search()
        eng.play(True)
    eng.status()
    s = Played(eng, 300, B)
    assert (s.lens[0] >= 0).all() and (s.lens[1] >= 0).any() and (s.lens[1] < 0).any(), s.lens.tolist()
    blk = Block(9, cap)
    p = blk.pack(s, cap)
    assert (p.n_rows, p.n_games, p.dropped) == (s.lens[s.lens >= 0].sum(), (s.lens >= 0).sum(), 0)
    raw = unpack_example_block(eng.example_block())
    same_rows(raw, direct_rows(s.arrays, s.lens, 300, B))
    _same_examples(unpack_packed_block(blk.dev), raw)
    _same_examples(unpack_packed_block(eng.pack_examples()), raw)
    unfinished = {300 + B + g for g in range(B) if s.lens[1, g] < 0}
    assert unfinished and not (unfinished & set(raw.game.tolist()))


@pytest.mark.parametrize("pipelines,n", [(3, 22), (4, 23)])
def test_ragged_pipelines_equal_the_engines_raw_unpacks(pipelines, n):
    sp = PipelinedSelfPlay("ttt", n, 16, "hash", pipelines=pipelines, temp_moves=4, seed=2, game_id_base=40, surprise=True,
                           search_value=True)
    assert len(set(sp.sizes)) == 2 and sum(sp.sizes) == n
    sp.run_iteration()
    sp.sync()
    want = concat_examples([unpack_example_block(e.example_block()) for e in sp.engines])
    kl, q = _kl_q(sp.engines)
    assert len(want) > 0 and sorted(set(want.game.tolist())) == list(range(40, 40 + n))
    for ex in (sp.examples(), sp.device_examples().cpu()):
        _same_examples(ex, want)
        assert np.array_equal(ex.kl.view(np.uint32), kl.view(np.uint32)) and np.array_equal(ex.q.view(np.uint32), q.view(np.uint32))
    h = packed_block_header(sp.pack_examples())
    assert (h["n_rows"], h["n_games"], h["dropped_rows"]) == (len(want), n, 0)
    blk = Block(9, len(want))  # and every byte of a block of exactly that many rows, engine by engine
    for i, e in enumerate(sp.engines):
        blk.pack(Played(e, 40 + sum(sp.sizes[:i]), n), len(want), append=i > 0)


def test_games_without_rows_in_a_chain_of_three_engines():
    """playout cap randomisation with few full searches: some games finish with ex_len = 0; the block counts them as games"""
    sp = PipelinedSelfPlay("ttt", 48, 40, "hash", pipelines=3, playout_cap=PlayoutCap(4, 0.25), temp_moves=9, seed=1,
                           dirichlet_alpha=0.3, dirichlet_eps=0.25, surprise=True, search_value=True)
    sp.run_iteration()
    sp.sync()
    lens = np.concatenate([e.winners()[1] for e in sp.engines], axis=1)
    assert (lens >= 0).all() and (lens == 0).any() and (lens > 0).any(), lens.tolist()
    want = concat_examples([unpack_example_block(e.example_block()) for e in sp.engines])
    assert len(want) == int(lens.sum())
    for cap in (sp.packed_capacity(), len(want)):
        blk = sp.pack_examples(cap_rows=cap)
        h = packed_block_header(blk)
        assert (h["n_rows"], h["n_games"], h["dropped_rows"]) == (len(want), 48, 0), (cap, h)
        _same_examples(unpack_packed_block(blk), want)
    kl, q = _kl_q(sp.engines)
    ex = sp.examples()
    _same_examples(ex, want)
    assert np.array_equal(ex.kl.view(np.uint32), kl.view(np.uint32)) and np.array_equal(ex.q.view(np.uint32), q.view(np.uint32))
    blk = Block(9, len(want))  # byte for byte, engine by engine, in a block of exactly the rows' size
    for i, e in enumerate(sp.engines):
        p = blk.pack(Played(e, sum(sp.sizes[:i]), 48), len(want), append=i > 0)
    assert (p.n_rows, p.n_games, p.dropped) == (len(want), 48, 0)


# ---------------------------------------------------------------- the engine's per-row extras, all three together
def _extras_want(engines):
    """kl, q, fown, fopp of the finished games' rows in (engine, round, slot, ply) order, from the engines' raw buffers:
    surprise_rows(), search_value_rows() and the ownership-row twin on ownership_rows() and the rows' mover"""
    from test_ownership_cpu import ownership_row
    want = {"kl": [np.zeros(0, np.float32)], "q": [np.zeros(0, np.float32)], "fown": [np.zeros(0, np.uint64)], "fopp": [np.zeros(0, np.uint64)]}
    for e in engines:
        t = e.example_tensors()
        lens, mover = t["len"].cpu().numpy(), t["mover"].cpu().numpy()
        kl, q = e.surprise_rows().cpu().numpy(), e.search_value_rows().cpu().numpy()
        fx, fo = (x.cpu().numpy().view(np.uint64) for x in e.ownership_rows())
        for r in range(lens.shape[0]):
            for b in range(lens.shape[1]):
                n = max(0, lens[r, b])
                a, o = ownership_row(np.full(n, fx[r, b]), np.full(n, fo[r, b]), mover[r, b, :n])
                for k, v in (("kl", kl[r, b, :n]), ("q", q[r, b, :n]), ("fown", a), ("fopp", o)):
                    want[k].append(v)
    return {k: np.concatenate(v) for k, v in want.items()}


def _check_extras(src, engines, packed):
    """examples() and device_examples() of `src` carry the engines' kl / q / fown / fopp, host and device alike; `packed`:
    {column: [cap_rows] device tensor} of the public pack calls, the same vectors"""
    want = _extras_want(engines)
    raw = concat_examples([unpack_example_block(e.example_block()) for e in engines])
    n = len(raw)
    assert n > 0 and all(len(v) == n for v in want.values()) and len(set(want["kl"].view(np.uint32).tolist())) > 1
    dev = src.device_examples()
    assert all(torch.is_tensor(getattr(dev, k)) and getattr(dev, k).is_cuda for k in want)
    for ex in (src.examples(), dev.cpu()):
        _same_examples(ex, raw)
        for k, w in want.items():
            a = getattr(ex, k)
            assert a.dtype == w.dtype and a.shape == w.shape and np.array_equal(a.view(np.uint8), w.view(np.uint8)), k
        assert ex.vt is None and ex.count is None
    for k, w in want.items():
        a = packed[k][:n].cpu().numpy()
        assert packed[k].dtype == getattr(dev, k).dtype and np.array_equal(a.view(np.uint8), w.view(np.uint8)), k


def test_one_engine_with_every_extra_on_two_rounds():
    """surprise, search_value and ownership together: examples() / device_examples() pack the rows once and attach all four
    columns; tic-tac-toe, 5 games, two rounds with restart"""
    eng = SelfPlayEngine("ttt", 5, 8, "uniform", rounds=2, temp_moves=4, seed=3, game_id_base=70, surprise=True, search_value=True,
                         ownership=True)
    eng.reset_games()
    for _ in range(2 * 9 + 2):
        eng.search()
        eng.play(True)
        if eng.status()[0] == 0:
            break
    assert (eng.winners()[1] > 0).all()
    eng.pack_examples()
    fown, fopp = eng.pack_ownership()
    _check_extras(eng, [eng], {"kl": eng.pack_surprise(), "q": eng.pack_search_value(), "fown": fown, "fopp": fopp})


def test_ragged_pipelines_with_every_extra_on():
    """3 pipelines over 7 games (3 + 2 + 2 slots): append chains of three for the block and for every extra column"""
    sp = PipelinedSelfPlay("ttt", 7, 8, "uniform", pipelines=3, temp_moves=4, seed=3, game_id_base=20, surprise=True, search_value=True,
                           ownership=True)
    assert sp.sizes == [3, 2, 2]
    sp.run_iteration()
    sp.sync()
    blk_kl, kl = sp.pack_examples_with_surprise()
    blk_q, q = sp.pack_examples_with_search_value()
    blk_own, fown, fopp = sp.pack_examples_with_ownership()
    _check_extras(sp, sp.engines, {"kl": kl, "q": q, "fown": fown, "fopp": fopp})
    raw = concat_examples([unpack_example_block(e.example_block()) for e in sp.engines])
    for blk in (blk_kl, blk_q, blk_own):
        _same_examples(unpack_packed_block(blk), raw)
