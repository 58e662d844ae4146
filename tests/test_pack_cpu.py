"""The packed example block (bz_abi.h "Packed examples") without a GPU: pack_twin, a sequential numpy restatement of what
k_pack_scan / k_pack_rows / k_pack_f32 (csrc/bz_mcts.hip) own of a block -- tests/test_gpu_pack.py pins the kernels
to it byte for byte -- and the host-side constructors and unpackers of betazero_amd/engine.py against it and against a direct
loop over (round, slot, ply).  The twin calls neither the library nor the functions of engine.py it is used to check."""
import numpy as np
import pytest
import torch

from betazero_amd import _lib
from betazero_amd import engine as E

PACKED_MAGIC = 0x425A50414B000001
NEVER = 2 ** 64 - 1  # dropped_rows of a block an append of another geometry met: final for the block
FIELDS = ("own", "opp", "pi", "game", "z", "mover", "act", "ply")
ROW_FIELDS = ("own", "opp", "pi", "z", "mover", "act")  # what the engine records per (round, slot, ply)


# ---------------------------------------------------------------- the twin
def twin_layout(na, cap):
    """(byte offsets of own, opp, pi, game id, z, mover, act, ply; total bytes): a 256-byte header, then the eight arrays of
    cap elements, each starting at the next multiple of 256"""
    offs, off = [], 256
    for esz in (8, 8, 4 * na, 8, 1, 1, 1, 1):
        offs.append(off)
        off += -(-cap * esz // 256) * 256
    return offs, off


class Packed:
    """what one pack call leaves: the block's bytes, pack_off per game, whether the append was bad, the header numbers,
    and the kl / q vectors when sources were given"""

    def __init__(self, block, pack_off, bad, n_rows, n_games, dropped, kl, q):
        self.block, self.pack_off, self.bad, self.n_rows, self.n_games, self.dropped, self.kl, self.q = \
            block, pack_off, bad, n_rows, n_games, dropped, kl, q


def pack_vec_twin(out, src, lens, pack_off, cap):
    """k_pack_f32: the per-row source [rounds, B, t_max] of the games with pack_off >= 0 into `out` at off + t,
    t < len and off + t < cap; every other element of `out` keeps its bits"""
    out = np.array(out, np.float32).view(np.uint32).copy()
    src = np.asarray(src, np.float32).view(np.uint32).reshape(len(pack_off), -1)
    for i, off in enumerate(pack_off):
        if off < 0:
            continue
        for t in range(int(lens.reshape(-1)[i])):
            if off + t < cap:
                out[off + t] = src[i, t]
    return out.view(np.float32)


def pack_twin(block_bytes, arrays, lens, id_base, id_stride, na, game, cap, append, kl=None, q=None):
    """one bz_engine_pack_examples call on a host copy of the block, as a plain loop over (round, slot).  `arrays`: numpy
    [rounds, B, t_max, ...] own, opp, pi, z, mover, act as example_tensors() holds them; lens int [rounds, B].
    kl / q = (source [rounds, B, t_max], vector to pack into): the bz_engine_pack_surprise / _search_value call behind it."""
    blk = np.array(block_bytes, np.uint8).copy()
    lens = np.asarray(lens, np.int64)
    R, B = lens.shape
    offs, total = twin_layout(na, cap)
    assert blk.size >= total
    hdr = blk[:256].view(np.uint64)  # (a view: writes land in blk)
    bad, carry, games0, dropped0 = False, 0, 0, 0
    if append:
        bad = (int(hdr[0]) != PACKED_MAGIC or int(hdr[3]) != cap or int(hdr[4]) != na or int(hdr[7]) != total or
               int(hdr[5]) != game or int(hdr[6]) == NEVER)
        carry, games0, dropped0 = int(hdr[1]) & 0xFFFFFFFF, int(hdr[2]) & 0xFFFFFFFF, int(hdr[6])
    esz = (8, 8, 4 * na, 8, 1, 1, 1, 1)
    src = {"own": np.ascontiguousarray(arrays["own"]).view(np.uint8).reshape(R * B, -1),
           "opp": np.ascontiguousarray(arrays["opp"]).view(np.uint8).reshape(R * B, -1),
           "pi": np.ascontiguousarray(arrays["pi"], np.float32).view(np.uint8).reshape(R * B, -1),
           "z": np.ascontiguousarray(arrays["z"]).view(np.uint8).reshape(R * B, -1),
           "mover": np.ascontiguousarray(arrays["mover"]).view(np.uint8).reshape(R * B, -1),
           "act": np.ascontiguousarray(arrays["act"]).view(np.uint8).reshape(R * B, -1)}
    pack_off = np.full(R * B, -1, np.int32)
    first, n_rows, n_fit = carry, carry, 0
    for r in range(R):
        for s in range(B):
            i, n = r * B + s, int(lens[r, s])
            if n >= 0 and not bad and first + n <= cap:
                pack_off[i] = first
                n_fit += 1
                n_rows = max(n_rows, first + n)
                if n > 0:
                    gid = np.full(n, (id_base + r * id_stride + s) & (2 ** 64 - 1), np.uint64).view(np.uint8)
                    ply = np.arange(n, dtype=np.uint8)
                    rows = {"own": src["own"][i, :8 * n], "opp": src["opp"][i, :8 * n], "pi": src["pi"][i, :4 * na * n],
                            "game": gid, "z": src["z"][i, :n], "mover": src["mover"][i, :n], "act": src["act"][i, :n], "ply": ply}
                    for name, off, e in zip(FIELDS, offs, esz):
                        blk[off + first * e:off + (first + n) * e] = rows[name]
            first += max(n, 0)
    hdr[0], hdr[3], hdr[4], hdr[5], hdr[7] = PACKED_MAGIC, cap, na, game, total
    hdr[8:16] = offs
    if bad:  # n_rows and n_games stay what they were
        n_rows, n_games, dropped = int(hdr[1]), int(hdr[2]), NEVER
    else:
        n_games, dropped = games0 + n_fit, (dropped0 + first - n_rows) & (2 ** 64 - 1)
        hdr[1], hdr[2] = n_rows, n_games
    hdr[6] = dropped
    vec = [None if v is None else pack_vec_twin(v[1], v[0], lens, pack_off, cap) for v in (kl, q)]
    return Packed(blk, pack_off, bad, n_rows, n_games, dropped, vec[0], vec[1])


def header_words(block):
    return [int(v) for v in np.asarray(block[:256]).view(np.uint64)]


# ---------------------------------------------------------------- test data
def random_bits_f32(rng, shape):
    """float32 values as raw bit patterns: every exponent, -0, subnormals, infinities and NaN payloads among them, so that
    a copy that goes through float arithmetic (or a conversion) shows"""
    bits = rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32)
    flat = bits.reshape(-1)
    special = np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC00001, 0xFFA5A5A5, 0x7F800001], np.uint32)
    k = min(flat.size, 4 * len(special))
    if k:
        flat[rng.choice(flat.size, size=k, replace=False)] = np.resize(special, k)
    return bits.view(np.float32)


POISON = {"own": 0x0DEAD0DEAD0DEAD0, "opp": 0x0BAD0BAD0BAD0BAD, "pi": 0xFFC0DEAD, "z": 0x5D, "mover": 0x5E, "act": 0xDD,
          "kl": 0xFFC0FFEE, "q": 0xFFC0BEEF}


def random_arrays(rng, R, B, T, na):
    """valid-looking rows everywhere: random 64-bit boards, pi / kl / q as random bit patterns, random bytes"""
    u64 = lambda: rng.integers(0, 2 ** 64, size=(R, B, T), dtype=np.uint64).view(np.int64)  # noqa: E731
    return {"own": u64(), "opp": u64(), "pi": random_bits_f32(rng, (R, B, T, na)),
            "z": rng.integers(-1, 2, size=(R, B, T)).astype(np.int8), "mover": (rng.integers(0, 2, size=(R, B, T)) * 2 - 1).astype(np.int8),
            "act": rng.integers(0, na, size=(R, B, T)).astype(np.uint8),
            "kl": random_bits_f32(rng, (R, B, T)), "q": random_bits_f32(rng, (R, B, T))}


def poisoned(arrays, lens):
    """a copy of `arrays` whose rows at and past each game's len hold POISON: a row copied from there shows"""
    T = arrays["own"].shape[2]
    past = np.arange(T)[None, None, :] >= np.maximum(np.asarray(lens), 0)[:, :, None]
    out = {}
    for name, a in arrays.items():
        a = a.copy()
        if a.dtype == np.float32:
            a.view(np.uint32)[past] = POISON[name]
        elif a.dtype == np.int64:
            a[past] = POISON[name]
        else:
            a.view(np.uint8)[past] = POISON[name]
        out[name] = a
    return out


def direct_rows(arrays, lens, id_base, id_stride):
    """the finished games' rows by a direct loop over (round, slot, ply < len): the reference of every unpacker"""
    R, B = lens.shape
    rows = {f: [] for f in FIELDS}
    for r in range(R):
        for s in range(B):
            for t in range(max(int(lens[r, s]), 0)):
                for f in ROW_FIELDS:
                    rows[f].append(arrays[f][r, s, t])
                rows["game"].append(id_base + r * id_stride + s)
                rows["ply"].append(t)
    na = arrays["pi"].shape[-1]
    return {"own": np.array(rows["own"], np.int64).view(np.uint64), "opp": np.array(rows["opp"], np.int64).view(np.uint64),
            "pi": np.array(rows["pi"], np.float32).reshape(-1, na), "game": np.array(rows["game"], np.int64),
            "z": np.array(rows["z"], np.int8), "mover": np.array(rows["mover"], np.int8), "act": np.array(rows["act"], np.uint8),
            "ply": np.array(rows["ply"], np.int32)}


def same_rows(ex, want):
    """Examples / DeviceExamples `ex` holds exactly the rows `want` (direct_rows), bit for bit and in the same dtypes"""
    for f in FIELDS:
        got = getattr(ex, f)
        got = got.cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
        w = want[f]
        if f == "pi":
            got, w = got.view(np.uint32), w.view(np.uint32)
        elif f in ("own", "opp"):
            got, w = got.view(np.uint64), w.view(np.uint64)
        assert got.shape == w.shape and np.array_equal(got, w), f


def _tensors(arrays, lens):
    t = {f: torch.from_numpy(arrays[f]) for f in ROW_FIELDS}
    t["len"] = torch.from_numpy(np.asarray(lens, np.int32))
    t["winner"] = torch.zeros(lens.shape, dtype=torch.int8)
    return t


# ---------------------------------------------------------------- the layout
HAND_LAYOUTS = {  # (na, cap): offsets of own, opp, pi, game id, z, mover, act, ply; total -- worked out by hand
    (9, 1): ([256, 512, 768, 1024, 1280, 1536, 1792, 2048], 2304),
    # 64 rows: own / opp / ids 512 B each, pi 64 * 260 = 16640 = 65 * 256, the byte arrays one 256-byte unit each
    (65, 64): ([256, 768, 1280, 17920, 18432, 18688, 18944, 19200], 19456),
    # 255 rows: 2040 -> 2048 B for the 8-byte arrays, pi 255 * 36 = 9180 -> 9216
    (9, 255): ([256, 2304, 4352, 13568, 15616, 15872, 16128, 16384], 16640),
    # 256 rows: exactly 2048, 9216 and 256
    (9, 256): ([256, 2304, 4352, 13568, 15616, 15872, 16128, 16384], 16640),
    # 257 rows: 2056 -> 2304, pi 9252 -> 9472, the byte arrays 257 -> 512
    (9, 257): ([256, 2560, 4864, 14336, 16640, 17152, 17664, 18176], 18688),
}


@pytest.mark.parametrize("na,cap", list(HAND_LAYOUTS))
def test_layout_equals_the_hand_computed_offsets_and_the_library(na, cap):
    offs, total = HAND_LAYOUTS[(na, cap)]
    assert twin_layout(na, cap) == (offs, total)
    assert E.packed_layout(na, cap) == (offs, total)
    assert _lib.lib().bz_examples_packed_bytes(na, cap) == total


def test_layout_equals_the_library_at_every_small_capacity():
    L = _lib.lib()
    for na in (9, 17, 37, 65):
        for cap in list(range(1, 70)) + [255, 256, 257, 511, 513, 9216, 27657, 65600, 196672]:
            assert twin_layout(na, cap)[1] == L.bz_examples_packed_bytes(na, cap) == E.packed_layout(na, cap)[1], (na, cap)
            assert twin_layout(na, cap)[0] == E.packed_layout(na, cap)[0]
    assert E.PACKED_MAGIC == PACKED_MAGIC


# ---------------------------------------------------------------- hand-written cases
def _hand(lens, cap, base=7, stride=100):
    """one round of four games, t_max 3, na 2: own = 100 * slot + ply, opp = own + 50, pi = (own, -own), z = slot - ply,
    mover = +-1 by ply, act = 10 * slot + ply"""
    R, B, T = 1, 4, 3
    s, t = np.arange(B)[None, :, None], np.arange(T)[None, None, :]
    own = (100 * s + t + np.zeros((R, B, T), np.int64)).astype(np.int64)
    arrays = {"own": own, "opp": own + 50, "pi": np.stack([own, -own], -1).astype(np.float32),
              "z": (s - t + np.zeros((R, B, T))).astype(np.int8), "mover": (1 - 2 * (t % 2) + np.zeros((R, B, T))).astype(np.int8),
              "act": (10 * s + t + np.zeros((R, B, T))).astype(np.uint8)}
    blk = np.full(twin_layout(2, cap)[1], 0xA5, np.uint8)
    return pack_twin(blk, arrays, np.array([lens]), base, stride, 2, 3, cap, False), blk


def _column(p, name, na, cap, dtype, n):
    off = twin_layout(na, cap)[0][FIELDS.index(name)]
    return p.block[off:off + n * np.dtype(dtype).itemsize].view(dtype).tolist()


A5_64 = 0xA5A5A5A5A5A5A5A5


def test_hand_case_overflow_in_the_middle():
    p, before = _hand([2, 1, 3, 1], cap=4)
    assert p.pack_off.tolist() == [0, 2, -1, -1]
    assert (p.n_rows, p.n_games, p.dropped, p.bad) == (3, 2, 4, False)
    # own, opp, pi (2 floats a row), ids: 4 * 8 = 32 B each -> 256; the four byte arrays 256 each
    assert header_words(p.block) == [PACKED_MAGIC, 3, 2, 4, 2, 3, 4, 2304, 256, 512, 768, 1024, 1280, 1536, 1792, 2048] + [A5_64] * 16
    assert _column(p, "own", 2, 4, np.uint64, 4) == [0, 1, 100, A5_64]  # row 3 is inside the capacity and stays unwritten
    assert _column(p, "opp", 2, 4, np.uint64, 4) == [50, 51, 150, A5_64]
    assert _column(p, "pi", 2, 4, np.float32, 6) == [0.0, -0.0, 1.0, -1.0, 100.0, -100.0]
    assert _column(p, "game", 2, 4, np.int64, 3) == [7, 7, 8]
    assert _column(p, "z", 2, 4, np.int8, 4) == [0, -1, 1, -91]
    assert _column(p, "mover", 2, 4, np.int8, 4) == [1, -1, 1, -91]
    assert _column(p, "act", 2, 4, np.uint8, 4) == [0, 1, 10, 0xA5]
    assert _column(p, "ply", 2, 4, np.uint8, 4) == [0, 1, 0, 0xA5]
    # nothing but the 16 header words and the three rows of each array changed
    changed = np.flatnonzero(p.block != before)
    own_rows = set(range(128)) | {o + k for o, e in zip(twin_layout(2, 4)[0], (8, 8, 8, 8, 1, 1, 1, 1)) for k in range(3 * e)}
    assert set(changed.tolist()) <= own_rows


def test_hand_case_capacity_one_short_of_the_total():
    p, _ = _hand([2, 1, 3, 1], cap=6)
    assert p.pack_off.tolist() == [0, 2, 3, -1]
    assert (p.n_rows, p.n_games, p.dropped) == (6, 3, 1)
    assert header_words(p.block)[:8] == [PACKED_MAGIC, 6, 3, 6, 2, 3, 1, 2304]
    assert _column(p, "own", 2, 6, np.uint64, 6) == [0, 1, 100, 200, 201, 202]
    assert _column(p, "game", 2, 6, np.int64, 6) == [7, 7, 8, 9, 9, 9]
    assert _column(p, "ply", 2, 6, np.uint8, 7) == [0, 1, 0, 0, 1, 2, 0xA5]
    assert _column(p, "z", 2, 6, np.int8, 6) == [0, -1, 1, 2, 1, 0]


def test_hand_case_a_trailing_game_without_rows_at_first_equal_cap_fits():
    p, _ = _hand([2, 1, 3, 0], cap=6)
    assert p.pack_off.tolist() == [0, 2, 3, 6]
    assert (p.n_rows, p.n_games, p.dropped) == (6, 4, 0)
    assert header_words(p.block)[:8] == [PACKED_MAGIC, 6, 4, 6, 2, 3, 0, 2304]
    assert _column(p, "own", 2, 6, np.uint64, 6) == [0, 1, 100, 200, 201, 202]


def test_hand_case_a_trailing_game_without_rows_at_first_above_cap_does_not_fit():
    p, _ = _hand([2, 1, 3, 0], cap=5)
    assert p.pack_off.tolist() == [0, 2, -1, -1]
    assert (p.n_rows, p.n_games, p.dropped) == (3, 2, 3)
    assert header_words(p.block)[:8] == [PACKED_MAGIC, 3, 2, 5, 2, 3, 3, 2304]
    assert _column(p, "own", 2, 5, np.uint64, 5) == [0, 1, 100, A5_64, A5_64]


def test_hand_case_appends_accumulate_and_the_sentinel_is_final():
    """A (cap 100) <- B with another capacity: bad.  C with B's capacity would match the header B rewrote; one of its rows does
    not fit, which without the sticky rule turns dropped_rows from ~0 into 0"""
    rng = np.random.default_rng(5)
    T, na = 9, 9

    def eng(lens):
        lens = np.array([lens])
        return poisoned(random_arrays(rng, 1, lens.shape[1], T, na), lens), lens

    blk = np.full(twin_layout(na, 100)[1], 0xA5, np.uint8)
    (a, la), (b, lb), (c, lc) = eng([9] * 4), eng([9, 9]), eng([9] * 6 + [1])
    pa = pack_twin(blk, a, la, 0, 4, na, 0, 100, False)
    assert (pa.n_rows, pa.n_games, pa.dropped) == (36, 4, 0)
    pb = pack_twin(pa.block, b, lb, 4, 2, na, 0, 90, True)
    assert pb.bad and (pb.n_rows, pb.n_games, pb.dropped) == (36, 4, NEVER) and (pb.pack_off == -1).all()
    assert header_words(pb.block)[:8] == [PACKED_MAGIC, 36, 4, 90, 9, 0, NEVER, twin_layout(na, 90)[1]]
    assert np.array_equal(pb.block[256:], pa.block[256:])
    pc = pack_twin(pb.block, c, lc, 6, 7, na, 0, 90, True)  # 36 + 55 = 91 rows: exactly one does not fit
    assert pc.bad and (pc.n_rows, pc.n_games, pc.dropped) == (36, 4, NEVER) and (pc.pack_off == -1).all()
    assert np.array_equal(pc.block, pb.block)
    with pytest.raises(RuntimeError, match="another geometry"):
        E.packed_block_header(torch.from_numpy(pc.block))
    # a healthy chain: the second and the third engine overflow, dropped_rows adds up
    p1 = pack_twin(blk, a, la, 0, 4, na, 0, 50, False)
    p2 = pack_twin(p1.block, b, lb, 4, 2, na, 0, 50, True)   # 36 + 9 fit, 9 dropped
    p3 = pack_twin(p2.block, c, lc, 6, 7, na, 0, 50, True)   # first = 54 > 50: nothing fits, 55 dropped
    assert (p2.n_rows, p2.n_games, p2.dropped, p2.pack_off.tolist()) == (45, 5, 9, [36, -1])
    assert (p3.n_rows, p3.n_games, p3.dropped) == (45, 5, 64) and (p3.pack_off == -1).all()


# ---------------------------------------------------------------- engine.py against the twin and the direct loop
@pytest.mark.parametrize("game,na,T,R,B", [("ttt", 9, 9, 1, 7), ("ttt", 9, 9, 3, 5), ("reversi", 65, 64, 2, 3)])
def test_build_packed_block_and_unpack_packed_block_equal_the_twin(game, na, T, R, B):
    rng = np.random.default_rng(R * 100 + B)
    lens = rng.choice([-1] + list(range(1, T + 1)), size=(R, B)).astype(np.int32)  # no game without rows: build_packed_block
    lens[0, 0], lens[-1, -1] = T, 1                                                 # counts the games by the ids of their rows
    arrays = poisoned(random_arrays(rng, R, B, T, na), lens)
    total = int(np.maximum(lens, 0).sum())
    raw = E.unpack_example_block(E.build_example_block(_tensors(arrays, lens), 1000, 50, game))
    for cap in (total, total + 5):
        p = pack_twin(np.zeros(twin_layout(na, cap)[1], np.uint8), arrays, lens, 1000, 50, na, E._GAMES[game], cap, False)
        assert (p.n_rows, p.n_games, p.dropped) == (total, int((lens >= 0).sum()), 0)
        built = E.build_packed_block(raw, cap, game).numpy()
        assert built.shape == p.block.shape and np.array_equal(built, p.block)
        same_rows(E.unpack_packed_block(torch.from_numpy(p.block)), direct_rows(arrays, lens, 1000, 50))
        ex = E.unpack_packed_block(torch.from_numpy(p.block))
        for f in FIELDS:
            a, b = np.asarray(getattr(ex, f)), np.asarray(getattr(raw, f))
            assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), f
        dev = E.unpack_packed_block_device(torch.from_numpy(p.block))
        same_rows(dev, direct_rows(arrays, lens, 1000, 50))


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("game,na,T,B", [("ttt", 9, 9, 11), ("reversi", 65, 64, 6)])
def test_the_raw_unpackers_equal_a_direct_loop(game, na, T, B, R):
    rng = np.random.default_rng(R * 7 + B)
    lens = rng.choice([-1, 0, 1, T], size=(R, B)).astype(np.int32)
    lens.reshape(-1)[:4] = [T, 0, -1, 1]  # every kind is there
    arrays = poisoned(random_arrays(rng, R, B, T, na), lens)
    base, stride = 2 ** 40 + 3, B + 9
    want = direct_rows(arrays, lens, base, stride)
    block = E.build_example_block(_tensors(arrays, lens), base, stride, game)
    same_rows(E.unpack_example_block(block), want)
    offs, off = [], 0  # the block's geometry, as SelfPlayEngine.block_geometry() describes an engine's
    for n in (8 * T, 8 * T, 4 * na * T, T, T, T, 4, 1):
        offs.append(off)
        off += -(-R * B * n // 256) * 256
    geom = {"B": B, "rounds": R, "t_max": T, "na": na, "game": E._GAMES[game], "size": E._SIZES[E._GAMES[game]], "offs": offs,
            "ex_bytes": off + 256}
    dev = E.unpack_example_block_device(block, geom)
    same_rows(dev, want)
    assert dev.ply.dtype == torch.int32 and dev.game.dtype == torch.int64
    with pytest.raises(ValueError):  # a block of another geometry with the same byte size is refused
        E.unpack_example_block_device(block, dict(geom, B=B + 1))


def test_pack_vec_twin_guards_the_capacity_and_touches_nothing_else():
    lens = np.array([[2, -1, 0, 3]])
    src = np.arange(12, dtype=np.float32).reshape(1, 4, 3) + 1
    out = np.full(8, -7.0, np.float32)
    got = pack_vec_twin(out, src, lens, np.array([0, -1, 2, 2]), 6)
    assert got.tolist() == [1.0, 2.0, 10.0, 11.0, 12.0, -7.0, -7.0, -7.0]
    # a vector shorter than the block's capacity: rows at and past its own capacity are not written
    assert pack_vec_twin(out, src, lens, np.array([0, -1, 2, 2]), 4).tolist() == [1.0, 2.0, 10.0, 11.0, -7.0, -7.0, -7.0, -7.0]
    assert out.tolist() == [-7.0] * 8
