"""Training rows and the blocks that carry them: COLUMNS, THE table of a row's columns; Examples (numpy, host) and
DeviceExamples (torch, GPU), the two row types; what is written once against the table for both -- columns, take, concat,
host <-> device --; and the engine's example block and the packed example block (include/bz_abi.h), with their unpackers
and host-side builders.  A new per-row column is a row of COLUMNS and a field of the two dataclasses ("Adding a
per-row column"); tests/test_example_columns_cpu.py holds the three equal and sends every column through every carrier."""
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np
import torch

from ._lib import GAME_REVERSI, GAME_REVERSI4, GAME_REVERSI6, GAME_TTT

_GAMES = {"ttt": GAME_TTT, "tic_tac_toe": GAME_TTT, "reversi": GAME_REVERSI, "reversi8": GAME_REVERSI,
          "reversi6": GAME_REVERSI6, "reversi4": GAME_REVERSI4, GAME_TTT: GAME_TTT, GAME_REVERSI: GAME_REVERSI,
          GAME_REVERSI6: GAME_REVERSI6, GAME_REVERSI4: GAME_REVERSI4}
_SIZES = {GAME_TTT: 3, GAME_REVERSI: 8, GAME_REVERSI6: 6, GAME_REVERSI4: 4}


class Column(NamedTuple):
    name: str
    host: type            # numpy dtype of Examples' array
    device: torch.dtype   # torch dtype of DeviceExamples' tensor (uint64 on the host = int64 bit patterns on the device)
    na: bool              # [n, NA] instead of [n]
    optional: bool        # None = the rows do not carry it
    label: str            # what concat's all-or-none message calls an optional column
    meaning: str


COLUMNS = (  # in the dataclasses' field order (`size`, the board size, stands between ply and kl)
    Column("own", np.uint64, torch.int64, False, False, None, "the side to move's stones: canonical bitboard (the bitboard form of "
           "generate_training_games.py:17-18)"),
    Column("opp", np.uint64, torch.int64, False, False, None, "the opponent's stones"),
    Column("pi", np.float32, torch.float32, True, False, None, "the search's policy target"),
    Column("z", np.int8, torch.int8, False, False, None, "the game's outcome for the mover, in {-1, 0, +1}"),
    Column("mover", np.int8, torch.int8, False, False, None, "the side to move in absolute colours, +1 / -1"),
    Column("act", np.uint8, torch.uint8, False, False, None, "the move played"),
    Column("game", np.int64, torch.int64, False, False, None, "global game id"),
    Column("ply", np.int32, torch.int32, False, False, None, "row index inside its game"),
    Column("kl", np.float32, torch.float32, False, True, "policy surprise", "policy surprise (DESIGN.md 3.17): KL(pi || raw prior); None = "
           "not recorded"),
    Column("q", np.float32, torch.float32, False, True, "search value", "search value (DESIGN.md 3.18): the root's sum W / sum N for the "
           "mover; None = not recorded"),
    Column("vt", np.float32, torch.float32, False, True, "value target", "value target (DESIGN.md 3.18, betazero_amd.value_targets); None "
           "= train on z"),
    Column("fown", np.uint64, torch.int64, False, True, "ownership target", "ownership target (DESIGN.md 3.22): the final board of the "
           "row's game in the row's side-to-move frame -- cell i is worth bit_i(fown) - bit_i(fopp); None = not recorded"),
    Column("fopp", np.uint64, torch.int64, False, True, "ownership target", "the other half of the ownership target"),
    Column("count", np.int32, torch.int32, False, True, "merge count", "position averaging (DESIGN.md 3.26): the rows merged into this "
           "one; None = not merged"),
)
COLUMN = {c.name: c for c in COLUMNS}


def _u64(t):
    """int64 tensor holding uint64 bit patterns -> numpy uint64"""
    return t.cpu().numpy().view(np.uint64)


@dataclass
class Examples:
    """(s, pi, z) rows on the host, numpy arrays of the columns' host dtypes (COLUMNS says what each column is)."""
    own: np.ndarray
    opp: np.ndarray
    pi: np.ndarray
    z: np.ndarray
    mover: np.ndarray
    act: np.ndarray
    game: np.ndarray
    ply: np.ndarray
    size: int
    kl: np.ndarray = None
    q: np.ndarray = None
    vt: np.ndarray = None
    fown: np.ndarray = None
    fopp: np.ndarray = None
    count: np.ndarray = None

    def __len__(self):
        return self.own.shape[0]

    def states(self):
        """canonical boards [n, size, size] int8: +1 = side to move, -1 = opponent"""
        s = self.size
        stride = 3 if s == 3 else 8
        sh = np.array([[stride * r + c for c in range(s)] for r in range(s)], dtype=np.uint64)
        a = ((self.own[:, None, None] >> sh) & np.uint64(1)).astype(np.int8)
        b = ((self.opp[:, None, None] >> sh) & np.uint64(1)).astype(np.int8)
        return a - b


@dataclass
class DeviceExamples:
    """The same rows as Examples, as torch tensors of the columns' device dtypes living on the GPU: what the device-resident
    pipeline gather -> augment -> train passes along (SL/train.py:24-52 then :85-136 in the reference's pipeline)."""
    own: torch.Tensor
    opp: torch.Tensor
    pi: torch.Tensor
    z: torch.Tensor
    mover: torch.Tensor
    act: torch.Tensor
    game: torch.Tensor
    ply: torch.Tensor
    size: int
    kl: torch.Tensor = None
    q: torch.Tensor = None
    vt: torch.Tensor = None
    fown: torch.Tensor = None
    fopp: torch.Tensor = None
    count: torch.Tensor = None

    def __len__(self):
        return int(self.own.shape[0])

    def cpu(self):
        """-> Examples (numpy, host): the arrays as they are, the bit patterns as uint64, ply as int32"""
        def host(c, t):
            a = t.cpu().numpy()
            return a.view(np.uint64) if c.host is np.uint64 else a.astype(np.int32) if c.name == "ply" else a
        return Examples(size=self.size, **{k: host(COLUMN[k], t) for k, t in columns(self).items()})

    @staticmethod
    def from_host(ex, device="cuda:0"):
        """Examples -> DeviceExamples on `device`, every column cast to its dtype of the table"""
        def dev(c, a):
            a = np.asarray(a, c.host)
            return torch.as_tensor(np.ascontiguousarray(a.view(np.int64) if c.host is np.uint64 else a)).to(device)
        return DeviceExamples(size=ex.size, **{k: dev(COLUMN[k], a) for k, a in columns(ex).items()})

    def states(self):
        """canonical boards [n, size, size] int8 on the device: +1 = side to move, -1 = opponent"""
        s = self.size
        stride = 3 if s == 3 else 8
        sh = torch.tensor([[stride * r + c for c in range(s)] for r in range(s)], dtype=torch.int64, device=self.own.device)
        a = ((self.own[:, None, None] >> sh) & 1).to(torch.int8)
        b = ((self.opp[:, None, None] >> sh) & 1).to(torch.int8)
        return a - b


def columns(ex):
    """{name: array} of the columns the rows carry, in the table's order (Examples or DeviceExamples)"""
    return {c.name: getattr(ex, c.name) for c in COLUMNS if getattr(ex, c.name) is not None}


def take(ex, idx):
    """the rows `idx` (an index array where the rows live) of ex, as the same type: every column the rows carry"""
    return type(ex)(size=ex.size, **{k: a[idx] for k, a in columns(ex).items()})


def concat(parts):
    """the parts' rows one after the other (all Examples or all DeviceExamples); an optional column is carried by every part
    or by none -- a mixture has no meaningful concatenation"""
    cat = np.concatenate if isinstance(parts[0], Examples) else torch.cat
    cols = {}
    for c in COLUMNS:
        have = [getattr(p, c.name) is not None for p in parts]
        if c.optional and any(have) and not all(have):
            raise ValueError(f"concatenating examples: every part must carry {c.name} ({c.label}), or none")
        if all(have):
            cols[c.name] = cat([getattr(p, c.name) for p in parts])
    return type(parts[0])(size=parts[0].size, **cols)


concat_examples = concat_device_examples = concat


# ---------------------------------------------------------------- the engine's example block (include/bz_abi.h)
EX_MAGIC = 0x425A455841000002
_EX_FIELDS = (("own", torch.int64, 8), ("opp", torch.int64, 8), ("pi", torch.float32, 4), ("z", torch.int8, 1),
              ("mover", torch.int8, 1), ("act", torch.uint8, 1), ("len", torch.int32, 4), ("winner", torch.int8, 1))


def example_block_views(block):
    """uint8 example block (device or host tensor) -> (dict of [R,B,T,...] tensor views, meta dict).
    The block describes itself through its trailing 256-byte header (include/bz_abi.h)."""
    meta = block[-256:].cpu().numpy().view(np.uint64)
    if int(meta[0]) != EX_MAGIC:
        raise ValueError("not a betazero_amd example block (bad magic)")
    base, stride, B, R, T, na, game = (int(v) for v in meta[1:8])
    offs = [int(v) for v in meta[8:16]]
    shapes = {"own": (R, B, T), "opp": (R, B, T), "pi": (R, B, T, na), "z": (R, B, T), "mover": (R, B, T),
              "act": (R, B, T), "len": (R, B), "winner": (R, B)}
    out = {}
    for (name, dt, esz), off in zip(_EX_FIELDS, offs):
        n = int(np.prod(shapes[name])) * esz
        out[name] = block[off:off + n].view(dt).view(*shapes[name])
    return out, {"game_id_base": base, "game_id_stride": stride, "B": B, "rounds": R, "t_max": T, "na": na,
                 "game": game, "size": _SIZES[game]}


def build_example_block(arrays, game_id_base, game_id_stride, game, device="cpu"):
    """host-side constructor of an example block with the engine's exact layout (256-byte aligned
    arrays + header): `arrays` = dict of [R,B,T,...] tensors as example_tensors() returns them.
    Used to re-load saved examples and by the CPU rehearsal of the multi-GPU path."""
    R, B, T = arrays["own"].shape
    na = arrays["pi"].shape[-1]
    offs, off = [], 0
    for name, dt, esz in _EX_FIELDS:
        offs.append(off)
        off += (arrays[name].numel() * esz + 255) & ~255
    block = torch.zeros(off + 256, dtype=torch.uint8, device=device)
    for (name, dt, esz), o in zip(_EX_FIELDS, offs):
        a = arrays[name].to(device=device, dtype=dt).contiguous()
        block[o:o + a.numel() * esz] = a.view(torch.uint8).reshape(-1)
    meta = np.zeros(32, np.uint64)
    meta[0:8] = [EX_MAGIC, game_id_base, game_id_stride, B, R, T, na, _GAMES[game]]
    meta[8:16] = offs
    block[off:off + 256] = torch.from_numpy(meta.view(np.uint8).copy()).to(device)
    return block


def unpack_example_block(block):
    """example block -> compact Examples of the finished games; the row selection runs where the
    block lives (on the GPU for a device block), so only valid rows are copied to the host"""
    t, m = example_block_views(block)
    T = m["t_max"]
    valid = torch.arange(T, device=block.device)[None, None, :] < t["len"][:, :, None]
    r, b, k = valid.nonzero(as_tuple=True)
    pick = lambda a: a[r, b, k].cpu().numpy()  # noqa: E731
    gid = m["game_id_base"] + r.cpu().numpy().astype(np.int64) * m["game_id_stride"] + b.cpu().numpy()
    return Examples(own=pick(t["own"]).view(np.uint64), opp=pick(t["opp"]).view(np.uint64), pi=pick(t["pi"]),
                    z=pick(t["z"]), mover=pick(t["mover"]), act=pick(t["act"]), game=gid,
                    ply=k.cpu().numpy().astype(np.int32), size=m["size"])


def unpack_example_block_device(block, geom):
    """device example block -> DeviceExamples of the finished games, entirely on the device: the array views come from
    `geom` (SelfPlayEngine.block_geometry() of an engine with the same configuration -- every rank's engines are built
    alike), the game-id base / stride are read from the block's own header AS DEVICE SCALARS, the row selection is a
    device-side nonzero().  No example data is copied to the host: the only host visits are the 112-byte header check and
    the size read-back of nonzero()."""
    R, B, T, na = geom["rounds"], geom["B"], geom["t_max"], geom["na"]
    assert block.numel() == geom["ex_bytes"], "example block of another geometry"
    # the block's own header must say what `geom` says (a peer built with another configuration can have the same byte
    # size): magic and words 3..15 (B, rounds, t_max, NA, game, the 8 array offsets) compared on the device
    want = torch.tensor([EX_MAGIC, B, R, T, na, geom["game"]] + list(geom["offs"]), dtype=torch.int64)
    got = block[-256:].view(torch.int64)
    if not torch.equal(torch.cat([got[0:1], got[3:16]]).cpu(), want):
        raise ValueError("example block does not have the local engine's geometry (header words differ)")
    shapes = {"own": (R, B, T), "opp": (R, B, T), "pi": (R, B, T, na), "z": (R, B, T), "mover": (R, B, T),
              "act": (R, B, T), "len": (R, B), "winner": (R, B)}
    t = {}
    for (name, dt, esz), off in zip(_EX_FIELDS, geom["offs"]):
        n = int(np.prod(shapes[name])) * esz
        t[name] = block[off:off + n].view(dt).view(*shapes[name])
    meta = block[-256:].view(torch.int64)  # header words: [1] = game-id base, [2] = stride (device scalars)
    valid = torch.arange(T, device=block.device)[None, None, :] < t["len"][:, :, None]
    r, b, k = valid.nonzero(as_tuple=True)
    pick = lambda a: a[r, b, k]  # noqa: E731
    return DeviceExamples(own=pick(t["own"]), opp=pick(t["opp"]), pi=pick(t["pi"]), z=pick(t["z"]), mover=pick(t["mover"]),
                          act=pick(t["act"]), game=meta[1] + r * meta[2] + b, ply=k.to(torch.int32), size=geom["size"])


# ---------------------------------------------------------------- packed example blocks (include/bz_abi.h)
PACKED_MAGIC = 0x425A50414B000001
_PK_FIELDS = (("own", torch.int64), ("opp", torch.int64), ("pi", torch.float32), ("game", torch.int64),
              ("z", torch.int8), ("mover", torch.int8), ("act", torch.uint8), ("ply", torch.uint8))


def packed_layout(na, cap_rows):
    """(byte offsets of the 8 arrays, total bytes) of a packed example block: 256-byte header, then own, opp, pi,
    game id, z, mover, act, ply -- each at a multiple of 256 bytes (== bz_examples_packed_bytes)"""
    offs, off = [], 256
    for esz in (8, 8, 4 * na, 8, 1, 1, 1, 1):
        offs.append(off)
        off += (cap_rows * esz + 255) & ~255
    return offs, off


def alloc_packed_block(na, cap_rows, device="cuda:0"):
    """an (uninitialised) packed example block: 1-D uint8 tensor, 256-byte aligned"""
    _, total = packed_layout(na, cap_rows)
    t = torch.empty(total + 256, dtype=torch.uint8, device=device)
    pad = (-t.data_ptr()) & 255
    return t[pad:pad + total]


def packed_block_header(block, strict=True):
    """the block's header as a dict (ONE 256-byte copy to the host when the block lives on a GPU).  strict: raise when
    the block overflowed (rows of finished games did not fit) -- unpacking such a block would silently lose games;
    strict=False only reports `dropped_rows` (bench.py's post-mortem of its own capacity estimate)."""
    h = block[:256].cpu().numpy().view(np.uint64)
    if int(h[0]) != PACKED_MAGIC:
        raise ValueError("not a betazero_amd packed example block (bad magic)")
    d = {"n_rows": int(h[1]), "n_games": int(h[2]), "cap_rows": int(h[3]), "na": int(h[4]), "game": int(h[5]),
         "dropped_rows": int(h[6]), "bytes": int(h[7]), "offs": [int(v) for v in h[8:16]]}
    if d["dropped_rows"] and strict:
        raise RuntimeError("packed example block overflow: " +
                           ("an engine of another geometry was appended" if d["dropped_rows"] == 2**64 - 1 else
                            f"{d['dropped_rows']} rows of finished games did not fit into cap_rows = {d['cap_rows']}"))
    return d


def _packed_views(block, h):
    n, na = h["n_rows"], h["na"]
    out = {}
    for (name, dt), off in zip(_PK_FIELDS, h["offs"]):
        per = na if name == "pi" else 1
        esz = torch.empty((), dtype=dt).element_size()
        v = block[off:off + n * per * esz].view(dt)
        out[name] = v.view(n, na) if name == "pi" else v
    return out


def unpack_packed_block_device(block):
    """packed example block on a GPU -> DeviceExamples (views of its first n_rows rows; one header read-back)"""
    h = packed_block_header(block)
    v = _packed_views(block, h)
    return DeviceExamples(own=v["own"], opp=v["opp"], pi=v["pi"], z=v["z"], mover=v["mover"], act=v["act"], game=v["game"],
                          ply=v["ply"].to(torch.int32), size=_SIZES[h["game"]])


def unpack_packed_block(block):
    """packed example block (device or host) -> host Examples; only the valid rows are copied"""
    h = packed_block_header(block)
    v = {k: t.cpu().numpy() for k, t in _packed_views(block, h).items()}
    return Examples(own=v["own"].view(np.uint64), opp=v["opp"].view(np.uint64), pi=v["pi"], z=v["z"], mover=v["mover"],
                    act=v["act"], game=v["game"], ply=v["ply"].astype(np.int32), size=_SIZES[h["game"]])


def build_packed_block(ex, cap_rows, game, device="cpu"):
    """host-side constructor of a packed block from Examples (saved examples, and the CPU rehearsal of the multi-GPU
    path): the same bytes bz_engine_pack_examples writes for these rows"""
    n, na = len(ex), int(ex.pi.shape[1])
    assert n <= cap_rows
    offs, total = packed_layout(na, cap_rows)
    block = torch.zeros(total, dtype=torch.uint8)
    hdr = np.zeros(32, np.uint64)
    hdr[0:8] = [PACKED_MAGIC, n, len(np.unique(ex.game)), cap_rows, na, _GAMES[game], 0, total]
    hdr[8:16] = offs
    block[:256] = torch.from_numpy(hdr.view(np.uint8).copy())
    src = {"own": ex.own.view(np.int64), "opp": ex.opp.view(np.int64), "pi": ex.pi.astype(np.float32),
           "game": np.asarray(ex.game, np.int64), "z": ex.z.astype(np.int8), "mover": ex.mover.astype(np.int8),
           "act": ex.act.astype(np.uint8), "ply": np.asarray(ex.ply).astype(np.uint8)}
    for (name, dt), off in zip(_PK_FIELDS, offs):
        a = torch.from_numpy(np.ascontiguousarray(src[name])).view(torch.uint8).reshape(-1)
        block[off:off + a.numel()] = a
    return block.to(device)
