#!/usr/bin/env python3
"""Search the chunk placements of the edge-aware tower tiling (csrc/bz_tile_map.h) on the CPU.

A placement puts 16-byte chunk ch of cell (row y, column x) of position p at slot sigma((ch + A x + B y + G p) mod 16) of
its 256-byte cell, sigma(s) = s >> 1 | (s & 1) << 3: additive, so a conv tap's shift adds the same constant for every lane
and a lane group that is conflict-free for one tap is so for all nine (and for every k-step, which adds 4 kq).

Bank model (ds_read_b128 on CDNA4): the 16-byte slot of an address is (address / 16) mod 16; a wave's 64 lanes are served
in four groups of 16 -- lanes {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32 -- and a group is conflict-free
when its lanes hit 16 distinct slots.  With lane = 16 g + c (g = the MFMA's k-group, which reads chunk 4 kq + g; c = the
tile's lane column), a group holds every c once: c in S0 = {0-3, 12-15} with one chunk parity and c in S1 = {4-11} with
the other.  So a tile of 16 (p, y, x) pairs can be cut into conflict-free halves exactly when v = A x + B y + G p takes
every value of ONE parity class exactly twice over the tile (each half then takes the class once).  The 8-byte epilogue
stores (ds_write_b64: groups of 16 consecutive lanes = one g, every c; banks mod 128 B) are 2-way under the same condition.

The script enumerates (A, B, G) in Z16^3 for the fixed edge tiles (rows 0 / 7 x 2 positions, columns 0 / 7 x rows 1..4,
columns {0, 7} x rows 5..6) and for the four ways to cut the 6 x 6 interior into nine translates of one 2 x 2 shape
(row / column stride 1 or 3), prints the survivors, and then checks the lane cut of bz_tile_map.h for the chosen placement
group by group.  usage: python tools/search_tile_placement.py"""
import itertools
from collections import Counter

S0 = (0, 1, 2, 3, 12, 13, 14, 15)
S1 = tuple(range(4, 12))


def sigma(s):
    return (s >> 1) | ((s & 1) << 3)


def edge_tiles():
    tiles = []
    for y in (0, 7):
        for b in (0, 1):
            tiles.append([(2 * b + q, y, x) for q in (0, 1) for x in range(8)])
    for x in (0, 7):
        tiles.append([(p, y, x) for p in range(4) for y in range(1, 5)])
    tiles.append([(p, y, x) for p in range(4) for y in (5, 6) for x in (0, 7)])
    return tiles


def interior_tiles(sy, sx):
    oy = (1, 3, 5) if sy == 1 else (1, 2, 3)
    ox = (1, 3, 5) if sx == 1 else (1, 2, 3)
    return [[(p, y0 + sy * i, x0 + sx * j) for p in range(4) for i in (0, 1) for j in (0, 1)] for y0 in oy for x0 in ox]


def cuttable(tile, A, B, G):
    v = Counter((A * x + B * y + G * p) & 15 for p, y, x in tile)
    return len({k & 1 for k in v}) == 1 and len(v) == 8 and set(v.values()) == {2}


def survivors():
    out = []
    for A, B, G in itertools.product(range(16), repeat=3):
        if not all(cuttable(t, A, B, G) for t in edge_tiles()):
            continue
        for sy, sx in itertools.product((1, 3), repeat=2):
            tiles = interior_tiles(sy, sx)
            assert sorted(c for t in tiles for c in t) == sorted((p, y, x) for p in range(4) for y in range(1, 7) for x in range(1, 7))
            if all(cuttable(t, A, B, G) for t in tiles):
                out.append((A, B, G, sy, sx))
    return out


# ---- the lane cut of bz_tile_map.h, written out again (tests/test_tower_tile_map_cpu.py checks the header itself)
def half(c):
    return ((c + 4) >> 3) & 1


def chosen_tiles():
    tiles = []
    for t in range(16):
        row = []
        for c in range(16):
            h, i = half(c), c & 7
            if t < 4:
                row.append((2 * (t & 1) + h, 7 * (t >> 1), i))
            elif t < 6:
                row.append((2 * (i >> 2) + h, 1 + (i & 3), 7 * (t - 4)))
            elif t == 6:
                row.append((i & 3, 5 + (i >> 2), 7 * h))
            else:
                row.append((i >> 1, 1 + 2 * ((t - 7) // 3) + h, 1 + 2 * ((t - 7) % 3) + (i & 1)))
        tiles.append(row)
    return tiles


def check_chosen(A=2, B=2, G=4):
    tiles = chosen_tiles()
    assert sorted(c for t in tiles for c in t) == sorted((p, y, x) for p in range(4) for y in range(8) for x in range(8))
    worst_store = 0
    for t, tap, kq, g0 in itertools.product(range(16), range(9), range(4), (0, 2)):
        dy, dx = tap // 3 - 1, tap % 3 - 1
        for first in (S0, S1):  # the two lane groups of a 32-lane half: `first` reads chunk 4 kq + g0, the rest + 1
            slots = set()
            for c in range(16):
                p, y, x = tiles[t][c]
                ch = 4 * kq + g0 + (0 if c in first else 1)
                slots.add(sigma((ch + A * (x + dx) + B * (y + dy) + G * p) & 15))
            assert len(slots) == 16, (t, tap, kq, g0)
    for t, ch in itertools.product(range(16), range(16)):  # epilogue: 16 lanes of one g, 8-byte stores, banks mod 128 B
        n = Counter(sigma((ch + A * x + B * y + G * p) & 15) & 7 for p, y, x in tiles[t])
        worst_store = max(worst_store, max(n.values()))
    return worst_store


def main():
    surv = survivors()
    place = sorted({s[:3] for s in surv})
    print(f"{len(place)} of {16 ** 3} placements (A, B, G) leave every tile cuttable, each with all four interior cuts: {len(surv) == 4 * len(place)}")
    print("all coefficients even:", all(v % 2 == 0 for s in place for v in s))
    print("with A = 2 (the column-only placement's coefficient):", [s for s in place if s[0] == 2])
    print("bz_tile_map.h's cut with (2, 2, 4): every read group conflict-free; epilogue stores", f"{check_chosen()}-way")


if __name__ == "__main__":
    main()
