"""The tables of the edge-aware cell tiling (csrc/bz_tile_map.h), read from the header itself: a small host
program includes it, prints every table, and the properties the kernel rests on are checked here --
the 16 tiles partition the wave's 256 (position, cell) pairs; a tap skips a tile exactly when it shifts all 16 pairs off
the board, which leaves 126 tile-taps; no lane of a tile that runs reads board row -1 or 8 (the LDS image has no such
rows); the register + immediate split of an address is the address; and under the bank model of ds_read_b128 (slot =
address / 16 mod 16; lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32; lane = 16 g + c reads chunk
4 kq + g of the cell of lane column c) every group of every (tile, tap, k-step) hits 16 distinct slots, while the 8-byte
epilogue stores (16 consecutive lanes, banks mod 128 B) stay 2-way."""
import itertools
import os
import shutil
import subprocess
from collections import Counter

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
CELL, NCELL, ROWC = 256, 73, 9

PROGRAM = r"""
#include <cstdio>
#include "bz_tile_map.h"
using namespace bz_tile_map;
static_assert(tiles_of_tap(4) == 16 && tiles_of_tap(0) == 13, "the tables are compile-time constants");
int main() {
    for (int t = 0; t < kTiles; ++t) {
        printf("tile %d %d %d", t, pattern(t), tile_cells(t));
        for (int c = 0; c < kPairs; ++c) printf(" %d,%d,%d,%d", pair_p(t, c), pair_y(t, c), pair_x(t, c), lane_cells(pattern(t), c));
        printf("\n");
    }
    for (int tap = 0; tap < 9; ++tap) {
        printf("tap %d %d %d %d %d", tap, tap_cells(tap), tiles_of_tap(tap), tiles_of_half(tap, 0), tiles_of_half(tap, 1));
        for (int t = 0; t < kTiles; ++t) printf(" %d", (int)skip(tap, t));
        printf("\n");
    }
    for (int t = 0; t < kTiles; ++t)
        for (int tap = 0; tap < 9; ++tap)
            for (int ch = 0; ch < 16; ++ch) {  // ch = even part + sub: the K-loop's (4 kq, g) and the epilogue's (4 wt + 2 a, g >> 1)
                printf("slot %d %d %d", t, tap, ch);
                for (int c = 0; c < kPairs; ++c)
                    printf(" %d,%d,%d", slot(ch, pair_p(t, c), pair_y(t, c) + tap / 3 - 1, pair_x(t, c) + tap % 3 - 1),
                           lane_slot(pattern(t), c, ch & 3, slot_rot(t, tap, ch & ~3)),
                           lane_slot(pattern(t), c, ch & 1, slot_rot(t, tap, ch & ~1)));
                printf("\n");
            }
    return 0;
}
"""


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    if not os.path.exists(CXX):
        pytest.skip("needs a host C++ compiler")
    d = tmp_path_factory.mktemp("tile_map")
    (d / "dump.cpp").write_text(PROGRAM)
    subprocess.check_call([CXX, "-std=c++17", "-O1", "-I", os.path.join(ROOT, "betazero_amd", "csrc"), "-o", str(d / "dump"), str(d / "dump.cpp")])
    tiles, taps, slots = {}, {}, {}
    for line in subprocess.check_output([str(d / "dump")], text=True).splitlines():
        f = line.split()
        if f[0] == "tile":
            tiles[int(f[1])] = {"pattern": int(f[2]), "imm": int(f[3]), "pairs": [tuple(map(int, v.split(","))) for v in f[4:]]}
        elif f[0] == "tap":
            taps[int(f[1])] = {"cells": int(f[2]), "n": int(f[3]), "half": (int(f[4]), int(f[5])), "skip": [bool(int(v)) for v in f[6:]]}
        else:
            slots[(int(f[1]), int(f[2]), int(f[3]))] = [tuple(map(int, v.split(","))) for v in f[4:]]
    assert len(tiles) == 16 and len(taps) == 9 and len(slots) == 16 * 9 * 16
    return tiles, taps, slots


def test_tiles_partition_the_pairs(tables):
    tiles, _, _ = tables
    pairs = [(p, y, x) for t in range(16) for p, y, x, _ in tiles[t]["pairs"]]
    assert sorted(pairs) == sorted(itertools.product(range(4), range(8), range(8)))
    for t in range(16):  # every lane column of one pattern shares its lane part; the tile part is the immediate
        assert len(tiles[t]["pairs"]) == 16
        for p, y, x, lane in tiles[t]["pairs"]:
            assert lane + tiles[t]["imm"] == p * NCELL + y * ROWC + x + 1   # = cell_at(y, x) / CELL of position p
    for a, b in itertools.combinations(range(16), 2):
        if tiles[a]["pattern"] == tiles[b]["pattern"]:
            assert [q[3] for q in tiles[a]["pairs"]] == [q[3] for q in tiles[b]["pairs"]]


def test_skip_set_is_exactly_the_all_halo_tiles(tables):
    tiles, taps, _ = tables
    total = 0
    for tap in range(9):
        dy, dx = tap // 3 - 1, tap % 3 - 1
        assert taps[tap]["cells"] == dy * ROWC + dx
        for t in range(16):
            off = [not (0 <= y + dy < 8 and 0 <= x + dx < 8) for _, y, x, _ in tiles[t]["pairs"]]
            assert taps[tap]["skip"][t] == all(off), (tap, t)
            if not taps[tap]["skip"][t]:
                total += 1
                for p, y, x, lane in tiles[t]["pairs"]:
                    assert 0 <= y + dy < 8, (tap, t)           # rows -1 and 8 are not in the LDS image
                    assert -1 <= x + dx <= 8                   # columns -1 and 8 are its zero cells
                    assert 0 <= lane + tiles[t]["imm"] + taps[tap]["cells"] < 4 * NCELL
        assert taps[tap]["n"] == 16 - sum(taps[tap]["skip"]) and 13 <= taps[tap]["n"] <= 16
        assert taps[tap]["half"] == tuple(sum(not taps[tap]["skip"][t] for t in range(h, 16, 2)) for h in (0, 1))
    assert total == 126


def test_register_and_rotation_split_is_the_slot(tables):
    _, _, slots = tables
    for key, row in slots.items():
        for direct, kloop, epi in row:
            assert direct == kloop == epi, key


def test_read_groups_are_conflict_free_and_stores_two_way(tables):
    tiles, taps, slots = tables
    S0 = (0, 1, 2, 3, 12, 13, 14, 15)
    for t, tap in itertools.product(range(16), range(9)):
        if taps[tap]["skip"][t]:
            continue
        for kq, g0 in itertools.product(range(4), (0, 2)):
            for first in (0, 1):  # the two lane groups of 32 lanes: c in S0 reads k-group g0 + first, the others the other one
                hit = {slots[(t, tap, 4 * kq + g0 + (first if c in S0 else 1 - first))][c][0] for c in range(16)}
                assert len(hit) == 16, (t, tap, kq, g0, first)
    for t, ch in itertools.product(range(16), range(16)):  # the cells themselves (centre tap), one chunk, both 8-byte halves alike
        n = Counter(s[0] & 7 for s in slots[(t, 4, ch)])
        assert max(n.values()) <= 2, (t, ch)
