// bz_tile_map.h -- the edge-aware cell tiling of the 128-channel throughput tower (Tw<128, 4, true, 1> in bz_tower.h,
// kernel k_edge_bf16 in bz_net.hip).  Plain constexpr C++: device code and host programs (the CPU test,
// tools/search_tile_placement.py's twin) read the same tables.
//
// A wave owns 32 output channels x 4 positions x 64 cells = 256 (position, cell) pairs = 16 N-tiles of a
// v_mfma_f32_16x16x32_bf16.  The pitch-9 LDS image gives every pair the same address offset per conv tap, so a tile may
// hold ANY 16 pairs; this map makes the board's edge cells tiles of their own, so that a tap which shifts them onto the
// zero halo skips the whole tile (its MFMAs and its ds_read_b128), along x as well as along y:
//   tile  0, 1   R  board row 0, columns 0..7, positions {0,1} / {2,3}      skipped for dy = -1
//   tile  2, 3   R  board row 7, likewise                                  skipped for dy = +1
//   tile  4      C  column 0, rows 1..4, positions 0..3                     skipped for dx = -1
//   tile  5      C  column 7, rows 1..4, positions 0..3                     skipped for dx = +1
//   tile  6      M  columns 0 and 7, rows 5..6, positions 0..3              never skipped
//   tile  7..15  I  the 2 x 2 block at row 1 + 2 i, column 1 + 2 j, positions 0..3 (i, j = 0..2)   never skipped
// 13..16 tiles per tap, 126 tile-taps per layer of 144 (the row skip alone: 132).  No lane of a tile that is not skipped
// reads board row -1 or 8 (the corners sit in the row tiles), so the image needs no zero rows.
//
// Lane column c (0..15) of a tile is pair (tile origin + lane part of the tile's pattern).  The 16 lanes of a
// ds_read_b128 lane group hold every c once: the eight c with half(c) = 0 read one 16-byte chunk of their cells, the
// eight with half(c) = 1 the next chunk (or the previous one: the second group of the same 32 lanes).  half(c) = bit 3 of
// c + 4 -- c = 0..3, 12..15 against c = 4..11 -- and idx(c) = c & 7 counts through either half.
//
// Chunk placement.  Chunk ch of cell (row y, column x) of position p sits at 16-byte position
//   sigma((ch + 2 x + 2 y + 4 p) mod 16),   sigma(s) = s >> 1 | (s & 1) << 3
// of its 256-byte cell -- additive over (chunk, column, row, position), so a tap's shift moves every lane's slot alike and
// what holds for one tap holds for all nine.  With w = (x + y + 2 p) mod 8, a lane group is conflict-free exactly when each
// half of the tile maps ONTO the eight values of w (the chunk parity then separates the halves: slots 2 w and 2 w + 1).
// The patterns below are cut that way: R: w = idx;  C: w = idx + 2 half;  M: w = 2 (idx & 3) + (idx >> 2);  I: w = idx.
// Every tile thus covers each w twice, which is also what the epilogue's 8-byte stores need: a 16-lane store group lands on
// each of the eight 16-byte positions mod 128 B twice (2-way, as the column-only placement pos16 had it).  The row must
// enter w (a column tile has nothing else to tell its four rows apart), which the column-only placement cannot give.
// tools/search_tile_placement.py enumerates every (A, B, G) of sigma((ch + A x + B y + G p) mod 16) against every tile and
// prints the ones that leave each tile such a cut: 56 placements, all with even coefficients; (2, 2, 4) keeps the old
// coefficient of x and is the smallest of them.
// Because the slot depends on the row now, a tile's slot differs from its pattern's by a compile-time rotation: the
// kernel keeps, per pattern, the lane's offset for each of the eight rotations u (slot_rot) and picks one by tile, tap
// and k-step at compile time -- nothing is recomputed between taps, a tap's (dy, dx) is an immediate offset plus a rotation.
#pragma once
#if defined(__HIPCC__)
#define BZ_TM_FN __host__ __device__ constexpr
#else
#define BZ_TM_FN constexpr
#endif

namespace bz_tile_map {
constexpr int kTiles = 16;      // N-tiles per wave
constexpr int kPairs = 16;      // (position, cell) pairs per tile = lane columns of the MFMA
constexpr int kRowC = 9;        // cells per board-row pitch of the LDS image
constexpr int kNCell = 73;      // cells per position of the LDS image
enum { kRow = 0, kCol = 1, kMix = 2, kIn = 3, kPatterns = 4 };

BZ_TM_FN int pattern(int t) { return t < 4 ? kRow : t < 6 ? kCol : t == 6 ? kMix : kIn; }
// tile origin: position, board row, column
BZ_TM_FN int tile_p(int t) { return t < 4 ? 2 * (t & 1) : 0; }
BZ_TM_FN int tile_y(int t) { return t < 4 ? 7 * (t >> 1) : t < 6 ? 1 : t == 6 ? 5 : 1 + 2 * ((t - 7) / 3); }
BZ_TM_FN int tile_x(int t) { return t < 5 ? 0 : t == 5 ? 7 : t == 6 ? 0 : 1 + 2 * ((t - 7) % 3); }
// lane column c of a pattern: its half of the ds_read_b128 lane group, its index there, and the pair relative to the origin
BZ_TM_FN int half(int c) { return ((c + 4) >> 3) & 1; }
BZ_TM_FN int idx(int c) { return c & 7; }
BZ_TM_FN int lane_p(int pat, int c) {
    return pat == kRow ? half(c) : pat == kCol ? 2 * (idx(c) >> 2) + half(c) : pat == kMix ? idx(c) & 3 : idx(c) >> 1;
}
BZ_TM_FN int lane_y(int pat, int c) { return pat == kRow ? 0 : pat == kCol ? idx(c) & 3 : pat == kMix ? idx(c) >> 2 : half(c); }
BZ_TM_FN int lane_x(int pat, int c) { return pat == kRow ? idx(c) : pat == kCol ? 0 : pat == kMix ? 7 * half(c) : idx(c) & 1; }
// pair c of tile t
BZ_TM_FN int pair_p(int t, int c) { return tile_p(t) + lane_p(pattern(t), c); }
BZ_TM_FN int pair_y(int t, int c) { return tile_y(t) + lane_y(pattern(t), c); }
BZ_TM_FN int pair_x(int t, int c) { return tile_x(t) + lane_x(pattern(t), c); }
// the same in cells of the LDS image (position pitch kNCell, row pitch kRowC, one leading zero cell): the lane part goes
// into a register, the tile part into the instruction's immediate offset
BZ_TM_FN int lane_cells(int pat, int c) { return lane_p(pat, c) * kNCell + lane_y(pat, c) * kRowC + lane_x(pat, c); }
BZ_TM_FN int tile_cells(int t) { return tile_p(t) * kNCell + tile_y(t) * kRowC + tile_x(t) + 1; }
BZ_TM_FN int tap_cells(int tap) { return (tap / 3 - 1) * kRowC + (tap % 3 - 1); }
// tap = 3 (dy + 1) + (dx + 1) reads only halo cells for every pair of tile t
BZ_TM_FN bool skip(int tap, int t) {
    return (t < 2 && tap / 3 == 0) || (t >= 2 && t < 4 && tap / 3 == 2) || (t == 4 && tap % 3 == 0) || (t == 5 && tap % 3 == 2);
}
BZ_TM_FN int tiles_of_tap(int tap) {
    int n = 0;
    for (int t = 0; t < kTiles; ++t) n += skip(tap, t) ? 0 : 1;
    return n;
}
BZ_TM_FN int tiles_of_half(int tap, int hf) {  // among the tiles 2 j + hf that one sub-step of the K-loop runs
    int n = 0;
    for (int t = hf; t < kTiles; t += 2) n += skip(tap, t) ? 0 : 1;
    return n;
}
// 16-byte position of chunk ch of cell (y, x) of position p inside the cell; x, y = -1 .. 8 (the halo keeps the rule)
BZ_TM_FN int sigma(int s) { return (s >> 1) | ((s & 1) << 3); }
BZ_TM_FN int slot(int ch, int p, int y, int x) { return sigma((ch + 2 * x + 2 * y + 4 * p) & 15); }
// ... = sigma(lane part + 2 rot): rot collects everything the lanes of a tile share and is even in s, so it rotates
// s >> 1 and leaves s & 1 alone.  lane_w: the lane's own part of w; `sub` = the odd rest the reader adds to the chunk
// index (the MFMA k-group g for the K-loop, g >> 1 for the epilogue).
BZ_TM_FN int lane_w(int pat, int c) { return lane_x(pat, c) + lane_y(pat, c) + 2 * lane_p(pat, c); }
BZ_TM_FN int slot_rot(int t, int tap, int ch_even) {  // ch_even: the even part of the chunk index
    return (ch_even / 2 + tile_x(t) + tile_y(t) + 2 * tile_p(t) + (tap / 3 - 1) + (tap % 3 - 1)) & 7;
}
BZ_TM_FN int lane_slot(int pat, int c, int sub, int rot) { return ((((sub >> 1) + lane_w(pat, c) + rot) & 7) | ((sub & 1) << 3)); }
constexpr int kCentre = 4;  // the tap with no shift (for addresses of the cells themselves: stem, epilogue, heads)
}  // namespace bz_tile_map
