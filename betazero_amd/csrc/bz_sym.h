// bz_sym.h -- the eight board symmetries of the evaluator, shared by the host entry points
// (bz_sym_index / bz_sym_board / bz_sym_action_map) and the symmetric net kernels of bz_net.hip.
//
// Elements s = 0..7.  0..6 are d4_src's transforms 0..6 (bz_env.hip, the reference's order, SL/train.py:27-36):
//   0 id, 1 flip rows, 2 flip columns, 3 rot90 x1, 4 rot90 x2, 5 rot90 x3, 6 transpose;
//   7 is the anti-transpose out[r][c] = x[n-1-c][n-1-r].  The reference's own list lacks it: its entry 7
//   (flip(dims=[0]).t()) equals its entry 5 under torch semantics, which k_augment_d4 reproduces as is.
// T_s is "out[r][c] = x[src_s(r, c)]" on the n x n corner of the 8x8 plane (bit = 8 row + col for every size);
// tau_s is the cell permutation it induces: a stone on cell j moves to tau_s(j).  Cells outside the corner and the
// pass action (64) stay where they are, so tau_s is a permutation of 0..63 for every size.
//
// Every element is "transpose or not, then flip rows or not, then flip columns or not":
//   out = Fc^fc(Fr^fr(Tr^tr(x))),  (tr, fr, fc) bit s of (0xE8, 0x9A, 0xB4)
// e.g. s = 3: out[r][c] = x[c][n-1-r] = Tr(x)[n-1-r][c].  On the bitboard the three steps are word arithmetic: three
// delta swaps, a byte swap, a bit reversal inside the bytes; a flip of the 8x8 plane leaves an n x n corner at the far
// edge, and one shift brings it back.
#pragma once
#include "bz_rules.h"

namespace bz_sym {
using bz::u64;
using bz::u32;

constexpr u32 kTr = 0xE8u, kFr = 0x9Au, kFc = 0xB4u;  // bit s: does element s transpose / flip rows / flip columns

// SplitMix-style hash of (position, seed) -> symmetry index 0..7; 64-bit wrapping arithmetic
BZ_HD u32 index(u64 seed, u64 own, u64 opp) {
    u64 h = seed ^ (own * 0x9E3779B97F4A7C15ULL);
    h = (h ^ (h >> 29)) * 0xBF58476D1CE4E5B9ULL;
    h ^= opp * 0xC2B2AE3D27D4EB4FULL;
    h = (h ^ (h >> 32)) * 0x94D049BB133111EBULL;
    return (u32)((h ^ (h >> 31)) >> 61);
}

// rows < n, columns < n of the 8x8 plane
BZ_HD u64 corner(int n) {
    const u64 cols = ((1ULL << n) - 1ULL) * 0x0101010101010101ULL;
    return n >= 8 ? ~0ULL : cols & ((1ULL << (8 * n)) - 1ULL);
}
BZ_HD u64 transpose8(u64 x) {  // bit 8r + c <-> bit 8c + r: three delta swaps
    u64 t = (x ^ (x >> 7)) & 0x00AA00AA00AA00AAULL;
    x ^= t ^ (t << 7);
    t = (x ^ (x >> 14)) & 0x0000CCCC0000CCCCULL;
    x ^= t ^ (t << 14);
    t = (x ^ (x >> 28)) & 0x00000000F0F0F0F0ULL;
    x ^= t ^ (t << 28);
    return x;
}
BZ_HD u64 flip_rows8(u64 x) { return __builtin_bswap64(x); }                            // row r -> 7 - r
BZ_HD u64 flip_cols8(u64 x) { return __builtin_bswap64(__builtin_bitreverse64(x)); }    // column c -> 7 - c

// T_s on the n x n corner of b; bits outside the corner stay where they are
BZ_HD u64 board(u64 b, int n, u32 s) {
    const u64 m = corner(n);
    u64 x = b & m;
    const u64 t = transpose8(x);
    x = (kTr >> s) & 1u ? t : x;
    const u64 fr = flip_rows8(x) >> (8 * (8 - n));
    x = (kFr >> s) & 1u ? fr : x;
    const u64 fc = flip_cols8(x) >> (8 - n);
    x = (kFc >> s) & 1u ? fc : x;
    return x | (b & ~m);
}

// tau_s(j): where a stone on cell j goes (j in 0..64; 64 = pass)
BZ_HD int tau(int n, u32 s, int j) {
    int r = j >> 3, c = j & 7;
    if (r >= n || c >= n) return j;  // off the corner, and the pass action (row 8)
    if ((kTr >> s) & 1u) { const int t = r; r = c; c = t; }
    if ((kFr >> s) & 1u) r = n - 1 - r;
    if ((kFc >> s) & 1u) c = n - 1 - c;
    return 8 * r + c;
}
// the cell that T_s moves onto cell a: tau_s(tau_inv(a)) = a (the flips undone first, then the transpose)
BZ_HD int tau_inv(int n, u32 s, int a) {
    int r = a >> 3, c = a & 7;
    if (r >= n || c >= n) return a;
    if ((kFr >> s) & 1u) r = n - 1 - r;
    if ((kFc >> s) & 1u) c = n - 1 - c;
    if ((kTr >> s) & 1u) { const int t = r; r = c; c = t; }
    return 8 * r + c;
}

// what a symmetric net kernel is told: mode BZ_SYM_FIXED (arg = s) or BZ_SYM_HASHED (arg = seed), and the board size
struct Args {
    u64 arg;
    int hashed, size;
};
// the symmetry of a row, from its UNTRANSFORMED bitboards
BZ_HD u32 of(const Args& y, u64 own, u64 opp) { return y.hashed ? index(y.arg, own, opp) : (u32)y.arg & 7u; }

}  // namespace bz_sym
