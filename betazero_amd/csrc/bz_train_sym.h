// bz_train_sym.h -- a board symmetry per row of a training batch: batch position p trains on row idx[p] of
// the data set under the element sym[p] of bz_sym.h.  The per-row rule, __host__ __device__ so that bz_train_sym_row (host) is
// the code k_train_sym_batch runs:
//   own, opp, fown, fopp  ->  bz_sym::board(b, size, s)
//   pi'[tau_s(j)] = pi[j], i.e. staged action a reads source action tau_inv(a); the pass entry (64) and the cells outside
//   the size x size corner stay in place.  The policy row is MOVED, never computed on: its entries travel as 32-bit patterns.
//   z, vt are copied.
#pragma once
#include "bz_sym.h"

namespace bz_train_sym {
using bz::u64;
using bz::u32;

// the row of batch position p: idx clamped into the data set as bz_train_ends.hip's batch_row clamps it
BZ_HD long long clamp_row(long long r, long long n_rows) {
    r = r < 0 ? 0 : r;
    return r < n_rows ? r : (n_rows > 0 ? n_rows - 1 : 0);
}
BZ_HD bool row_bad(long long r, long long n_rows) { return r < 0 || r >= n_rows; }
// a symmetry outside 0..7 is an error of the caller like an index outside the data set: counted, and taken & 7
BZ_HD bool sym_bad(u32 s) { return s > 7u; }
BZ_HD u32 sym_of(u32 s) { return s & 7u; }

BZ_HD u64 board(u64 b, int size, u32 s) { return bz_sym::board(b, size, s); }
// the source action whose policy entry lands on staged action a (a in 0..64)
BZ_HD int pi_source(int size, u32 s, int a) { return bz_sym::tau_inv(size, s, a); }

}  // namespace bz_train_sym
