// bz_pace.h -- pacing of a replay-seeded slot's walks over the launches of a move ("The replay seed"): a slot that
// starts its search with `seeded` simulations already in its tree has r = sims - seeded walks left and the move's `sims` launches
// to make them in.  It walks in launch L iff the running quota floor((L + 1) r / sims) moves past floor(L r / sims); the walk is
// then its simulation number seeded + floor(L r / sims).  Integer arithmetic, __host__ __device__ so that bz_pace_walk (host) is
// the code the paced step kernel runs: no feedback, exactly r walks, in order, the last one in launch sims - 1.
#pragma once
#include "bz_math.h"

namespace bz {

// walks made before launch L (0 <= L <= sims, r <= sims <= 8189: the product stays below 2^27)
BZ_HD u32 pace_done(u32 L, u32 r, u32 sims) { return (L * r) / sims; }
BZ_HD bool pace_walks(u32 L, u32 r, u32 sims) { return pace_done(L + 1u, r, sims) > pace_done(L, r, sims); }

// what the seed kernel leaves in a slot's `seeded` word when the slot has no search to run
constexpr u32 kPaceIdle = ~0u;

}  // namespace bz
