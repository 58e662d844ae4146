// bz_resign.h -- resignation in self-play: the streak rule a search's root value goes through and the draw that
// marks a game as played out, __host__ __device__ so that bz_resign_step / bz_resign_playout (host) are the code the kernels run.
// One float32 comparison and integer arithmetic: nothing rounds.
#pragma once
#include "bz_math.h"

namespace bz {

constexpr u64 kResignKey = 0x72657369676E6564ULL;  // BZ_RESIGN_KEY (bz_abi.h)
constexpr int kResignMaxStreak = 255;              // a streak is one byte

// One full search of a side whose streak so far is streak_in (0 .. 255) ended with root value q: *streak_out = the side's streak
// behind it -- min(streak_in + 1, 255) if q < threshold (strict, binary32; a NaN q is not below anything), else 0 -- and the
// return value says whether the side fires: its streak has reached `consecutive` (1 .. 255).
BZ_HD bool resign_step(float q, float threshold, int consecutive, int streak_in, int* streak_out) {
    int s = 0;
    if (q < threshold) s = streak_in < kResignMaxStreak ? streak_in + 1 : kResignMaxStreak;
    *streak_out = s;
    return s >= consecutive;
}

// the game with global id gid never resigns (it only records where it would have): 16 bits of a draw keyed by (seed, gid) alone
// against playout_q = the share of such games in units of 2^-16 (0: none, 65536: all)
BZ_HD bool resign_played_out(u64 seed, u64 gid, u32 playout_q) {
    return (u32)(rng_draw(seed ^ kResignKey, gid, 0ULL) & 0xFFFFULL) < playout_q;
}

}  // namespace bz
