// bz_early_stop.h -- exact early stop of a search whose move is decided: the rule that says the remaining
// simulations can no longer change the first maximum of the root's visits, __host__ __device__ so that bz_early_stop_decided
// (host) is the code the stop kernels run.  All of it is integer arithmetic: nothing rounds, no order matters.
#pragma once
#include "bz_math.h"

namespace bz {

// ---- the leader.  Every edge contributes the key (N << 8) | (255 - i), i its index among the root's edges in ascending action
// order (< 256; N < 2^24), and the keys of a root's edges are max-ed -- by one lane after the other, across a lane group, on the host, in
// any order: the maximum is the first maximum of N, the edge DESIGN.md 3.7 would play now.
BZ_HD u32 early_stop_key(u32 N, int i) { return (N << 8) | (u32)(255 - i); }
BZ_HD u32 early_stop_leader_N(u32 key) { return key >> 8; }
BZ_HD int early_stop_leader(u32 key) { return 255 - (int)(key & 0xFFu); }
// can edge j (N_j visits), given every one of the `left` remaining simulations, still be played instead of the leader L (N_L
// visits)?  It can when it would pass the leader, or tie with it from a lower action (a tie goes to the lower action).
// (N_j <= N_L: written over the gap N_L - N_j, so that no `left` overflows)
BZ_HD bool early_stop_catches(u32 Nj, int j, u32 NL, int L, u32 left) {
    const u32 gap = NL - Nj;
    return j != L && (left > gap || (left == gap && j < L));
}
// the bound that lets a caller skip the rule: with n >= 2 edges a search is never decided before max N >= left, and max N <= s,
// the simulations done, so never while s < left; a one-edge root is decided from s = 1 on.  False implies "not decided".
BZ_HD bool early_stop_possible(int n, u32 s, u32 left) { return s >= 1u && (n == 1 || s >= left); }

// ---- the rule over a root with n edges (N_i) in ascending action order and `left` simulations to go: decided when at least one
// simulation is done and no edge catches the leader.
template <class NAt>
BZ_HD bool early_stop_decided(int n, u32 left, NAt&& N_at) {
    u32 key = 0, s = 0;
    for (int i = 0; i < n; ++i) { const u32 N = N_at(i); s += N; const u32 k = early_stop_key(N, i); key = k > key ? k : key; }
    if (n <= 0 || s == 0u) return false;
    const u32 NL = early_stop_leader_N(key);
    const int L = early_stop_leader(key);
    for (int j = 0; j < n; ++j)
        if (early_stop_catches(N_at(j), j, NL, L, left)) return false;
    return true;
}

}  // namespace bz
