// bz_solver.h -- proven wins, losses and draws in the search tree (MCTS-Solver): the node rule that decides a
// node from its edges and the move rule at a root with decided edges, __host__ __device__ so that bz_solver_node /
// bz_solver_pick (host) are the code the kernels run.  All of it is integer arithmetic: nothing rounds, no order matters.
#pragma once
#include "bz_math.h"

namespace bz {

// the decided value of an edge for the mover at its child: -1, 0, +1, or kSolverUndecided
constexpr int kSolverUndecided = 2;

// ---- node rule.  Every edge contributes a word of flags and the words of a node's edges are OR-ed -- by one lane after the
// other, across a lane group, on the host, in any order: bit 0 = some edge is decided -1 (the move wins), bit 1 = some edge is
// undecided, bit 2 = some edge is decided 0 or -1 (the node is worth at least a draw).
BZ_HD u32 solver_edge_bits(int c) { return c == -1 ? 5u : (c == 0 ? 4u : (c == 1 ? 0u : 2u)); }
// the node's value for its mover from the OR over its n edges: +1 as soon as one move wins, else undecided while an edge is,
// else max over the edges of -c
BZ_HD int solver_node_value(u32 bits, int n) {
    if (bits & 1u) return 1;
    if (n <= 0 || (bits & 2u)) return kSolverUndecided;
    return (bits & 4u) ? 0 : -1;
}
template <class CAt>
BZ_HD int solver_node(int n, CAt&& c_at) {
    u32 bits = 0;
    for (int i = 0; i < n; ++i) bits |= solver_edge_bits(c_at(i));
    return solver_node_value(bits, n);
}

// ---- move rule at a root with edges (N_i, c_i) in ascending action order: the lowest winning edge if there is one; else the
// plain rule of DESIGN.md 3.7 over the edges that are not decided lost (c = +1) -- tau1: the first edge whose running visit
// sum exceeds draw % (their visit sum), else the first maximum of N; when every edge is lost or the remaining edges have no
// visit, the plain rule over all edges.
template <class NAt, class CAt>
BZ_HD int solver_pick(int n, NAt&& n_at, CAt&& c_at, bool tau1, u64 draw) {
    u64 all = 0, rem = 0;
    for (int i = 0; i < n; ++i) {
        const int c = c_at(i);
        if (c == -1) return i;
        all += n_at(i);
        if (c != 1) rem += n_at(i);
    }
    const bool drop = rem > 0;  // (else: every edge lost, or nothing left to choose by)
    const u64 sum = drop ? rem : all;
    int pick = 0;
    if (tau1) {
        if (sum == 0) return 0;
        const u64 rr = draw % sum;
        u64 cum = 0;
        for (int i = 0; i < n; ++i) {
            if (drop && c_at(i) == 1) continue;
            cum += n_at(i);
            if (cum > rr) return i;
        }
    } else {
        u64 bn = 0;
        for (int i = 0; i < n; ++i) {
            if (drop && c_at(i) == 1) continue;
            const u64 N = n_at(i);
            if (N > bn) { bn = N; pick = i; }
        }
    }
    return pick;
}

}  // namespace bz
