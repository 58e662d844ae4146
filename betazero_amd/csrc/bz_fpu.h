// bz_fpu.h -- first-play urgency reduction: the visited prior mass of a node as an exact integer and the value an
// unvisited child of that node is scored with, __host__ __device__ so that bz_fpu_mass / bz_fpu_value (host) are the code the
// kernels run.  Float discipline of DESIGN.md 3.4: every operation is one binary32 operation in the written order.
#pragma once
#include "bz_math.h"

namespace bz {

// a visited edge's prior in units of 2^-24: the product is an exact scaling by a power of two, the conversion truncates; a NaN or
// a negative prior (and a denormal one, whose product is below 1) gives 0
BZ_HD u32 fpu_pq(float P) { return P > 0.0f ? (u32)(P * 16777216.0f) : 0u; }

// S = sum of fpu_pq over the n edges with N > 0.  An integer sum has no order: the lanes of a game's group add their edges in
// any order and reduce across the group, the host adds them one by one -- the same S.  With <= 34 edges and P <= 1, S < 2^30.
// n_at(i) / p_at(i): the visit count and the prior of edge i.
template <class NAt, class PAt>
BZ_HD u32 fpu_mass(int n, NAt&& n_at, PAt&& p_at) {
    u32 S = 0;
    for (int i = 0; i < n; ++i)
        if (n_at(i) > 0u) S += fpu_pq(p_at(i));
    return S;
}

// what an unvisited child of a node with value q_node and visited mass S is worth: f = q_node - reduction * fsqrt(S * 2^-24).
// (float)S rounds above 2^24; the scaling back by 2^-24 is exact.  No clamp: f may be below -1.
BZ_HD float fpu_value(u32 S, float q_node, float reduction) {
    float m = (float)S;
    m = m * 5.9604644775390625e-08f;
    m = fsqrt(m);
    const float red = reduction * m;
    return q_node - red;
}

}  // namespace bz
