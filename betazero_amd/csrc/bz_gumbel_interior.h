// bz_gumbel_interior.h -- the Gumbel interior rule (Danihelka et al., ICLR 2022, mctx's
// gumbel_muzero_interior_action_selection): below the root a walk takes the action whose visit share lags the improved policy
// softmax(logf(P~) + sigma(completed Q)) of the node the most.  The per-edge and per-node expressions are __host__ __device__:
// the tree step (k_gfull_step) and bz_gumbel_interior_pick (host) run these functions.  Float discipline of DESIGN.md 3.4:
// every operation is one binary32 operation in the written order; the three sums run in ascending edge order.
#pragma once
#include "bz_math.h"

namespace bz {

constexpr float kGiFltMin = 1.17549435e-38f;  // 2^-126
BZ_HD float gi_pfloor(float P) { return P > kGiFltMin ? P : kGiFltMin; }

// the node's mixed value from S = the visit sum of its children, sp = sum of P~ and spq = sum of P~ q over the visited edges
BZ_HD float gi_vmix(u32 S, float sp, float spq, float v_node) {
    const float wq = sp > 0.0f ? fdiv(spq, sp) : 0.0f;
    if (S == 0) return v_node;
    const float t = (float)S * wq;
    const float a = v_node + t;
    const float b = (float)S + 1.0f;
    return fdiv(a, b);
}

// sigma_i = s * ((cq_i - lo) / d)
struct GiScale { float lo, d, s; };
BZ_HD GiScale gi_scale(float lo, float hi, u32 nmax, float mvi, float vs) {
    GiScale sc;
    const float d = hi - lo;
    sc.d = d < 1e-8f ? 1e-8f : d;
    sc.lo = lo;
    const float s = mvi + (float)nmax;
    sc.s = s * vs;
    return sc;
}
BZ_HD float gi_sigma(const GiScale& sc, float cq) { return sc.s * fdiv(cq - sc.lo, sc.d); }
// x_i = logf(P~_i) + sigma_i
BZ_HD float gi_x(const GiScale& sc, float P, float cq) { return logf_spec(gi_pfloor(P)) + gi_sigma(sc, cq); }
// sc_i = p_i - N_i / (1 + S)
BZ_HD float gi_score(float p, u32 N, float den) {
    const float r = fdiv((float)N, den);
    return p - r;
}

// The rule for one node, serially: the definition.  N, W, P [n] the edges' statistics in edge order, S the visit sum of the
// children, v_node the node's own value.  Fills p [n] and sc [n] (either may be null) and returns the chosen edge.
// kMaxN bounds the scratch; n in 2 .. kMaxN (n == 1 is the forced pass: the caller takes edge 0).
constexpr int kGiMaxN = 64;
inline int gi_pick_serial(const u32* N, const float* W, const float* P, int n, float v_node, float mvi, float vs, float* p_out,
                          float* sc_out) {
    u32 S = 0, nmax = 0;
    float sp = 0.0f, spq = 0.0f;
    for (int i = 0; i < n; ++i) {
        S += N[i];
        nmax = N[i] > nmax ? N[i] : nmax;
        if (N[i] > 0) {
            const float q = fdiv(W[i], (float)N[i]), pf = gi_pfloor(P[i]);
            sp = sp + pf;
            const float t = pf * q;
            spq = spq + t;
        }
    }
    const float vmix = gi_vmix(S, sp, spq, v_node);
    float cq[kGiMaxN], x[kGiMaxN];
    float lo = 0.0f, hi = 0.0f;
    for (int i = 0; i < n; ++i) {
        cq[i] = N[i] > 0 ? fdiv(W[i], (float)N[i]) : vmix;
        lo = (i == 0 || cq[i] < lo) ? cq[i] : lo;
        hi = (i == 0 || cq[i] > hi) ? cq[i] : hi;
    }
    const GiScale sc = gi_scale(lo, hi, nmax, mvi, vs);
    float m = 0.0f;
    for (int i = 0; i < n; ++i) {
        x[i] = gi_x(sc, P[i], cq[i]);
        m = (i == 0 || x[i] > m) ? x[i] : m;
    }
    float s = 0.0f;
    for (int i = 0; i < n; ++i) {
        x[i] = expf_spec(x[i] - m);
        s = s + x[i];
    }
    const float den = 1.0f + (float)S;
    int best = 0;
    float bests = 0.0f;
    for (int i = 0; i < n; ++i) {
        const float p = fdiv(x[i], s);
        const float score = gi_score(p, N[i], den);
        if (p_out) p_out[i] = p;
        if (sc_out) sc_out[i] = score;
        if (i == 0 || score > bests) { best = i; bests = score; }
    }
    return best;
}

}  // namespace bz
