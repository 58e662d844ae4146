// bz_value.h -- search-value targets: the root's search value of a recorded row and the TD(lambda) value
// targets of one game's rows, __host__ __device__ so that bz_root_value / bz_value_targets_segment (host) are the code the
// kernels run.  Float discipline of DESIGN.md 3.4: every operation is one binary32 operation in the written order.
#pragma once
#include "bz_math.h"

namespace bz {

constexpr int kValueMaxSegment = 1024;  // rows one lane walks; a longer segment keeps vt = (float)z and is counted

// q = fdiv(sum W, (float)sum N) over the root's n edges in edge order (ascending action), W summed sequentially from 0.0f;
// sum N == 0: 0.  W is stored for the mover at the root: q is the mover's expected outcome.
// n_at(i) / w_at(i): the raw visit count and value sum of edge i.
template <class NAt, class WAt>
BZ_HD float root_value(int n, NAt&& n_at, WAt&& w_at) {
    float sW = 0.0f;
    u32 sN = 0;
    for (int i = 0; i < n; ++i) {
        sW = sW + w_at(i);
        sN += n_at(i);
    }
    return sN > 0 ? fdiv(sW, (float)sN) : 0.0f;
}

// a search value as the targets read it: NaN -> 0, clamped to [-1, 1]
BZ_HD float value_clean(float q) { return q != q ? 0.0f : (q < -1.0f ? -1.0f : (q > 1.0f ? 1.0f : q)); }
BZ_HD float value_abs(float x, int mover) { return mover == 1 ? x : -x; }  // mover's frame <-> absolute frame: an exact sign flip

// One segment = one game's T recorded rows in ply order (q, z, mover: the segment's first row).  Backward from the last row:
//   G[T-1] = Z = (float)(mover[T-1] * z[T-1]);  G[t] = (1 - lam) * A[t+1] + lam * G[t+1],  A = the cleaned q in the absolute frame
//   vt[t]  = clamp((1 - q_mix) * G[t] + q_mix * A[t]) back in the mover's frame
// lam = 1, q_mix = 0: vt == (float)z by value;  lam = 0, q_mix = 1: vt == the cleaned q.
BZ_HD void value_targets_segment(const float* q, const int8_t* z, const int8_t* mover, int T, float lam, float q_mix, float* vt) {
    float G = (float)((int)mover[T - 1] * (int)z[T - 1]);
    float A_next = 0.0f;
    for (int t = T - 1; t >= 0; --t) {
        const int m = (int)mover[t];
        const float A = value_abs(value_clean(q[t]), m);
        if (t < T - 1) {
            float a = 1.0f - lam;
            a = a * A_next;
            const float b = lam * G;
            G = a + b;
        }
        float c = 1.0f - q_mix;
        c = c * G;
        const float d = q_mix * A;
        float Tt = c + d;
        Tt = Tt < -1.0f ? -1.0f : (Tt > 1.0f ? 1.0f : Tt);
        vt[t] = value_abs(Tt, m);
        A_next = A;
    }
}

}  // namespace bz
