// bz_merge.h -- position averaging: the arithmetic that turns the rows of one position into one row, __host__
// __device__ so that bz_merge_group (host) is the code the kernels of bz_merge.hip run.  Every sum is an integer sum of
// fixed-point values: independent of the order of the rows and of how a reduction is split.
#pragma once
#include "bz_math.h"

namespace bz {

constexpr int kMergeUnitBits = 32;  // pi in [0, 1]; the value target and q in [-1, 1]
constexpr int kMergeKlBits = 24;    // kl in [0, 128]
constexpr float kMergeKlMax = 128.0f;

// fix_k(x) = (int64)(x * 2^k), truncating; the product is exact in binary32 (a power of two, no overflow inside the range).
// false -- and nothing written -- when x is NaN or outside [lo, hi]: such a row is not summed.
BZ_HD bool merge_fix(float x, float lo, float hi, int k, int64_t* out) {
    if (!(x >= lo && x <= hi)) return false;
    *out = (int64_t)(x * (float)(int64_t(1) << k));
    return true;
}

// M = floor((2 S + n) / (2 n)) -- round half up, a true floor for negative S -- then (float)((double)M * 2^-k): the double is
// exact (|M| <= 2^32), the one rounding is double -> float.  No floating-point division.
BZ_HD float merge_mean(int64_t S, int64_t n, int k) {
    const int64_t num = 2 * S + n, den = 2 * n;
    int64_t M = num / den;
    if (num % den < 0) --M;
    return (float)((double)M * (1.0 / (double)(int64_t(1) << k)));
}

BZ_HD int8_t merge_sign(int64_t S) { return (int8_t)((S > 0) - (S < 0)); }

// the value input of a row: vt when the examples carry it, otherwise (float)z
BZ_HD float merge_value_in(const float* vt, const int8_t* z, int64_t i) { return vt ? vt[i] : (float)z[i]; }

// One group: n rows of the same position (pi [n][na]; vt, q, kl [n] or null; z [n]) -> one row.  A row holding a value that is
// not finite or outside its range adds to no sum and is counted in the return value; n stays the number of rows.  n == 1: the
// row itself, bit for bit, with vt = its value input.
inline int32_t merge_group(const float* pi, const float* vt, const int8_t* z, const float* q, const float* kl, int32_t n, int32_t na,
                           float* pi_out, float* vt_out, int8_t* z_out, float* q_out, float* kl_out) {
    int32_t bad = 0;
    int64_t S[68] = {0};  // na <= 65 action sums, then the value, q and kl
    for (int32_t r = 0; r < n; ++r) {
        int64_t f[68] = {0};
        bool ok = merge_fix(merge_value_in(vt, z, r), -1.0f, 1.0f, kMergeUnitBits, &f[na]);
        for (int32_t a = 0; a < na; ++a) ok = merge_fix(pi[(int64_t)r * na + a], 0.0f, 1.0f, kMergeUnitBits, &f[a]) && ok;
        if (q) ok = merge_fix(q[r], -1.0f, 1.0f, kMergeUnitBits, &f[na + 1]) && ok;
        if (kl) ok = merge_fix(kl[r], 0.0f, kMergeKlMax, kMergeKlBits, &f[na + 2]) && ok;
        if (!ok) { ++bad; continue; }
        for (int32_t c = 0; c < na + 3; ++c) S[c] += f[c];
    }
    *z_out = merge_sign(S[na]);
    if (n == 1) {
        for (int32_t a = 0; a < na; ++a) pi_out[a] = pi[a];
        *vt_out = merge_value_in(vt, z, 0);
        if (q) *q_out = q[0];
        if (kl) *kl_out = kl[0];
        return bad;
    }
    for (int32_t a = 0; a < na; ++a) pi_out[a] = merge_mean(S[a], n, kMergeUnitBits);
    *vt_out = merge_mean(S[na], n, kMergeUnitBits);
    if (q) *q_out = merge_mean(S[na + 1], n, kMergeUnitBits);
    if (kl) *kl_out = merge_mean(S[na + 2], n, kMergeKlBits);
    return bad;
}

}  // namespace bz
