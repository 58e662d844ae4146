// bz_surprise.h -- policy surprise weighting (KataGo, Wu 2019, section 3.3): the per-row functions the
// kernels run, __host__ __device__ so that bz_surprise_kl / bz_surprise_count (host) are the same code.  Float discipline of
// every operation is one binary32 operation in the written order.
#pragma once
#include "bz_math.h"

namespace bz {

constexpr float kSurpFltMin = 1.17549435e-38f;  // FLT_MIN: the floor of a prior inside the logarithm
constexpr float kSurpKlMax = 128.0f;            // the resampler's clamp of a row's kl (ln(1 / FLT_MIN) = 87.3 bounds a real one)
constexpr float kSurpQ = 1073741824.0f;         // 2^30: the quantisation of the exact integer mean
constexpr float kSurpWMax = 1073741824.0f;      // the clamp of a row's weight (a count fits 32 bits whatever the caller hands in)
constexpr u64 kSurpKey = 0x7375727072697365ULL; // "surprise": the resampler's RNG key constant

// kl = sum over the n root edges (ascending action) with pi > 0 of pi * (logf(pi) - logf(max(P, FLT_MIN))), then kl > 0 ? kl : 0:
// a rounding negative or a NaN gives 0.  (logf_spec is defined on normal positive numbers: a NaN prior is carried as a NaN
// instead of being read as a number.)  pi_at(i) / p_at(i): the row's pi and the root's raw prior at edge i.
template <class PiAt, class PAt>
BZ_HD float surprise_kl(int n, PiAt&& pi_at, PAt&& p_at) {
    float kl = 0.0f;
    for (int i = 0; i < n; ++i) {
        const float p = pi_at(i);
        if (!(p > 0.0f)) continue;
        float q = p_at(i);
        q = q < kSurpFltMin ? kSurpFltMin : q;  // (a NaN stays)
        const float lq = q == q ? logf_spec(q) : q;
        float t = logf_spec(p) - lq;
        t = p * t;
        kl = kl + t;
    }
    return kl > 0.0f ? kl : 0.0f;
}

// the resampler's view of a row's kl: negative or NaN -> 0, above 128 -> 128
BZ_HD float surprise_clean(float kl) {
    const float k = kl > 0.0f ? kl : 0.0f;
    return k < kSurpKlMax ? k : kSurpKlMax;
}
// q_i = (u64)(kl_i * 2^30): exact (a power-of-two product), <= 2^37, so 2^26 of them sum below 2^64
BZ_HD u64 surprise_quant(float kl) { return (u64)(surprise_clean(kl) * kSurpQ); }
// mean = float(double(sum q) / (double(n) * 2^30))
BZ_HD float surprise_mean(u64 sum_q, u64 n) { return (float)((double)sum_q / ((double)n * 1073741824.0)); }

// w = u + (1 - u) * fdiv(kl, mean); mean == 0 (nothing surprising anywhere): 1
BZ_HD float surprise_weight(float kl, float mean, float u) {
    if (!(mean > 0.0f)) return 1.0f;
    float t = 1.0f - u;
    t = t * fdiv(surprise_clean(kl), mean);
    const float w = u + t;
    return w < kSurpWMax ? w : kSurpWMax;
}
// the row's 24 random bits: keyed by (seed ^ kSurpKey) and the row's CONTENT -- game id, ply, own, opp -- never by its index
BZ_HD u32 surprise_draw(u64 seed, u64 game, u64 ply, u64 own, u64 opp) {
    const u64 h = rng_draw(seed ^ kSurpKey, game, ply);
    return (u32)(mix64(h ^ hash_pos(own, opp)) >> 40);
}
// count = floor(w) + [draw < (u32)(frac(w) * 2^24)]
BZ_HD u32 surprise_count(float kl, float mean, float u, u64 seed, u64 game, u64 ply, u64 own, u64 opp) {
    const float w = surprise_weight(kl, mean, u);
    const float fl = __builtin_floorf(w);
    const float fr = w - fl;
    const u32 thr = (u32)(fr * 16777216.0f);
    return (u32)fl + (surprise_draw(seed, game, ply, own, opp) < thr ? 1u : 0u);
}

}  // namespace bz
