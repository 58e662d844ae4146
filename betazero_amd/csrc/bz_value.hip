// bz_value.hip -- search-value targets: from the rows' recorded root value q and the games' outcomes z to the
// value targets vt the training step's head kernel reads (bz_train_heads_vt).  Two launches, nothing read back:
//   k_value_init   vt = (float)z on every row, the status word = 0
//   k_value_tails  one lane per segment tail walks its segment backward (bz_value.h: the recurrence is sequential by
//                  specification -- a parallel scan would round differently) and overwrites the segment's vt; a segment
//                  longer than kValueMaxSegment rows keeps (float)z and is counted in the status word
// A segment is one game's recorded rows in ply order, the way the packed block delivers them.  The per-segment arithmetic lives
// in bz_value.h, shared with the host entry point bz_value_targets_segment.
#include "bz_common.h"
#include "bz_value.h"

using namespace bz;

namespace {

constexpr int64_t kMaxRows = int64_t(1) << 26;

__global__ void __launch_bounds__(256) k_value_init(const int8_t* z, int64_t n, float* vt, unsigned long long* status) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *status = 0ULL;
    if (i < n) vt[i] = (float)z[i];
}

__device__ __forceinline__ bool seg_start(const int64_t* game, const int32_t* ply, int64_t i) {
    return i == 0 || game[i] != game[i - 1] || ply[i] <= ply[i - 1];
}

__global__ void __launch_bounds__(256) k_value_tails(const float* q, const int8_t* z, const int8_t* mover, const int64_t* game,
                                                     const int32_t* ply, int64_t n, float lam, float q_mix, float* vt,
                                                     unsigned long long* status) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (i != n - 1 && !seg_start(game, ply, i + 1)) return;  // not a tail
    int64_t s = i;
    int T = 1;
    while (!seg_start(game, ply, s)) {
        if (T == kValueMaxSegment) {  // too long for one lane: its rows keep (float)z
            atomicAdd(status, 1ULL);
            return;
        }
        --s; ++T;
    }
    value_targets_segment(q + s, z + s, mover + s, T, lam, q_mix, vt + s);
}

}  // namespace

BZ_EXPORT int32_t bz_value_targets_segment(const float* q, const int8_t* z, const int8_t* mover, int32_t T, float lam, float q_mix,
                                           float* vt) {
    BZ_REQUIRE(q && z && mover && vt, "bz_value_targets_segment: null pointer");
    BZ_REQUIRE(T >= 1 && T <= kValueMaxSegment, "bz_value_targets_segment: T must be in 1 .. 1024");
    BZ_REQUIRE(lam >= 0.0f && lam <= 1.0f, "bz_value_targets_segment: lam must be in [0, 1]");
    BZ_REQUIRE(q_mix >= 0.0f && q_mix <= 1.0f, "bz_value_targets_segment: q_mix must be in [0, 1]");
    value_targets_segment(q, z, mover, T, lam, q_mix, vt);
    return BZ_OK;
}

BZ_EXPORT int32_t bz_value_targets(const float* q, const int8_t* z, const int8_t* mover, const int64_t* game, const int32_t* ply,
                                   int64_t n, float lam, float q_mix, float* vt, uint64_t* status_dev, void* stream) {
    BZ_REQUIRE(n >= 0 && n <= kMaxRows, "bz_value_targets: n must be in 0 .. 2^26");
    BZ_REQUIRE(lam >= 0.0f && lam <= 1.0f, "bz_value_targets: lam must be in [0, 1]");
    BZ_REQUIRE(q_mix >= 0.0f && q_mix <= 1.0f, "bz_value_targets: q_mix must be in [0, 1]");
    BZ_REQUIRE(status_dev && (reinterpret_cast<uintptr_t>(status_dev) & 7) == 0, "bz_value_targets: the status word is null or not 8-byte aligned");
    BZ_REQUIRE(n == 0 || (q && z && mover && game && ply && vt), "bz_value_targets: null pointer");
    if (bz_device_count() <= 0) { set_error("bz_value_targets: no HIP device (the value targets have no CPU path)"); return BZ_ENOGPU; }
    hipStream_t s = (hipStream_t)stream;
    const unsigned nb = (unsigned)((n + 255) / 256);
    unsigned long long* st = reinterpret_cast<unsigned long long*>(status_dev);
    hipLaunchKernelGGL(k_value_init, dim3(nb ? nb : 1u), dim3(256), 0, s, z, n, vt, st);
    BZ_LAUNCH_CHECK("k_value_init");
    if (n == 0) return BZ_OK;
    hipLaunchKernelGGL(k_value_tails, dim3(nb), dim3(256), 0, s, q, z, mover, game, ply, n, lam, q_mix, vt, st);
    BZ_LAUNCH_CHECK("k_value_tails");
    return BZ_OK;
}
