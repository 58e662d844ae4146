// bz_train_sym.hip -- a board symmetry per row inside the training step: ONE staging kernel in front of the
// stem.  k_train_sym_batch gathers the batch's n rows by idx, transforms each by its own sym[p] (bz_train_sym.h: the boards
// through bz_sym::board, the policy row as a permutation of its 65 entries, z / vt copied) and writes them into a staging
// batch the plan owns; the step's own descriptor points at that staging batch with idx = null, so k_train_stem, the head
// kernels and k_train_stem_wgrad (bz_train_ends.hip) run as they are, on rows that are already transformed.
//
// The data set's addresses -- own / opp / pi / z / idx / n_rows (a bz_train_batch) and vt / fown / fopp / sym (a
// bz_train_sym_cols) -- are read from DEVICE memory at launch time: a captured graph keeps working when the host points the
// two blocks at a new data set.  An index outside the data set is clamped as the step's kernels clamp it, a symmetry outside
// 0..7 is taken & 7; either makes its batch position count in the error words, one per workgroup, each added to by its own
// workgroup only (no atomics, nothing to zero inside a graph): the host sums and zeroes them where it reads the losses.
//
// kSymRowsPerWorkgroup = 64 rows per workgroup of 4 waves, 16 rows per wave.  Lanes 0..15 of a wave take one row each for
// the index, the symmetry, the 8-byte columns and the row's pass entry; then the wave walks its 16 policy rows with one lane
// per cell action, the row and its symmetry broadcast from the lane that holds them -- every policy load of the wave is
// independent of the others, so all 16 are in flight behind ONE round trip for the indices.
#include "bz_common.h"
#include "bz_train_sym.h"

using namespace bz;

namespace {

constexpr int kSymRowsPerWorkgroup = 64, kSymRowsPerWave = 16;
constexpr int kSymMaxBatch = 1 << 24;

struct SymStage {
    unsigned long long *own, *opp;
    unsigned* pi;          // [n][65], moved as bit patterns
    int8_t* z;
    unsigned* vt;          // [n] or null
    unsigned long long *fown, *fopp;   // [n] or null (both or neither)
};

__device__ __forceinline__ long long lane_ll(long long v, int lane) {   // lane: a constant after unrolling
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(unsigned long long)v, lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v >> 32), lane);
    return (long long)(((unsigned long long)hi << 32) | lo);
}

__global__ __launch_bounds__(256) void k_train_sym_batch(const bz_train_batch* __restrict__ src, const bz_train_sym_cols* __restrict__ cols,
                                                         int n, int size, SymStage S, unsigned* __restrict__ bad) {
    __shared__ int wave_bad[4];
    const bz_train_batch B = *src;
    const bz_train_sym_cols X = *cols;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p0 = blockIdx.x * kSymRowsPerWorkgroup + wave * kSymRowsPerWave;
    const unsigned* __restrict__ pi = reinterpret_cast<const unsigned*>(B.pi);

    // lanes 0..15: one batch position each
    long long row = 0;
    unsigned s = 0;
    bool is_bad = false;
    const int p = p0 + lane;
    if (lane < kSymRowsPerWave && p < n) {
        const long long r = B.idx ? (long long)B.idx[p] : (long long)p;
        const unsigned sr = X.sym[p];
        is_bad = bz_train_sym::row_bad(r, B.n_rows) || bz_train_sym::sym_bad(sr);
        row = bz_train_sym::clamp_row(r, B.n_rows);
        s = bz_train_sym::sym_of(sr);
        S.own[p] = bz_train_sym::board(B.own[row], size, s);
        S.opp[p] = bz_train_sym::board(B.opp[row], size, s);
        S.z[p] = B.z[row];
        S.pi[(long long)p * 65 + 64] = pi[row * 65 + 64];   // the pass entry stays in place
        if (S.vt && X.vt) S.vt[p] = reinterpret_cast<const unsigned*>(X.vt)[row];
        if (S.fown && X.fown && X.fopp) {
            S.fown[p] = bz_train_sym::board(X.fown[row], size, s);
            S.fopp[p] = bz_train_sym::board(X.fopp[row], size, s);
        }
    }
    // the policy rows' cells: lane a owns staged action a.  Every load first, then every store: the loads do not wait for one
    // another (a position past n reads row 0, which exists, and stores nothing)
    unsigned v[kSymRowsPerWave];
#pragma unroll
    for (int i = 0; i < kSymRowsPerWave; ++i) {
        const long long ri = lane_ll(row, i);
        const unsigned si = (unsigned)__builtin_amdgcn_readlane((int)s, i);
        v[i] = pi[ri * 65 + bz_train_sym::pi_source(size, si, lane)];
    }
#pragma unroll
    for (int i = 0; i < kSymRowsPerWave; ++i)
        if (p0 + i < n) S.pi[(long long)(p0 + i) * 65 + lane] = v[i];   // (wave-uniform)
    // the error word of this workgroup: += the batch positions with an index or a symmetry out of range
    const int nb = __popcll(__ballot(is_bad));
    if (lane == 0) wave_bad[wave] = nb;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int total = wave_bad[0] + wave_bad[1] + wave_bad[2] + wave_bad[3];
        if (total) bad[blockIdx.x] += (unsigned)total;
    }
}

}  // namespace

BZ_EXPORT int32_t bz_train_sym_rows_per_workgroup(void) { return kSymRowsPerWorkgroup; }

BZ_EXPORT int32_t bz_train_sym_row(uint64_t own, uint64_t opp, const float* pi, uint64_t fown, uint64_t fopp, int32_t size, int32_t s,
                                   uint64_t* own_out, uint64_t* opp_out, float* pi_out, uint64_t* fown_out, uint64_t* fopp_out) {
    BZ_REQUIRE(size >= 1 && size <= 8 && s >= 0 && s < 8, "bz_train_sym_row: size must be 1..8, s 0..7");
    BZ_REQUIRE(pi && own_out && opp_out && pi_out && pi != pi_out, "bz_train_sym_row: null pointer, or pi_out is pi (the row is not permuted in place)");
    const u32 e = bz_train_sym::sym_of((u32)s);
    *own_out = bz_train_sym::board(own, size, e);
    *opp_out = bz_train_sym::board(opp, size, e);
    if (fown_out) *fown_out = bz_train_sym::board(fown, size, e);
    if (fopp_out) *fopp_out = bz_train_sym::board(fopp, size, e);
    const uint32_t* from = reinterpret_cast<const uint32_t*>(pi);
    uint32_t* to = reinterpret_cast<uint32_t*>(pi_out);
    for (int a = 0; a < 65; ++a) to[a] = from[bz_train_sym::pi_source(size, e, a)];
    return BZ_OK;
}

BZ_EXPORT int32_t bz_train_sym_batch(const bz_train_batch* src_dev, const bz_train_sym_cols* cols_dev, int32_t n, int32_t size,
                                     const bz_train_sym_stage* stage, uint32_t* bad_dev, void* stream) {
    BZ_REQUIRE(src_dev && cols_dev && stage && bad_dev, "bz_train_sym_batch: null pointer");
    BZ_REQUIRE(n >= 1 && n <= kSymMaxBatch, "bz_train_sym_batch: n must be in 1 .. 2^24");
    BZ_REQUIRE(size >= 1 && size <= 8, "bz_train_sym_batch: size must be 1..8");
    BZ_REQUIRE(stage->own && stage->opp && stage->pi && stage->z, "bz_train_sym_batch: a staging pointer (own, opp, pi, z) is null");
    BZ_REQUIRE(!stage->fown == !stage->fopp, "bz_train_sym_batch: the staging batch has fown and fopp, or neither");
    if (bz_device_count() <= 0) { set_error("bz_train_sym_batch: no HIP device (the training kernels have no CPU path)"); return BZ_ENOGPU; }
    SymStage S;
    S.own = reinterpret_cast<unsigned long long*>(stage->own); S.opp = reinterpret_cast<unsigned long long*>(stage->opp);
    S.pi = reinterpret_cast<unsigned*>(stage->pi); S.z = stage->z; S.vt = reinterpret_cast<unsigned*>(stage->vt);
    S.fown = reinterpret_cast<unsigned long long*>(stage->fown); S.fopp = reinterpret_cast<unsigned long long*>(stage->fopp);
    const unsigned grid = (unsigned)((n + kSymRowsPerWorkgroup - 1) / kSymRowsPerWorkgroup);
    hipLaunchKernelGGL(k_train_sym_batch, dim3(grid), dim3(256), 0, (hipStream_t)stream, src_dev, cols_dev, (int)n, (int)size, S, bad_dev);
    BZ_LAUNCH_CHECK("k_train_sym_batch");
    return BZ_OK;
}
