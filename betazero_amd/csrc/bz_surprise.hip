// bz_surprise.hip -- policy surprise weighting, the resampler: from the rows' kl to repeat counts and the
// index list the training step gathers by (bz_train_batch.idx).  Four launches, nothing read back:
//   k_surp_sum    sum of the quantised kl, 64-bit integer adds (order-independent: the mean is the same bits every run)
//   k_surp_count  count_i of every row and every 1024-row block's sum
//   k_surp_scan   one workgroup: exclusive scan of the block sums, the total and the dropped-row word
//   k_surp_emit   every block scans its own 1024 counts and writes row i count_i times from its offset
// The per-row arithmetic lives in bz_surprise.h, shared with the host entry points bz_surprise_kl / bz_surprise_count.
#include "bz_common.h"
#include "bz_surprise.h"

using namespace bz;

namespace {

constexpr int kRowsPerBlock = 1024;  // 256 threads x 4 rows
constexpr int64_t kMaxRows = int64_t(1) << 26;

// the head of the workspace (256 bytes), then the blocks' sums u32 [nb] and offsets u64 [nb], each 256-byte aligned
struct SurpHdr { u64 sum_q, total, dropped; u64 pad[29]; };
static_assert(sizeof(SurpHdr) == 256, "resampler workspace header");
struct SurpWs { int64_t bsum, boff, total; };
SurpWs surp_ws(int64_t n) {
    const int64_t nb = (n + kRowsPerBlock - 1) / kRowsPerBlock;
    SurpWs w{};
    w.bsum = 256;
    w.boff = w.bsum + ((nb * 4 + 255) & ~int64_t(255));
    w.total = w.boff + ((nb * 8 + 255) & ~int64_t(255));
    return w;
}

__global__ void __launch_bounds__(256) k_surp_sum(const float* kl, int64_t n, SurpHdr* hdr) {
    u64 s = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) s += surprise_quant(kl[i]);
    u32 lo = (u32)s, hi = (u32)(s >> 32);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {  // 64-bit wave sum through two 32-bit shuffles
        const u64 y = (u64)__shfl_xor(lo, o, 64) | ((u64)__shfl_xor(hi, o, 64) << 32);
        s += y;
        lo = (u32)s; hi = (u32)(s >> 32);
    }
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(reinterpret_cast<unsigned long long*>(&hdr->sum_q), (unsigned long long)s);
}

__global__ void __launch_bounds__(256) k_surp_count(const float* kl, const int64_t* game, const int32_t* ply, const u64* own,
                                                    const u64* opp, int64_t n, float u, u64 seed, const SurpHdr* hdr,
                                                    int32_t* count, u32* bsum) {
    __shared__ float s_mean;
    __shared__ u32 s_w[4];
    if (threadIdx.x == 0) s_mean = surprise_mean(hdr->sum_q, (u64)n);
    __syncthreads();
    const float mean = s_mean;
    const int64_t base = (int64_t)blockIdx.x * kRowsPerBlock;
    u32 s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t i = base + j * 256 + threadIdx.x;
        if (i < n) {
            const u32 c = surprise_count(kl[i], mean, u, seed, (u64)game[i], (u64)(u32)ply[i], own[i], opp[i]);
            count[i] = (int32_t)c;
            s += c;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) bsum[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// (a block's sum and 1024 of them stay far below 2^32: the weights sum to < 2 n and the draws add at most n, n <= 2^26)
__global__ void __launch_bounds__(1024) k_surp_scan(const u32* bsum, u64* boff, int64_t nb, SurpHdr* hdr, u64 idx_cap, int64_t* n_out) {
    __shared__ u32 wsum[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    u64 carry = 0;
    for (int64_t c0 = 0; c0 < nb; c0 += 1024) {
        const int64_t i = c0 + threadIdx.x;
        const u32 v = i < nb ? bsum[i] : 0u;
        u32 x = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const u32 y = __shfl_up(x, o, 64); if (lane >= o) x += y; }
        if (lane == 63) wsum[wave] = x;
        __syncthreads();
        u32 woff = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) { const u32 sw = wsum[w]; tot += sw; if (w < wave) woff += sw; }
        if (i < nb) boff[i] = carry + woff + x - v;
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        hdr->total = carry;
        hdr->dropped = carry > idx_cap ? carry - idx_cap : 0ULL;
        *n_out = (int64_t)(carry > idx_cap ? idx_cap : carry);
    }
}

__global__ void __launch_bounds__(256) k_surp_emit(const int32_t* count, const u64* boff, int64_t n, int64_t* idx_out, u64 idx_cap) {
    __shared__ u32 s_w[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * kRowsPerBlock + (int64_t)threadIdx.x * 4;  // four consecutive rows per thread
    u32 c[4], s = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) { c[j] = r0 + j < n ? (u32)count[r0 + j] : 0u; s += c[j]; }
    u32 x = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const u32 y = __shfl_up(x, o, 64); if (lane >= o) x += y; }
    if (lane == 63) s_w[wave] = x;
    __syncthreads();
    u32 woff = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) if (w < wave) woff += s_w[w];
    u64 o = boff[blockIdx.x] + woff + x - s;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        for (u32 k = 0; k < c[j] && o < idx_cap; ++k, ++o) idx_out[o] = r0 + j;  // (o >= idx_cap: the row is dropped, counted by k_surp_scan)
        if (o >= idx_cap) break;
    }
}

}  // namespace

BZ_EXPORT int32_t bz_surprise_kl(const float* pi, const float* P, int32_t n, float* kl) {
    BZ_REQUIRE(pi && P && kl && n >= 1 && n <= 255, "bz_surprise_kl: null pointer or n outside 1 .. 255");
    *kl = surprise_kl(n, [pi](int i) { return pi[i]; }, [P](int i) { return P[i]; });
    return BZ_OK;
}

BZ_EXPORT int32_t bz_surprise_count(float kl, float mean, float uniform_frac, uint64_t seed, int64_t game, int32_t ply, uint64_t own,
                                    uint64_t opp, int32_t* count) {
    BZ_REQUIRE(count, "bz_surprise_count: null pointer");
    BZ_REQUIRE(uniform_frac >= 0.0f && uniform_frac <= 1.0f, "bz_surprise_count: uniform_frac must be in [0, 1]");
    *count = (int32_t)surprise_count(kl, mean, uniform_frac, seed, (u64)game, (u64)(u32)ply, own, opp);
    return BZ_OK;
}

BZ_EXPORT int64_t bz_surprise_resample_workspace_bytes(int64_t n) {
    if (n < 0 || n > kMaxRows) { set_error("bz_surprise_resample_workspace_bytes: n must be in 0 .. 2^26"); return -1; }
    return surp_ws(n).total;
}

BZ_EXPORT int32_t bz_surprise_resample(const float* kl, const int64_t* game, const int32_t* ply, const uint64_t* own, const uint64_t* opp,
                                       int64_t n, float uniform_frac, uint64_t seed, void* ws, int64_t ws_bytes, int32_t* count,
                                       int64_t* idx_out, int64_t idx_cap, int64_t* n_out, void* stream) {
    BZ_REQUIRE(n >= 0 && n <= kMaxRows, "bz_surprise_resample: n must be in 0 .. 2^26");
    BZ_REQUIRE(uniform_frac >= 0.0f && uniform_frac <= 1.0f, "bz_surprise_resample: uniform_frac must be in [0, 1]");
    BZ_REQUIRE(idx_cap >= 0 && ws && n_out && (idx_out || idx_cap == 0), "bz_surprise_resample: null pointer or a negative idx_cap");
    BZ_REQUIRE(n == 0 || (kl && game && ply && own && opp && count), "bz_surprise_resample: null pointer");
    BZ_REQUIRE((reinterpret_cast<uintptr_t>(ws) & 255) == 0, "bz_surprise_resample: the workspace must be 256-byte aligned");
    const SurpWs w = surp_ws(n);
    if (ws_bytes < w.total) { set_error("bz_surprise_resample: workspace too small (%lld < %lld)", (long long)ws_bytes, (long long)w.total); return BZ_ENOMEM; }
    hipStream_t s = (hipStream_t)stream;
    SurpHdr* hdr = static_cast<SurpHdr*>(ws);
    BZ_HIP(hipMemsetAsync(hdr, 0, sizeof(SurpHdr), s));
    if (n == 0) {
        BZ_HIP(hipMemsetAsync(n_out, 0, 8, s));
        return BZ_OK;
    }
    const int64_t nb = (n + kRowsPerBlock - 1) / kRowsPerBlock;
    u32* bsum = reinterpret_cast<u32*>(static_cast<char*>(ws) + w.bsum);
    u64* boff = reinterpret_cast<u64*>(static_cast<char*>(ws) + w.boff);
    hipLaunchKernelGGL(k_surp_sum, dim3((unsigned)(nb < 1024 ? nb : 1024)), dim3(256), 0, s, kl, n, hdr);
    BZ_LAUNCH_CHECK("k_surp_sum");
    hipLaunchKernelGGL(k_surp_count, dim3((unsigned)nb), dim3(256), 0, s, kl, game, ply, own, opp, n, uniform_frac, (u64)seed,
                       static_cast<const SurpHdr*>(hdr), count, bsum);
    BZ_LAUNCH_CHECK("k_surp_count");
    hipLaunchKernelGGL(k_surp_scan, dim3(1), dim3(1024), 0, s, static_cast<const u32*>(bsum), boff, nb, hdr, (u64)idx_cap, n_out);
    BZ_LAUNCH_CHECK("k_surp_scan");
    hipLaunchKernelGGL(k_surp_emit, dim3((unsigned)nb), dim3(256), 0, s, static_cast<const int32_t*>(count),
                       static_cast<const u64*>(boff), n, idx_out, (u64)idx_cap);
    BZ_LAUNCH_CHECK("k_surp_emit");
    return BZ_OK;
}
