// bz_merge.hip -- position averaging: the rows of a training window that share a position (own, opp) become
// one row carrying the mean pi, the mean value target and a count.  The caller groups (two stable sorts, a neighbour compare:
// plumbing) and hands over, per SORTED position i, order[i] = the row standing there, start[i] = the sorted position of the head
// of its run and dst[i] = the output row of its group; per OUTPUT row d, head[d] = its first row and count[d] = its rows.
// Three launches, nothing read back:
//   k_merge_zero    zeroes the accumulator rows of the groups that cross a chunk boundary, and the status word
//   k_merge_reduce  walks the sorted order in chunks of kMergeChunk rows, one lane per column (NA actions, then the value, q
//                   and kl), summing fixed-point values in a register while the group stays the same.  A group of two or more
//                   rows inside one chunk is stored; a group crossing a chunk boundary is added into its accumulator row
//                   with 64-bit atomics: integer adds, so the arrival order does not matter.  A group of one row is not
//                   written at all -- the finish copies the row
//   k_merge_finish  one lane per (group, column): the mean (bz_merge.h), the verbatim copy of a single row, sign(z) and the
//                   columns carried from the group's first row
// The arithmetic lives in bz_merge.h, shared with the host entry point bz_merge_group.
#include "bz_common.h"
#include "bz_merge.h"

using namespace bz;

namespace {

constexpr int64_t kMaxRows = int64_t(1) << 26;
constexpr int kMergeChunk = 64;   // rows one lane group walks
constexpr int kMergeBlock = 128;  // threads of k_merge_reduce

template <int NA> struct MergeShape {
    static constexpr int kCols = NA + 3;                                // pi, value, q, kl
    static constexpr int kLanes = NA == 9 ? 16 : 128;                   // lanes per chunk: the next power of two >= kCols
    static constexpr int kRows = kMergeChunk * (kMergeBlock / kLanes);  // rows per workgroup
    static_assert(kCols <= kLanes && kMergeBlock % kLanes == 0, "one lane per column");
};

int64_t ws_bytes_of(int64_t n, int32_t na) { return (n * (na + 3) * 8 + 255) / 256 * 256; }

// boundary b (b >= 1) lies at sorted position p = b * kMergeChunk.  The group standing there crosses it iff its head is not p;
// it is zeroed at the FIRST boundary it crosses (its head lies in the chunk in front of p), once.
__global__ void __launch_bounds__(256) k_merge_zero(const int32_t* start, const int32_t* dst, int64_t n, int cols, int64_t* ws,
                                                    unsigned long long* status) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *status = 0ULL;
    const int64_t b = i / cols + 1;
    const int c = (int)(i - (b - 1) * cols);
    const int64_t p = b * kMergeChunk;
    if (p >= n) return;
    const int64_t s = start[p];
    const int32_t d = dst[p];
    if (s != p && s >= p - kMergeChunk && (uint64_t)d < (uint64_t)n) ws[(int64_t)d * cols + c] = 0;
}

template <int NA>
__global__ void __launch_bounds__(kMergeBlock) k_merge_reduce(bz_merge_rows in, int64_t n, const int64_t* order, const int32_t* start,
                                                              const int32_t* dst, int64_t* ws, unsigned long long* status) {
    using S = MergeShape<NA>;
    constexpr int RB = S::kRows, NC = S::kCols, LG = S::kLanes;
    __shared__ float s_pi[RB * NA];
    __shared__ float s_val[RB], s_q[RB], s_kl[RB];
    __shared__ int64_t s_order[RB];
    __shared__ int32_t s_start[RB + 1], s_dst[RB];
    __shared__ unsigned s_bad[RB];
    const int tid = threadIdx.x;
    const int64_t base = (int64_t)blockIdx.x * RB;
    const int rows = (int)(n - base < RB ? n - base : RB);
    // the scalar columns, checked by one lane per row
    for (int r = tid; r < rows; r += kMergeBlock) {
        int64_t o = order[base + r];
        int32_t d = dst[base + r];
        const bool inside = (uint64_t)o < (uint64_t)n && (uint64_t)d < (uint64_t)n;  // a broken index list: counted, never followed
        if (!inside) { o = 0; d = 0; }
        int64_t f;
        const float v = merge_value_in(in.vt, in.z, o);
        bool ok = merge_fix(v, -1.0f, 1.0f, kMergeUnitBits, &f) && inside;
        float q = 0.0f, kl = 0.0f;
        if (in.q) { q = in.q[o]; ok = merge_fix(q, -1.0f, 1.0f, kMergeUnitBits, &f) && ok; }
        if (in.kl) { kl = in.kl[o]; ok = merge_fix(kl, 0.0f, kMergeKlMax, kMergeKlBits, &f) && ok; }
        s_order[r] = o; s_start[r] = start[base + r]; s_dst[r] = d;
        s_val[r] = v; s_q[r] = q; s_kl[r] = kl; s_bad[r] = ok ? 0u : 1u;
    }
    if (tid == 0) s_start[rows] = base + rows < n ? start[base + rows] : (int32_t)(base + rows);  // behind the last row: a head
    __syncthreads();
    // pi, row after row as the sorted order names them: consecutive lanes read consecutive words of a row
    for (int j = tid; j < rows * NA; j += kMergeBlock) {
        const int r = j / NA, a = j - r * NA;
        const float v = in.pi[s_order[r] * NA + a];
        int64_t f;
        if (!merge_fix(v, 0.0f, 1.0f, kMergeUnitBits, &f)) atomicOr(&s_bad[r], 1u);
        s_pi[j] = v;
    }
    __syncthreads();
    for (int r = tid; r < rows; r += kMergeBlock)
        if (s_bad[r]) atomicAdd(status, 1ULL);
    // one lane per column walks its chunk
    const int c = tid % LG;
    const int cb = (tid / LG) * kMergeChunk;
    const int ce = cb + kMergeChunk < rows ? cb + kMergeChunk : rows;
    if (c >= NC || cb >= ce || (c == NA + 1 && !in.q) || (c == NA + 2 && !in.kl)) return;
    const float* src = c < NA ? s_pi + c : (c == NA ? s_val : (c == NA + 1 ? s_q : s_kl));
    const int stride = c < NA ? NA : 1;
    const float scale = (float)(int64_t(1) << (c == NA + 2 ? kMergeKlBits : kMergeUnitBits));
    const int32_t chunk0 = (int32_t)(base + cb);
    // a run [head, end) that ends at sorted position `end`; last = the block row of its last row
    auto flush = [&](int32_t head, int32_t end, bool closed, int last, int64_t acc) {
        int64_t* cell = ws + (int64_t)s_dst[last] * NC + c;
        if (head >= chunk0 && closed) {
            if (end - head > 1) *cell = acc;
        } else {
            atomicAdd(reinterpret_cast<unsigned long long*>(cell), (unsigned long long)acc);
        }
    };
    int64_t acc = 0;
    int32_t cur = s_start[cb];
    for (int r = cb; r < ce; ++r) {
        const int32_t s = s_start[r];
        if (s != cur) {
            flush(cur, (int32_t)(base + r), true, r - 1, acc);
            acc = 0;
            cur = s;
        }
        if (!s_bad[r]) acc += (int64_t)(src[r * stride] * scale);
    }
    flush(cur, (int32_t)(base + ce), s_start[ce] != cur, ce - 1, acc);
}

template <int NA>
__global__ void __launch_bounds__(256) k_merge_finish(bz_merge_rows in, int64_t n, const int64_t* head, const int32_t* count,
                                                      const int64_t* n_groups, const int64_t* ws, bz_merge_rows out) {
    constexpr int NC = MergeShape<NA>::kCols;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t d = i / NC;
    const int c = (int)(i - d * NC);
    if (d >= n || d >= *n_groups) return;
    int64_t h = head[d];
    if ((uint64_t)h >= (uint64_t)n) h = 0;
    const int64_t nd = count[d];
    const int64_t S = nd > 1 ? ws[d * NC + c] : 0;
    if (c < NA) {
        out.pi[d * NA + c] = nd > 1 ? merge_mean(S, nd, kMergeUnitBits) : in.pi[h * NA + c];
    } else if (c == NA) {  // the value lane also carries the head's columns
        const float v = merge_value_in(in.vt, in.z, h);
        int64_t one = 0;
        if (nd == 1) merge_fix(v, -1.0f, 1.0f, kMergeUnitBits, &one);
        out.vt[d] = nd > 1 ? merge_mean(S, nd, kMergeUnitBits) : v;
        out.z[d] = merge_sign(nd > 1 ? S : one);
        out.own[d] = in.own[h]; out.opp[d] = in.opp[h]; out.mover[d] = in.mover[h]; out.act[d] = in.act[h];
        out.game[d] = in.game[h]; out.ply[d] = in.ply[h];
    } else if (c == NA + 1) {
        if (in.q) out.q[d] = nd > 1 ? merge_mean(S, nd, kMergeUnitBits) : in.q[h];
    } else {
        if (in.kl) out.kl[d] = nd > 1 ? merge_mean(S, nd, kMergeKlBits) : in.kl[h];
    }
}

template <int NA>
int32_t merge_launch(const bz_merge_rows& in, int64_t n, const int64_t* order, const int32_t* start, const int32_t* dst,
                     const int64_t* head, const int32_t* count, const int64_t* n_groups, int64_t* ws, const bz_merge_rows& out,
                     unsigned long long* st, hipStream_t s) {
    using S = MergeShape<NA>;
    const int64_t cells = ((n - 1) / kMergeChunk) * S::kCols;  // (boundaries inside the rows) x columns
    hipLaunchKernelGGL(k_merge_zero, dim3((unsigned)(cells / 256 + 1)), dim3(256), 0, s, start, dst, n, S::kCols, ws, st);
    BZ_LAUNCH_CHECK("k_merge_zero");
    hipLaunchKernelGGL(k_merge_reduce<NA>, dim3((unsigned)((n + S::kRows - 1) / S::kRows)), dim3(kMergeBlock), 0, s, in, n, order,
                       start, dst, ws, st);
    BZ_LAUNCH_CHECK("k_merge_reduce");
    hipLaunchKernelGGL(k_merge_finish<NA>, dim3((unsigned)((n * S::kCols + 255) / 256)), dim3(256), 0, s, in, n, head, count,
                       n_groups, ws, out);
    BZ_LAUNCH_CHECK("k_merge_finish");
    return BZ_OK;
}

}  // namespace

BZ_EXPORT int32_t bz_merge_group(const float* pi, const float* vt, const int8_t* z, const float* q, const float* kl, int32_t n,
                                 int32_t na, float* pi_out, float* vt_out, int8_t* z_out, float* q_out, float* kl_out, int32_t* bad) {
    BZ_REQUIRE(pi && z && pi_out && vt_out && z_out && bad, "bz_merge_group: null pointer");
    BZ_REQUIRE((!q || q_out) && (!kl || kl_out), "bz_merge_group: q / kl given without a place for the result");
    BZ_REQUIRE(n >= 1 && n <= kMaxRows, "bz_merge_group: n must be in 1 .. 2^26");
    BZ_REQUIRE(na == 9 || na == 65, "bz_merge_group: na must be 9 (tic-tac-toe) or 65 (Reversi)");
    *bad = merge_group(pi, vt, z, q, kl, n, na, pi_out, vt_out, z_out, q_out, kl_out);
    return BZ_OK;
}

BZ_EXPORT int64_t bz_merge_workspace_bytes(int64_t n, int32_t na) {
    if (n < 0 || n > kMaxRows || (na != 9 && na != 65)) {
        set_error("bz_merge_workspace_bytes: n must be in 0 .. 2^26 and na 9 or 65");
        return -1;
    }
    return ws_bytes_of(n, na);
}

BZ_EXPORT int32_t bz_merge_positions(const bz_merge_rows* in, int64_t n, int32_t na, const int64_t* order, const int32_t* start,
                                     const int32_t* dst, const int64_t* head, const int32_t* count, const int64_t* n_groups, void* ws,
                                     int64_t ws_bytes, const bz_merge_rows* out, uint64_t* status_dev, void* stream) {
    BZ_REQUIRE(n >= 0 && n <= kMaxRows, "bz_merge_positions: n must be in 0 .. 2^26");
    BZ_REQUIRE(na == 9 || na == 65, "bz_merge_positions: na must be 9 (tic-tac-toe) or 65 (Reversi)");
    if (n == 0) return BZ_OK;  // nothing launched, nothing dereferenced
    BZ_REQUIRE(in && out && order && start && dst && head && count && n_groups, "bz_merge_positions: null pointer");
    BZ_REQUIRE(in->own && in->opp && in->pi && in->z && in->mover && in->act && in->game && in->ply, "bz_merge_positions: null input column");
    BZ_REQUIRE(out->own && out->opp && out->pi && out->z && out->mover && out->act && out->game && out->ply && out->vt,
               "bz_merge_positions: null output column");
    BZ_REQUIRE((!in->q || out->q) && (!in->kl || out->kl), "bz_merge_positions: q / kl given without a place for the result");
    BZ_REQUIRE(status_dev && (reinterpret_cast<uintptr_t>(status_dev) & 7) == 0, "bz_merge_positions: the status word is null or not 8-byte aligned");
    BZ_REQUIRE(ws && (reinterpret_cast<uintptr_t>(ws) & 255) == 0, "bz_merge_positions: the workspace is null or not 256-byte aligned");
    if (ws_bytes < ws_bytes_of(n, na)) { set_error("bz_merge_positions: the workspace is too small"); return BZ_ENOMEM; }
    if (bz_device_count() <= 0) { set_error("bz_merge_positions: no HIP device (the merge has no CPU path)"); return BZ_ENOGPU; }
    hipStream_t s = (hipStream_t)stream;
    unsigned long long* st = reinterpret_cast<unsigned long long*>(status_dev);
    return na == 9 ? merge_launch<9>(*in, n, order, start, dst, head, count, n_groups, (int64_t*)ws, *out, st, s)
                   : merge_launch<65>(*in, n, order, start, dst, head, count, n_groups, (int64_t*)ws, *out, st, s);
}
