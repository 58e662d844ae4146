// bz_probe.hip -- the float primitives of bz_math.h, one at a time, from the host build or from the gfx950 build
// (DESIGN.md 3.4): the entry point tests/test_spec_math_cpu.py and tests/test_gpu_spec_math.py compare the two builds
// through.  Both cases call the functions of bz_math.h themselves.  Nothing of the engine calls this file.
//   map    out[i] = op(a[i] (, b[i])), n elements
//   sweep  every 32-bit pattern p in [lo, hi): out[(p >> 24) - (lo >> 24)] += mix64(p << 32 | canon(bits(op(p)))) mod 2^64,
//          canon = every NaN -> 0x7FC00000.  A sum of 64-bit integers: the same number in any evaluation order.
#include "bz_common.h"
#include "bz_math.h"

using namespace bz;

namespace {

BZ_HD u32 probe_canon(u32 b) { return (b & 0x7FFFFFFFu) > 0x7F800000u ? 0x7FC00000u : b; }

template <int OP>
BZ_HD float probe_unary(float x) {
    if constexpr (OP == BZ_PROBE_EXPF) return expf_spec(x);
    else if constexpr (OP == BZ_PROBE_LOGF) return logf_spec(x);
    else if constexpr (OP == BZ_PROBE_TANHF) return tanhf_spec(x);
    else return fsqrt(x);
}

// element i of a map; the result's bits
template <int OP>
BZ_HD u32 probe_map_one(const void* a, const void* b, int64_t i) {
    const float* fa = static_cast<const float*>(a);
    const float* fb = static_cast<const float*>(b);
    const u64* ua = static_cast<const u64*>(a);
    const u64* ub = static_cast<const u64*>(b);
    float r;
    if constexpr (OP <= BZ_PROBE_FSQRT) r = probe_unary<OP>(fa[i]);
    else if constexpr (OP == BZ_PROBE_FDIV) r = fdiv(fa[i], fb[i]);
    else if constexpr (OP == BZ_PROBE_U01) r = u01_spec(ua[i]);
    else if constexpr (OP == BZ_PROBE_HASH_LOGIT) r = hash_logit(ua[i], (int)ub[i]);
    else if constexpr (OP == BZ_PROBE_HASH_VALUE) r = hash_value(ua[i]);
    else r = gamma_spec(fa[i], ub[4 * i], ub[4 * i + 1], ub[4 * i + 2], (int)ub[4 * i + 3]);
    return f_to_bits(r);
}

template <int OP>
BZ_HD u64 probe_sweep_one(u64 p) {
    const u32 y = f_to_bits(probe_unary<OP>(f_from_bits((u32)p)));
    return mix64(p << 32 | (u64)probe_canon(y));
}

template <int OP>
__global__ void __launch_bounds__(256) k_probe_map(const void* a, const void* b, int64_t n, u32* out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) out[i] = probe_map_one<OP>(a, b, i);
}

// blockIdx.y = the chunk (relative to lo >> 24), blockIdx.x strides over that chunk's patterns inside [lo, hi)
template <int OP>
__global__ void __launch_bounds__(256) k_probe_sweep(u64 lo, u64 hi, u64* out) {
    const u64 c0 = ((lo >> 24) + blockIdx.y) << 24, c1 = c0 + (1ULL << 24);
    const u64 p0 = c0 > lo ? c0 : lo, p1 = c1 < hi ? c1 : hi;
    u64 s = 0;
    for (u64 p = p0 + (u64)blockIdx.x * 256 + threadIdx.x; p < p1; p += (u64)gridDim.x * 256) s += probe_sweep_one<OP>(p);
    u32 l = (u32)s, h = (u32)(s >> 32);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {  // 64-bit wave sum through two 32-bit shuffles
        const u64 y = (u64)__shfl_xor(l, o, 64) | ((u64)__shfl_xor(h, o, 64) << 32);
        s += y;
        l = (u32)s; h = (u32)(s >> 32);
    }
    if ((threadIdx.x & 63) == 0) atomicAdd(reinterpret_cast<unsigned long long*>(&out[blockIdx.y]), (unsigned long long)s);
}

template <int OP>
int32_t probe_map(int where, const void* a, const void* b, int64_t n, u32* out, hipStream_t s) {
    if (where == BZ_PROBE_HOST) {
        for (int64_t i = 0; i < n; ++i) out[i] = probe_map_one<OP>(a, b, i);
        return BZ_OK;
    }
    const int64_t nb = (n + 255) / 256;
    hipLaunchKernelGGL(k_probe_map<OP>, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, s, a, b, n, out);
    BZ_LAUNCH_CHECK("k_probe_map");
    return BZ_OK;
}

template <int OP>
int32_t probe_sweep(int where, u64 lo, u64 hi, u64* out, hipStream_t s) {
    const u64 nc = ((hi - 1) >> 24) - (lo >> 24) + 1;
    if (where == BZ_PROBE_HOST) {
        for (u64 c = 0; c < nc; ++c) out[c] = 0;
        for (u64 p = lo; p < hi; ++p) out[(p >> 24) - (lo >> 24)] += probe_sweep_one<OP>(p);
        return BZ_OK;
    }
    BZ_HIP(hipMemsetAsync(out, 0, nc * sizeof(u64), s));
    hipLaunchKernelGGL(k_probe_sweep<OP>, dim3(64, (unsigned)nc), dim3(256), 0, s, lo, hi, out);
    BZ_LAUNCH_CHECK("k_probe_sweep");
    return BZ_OK;
}

template <int OP>
int32_t probe_op(int where, int mode, const void* a, const void* b, int64_t n, u64 lo, u64 hi, void* out, hipStream_t s) {
    if (mode == BZ_PROBE_MAP) return probe_map<OP>(where, a, b, n, static_cast<u32*>(out), s);
    if constexpr (OP <= BZ_PROBE_FSQRT) return probe_sweep<OP>(where, lo, hi, static_cast<u64*>(out), s);
    return BZ_EINVAL;  // (refused by bz_spec_probe before it gets here)
}

}  // namespace

BZ_EXPORT int32_t bz_spec_probe(int32_t op, int32_t where, int32_t mode, const void* a, const void* b, int64_t n, uint64_t lo,
                                uint64_t hi, void* out, void* stream) {
    BZ_REQUIRE(op >= BZ_PROBE_EXPF && op <= BZ_PROBE_GAMMA, "bz_spec_probe: unknown op");
    BZ_REQUIRE(where == BZ_PROBE_HOST || where == BZ_PROBE_DEVICE, "bz_spec_probe: where must be BZ_PROBE_HOST or BZ_PROBE_DEVICE");
    BZ_REQUIRE(mode == BZ_PROBE_MAP || mode == BZ_PROBE_SWEEP, "bz_spec_probe: mode must be BZ_PROBE_MAP or BZ_PROBE_SWEEP");
    BZ_REQUIRE(out, "bz_spec_probe: null output");
    if (mode == BZ_PROBE_MAP) {
        const bool two = op == BZ_PROBE_FDIV || op == BZ_PROBE_HASH_LOGIT || op == BZ_PROBE_GAMMA;
        BZ_REQUIRE(n >= 0 && (n == 0 || (a && (b || !two))), "bz_spec_probe: negative n or a null operand");
    } else {
        BZ_REQUIRE(op <= BZ_PROBE_FSQRT, "bz_spec_probe: sweep takes an op whose input is one 32-bit pattern");
        BZ_REQUIRE(lo < hi && hi <= (1ULL << 32), "bz_spec_probe: sweep needs lo < hi <= 2^32");
    }
    hipStream_t s = (hipStream_t)stream;
    switch (op) {
        case BZ_PROBE_EXPF: return probe_op<BZ_PROBE_EXPF>(where, mode, a, b, n, lo, hi, out, s);
        case BZ_PROBE_LOGF: return probe_op<BZ_PROBE_LOGF>(where, mode, a, b, n, lo, hi, out, s);
        case BZ_PROBE_TANHF: return probe_op<BZ_PROBE_TANHF>(where, mode, a, b, n, lo, hi, out, s);
        case BZ_PROBE_FSQRT: return probe_op<BZ_PROBE_FSQRT>(where, mode, a, b, n, lo, hi, out, s);
        case BZ_PROBE_FDIV: return probe_op<BZ_PROBE_FDIV>(where, mode, a, b, n, lo, hi, out, s);
        case BZ_PROBE_U01: return probe_op<BZ_PROBE_U01>(where, mode, a, b, n, lo, hi, out, s);
        case BZ_PROBE_HASH_LOGIT: return probe_op<BZ_PROBE_HASH_LOGIT>(where, mode, a, b, n, lo, hi, out, s);
        case BZ_PROBE_HASH_VALUE: return probe_op<BZ_PROBE_HASH_VALUE>(where, mode, a, b, n, lo, hi, out, s);
        default: return probe_op<BZ_PROBE_GAMMA>(where, mode, a, b, n, lo, hi, out, s);
    }
}
