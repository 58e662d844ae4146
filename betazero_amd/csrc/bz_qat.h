// bz_qat.h -- fp8 quantisation-aware training: the fp8 net's quantisation rule (quant.py, bz_net.hip's host
// packing and fp8 epilogue), stated once, __host__ __device__, so that bz_qat_weight_row / bz_qat_act (host) are the code the
// k_qat_* kernels run.  Every value this rule produces -- an e4m3 value times a power of two -- is exact in bf16, which is why
// the bf16 MFMA training tower can run the fp8 net's forward on exact operands.
//   weights     : w_b = bf16_RNE(w);  m = max |w_b| over the output channel (a NaN is skipped, as fmaxf does in the host packing);
//                 s = 2^floor(log2(448 / m)) (1 for m == 0);  w_q = e4m3_RNE_sat(w_b s) / s   (a NaN weight stays a NaN)
//   activations : a = e4m3_RNE_sat(16 maximum(v, +0)) / 16 from the fp32 value: ONE rounding; a NaN passes, +inf -> 28
#pragma once
#include "bz_math.h"

namespace bz {

BZ_HD u32 qat_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(f);
#else
    u32 u;
    __builtin_memcpy(&u, &f, 4);
    return u;
#endif
}

// bf16 round to nearest even, widened again (bz_net.hip's f2bf: infinities keep their bits, a NaN stays a NaN, quiet bit set)
BZ_HD float qat_bf16(float f) {
    const u32 u = qat_bits(f);
    if ((u & 0x7F800000u) == 0x7F800000u) return f_from_bits((u & 0xFFFF0000u) | ((u & 0x7FFFFFu) ? 0x400000u : 0u));
    return f_from_bits((u + 0x7FFFu + ((u >> 16) & 1u)) & 0xFFFF0000u);
}

// the running maximum of |w_b| over a channel: a NaN never wins the comparison, so it is skipped (fmaxf in the host packing)
BZ_HD float qat_absmax(float m, float w_b) {
    const float a = __builtin_fabsf(w_b);
    return a > m ? a : m;
}

// 2^k
BZ_HD float qat_pow2(int k) { return f_from_bits((u32)(k + 127) << 23); }

// the largest power of two s with m s <= 448 (bz_net.hip's pow2_scale, quant.channel_scale): s = 2^floor(log2(448 / m)), in
// integer arithmetic on m's exponent -- no division, the same on both sides.  m = f 2^e, f in [1, 2): 448 / m = (1.75 / f) 2^(8 - e),
// so floor(log2) = 8 - e for f <= 1.75 and 7 - e above.  m below 1e-30 counts as 1e-30 (channel_scale's floor: 448 / m stays
// finite; such a channel's weights all round to 0 either way); m == 0 or an all-NaN channel (m stays 0) give 1, an infinite m
// 0.5 (what frexp makes of 448 / inf = 0 in both).
BZ_HD float qat_pow2_scale(float m) {
    if (!(m > 0.0f)) return 1.0f;
    if (m > 3.4028234e38f) return 0.5f;
    if (m < 1e-30f) m = 1e-30f;
    const u32 u = qat_bits(m);
    const int e = (int)(u >> 23) - 127;
    return qat_pow2(((u & 0x7FFFFFu) <= 0x600000u ? 8 : 7) - e);
}
// 1 / s for a power of two s in [2^-126, 2^126]
BZ_HD float qat_pow2_inv(float s) { return f_from_bits(0x7F000000u - qat_bits(s)); }

// the nearest OCP e4m3fn value (round to nearest even, saturating at +-448, subnormal step 2^-9) as a float; NaN in, NaN out
BZ_HD float qat_e4m3(float x) {
    if (x != x) return x;
    const u32 sign = qat_bits(x) & 0x80000000u;
    float a = __builtin_fabsf(x);
    if (a == 0.0f) return 0.0f;   // +-0 -> +0 (f2e4m3, quant.e4m3_round); a negative value that ROUNDS to 0 keeps its sign
    if (a >= 448.0f) return f_from_bits(sign | 0x43E00000u);   // 448
    if (a < 0.015625f) {   // below 2^-6: multiples of 2^-9 -- the float grid at 2^14, so one add rounds to nearest even
        a = (a + 16384.0f) - 16384.0f;
        return f_from_bits(sign | qat_bits(a));
    }
    u32 u = qat_bits(a);   // 3 mantissa bits: round the low 20 away (a carry moves into the exponent, as it should)
    u = (u + 0x7FFFFu + ((u >> 20) & 1u)) & 0xFFF00000u;
    return f_from_bits(sign | u);
}

// one weight of a channel with scale s
BZ_HD float qat_weight(float w_b, float s) { return qat_e4m3(w_b * s) * qat_pow2_inv(s); }

// IEEE maximum(v, +0): a NaN passes, -0 and negatives become +0
BZ_HD float qat_relu(float v) { return v != v ? v : (v > 0.0f ? v : 0.0f); }

// the stored activation of the fp8 net, from the fp32 value (accumulator + bias + skip)
BZ_HD float qat_act(float v) { return qat_e4m3(16.0f * qat_relu(v)) * 0.0625f; }

#if defined(__HIPCC__)
typedef __attribute__((ext_vector_type(2))) float qat_f32x2;
typedef __attribute__((ext_vector_type(4))) float qat_f32x4;
// The device form the k_qat_* epilogues run: the inference fp8 epilogue's own conversion (bz_net.hip: minimum(., 448), then
// v_cvt_pk_fp8_f32, which stores a NaN as the e4m3fn NaN code) and straight back through v_cvt_pk_f32_fp8.  v has been through the
// ReLU already (IEEE maximum(., +0)).  tests/test_gpu_qat.py pins it to qat_act over every bf16 pattern and every e4m3 tie.
__device__ __forceinline__ qat_f32x4 qat_act_dev4(qat_f32x4 v) {
    const qat_f32x4 t = __builtin_elementwise_minimum(v * 16.0f, (qat_f32x4)(448.0f));
    int pk = __builtin_amdgcn_cvt_pk_fp8_f32(t[0], t[1], 0, false);
    pk = __builtin_amdgcn_cvt_pk_fp8_f32(t[2], t[3], pk, true);
    const qat_f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(pk, false), hi = __builtin_amdgcn_cvt_pk_f32_fp8(pk, true);
    const qat_f32x4 a = {lo[0], lo[1], hi[0], hi[1]};
    return a * 0.0625f;
}
#endif

}  // namespace bz
