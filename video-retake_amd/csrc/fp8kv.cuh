// fp8kv.cuh - the e4m3 row format of the compressed video K / V rows (retake_hip.h "FP8 rows of the compressed cache"):
// D one-byte OCP e4m3fn codes and one power-of-two fp32 scale per (kv head, row).  Shared by the archive kernel (quantise),
// rtk_fp8kv_dequant and the chunk attention's archive tiles (dequantise): one definition of each direction.
#pragma once
#include "common.cuh"

namespace rtk {

// scale = 2^e of a row whose largest magnitude is amax (finite): amax = m 2^E, m in [0.5, 1) -> e = E - 9 (m <= 0.875) or
// E - 8, so amax / scale lies in (224, 448] and no code saturates; amax == 0 -> e = 0.
__device__ __forceinline__ int fp8_row_exp(float amax) {
    if (amax == 0.f) return 0;
    const int E = __builtin_amdgcn_frexp_expf(amax);
    const float m = __builtin_amdgcn_frexp_mantf(amax);
    return E - (m <= 0.875f ? 9 : 8);
}
// 2^e as fp32 for e in [-149, 127], from its bits (no dependence on the denormal mode)
__device__ __forceinline__ float fp8_exp2i(int e) {
    return __uint_as_float(e >= -126 ? (uint32_t)(e + 127) << 23 : 1u << (e + 149));
}
// four values * 2^ne (exact: v_ldexp_f32) -> four e4m3fn codes, round to nearest even (v_cvt_pk_fp8_f32)
__device__ __forceinline__ uint32_t fp8_quant4(float a, float b, float c, float d, int ne) {
    int r = __builtin_amdgcn_cvt_pk_fp8_f32(__builtin_ldexpf(a, ne), __builtin_ldexpf(b, ne), 0, false);
    r = __builtin_amdgcn_cvt_pk_fp8_f32(__builtin_ldexpf(c, ne), __builtin_ldexpf(d, ne), r, true);
    return (uint32_t)r;
}
// 8 values of the model dtype (one 16-byte chunk) -> 8 codes
template <int DT> __device__ __forceinline__ void fp8_quant_chunk(const u32x4& x, int ne, uint32_t& c0, uint32_t& c1) {
    float f[8];
    Vec16<DT>::unpack(x, f);
    c0 = fp8_quant4(f[0], f[1], f[2], f[3], ne);
    c1 = fp8_quant4(f[4], f[5], f[6], f[7], ne);
}
// max |x| over one 16-byte chunk of 16-bit floats, as fp32
template <int DT> __device__ __forceinline__ float fp8_chunk_amax(const u32x4& x) {
    float f[8];
    Vec16<DT>::unpack(x, f);
    float a = __builtin_fabsf(f[0]);
#pragma unroll
    for (int e = 1; e < 8; ++e) a = fmaxf(a, __builtin_fabsf(f[e]));
    return a;
}
// (scale: a NORMAL fp32 power of two - rows with amax >= 2^-117, the supported range of retake_hip.h)
// four codes -> two packed pairs of the model dtype: dtype(float(code) * scale), scale a power of two (the product is
// exact, and exactly representable in bf16) - v_cvt_scalef32_pk_{bf16,f16}_fp8, one instruction per pair
template <int DT> __device__ __forceinline__ void fp8_dequant4(uint32_t c, float scale, uint32_t& lo, uint32_t& hi) {
    if constexpr (DT == RTK_BF16) {
        lo = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c, scale, false));
        hi = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(c, scale, true));
    } else {
        lo = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c, scale, false));
        hi = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(c, scale, true));
    }
}
// 16 codes -> 16 values: the two 16-byte chunks a 16-bit row holds in their place
template <int DT> __device__ __forceinline__ void fp8_dequant16(const u32x4& c, float scale, u32x4& a, u32x4& b) {
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) fp8_dequant4<DT>(c[i], scale, w[2 * i], w[2 * i + 1]);
    a = u32x4{w[0], w[1], w[2], w[3]};
    b = u32x4{w[4], w[5], w[6], w[7]};
}

}  // namespace rtk
