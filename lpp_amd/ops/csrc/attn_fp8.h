// FP8 KV cache format (OCP e4m3, gfx950 conversion instructions), shared by
// attention_decode_fp8.hip and the fp8 instantiations of attention_extend.hip.
//
// A cached row (the 128 values of one token and kv head) is 128 e4m3 bytes and
// one fp32 scale 2^e.  With amax = m 2^E, 0.5 <= m < 1: e = E - 9 if m <= 0.875,
// else E - 8; e >= -100; e = 0 for a row of zeros.  Then |x| / scale <= 448, so
// nothing saturates, and byte * scale has 4 significant bits and an exponent in
// range: it is exact in bf16.  The kernels therefore turn fp8 into bf16 in
// registers and feed the bf16 MFMA paths with no extra rounding.
// ops/attention.py, quantize_kv_rows_fp8, is the same rule in torch.
#pragma once

#include "attn_tile.h"

namespace lpp {

typedef __attribute__((ext_vector_type(2))) __bf16 fp8_bf16x2;
typedef __attribute__((ext_vector_type(2))) float fp8_f32x2;

constexpr int kFp8MinExp = -100;

// e of a row from its amax (>= 0, finite), on the float's bits: amax =
// 1.f 2^(b-127) = (1.f / 2) 2^(b-126), and m <= 0.875 iff 1.f <= 1.75.  A
// subnormal amax (b = 0) lands below the clamp either way.
__device__ __forceinline__ int fp8_row_exp(float amax) {
  const uint32_t u = __builtin_bit_cast(uint32_t, amax);
  if (u == 0u) return 0;
  const int E = (int)(u >> 23) - 126;
  const int e = (u & 0x7fffffu) <= 0x600000u ? E - 9 : E - 8;
  return e < kFp8MinExp ? kFp8MinExp : e;
}
// 2^e as a float, -126 <= e <= 127
__device__ __forceinline__ float fp8_pow2(int e) {
  return __builtin_bit_cast(float, (uint32_t)(e + 127) << 23);
}

// Two floats, already divided by the scale, to two e4m3 bytes (bits 0..15).
__device__ __forceinline__ uint32_t fp8_pack2(float a, float b) {
  return (uint32_t)__builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false) & 0xffffu;
}
// Those two bytes back to floats (unscaled).
__device__ __forceinline__ fp8_f32x2 fp8_unpack2(uint32_t w) {
  return __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
}

// 8 e4m3 bytes (lo: elements 0..3, hi: 4..7) times a power-of-two scale to
// bf16x8: four v_cvt_scalef32_pk_bf16_fp8, the scale folded in, exact.
__device__ __forceinline__ bf16x8 fp8x8_to_bf16(uint32_t lo, uint32_t hi, float scale) {
  const fp8_bf16x2 r[4] = {__builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)lo, scale, false),
                           __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)lo, scale, true),
                           __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)hi, scale, false),
                           __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8((int)hi, scale, true)};
  return __builtin_bit_cast(bf16x8, r);
}

}  // namespace lpp
