// fp8 (OCP e4m3fn) KV-cache element conversions shared by the KV writer (rope_kv.hip), the
// attention kernels (attention.hip) and the dequantiser (kv_dequant.hip).
#pragma once
#include "common.h"

#define KV_FP8_MAX 448.f

// Quantiser input: clamp to the e4m3 range explicitly (the convert instruction's overflow behaviour
// is not relied on); a NaN is selected around the clamp so it stays a NaN code -- a min/max clamp
// alone would launder it into +-448.
__device__ __forceinline__ float kv_fp8_clamp(float y) {
  const float c = fminf(fmaxf(y, -KV_FP8_MAX), KV_FP8_MAX);
  return y != y ? y : c;
}

// 8 values x inv_scale -> 8 e4m3 codes (round to nearest even), element i in byte i
__device__ __forceinline__ uint2 kv_fp8_quant8(const float* x, float inv) {
  float y[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) y[i] = kv_fp8_clamp(x[i] * inv);
  uint32_t w0 = 0, w1 = 0;
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], w0, false);
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], w0, true);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], w1, false);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], w1, true);
  return make_uint2(w0, w1);
}

// 8 e4m3 codes (two dwords, element i in byte i) -> one bf16 MFMA operand fragment, exactly
__device__ __forceinline__ bf16x8 kv_fp8_to_bf16x8(uint32_t lo, uint32_t hi) {
  const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false);
  const bf16x2 b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true);
  const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false);
  const bf16x2 d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true);
  return bf16x8{a[0], a[1], b[0], b[1], c[0], c[1], d[0], d[1]};
}
