// fp8 (e4m3) paged KV tiles -> bf16 tiles in the bf16 fragment-native layout (kv_layout.h).
//
// src [tiles, 64*D] bytes, dst [tiles, 64*D] bf16, tile i belonging to kv head i % Hkv.  The two
// layouts share the fragment decomposition: the 16-B piece p = (f >> 1) * 64 + lane of an fp8 tile
// holds lane `lane`'s fragments f and f + 1 (bytes 0-7 and 8-15), which are the bf16 tile's 16-B
// pieces f * 64 + lane and (f + 1) * 64 + lane -- the same for K and V.  The conversion is the
// attention kernels' own helper (kv_fp8.h), so a test of this kernel over all 256 codes pins it.
// scales [Hkv] f32 (optional): values are multiplied by their head's scale before the bf16 rounding.
#include "common.h"
#include "kv_layout.h"
#include "kv_fp8.h"

union DqFrag {
  uint4 u;
  bf16x8 v;
};

__global__ void __launch_bounds__(256) kv_dequant_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                         const float* __restrict__ scales, int Hkv, int pieces) {
  const long tile = blockIdx.x;
  const float sc = scales ? scales[tile % Hkv] : 1.f;
  const uint4* s = src + tile * pieces;
  uint4* d = dst + tile * pieces * 2;
  for (int p = threadIdx.x; p < pieces; p += blockDim.x) {
    const uint4 raw = s[p];
    const int f2 = p >> 6, lane = p & 63;
    DqFrag a, b;
    a.v = kv_fp8_to_bf16x8(raw.x, raw.y);
    b.v = kv_fp8_to_bf16x8(raw.z, raw.w);
    if (scales) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        a.v[e] = (bf16)((float)a.v[e] * sc);
        b.v[e] = (bf16)((float)b.v[e] * sc);
      }
    }
    d[(2 * f2) * 64 + lane] = a.u;
    d[(2 * f2 + 1) * 64 + lane] = b.u;
  }
}

PENNY_API int penny_kv_dequant_fp8(const void* src, void* dst, const float* scales, long tiles, int Hkv, int D,
                                   hipStream_t stream) {
  if (tiles <= 0) return 0;
  if (D != 128 || Hkv <= 0 || tiles > 0x7fffffffL) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(kv_dequant_kernel, dim3((unsigned)tiles), dim3(256), 0, stream, (const uint4*)src, (uint4*)dst,
                     scales, Hkv, KV_BS * D / 16);
  PENNY_RETURN_LAUNCH();
}
