// Paged KV-cache layout shared by the KV writer (rope_kv.hip) and the attention kernels.
//
// A block holds KV_BS = 64 tokens of one kv head = exactly one 64-key attention tile, and is
// stored in **MFMA-fragment-native order**: the 16-byte operand fragment that lane l of a wave
// feeds to v_mfma_f32_16x16x32_bf16 for fragment f lives at byte 16*(64*f + l).  Hence
//   * decode streams a block with perfectly coalesced 1-KiB wave-instructions straight into
//     VGPRs (no LDS hop, no over-fetch), and
//   * prefill stages a block into LDS with lane-linear global_load_lds (no swizzle needed) and
//     reads fragments back with conflict-free consecutive ds_read_b128.
//
// K (A operand of S^T = K.Q^T): fragment f = t*(D/32) + c for key tile t (16 keys) and k-chunk c
//   (32 dims); lane = 16*g + r holds key 16t+r, dims 32c + 8g + 0..7.
// V (A operand of O^T = V^T.P^T): fragment f = 2*dt + s for dim tile dt (16 dims) and key step s
//   (32 keys); lane = 16*g + row holds dim 16dt+row and the 8 keys whose scores lane group g
//   already holds in registers after the S^T MFMA: 32s + 4g + 0..3 and 32s + 16 + 4g + 0..3.
//
// fp8 (OCP e4m3fn) cache, 1-byte elements: the same fragment decomposition, two consecutive
// fragments sharing one lane's 16 bytes.  With f, lane, j as above, element j of fragment f sits at
//   byte ((f >> 1) * 64 + lane) * 16 + (f & 1) * 8 + j
// so a lane's 16-B load is still one 1-KiB wave instruction (now two MFMA operand fragments, bytes
// 0-7 and 8-15), an LDS read back is still a lane-linear ds_read_b128, and a (block, kv head) tile
// is 64 * D bytes.  Every e4m3 value is exact in bf16: the attention kernels convert fragments in
// registers (kv_fp8.h) and run the bf16 MFMA math unchanged.
#pragma once

#define KV_BS 64

// element index inside one (block, kv head) tile of K
__host__ __device__ __forceinline__ int k_index(int key, int d, int D) {
  const int t = key >> 4, r = key & 15, c = d >> 5, g = (d >> 3) & 3, j = d & 7;
  return (((t * (D >> 5) + c) * 64 + g * 16 + r) << 3) + j;
}

// element index inside one (block, kv head) tile of V
__host__ __device__ __forceinline__ int v_index(int key, int d, int D) {
  const int dt = d >> 4, row = d & 15, s = key >> 5, k = key & 31;
  const int g = (k & 15) >> 2, j = ((k >> 4) << 2) + (k & 3);
  return (((dt * 2 + s) * 64 + g * 16 + row) << 3) + j;
}

// byte index inside one (block, kv head) tile of an fp8 K cache
__host__ __device__ __forceinline__ int k_index8(int key, int d, int D) {
  const int t = key >> 4, r = key & 15, c = d >> 5, g = (d >> 3) & 3, j = d & 7;
  const int f = t * (D >> 5) + c;
  return (((f >> 1) * 64 + g * 16 + r) << 4) + ((f & 1) << 3) + j;
}

// byte index inside one (block, kv head) tile of an fp8 V cache
__host__ __device__ __forceinline__ int v_index8(int key, int d, int D) {
  const int dt = d >> 4, row = d & 15, s = key >> 5, k = key & 31;
  const int g = (k & 15) >> 2, j = ((k >> 4) << 2) + (k & 3);
  const int f = dt * 2 + s;
  return (((f >> 1) * 64 + g * 16 + row) << 4) + ((f & 1) << 3) + j;
}
