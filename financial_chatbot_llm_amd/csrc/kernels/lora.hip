// Multi-LoRA delta for one projection of a step (ops/lora.py): rows of one batch run on different
// adapters ("slots") of one table, or on none.
//
// For a row m with slot a = row_slot[m] in [0, slots) and a projection with base output `base`:
//   t[m, :] = bf16( sum_k x[m, k] * A_a[:, k] )                 f32 accumulation, ONE rounding
//   y[m, n] = base[m, n] + scale_a * sum_j t[m, g R + j] * B_a[n, j]   for n in column segment g
// A_a [C, K] (C = segments * R: the segments' A matrices stacked), B_a [N, R], both bf16 and
// zero-padded to the table rank R (32 or 64); scale_a f32.  `base` is a bf16 [M, N] tensor rewritten
// in place (float(base) + delta in f32, then one round-to-nearest-even) or slab 0 of a split-K GEMM's
// f32 slabs (the f32 delta is added; the consumer's slab sum does the rest).  A row whose slot is
// outside the table, and the columns of a segment its adapter does not target (bit g of present[a]
// clear), keep every bit.
//
// Two launches, no atomics, nothing data-dependent in the order of any sum:
//   shrink  t partials [S, M, C] f32: a workgroup owns 16 rows x 512 k (S = ceil(K / 512), a function of
//           K alone, so that a decode-size step still spreads over the chip), its 4 waves 128 k each
//           -- four MFMA k steps, unrolled so their loads are in flight together -- summed through LDS
//           in wave order
//   expand  sums the S partials in order, rounds t to bf16 once, rank-R MFMA against B rows, epilogue
// Both use v_mfma_f32_16x16x32_bf16 transposed (the table rows are the MFMA A operand, the step's rows
// the B operand), so a lane owns ONE step row (lane & 15) and 4 consecutive output columns.  A 16-row
// tile that holds several slots loops over them (wave-uniform); the rows of the other slots enter
// that pass as zero fragments, which add +0 to an accumulator that is never -0: a row's bits do not
// depend on its tile mates, its position or M.
#include "common.h"

static constexpr int LORA_THREADS = 256;
static constexpr int LORA_KW = 128;                  // k per wave of a shrink workgroup (K is a multiple of it)
static constexpr int LORA_KB = 4 * LORA_KW;          // k per shrink workgroup

struct LoraSegs {
  int n;                                             // 1..3 column segments
  int end[3];                                        // segment g covers columns [end[g-1], end[g])
};

__device__ __forceinline__ bf16x8 lora_zero8() {
  Pack8 p;
  p.u = make_uint4(0u, 0u, 0u, 0u);
  return p.v;
}

__device__ __forceinline__ bf16x8 lora_load8(const bf16* p) {
  Pack8 v;
  v.u = *reinterpret_cast<const uint4*>(p);
  return v.v;
}

// the lane's row slot, -1 for a row past M or a slot outside the table
__device__ __forceinline__ int lora_row_slot(const int* __restrict__ row_slot, int m, int M, int slots) {
  if (m >= M) return -1;
  const int s = row_slot[m];
  return (s < 0 || s >= slots) ? -1 : s;
}

// grid (ceil(M / 16), S): part[s, m, c] = sum over the workgroup's k of x[m, k] * A_slot(m)[c, k]; rows
// without a slot are written as 0 in a tile that holds a slot, and not at all in one that holds none
// (the expand never reads them).
template <int NCT>
__global__ void __launch_bounds__(LORA_THREADS) lora_shrink_kernel(const bf16* __restrict__ x, long xs,
                                                                   const int* __restrict__ row_slot,
                                                                   const bf16* __restrict__ A, int slots,
                                                                   float* __restrict__ part, int M, int K) {
  constexpr int C = NCT * 16;
  __shared__ float red[4 * 16 * C];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int m0 = blockIdx.x * 16, m = m0 + r;
  const int slot = lora_row_slot(row_slot, m, M, slots);
  unsigned long long todo = __ballot(slot >= 0);
  if (todo == 0) return;                             // the same for all 4 waves: no barrier is skipped
  f32x4 acc[NCT];
#pragma unroll
  for (int c = 0; c < NCT; ++c) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int kb = blockIdx.y * LORA_KB + w * LORA_KW;
  const bool live = kb < K;                          // wave-uniform: K % LORA_KW == 0, a wave has all its k or none
  const bf16* xrow = x + (size_t)(slot >= 0 ? m : m0) * xs + q * 8;     // m0 < M: never past the tensor
  while (todo) {
    const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
    const int cur = __builtin_amdgcn_readlane(slot, src);
    const bool mine = slot == cur;
    todo &= ~__ballot(mine);
    const bf16* Ab = A + ((size_t)cur * C + r) * K + q * 8;
    if (!live) continue;
#pragma unroll
    for (int kk = 0; kk < LORA_KW / 32; ++kk) {
      const int k = kb + 32 * kk;
      const bf16x8 xf = mine ? lora_load8(xrow + k) : lora_zero8();
#pragma unroll
      for (int c = 0; c < NCT; ++c)
        acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lora_load8(Ab + (size_t)c * 16 * K + k), xf, acc[c], 0, 0, 0);
    }
  }
  // lane: row r, columns 16 c + 4 q + (0..3)
#pragma unroll
  for (int c = 0; c < NCT; ++c)
    *reinterpret_cast<f32x4*>(red + (w * 16 + r) * C + 16 * c + 4 * q) = acc[c];
  __syncthreads();
  float* dst = part + ((size_t)blockIdx.y * M + m0) * C;
  const int rows = min(16, M - m0);
  for (int e = threadIdx.x * 4; e < rows * C; e += LORA_THREADS * 4) {
    f32x4 s = *reinterpret_cast<const f32x4*>(red + e);
#pragma unroll
    for (int v = 1; v < 4; ++v) s += *reinterpret_cast<const f32x4*>(red + v * 16 * C + e);
    *reinterpret_cast<f32x4*>(dst + e) = s;
  }
}

// 8 consecutive t values of a row: the S partials summed in order, rounded to bf16 once
__device__ __forceinline__ bf16x8 lora_t8(const float* __restrict__ p, int S, size_t ss) {
  f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll 4
  for (int s = 1; s < S; ++s) {
    a += *reinterpret_cast<const f32x4*>(p + s * ss);
    b += *reinterpret_cast<const f32x4*>(p + s * ss + 4);
  }
  Pack8 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    o.e[j] = (bf16)a[j];
    o.e[4 + j] = (bf16)b[j];
  }
  return o.v;
}

// grid (ceil(M / 16), ceil(N / 16 / ct_per_wave / 4)): a wave owns 16 rows x ct_per_wave column tiles.
// T = bf16: out[m, n] = bf16(float(out[m, n]) + delta); T = float: out[m, n] += delta (slab 0).
template <typename T, int KS>
__global__ void __launch_bounds__(LORA_THREADS) lora_expand_kernel(const float* __restrict__ part, int S,
                                                                   const int* __restrict__ row_slot,
                                                                   const bf16* __restrict__ B,
                                                                   const int* __restrict__ present,
                                                                   const float* __restrict__ scale, int slots,
                                                                   LoraSegs segs, T* __restrict__ out, long os, int M,
                                                                   int N, int ct_per_wave) {
#pragma clang fp contract(off)
  constexpr int R = 32 * KS;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = lane & 15, q = lane >> 4;
  const int m0 = blockIdx.x * 16, m = m0 + r;
  const int slot = lora_row_slot(row_slot, m, M, slots);
  const unsigned long long all = __ballot(slot >= 0);
  if (all == 0) return;
  const int C = segs.n * R;
  const size_t ss = (size_t)M * C;
  const int ct0 = (blockIdx.y * 4 + w) * ct_per_wave;
  const int ct1 = min(N / 16, ct0 + ct_per_wave);
  const int pres = slot >= 0 ? present[slot] : 0;
  const float sc = slot >= 0 ? scale[slot] : 0.f;
  // Four column tiles at a time: per slot of the row tile, the tiles' B fragments are loaded together
  // (one memory latency per slot, not per slot and tile), each tile into its own accumulator.
  int g = -1;
  bf16x8 tf[KS];                                     // t of the current segment
  for (int ctb = ct0; ctb < ct1; ctb += 4) {
    bf16x8 tfs[4][KS];
    int gs[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n0 = min(ctb + j, ct1 - 1) * 16;     // a tile past the wave's range repeats the last one, unwritten
      int gn = 0;
      while (gn < segs.n - 1 && n0 >= segs.end[gn]) ++gn;
      if (gn != g) {                                 // wave-uniform: the tile's segment changed
        g = gn;
#pragma unroll
        for (int kk = 0; kk < KS; ++kk)
          tf[kk] = slot >= 0 ? lora_t8(part + (size_t)m * C + g * R + kk * 32 + q * 8, S, ss) : lora_zero8();
      }
      gs[j] = gn;
#pragma unroll
      for (int kk = 0; kk < KS; ++kk) tfs[j][kk] = tf[kk];
    }
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    unsigned long long todo = all;
    while (todo) {
      const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
      const int cur = __builtin_amdgcn_readlane(slot, src);
      const bool mine = slot == cur;
      todo &= ~__ballot(mine);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n0 = min(ctb + j, ct1 - 1) * 16;
        const bf16* Bb = B + ((size_t)cur * N + n0 + r) * R + q * 8;
#pragma unroll
        for (int kk = 0; kk < KS; ++kk)
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lora_load8(Bb + kk * 32), mine ? tfs[j][kk] : lora_zero8(),
                                                           acc[j], 0, 0, 0);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      // the row, this segment of it, or a tile past the range keeps its bits
      if (slot < 0 || ctb + j >= ct1 || !((pres >> gs[j]) & 1)) continue;
      T* o = out + (size_t)m * os + (ctb + j) * 16 + 4 * q;      // lane: row r, columns n0 + 4 q + (0..3)
      if (sizeof(T) == 2) {
        bf16x4 b = *reinterpret_cast<const bf16x4*>(o);
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i] = (bf16)((float)b[i] + sc * acc[j][i]);
        *reinterpret_cast<bf16x4*>(o) = b;
      } else {
        f32x4 b = *reinterpret_cast<const f32x4*>(o);
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i] = b[i] + sc * acc[j][i];
        *reinterpret_cast<f32x4*>(o) = b;
      }
    }
  }
}

static bool lora_segs_ok(const int* seg_end, int nseg, int N) {
  if (!seg_end || nseg < 1 || nseg > 3) return false;
  int prev = 0;
  for (int g = 0; g < nseg; ++g) {
    if (seg_end[g] <= prev || seg_end[g] % 16) return false;
    prev = seg_end[g];
  }
  return prev == N;
}

static bool lora_common_ok(const void* row_slot, const void* part, int slots, int M, int R, int nseg) {
  return row_slot && part && ((uintptr_t)part & 15) == 0 && ((uintptr_t)row_slot & 3) == 0 && slots > 0 && M > 0 &&
         (R == 32 || R == 64) && nseg >= 1 && nseg <= 3;
}

// part [ceil(K / 512), M, nseg * R] f32 <- x [M, K] bf16 (row stride xs elements, K a multiple of 128)
// against the stacked A [slots, nseg * R, K] of the rows' slots.
PENNY_API int penny_lora_shrink(const void* x, long xs, const int* row_slot, const void* A, int slots, int nseg, int R,
                                void* part, int M, int K, hipStream_t stream) {
  if (M == 0) return 0;
  if (!lora_common_ok(row_slot, part, slots, M, R, nseg) || !x || !A || ((uintptr_t)x & 15) || ((uintptr_t)A & 15) ||
      K <= 0 || K % LORA_KW || xs % 8 || xs < K)
    return (int)hipErrorInvalidValue;
  const dim3 grid((M + 15) / 16, (K + LORA_KB - 1) / LORA_KB);
  if (grid.y > 65535) return (int)hipErrorInvalidValue;
#define LORA_SHRINK(NCT)                                                                                     \
  hipLaunchKernelGGL(lora_shrink_kernel<NCT>, grid, dim3(LORA_THREADS), 0, stream, (const bf16*)x, xs, row_slot, \
                     (const bf16*)A, slots, (float*)part, M, K)
  switch (nseg * R / 16) {
    case 2: LORA_SHRINK(2); break;
    case 4: LORA_SHRINK(4); break;
    case 6: LORA_SHRINK(6); break;
    case 8: LORA_SHRINK(8); break;
    case 12: LORA_SHRINK(12); break;
    default: return (int)hipErrorInvalidValue;
  }
#undef LORA_SHRINK
  PENNY_RETURN_LAUNCH();
}

// out [M, N] (bf16, or f32 with out_f32; row stride os elements) += scale * t . B^T per row, t from the
// shrink's S partial slabs; B [slots, N, R] bf16, present [slots] int32 (bit g: segment g targeted),
// scale [slots] f32, seg_end [nseg] host ints (multiples of 16, increasing, the last = N).
PENNY_API int penny_lora_expand(const void* part, int S, const int* row_slot, const void* B, const int* present,
                                const float* scale, int slots, const int* seg_end, int nseg, int R, void* out,
                                int out_f32, long os, int M, int N, hipStream_t stream) {
  if (M == 0) return 0;
  if (!lora_common_ok(row_slot, part, slots, M, R, nseg) || !B || !present || !scale || !out || ((uintptr_t)B & 15) ||
      ((uintptr_t)out & 15) || ((uintptr_t)present & 3) || ((uintptr_t)scale & 3) || S < 1 || N <= 0 || N % 16 ||
      os % 8 || os < N || !lora_segs_ok(seg_end, nseg, N))
    return (int)hipErrorInvalidValue;
  LoraSegs segs;
  segs.n = nseg;
  for (int g = 0; g < 3; ++g) segs.end[g] = g < nseg ? seg_end[g] : N;
  // column tiles per wave: a speed choice only (every output element is computed the same way)
  const int cpw = M <= 256 ? 4 : 16;
  const dim3 grid((M + 15) / 16, (N / 16 + 4 * cpw - 1) / (4 * cpw));
  if (grid.y > 65535) return (int)hipErrorInvalidValue;
#define LORA_EXPAND(T, KS)                                                                                      \
  hipLaunchKernelGGL((lora_expand_kernel<T, KS>), grid, dim3(LORA_THREADS), 0, stream, (const float*)part, S, row_slot, \
                     (const bf16*)B, present, scale, slots, segs, (T*)out, os, M, N, cpw)
  if (out_f32) {
    if (R == 32) LORA_EXPAND(float, 1); else LORA_EXPAND(float, 2);
  } else {
    if (R == 32) LORA_EXPAND(bf16, 1); else LORA_EXPAND(bf16, 2);
  }
#undef LORA_EXPAND
  PENNY_RETURN_LAUNCH();
}
