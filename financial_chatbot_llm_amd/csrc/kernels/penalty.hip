// Repetition / presence / frequency penalties (ops/penalty.py): a per-sequence token-count table on
// the device and the kernel that applies the penalties to a step's logits before the sampler.
//
// Table: [slots, Vs] int16, Vs = V rounded up to 8 (16-byte rows).  Bit 15 of an entry: the token
// occurs in the slot's prompt; bits 0-14: how often the slot's sequence has emitted it (<= 32767).
// Two entries share a 32-bit word, so both writers use 32-bit atomics on the containing word:
// duplicates within one call all land, and the neighbour's half-word never moves.
//
// Per logit l of a row with slot >= 0 (f32, not contracted, in this order):
//   c    = count (+ 1 where the token is the row's pending token: its previous token, still on the
//          device and not yet in the table)
//   seen = c > 0 || prompt bit
//   q    = (seen && rep != 1) ? (l > 0 ? l / rep : l * rep) : l
//   pen  = fma(freq, float(c), c > 0 ? pres : 0)
//   l'   = q - pen, rounded once to the logits' dtype
// A row with rep = 1, pres = 0, freq = 0 (and every row with slot < 0) keeps its bits.
#include "common.h"

static constexpr int PEN_THREADS = 256;

// grid (ceil(Vs / 8 / 256)): one 16-B store of 8 entries per lane
__global__ void __launch_bounds__(PEN_THREADS) pen_zero_kernel(uint4* __restrict__ row, int groups) {
  const int g = blockIdx.x * PEN_THREADS + threadIdx.x;
  if (g < groups) row[g] = make_uint4(0u, 0u, 0u, 0u);
}

// grid (ceil(n / 256)): the prompt bit of ids[i]; ids outside [0, V) set nothing
__global__ void __launch_bounds__(PEN_THREADS) pen_prompt_kernel(uint32_t* __restrict__ row_words,
                                                                 const int* __restrict__ ids, int n, int V) {
  const int i = blockIdx.x * PEN_THREADS + threadIdx.x;
  if (i >= n) return;
  const int v = ids[i];
  PENNY_DASSERT(v >= 0 && v < V);
  if (v < 0 || v >= V) return;
  atomicOr(row_words + (v >> 1), 0x8000u << (16 * (v & 1)));
}

// grid (ceil(n / 256)): count[slot, token] += 1 per pair; a pair outside the table adds nothing
__global__ void __launch_bounds__(PEN_THREADS) pen_add_kernel(uint32_t* __restrict__ words,
                                                              const int* __restrict__ pairs, int n, int slots,
                                                              int V, int Vs) {
  const int i = blockIdx.x * PEN_THREADS + threadIdx.x;
  if (i >= n) return;
  const int s = pairs[2 * i], v = pairs[2 * i + 1];
  PENNY_DASSERT(s >= 0 && s < slots && v >= 0 && v < V);
  if (s < 0 || s >= slots || v < 0 || v >= V) return;
  atomicAdd(words + (((size_t)s * Vs + v) >> 1), 1u << (16 * (v & 1)));
}

__device__ __forceinline__ float pen_one(float l, int e, int v, int pend, float rep, float pres, float freq) {
#pragma clang fp contract(off)
  const int c = (e & 0x7FFF) + (v == pend ? 1 : 0);
  const bool seen = c > 0 || (e & 0x8000);
  const float q = (seen && rep != 1.f) ? (l > 0.f ? l / rep : l * rep) : l;
  const float pen = __builtin_fmaf(freq, (float)c, c > 0 ? pres : 0.f);
  return q - pen;
}

union PenCounts {
  uint4 u;
  unsigned short e[8];
};

// grid (ceil(V / 8 / 256), S): lane g of row r owns logits [8 g, 8 g + 8).  T = bf16: one 16-B load
// of 8 logits; T = float: two.  Rows start on 16 B (row_stride % 8 == 0); a V that is no multiple of
// 8 ends in a scalar group.  out (same row stride) may be null: in place.
template <typename T>
__global__ void __launch_bounds__(PEN_THREADS) pen_apply_kernel(T* __restrict__ logits, long row_stride,
                                                                const int* __restrict__ slot,
                                                                const int* __restrict__ pending_tok,
                                                                const float* __restrict__ rep_,
                                                                const float* __restrict__ pres_,
                                                                const float* __restrict__ freq_,
                                                                const unsigned short* __restrict__ table,
                                                                T* __restrict__ out, int V, int Vs, int slots) {
  const int r = blockIdx.y;
  const int v0 = (blockIdx.x * PEN_THREADS + threadIdx.x) * 8;
  if (v0 >= V) return;
  const int s = slot[r];
  const T* src = logits + (size_t)r * row_stride + v0;
  T* dst = (out ? out : logits) + (size_t)r * row_stride + v0;
  const bool full = v0 + 8 <= V;
  const float rep = rep_[r], pres = pres_[r], freq = freq_[r];
  PENNY_DASSERT(s < slots);
  const bool neutral = s < 0 || s >= slots || (rep == 1.f && pres == 0.f && freq == 0.f);
  if (neutral) {                                          // block-uniform: the bits pass through
    if (!out) return;
    if (full) {
      const uint4* a = reinterpret_cast<const uint4*>(src);
      uint4* b = reinterpret_cast<uint4*>(dst);
      b[0] = a[0];
      if (sizeof(T) == 4) b[1] = a[1];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (v0 + j < V) dst[j] = src[j];
    }
    return;
  }
  const int pend = pending_tok[r];
  PenCounts c;
  c.u = *reinterpret_cast<const uint4*>(table + (size_t)s * Vs + v0);   // v0 + 8 <= Vs always
  float f[8];
  if (!full) {
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = v0 + j < V ? (float)src[j] : 0.f;
  } else if (sizeof(T) == 2) {
    unpack8(*reinterpret_cast<const uint4*>(src), f);
  } else {
    const f32x4 a = *reinterpret_cast<const f32x4*>(src), b = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      f[j] = a[j];
      f[4 + j] = b[j];
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) f[j] = pen_one(f[j], c.e[j], v0 + j, pend, rep, pres, freq);
  if (!full) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (v0 + j < V) dst[j] = (T)f[j];
  } else if (sizeof(T) == 2) {
    *reinterpret_cast<uint4*>(dst) = pack8(f);
  } else {
    f32x4 a, b;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      a[j] = f[j];
      b[j] = f[4 + j];
    }
    *reinterpret_cast<f32x4*>(dst) = a;
    *reinterpret_cast<f32x4*>(dst + 4) = b;
  }
}

static bool pen_table_ok(const void* table, int slots, int V, int Vs) {
  return table && ((uintptr_t)table & 15) == 0 && slots > 0 && V > 0 && Vs % 8 == 0 && Vs >= V && Vs - V < 8;
}

// Zero slot's row, then set the prompt bit of ids[0 .. n) (device int32; duplicates fine).
PENNY_API int penny_pen_reset(void* table, int slots, int V, int Vs, int slot, const int* prompt_ids, int n,
                              hipStream_t stream) {
  if (!pen_table_ok(table, slots, V, Vs) || slot < 0 || slot >= slots || n < 0 || (n > 0 && !prompt_ids))
    return (int)hipErrorInvalidValue;
  unsigned short* row = (unsigned short*)table + (size_t)slot * Vs;
  const int groups = Vs / 8;
  hipLaunchKernelGGL(pen_zero_kernel, dim3((groups + PEN_THREADS - 1) / PEN_THREADS), dim3(PEN_THREADS), 0, stream,
                     (uint4*)row, groups);
  if (n > 0)
    hipLaunchKernelGGL(pen_prompt_kernel, dim3((n + PEN_THREADS - 1) / PEN_THREADS), dim3(PEN_THREADS), 0, stream,
                       (uint32_t*)row, prompt_ids, n, V);
  PENNY_RETURN_LAUNCH();
}

// count[slot, token] += 1 for each of the n (slot, token) int32 pairs on the device.
PENNY_API int penny_pen_add(void* table, int slots, int V, int Vs, const int* pairs, int n, hipStream_t stream) {
  if (n == 0) return 0;
  if (!pen_table_ok(table, slots, V, Vs) || n < 0 || !pairs) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(pen_add_kernel, dim3((n + PEN_THREADS - 1) / PEN_THREADS), dim3(PEN_THREADS), 0, stream,
                     (uint32_t*)table, pairs, n, slots, V, Vs);
  PENNY_RETURN_LAUNCH();
}

// logits [S, V] (row_stride elements, a multiple of 8; base on 16 B) -> penalised, in place or into out
// (same stride).  slot[r] < 0: the row is untouched (copied when out is given).  The slots of one
// call's rows are distinct from each other (not checked: equal slots only read the same counts).
PENNY_API int penny_pen_apply(void* logits, int is_f32, long row_stride, const int* slot, const int* pending_tok,
                              const float* rep, const float* pres, const float* freq, const void* table, int slots,
                              int Vs, void* out, int S, int V, hipStream_t stream) {
  if (S == 0) return 0;
  if (!pen_table_ok(table, slots, V, Vs) || !logits || !slot || !pending_tok || !rep || !pres || !freq || S < 0 ||
      S > 65535 || row_stride % 8 != 0 || row_stride < V || ((uintptr_t)logits & 15) || ((uintptr_t)out & 15))
    return (int)hipErrorInvalidValue;
  const dim3 grid(((V + 7) / 8 + PEN_THREADS - 1) / PEN_THREADS, S);
  if (is_f32)
    hipLaunchKernelGGL(pen_apply_kernel<float>, grid, dim3(PEN_THREADS), 0, stream, (float*)logits, row_stride, slot,
                       pending_tok, rep, pres, freq, (const unsigned short*)table, (float*)out, V, Vs, slots);
  else
    hipLaunchKernelGGL(pen_apply_kernel<bf16>, grid, dim3(PEN_THREADS), 0, stream, (bf16*)logits, row_stride, slot,
                       pending_tok, rep, pres, freq, (const unsigned short*)table, (bf16*)out, V, Vs, slots);
  PENNY_RETURN_LAUNCH();
}
