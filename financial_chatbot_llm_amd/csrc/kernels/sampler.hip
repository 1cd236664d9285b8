// K12: fused temperature + Gumbel-max sampler / greedy argmax over the full vocabulary.
//
// argmax_i(logit_i / T + Gumbel_i) is an exact sample from softmax(logit / T), so one read of
// the logits row replaces softmax + cumsum + search.  Noise is counter-based (splitmix64 of
// (per-row seed, token index)): a request's sample depends only on its own seed and the step,
// never on batch composition or launch order.  T <= 0 selects greedy argmax.  Ties resolve to
// the smallest index.  One 1024-thread workgroup per row; the vocab (128256 for Llama-3) is
// read 16 B per lane.
//
// top-k / top-p (nucleus) without a sort: a per-row radix select finds a logit THRESHOLD and the
// sampler treats every logit below it as -inf.  top-k: 4 passes of an 8-bit-digit histogram over
// order-preserving uint32 keys find the k-th largest logit exactly.  top-p (over the
// temperature-scaled distribution renormalised to the top-k survivors, as vLLM/HF apply them):
// the same 4 passes histogram probability MASS instead of counts and descend to the smallest
// logit whose cumulative mass from the top reaches p.  Everything stays on the device (no host
// sync, no sort buffers), so the filter is captured in the decode hipGraphs; rows with k <= 0 and
// p >= 1 leave after reading their two parameters.
#include "common.h"

template <typename T>
__device__ __forceinline__ void load8(const T* p, float* f);
template <>
__device__ __forceinline__ void load8<bf16>(const bf16* p, float* f) {
  unpack8(*reinterpret_cast<const uint4*>(p), f);
}
template <>
__device__ __forceinline__ void load8<float>(const float* p, float* f) {
  const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}

__device__ __forceinline__ uint32_t fkey(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float keyf(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

template <typename T>
__device__ __forceinline__ float ld1(const T* p) { return (float)*p; }

// 256 bins (bins[0..255], ascending digit) -> the digit whose bin holds the `target`-th unit of
// weight counting from the TOP, and the weight above it.  One wave: lane l owns bins 4l..4l+3.
__device__ __forceinline__ void find_from_top(const float* bins, float target, int& digit, float& above) {
  const int lane = threadIdx.x & 63;
  const float b0 = bins[4 * lane], b1 = bins[4 * lane + 1], b2 = bins[4 * lane + 2], b3 = bins[4 * lane + 3];
  const float seg = b0 + b1 + b2 + b3;
  float suf = seg;                                   // inclusive suffix sum over lanes >= l
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float v = __shfl_down(suf, o, 64);
    if (lane + o < 64) suf += v;
  }
  const float total = __shfl(suf, 0, 64);
  target = fminf(fmaxf(target, 0.f), total);         // rounding guard (mass sums)
  const float abv = suf - seg;
  // crossing lane: abv < target <= abv + seg (the highest such lane when target <= 0)
  const bool hit = seg > 0.f && abv < target && target <= suf;
  unsigned long long m = __ballot(hit);
  if (m == 0) m = __ballot(seg > 0.f);               // target == 0 or rounding: highest nonzero
  const int src = m ? 63 - __clzll(m) : 0;
  float a = __shfl(abv, src, 64);
  const float c3 = __shfl(b3, src, 64), c2 = __shfl(b2, src, 64), c1 = __shfl(b1, src, 64);
  int d = 4 * src;
  if (a + c3 >= target && c3 > 0.f) d += 3;
  else if ((a += c3, a + c2 >= target) && c2 > 0.f) d += 2;
  else if ((a += c2, a + c1 >= target) && c1 > 0.f) d += 1;
  else a += c1;
  digit = d;
  above = a;
}

// Token-automaton constraint (constrain.hip builds the tables): a row in automaton state st >= 0 may
// only pick tokens whose bit is set in masks[st, :] (W 32-bit words per state, token i = bit i & 31
// of word i >> 5); every other token counts as -inf.  st < 0: the row is unconstrained.  A state
// outside the table admits nothing (the row then emits eot).
struct FsmMask {
  const int* state;            // [B]
  const uint32_t* masks;       // [S, W]
  int W, S;
};
__device__ __forceinline__ const uint32_t* fsm_row(const FsmMask& fm, int row, bool& con, bool& none) {
  const int st = fm.state[row];
  con = st >= 0;
  none = st >= fm.S;
  PENNY_DASSERT(st < fm.S);
  return fm.masks + (size_t)(con && !none ? st : 0) * fm.W;
}
__device__ __forceinline__ bool fsm_bit(const uint32_t* mrow, int i) { return (mrow[i >> 5] >> (i & 31)) & 1u; }

// One 1024-thread workgroup per row -> thresh[row] (a logit; -inf = keep everything).  MASKED: the
// constraint applies BEFORE top-k / top-p -- disallowed tokens are neither counted nor weighed.
template <typename T, bool MASKED>
__global__ void __launch_bounds__(1024) topk_topp_threshold_kernel(const T* __restrict__ logits, long row_stride,
                                                                   const float* __restrict__ temps,
                                                                   const int* __restrict__ topk,
                                                                   const float* __restrict__ topp,
                                                                   float* __restrict__ thresh, int V, FsmMask fm) {
  // per-wave digit histograms in INTEGERS: counts for top-k, probability mass in 2^-44 fixed point
  // for top-p -- integer adds commute, so the threshold is bitwise independent of the order in
  // which waves and lanes reach the atomics (float atomics made the nucleus edge run-dependent)
  __shared__ unsigned long long hist[16][256];
  __shared__ float red[16];
  __shared__ float bins[256];
  __shared__ uint32_t s_prefix;
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int k = topk[row];
  const float p = topp[row], temp = temps[row];
  const bool do_k = k > 0 && k < V, do_p = p < 1.f;
  if (!(temp > 0.f) || (!do_k && !do_p)) {
    if (tid == 0) thresh[row] = -INFINITY;
    return;
  }
  const T* lr = logits + row * row_stride;
  const float inv_t = 1.f / temp;
  bool con = false, none = false;
  const uint32_t* mrow = nullptr;
  if (MASKED) mrow = fsm_row(fm, row, con, none);
  if (MASKED && none) {                // nothing admitted: the sampler emits eot whatever the cut
    if (tid == 0) thresh[row] = -INFINITY;
    return;
  }
  uint32_t prefix = 0, pmask = 0;      // selected high digits so far (keys matching are candidates)
  // ---- top-k: radix select of the k-th largest key ---------------------------------------------
  if (do_k) {
    float want = (float)k;
    for (int shift = 24; shift >= 0; shift -= 8) {
      for (int i = tid; i < 16 * 256; i += 1024) (&hist[0][0])[i] = 0ull;
      __syncthreads();
      for (int i = tid; i < V; i += 1024) {
        if (MASKED && con && !fsm_bit(mrow, i)) continue;
        const uint32_t key = fkey(ld1(lr + i));
        if ((key & pmask) == prefix) atomicAdd(&hist[wid][(key >> shift) & 255], 1ull);
      }
      __syncthreads();
      if (tid < 256) {
        unsigned long long t = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) t += hist[w][tid];
        bins[tid] = (float)t;
      }
      __syncthreads();
      if (wid == 0) {
        int d;
        float above;
        find_from_top(bins, want, d, above);
        if (lane == 0) {
          s_prefix = prefix | ((uint32_t)d << shift);
          red[0] = want - above;
        }
      }
      __syncthreads();
      prefix = s_prefix;
      want = red[0];
      pmask |= 255u << shift;
      __syncthreads();
    }
  }
  const uint32_t kfloor = do_k ? prefix : 0u;        // keys >= kfloor survive top-k
  if (!do_p) {
    if (tid == 0) thresh[row] = keyf(kfloor);
    return;
  }
  // ---- top-p over the renormalised top-k survivors --------------------------------------------
  float mx = -INFINITY;
  for (int i = tid; i < V; i += 1024) {
    if (MASKED && con && !fsm_bit(mrow, i)) continue;
    mx = fmaxf(mx, ld1(lr + i));
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  if (lane == 0) red[wid] = mx;
  __syncthreads();
  mx = red[0];
#pragma unroll
  for (int w = 1; w < 16; ++w) mx = fmaxf(mx, red[w]);
  __syncthreads();
  prefix = 0;
  pmask = 0;
  float want = -1.f;                                  // set from the first pass's total
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int i = tid; i < 16 * 256; i += 1024) (&hist[0][0])[i] = 0ull;
    __syncthreads();
    for (int i = tid; i < V; i += 1024) {
      if (MASKED && con && !fsm_bit(mrow, i)) continue;
      const float l = ld1(lr + i);
      const uint32_t key = fkey(l);
      // exp <= 1 (l <= mx): x 2^44 fits 45 bits, a 128k-entry vocabulary sums below 2^62
      if (key >= kfloor && (key & pmask) == prefix)
        atomicAdd(&hist[wid][(key >> shift) & 255],
                  (unsigned long long)(__expf((l - mx) * inv_t) * 17592186044416.f));
    }
    __syncthreads();
    if (tid < 256) {
      unsigned long long t = 0;
#pragma unroll
      for (int w = 0; w < 16; ++w) t += hist[w][tid];
      bins[tid] = (float)t * 5.684341886080802e-14f;   // 2^-44
    }
    __syncthreads();
    if (wid == 0) {
      if (want < 0.f) {                                // first pass: total mass of the survivors
        float z = bins[4 * lane] + bins[4 * lane + 1] + bins[4 * lane + 2] + bins[4 * lane + 3];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) z += __shfl_xor(z, o, 64);
        want = p * z;
      }
      int d;
      float above;
      find_from_top(bins, want, d, above);
      if (lane == 0) {
        s_prefix = prefix | ((uint32_t)d << shift);
        red[0] = want - above;
      }
    }
    __syncthreads();
    prefix = s_prefix;
    want = red[0];
    pmask |= 255u << shift;
    __syncthreads();
  }
  if (tid == 0) thresh[row] = keyf(max(prefix, kfloor));
}

// Pass 1: grid (B, SPLITS); each 256-thread workgroup scans one vocab slice of one row and writes
// its (best value, index).  Pass 2: one wave per row merges the SPLITS candidates.  Splitting the
// row keeps the whole chip busy at decode batch sizes (B = 64 rows alone would occupy 64 CUs,
// and the per-element noise generation makes this pass VALU-, not bandwidth-, bound).
#define SAMPLE_SPLITS 16

// MASKED: each 8-logit chunk reads one byte of the row's state mask.
template <typename T, bool MASKED>
__global__ void __launch_bounds__(256) sample_partial_kernel(const T* __restrict__ logits, long row_stride,
                                                             const float* __restrict__ temps,
                                                             const unsigned long long* __restrict__ seeds,
                                                             const float* __restrict__ thresh,
                                                             float* __restrict__ pv, int* __restrict__ pi, int V,
                                                             int voff, FsmMask fm) {
  __shared__ float sv[4];
  __shared__ int si[4];
  const int row = blockIdx.x, split = blockIdx.y;
  const T* lr = logits + row * row_stride;
  const float temp = temps[row];
  const bool greedy = !(temp > 0.f);
  const float inv_t = greedy ? 1.f : 1.f / temp;
  const unsigned long long seed = seeds[row];
  const float floor_l = (thresh != nullptr && !greedy) ? thresh[row] : -INFINITY;   // top-k/top-p cut
  bool con = false, none = false;
  const uint32_t* mrow = nullptr;
  if (MASKED) mrow = fsm_row(fm, row, con, none);
  const uint8_t* mbytes = reinterpret_cast<const uint8_t*>(mrow);
  const int nch = V >> 3;
  const int per = (nch + SAMPLE_SPLITS - 1) / SAMPLE_SPLITS;
  const int c0 = split * per, c1 = min(nch, c0 + per);
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  for (int c = c0 + threadIdx.x; c < c1; c += blockDim.x) {
    uint32_t mb = 0xffu;
    if (MASKED && con) {
      mb = none ? 0u : mbytes[c];
      if (mb == 0u) continue;
    }
    float f[8];
    load8<T>(lr + c * 8, f);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int idx = voff + c * 8 + k;     // global token id (vocab shard offset)
      float v = f[k];
      if (MASKED && !((mb >> k) & 1u)) continue;
      if (v < floor_l) continue;
      if (!greedy) {
        v = v * inv_t + gumbel_noise(seed, idx);
      }
      better(bv, bi, v, idx);
    }
  }
  if (split == SAMPLE_SPLITS - 1) {  // tail (V not a multiple of 8)
    for (int loc = (V & ~7) + threadIdx.x; loc < V; loc += blockDim.x) {
      const int idx = voff + loc;
      if (MASKED && con && (none || !fsm_bit(mrow, loc))) continue;
      float v = (float)lr[loc];
      if (v < floor_l) continue;
      if (!greedy) {
        v = v * inv_t + gumbel_noise(seed, idx);
      }
      better(bv, bi, v, idx);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    better(bv, bi, ov, oi);
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0) {
    sv[wid] = bv;
    si[wid] = bi;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) better(bv, bi, sv[w], si[w]);
    pv[row * SAMPLE_SPLITS + split] = bv;
    pi[row * SAMPLE_SPLITS + split] = bi;
  }
}

__global__ void sample_final_kernel(const float* __restrict__ pv, const int* __restrict__ pi, int* __restrict__ out,
                                    int* __restrict__ pairs) {
  const int row = blockIdx.x, lane = threadIdx.x;
  float bv = lane < SAMPLE_SPLITS ? pv[row * SAMPLE_SPLITS + lane] : -INFINITY;
  int bi = lane < SAMPLE_SPLITS ? pi[row * SAMPLE_SPLITS + lane] : 0x7fffffff;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    better(bv, bi, ov, oi);
  }
  if (lane == 0) {
    if (out) out[row] = bi;
    if (pairs) {
      pairs[2 * row] = __float_as_int(bv);
      pairs[2 * row + 1] = bi;
    }
  }
}

// workspace: B * SAMPLE_SPLITS floats + B * SAMPLE_SPLITS ints + B floats (thresholds)
// top_k / top_p: per-row filters (nullptr: none in this launch)
PENNY_API int penny_sample(const void* logits, int is_fp32, long row_stride, const float* temps,
                           const unsigned long long* seeds, const int* top_k, const float* top_p, int* out,
                           void* workspace, int B, int V, hipStream_t stream) {
  if (B <= 0) return 0;
  float* pv = (float*)workspace;
  int* pi = (int*)(pv + (long)B * SAMPLE_SPLITS);
  float* th = nullptr;
  if (top_k != nullptr && top_p != nullptr) {
    th = (float*)(pi + (long)B * SAMPLE_SPLITS);
    if (is_fp32) {
      hipLaunchKernelGGL((topk_topp_threshold_kernel<float, false>), dim3(B), dim3(1024), 0, stream, (const float*)logits,
                         row_stride, temps, top_k, top_p, th, V, FsmMask{});
    } else {
      hipLaunchKernelGGL((topk_topp_threshold_kernel<bf16, false>), dim3(B), dim3(1024), 0, stream, (const bf16*)logits,
                         row_stride, temps, top_k, top_p, th, V, FsmMask{});
    }
  }
  dim3 grid(B, SAMPLE_SPLITS);
  if (is_fp32) {
    hipLaunchKernelGGL((sample_partial_kernel<float, false>), grid, dim3(256), 0, stream, (const float*)logits, row_stride,
                       temps, seeds, th, pv, pi, V, 0, FsmMask{});
  } else {
    hipLaunchKernelGGL((sample_partial_kernel<bf16, false>), grid, dim3(256), 0, stream, (const bf16*)logits, row_stride,
                       temps, seeds, th, pv, pi, V, 0, FsmMask{});
  }
  hipLaunchKernelGGL(sample_final_kernel, dim3(B), dim3(64), 0, stream, pv, pi, out, (int*)nullptr);
  PENNY_RETURN_LAUNCH();
}

// Vocabulary-parallel sampling of one TP rank's logit shard [B, V] (global ids voff .. voff+V-1):
// pairs [B, 2] int32 = each row's best (score bits, global token id); the ranks' pairs are then
// all-gathered and the best taken (ops.sampling.pick_pairs) -- [B, 2] on the wire instead of the
// [B, V*tp] logits.  No top-k / top-p (they need the whole distribution).
// workspace: B * SAMPLE_SPLITS floats + as many ints.
PENNY_API int penny_sample_shard(const void* logits, int is_fp32, long row_stride, const float* temps,
                                 const unsigned long long* seeds, int* pairs, void* workspace, int B, int V, int voff,
                                 hipStream_t stream) {
  if (B <= 0) return 0;
  if (!pairs || !workspace || V <= 0 || voff < 0) return (int)hipErrorInvalidValue;
  float* pv = (float*)workspace;
  int* pi = (int*)(pv + (long)B * SAMPLE_SPLITS);
  dim3 grid(B, SAMPLE_SPLITS);
  if (is_fp32) {
    hipLaunchKernelGGL((sample_partial_kernel<float, false>), grid, dim3(256), 0, stream, (const float*)logits, row_stride,
                       temps, seeds, (const float*)nullptr, pv, pi, V, voff, FsmMask{});
  } else {
    hipLaunchKernelGGL((sample_partial_kernel<bf16, false>), grid, dim3(256), 0, stream, (const bf16*)logits, row_stride,
                       temps, seeds, (const float*)nullptr, pv, pi, V, voff, FsmMask{});
  }
  hipLaunchKernelGGL(sample_final_kernel, dim3(B), dim3(64), 0, stream, pv, pi, (int*)nullptr, pairs);
  PENNY_RETURN_LAUNCH();
}

// Constrained sampling: the merge of a row's candidates, then one lane advances the row's automaton
// state over the chosen token's bytes (eot -> the automaton's done state).  A constrained row left
// without a candidate (its mask admits nothing) emits eot and goes to done; unconstrained rows
// (state < 0) write state_out = -1.  state_out may alias state.
struct FsmWalk {
  const unsigned short* byte_next;   // [S, 256], 0xFFFF = dead
  const int* tok_off;                // [nt + 1]
  const unsigned char* tok_bytes;
  const int* done_of;                // [S] the done state of the automaton each state belongs to
  int nt, eot;
};

__global__ void sample_final_fsm_kernel(const float* __restrict__ pv, const int* __restrict__ pi,
                                        int* __restrict__ out, const int* state, int* state_out, int S,
                                        FsmWalk fw) {
  const int row = blockIdx.x, lane = threadIdx.x;
  float bv = lane < SAMPLE_SPLITS ? pv[row * SAMPLE_SPLITS + lane] : -INFINITY;
  int bi = lane < SAMPLE_SPLITS ? pi[row * SAMPLE_SPLITS + lane] : 0x7fffffff;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    better(bv, bi, ov, oi);
  }
  if (lane != 0) return;
  const int st = state[row];
  if (st < 0) {
    out[row] = bi;
    state_out[row] = -1;
    return;
  }
  if (st >= S) {                      // not a state of the table: nothing admitted, nothing to walk
    out[row] = fw.eot;
    state_out[row] = st;
    return;
  }
  int tok = bi, ns = fw.done_of[st];
  if (bi == 0x7fffffff) tok = fw.eot;
  if (tok != fw.eot && tok >= 0 && tok < fw.nt) {
    int cur = st;
    for (int j = fw.tok_off[tok], e = fw.tok_off[tok + 1]; j < e; ++j) {
      cur = fw.byte_next[(size_t)cur * 256 + fw.tok_bytes[j]];
      if (cur >= S) break;            // dead (0xFFFF): an admitted token never dies
    }
    PENNY_DASSERT(cur < S);
    if (cur < S) ns = cur;
  }
  out[row] = tok;
  state_out[row] = ns;
}

// penny_sample with a token-automaton constraint per row (state[B], < 0: none).  Same noise, tie
// rule and top-k / top-p as penny_sample; the mask applies before the top-k / top-p threshold.
// workspace: as penny_sample.
PENNY_API int penny_sample_fsm(const void* logits, int is_fp32, long row_stride, const float* temps,
                               const unsigned long long* seeds, const int* top_k, const float* top_p, int* out,
                               void* workspace, int B, int V, const int* state, int* state_out,
                               const unsigned int* masks, int W, int S, const unsigned short* byte_next,
                               const int* tok_off, const unsigned char* tok_bytes, int nt, const int* done_of,
                               int eot, hipStream_t stream) {
  if (B <= 0) return 0;
  if (!state || !state_out || !masks || !byte_next || !tok_off || !tok_bytes || !done_of || S <= 0 || nt <= 0 ||
      eot < 0 || (long)W * 32 < V)
    return (int)hipErrorInvalidValue;
  float* pv = (float*)workspace;
  int* pi = (int*)(pv + (long)B * SAMPLE_SPLITS);
  const FsmMask fm{state, masks, W, S};
  float* th = nullptr;
  if (top_k != nullptr && top_p != nullptr) {
    th = (float*)(pi + (long)B * SAMPLE_SPLITS);
    if (is_fp32) {
      hipLaunchKernelGGL((topk_topp_threshold_kernel<float, true>), dim3(B), dim3(1024), 0, stream,
                         (const float*)logits, row_stride, temps, top_k, top_p, th, V, fm);
    } else {
      hipLaunchKernelGGL((topk_topp_threshold_kernel<bf16, true>), dim3(B), dim3(1024), 0, stream,
                         (const bf16*)logits, row_stride, temps, top_k, top_p, th, V, fm);
    }
  }
  dim3 grid(B, SAMPLE_SPLITS);
  if (is_fp32) {
    hipLaunchKernelGGL((sample_partial_kernel<float, true>), grid, dim3(256), 0, stream, (const float*)logits,
                       row_stride, temps, seeds, th, pv, pi, V, 0, fm);
  } else {
    hipLaunchKernelGGL((sample_partial_kernel<bf16, true>), grid, dim3(256), 0, stream, (const bf16*)logits,
                       row_stride, temps, seeds, th, pv, pi, V, 0, fm);
  }
  const FsmWalk fw{byte_next, tok_off, tok_bytes, done_of, nt, eot};
  hipLaunchKernelGGL(sample_final_fsm_kernel, dim3(B), dim3(64), 0, stream, pv, pi, out, state, state_out, S, fw);
  PENNY_RETURN_LAUNCH();
}

// Threshold only (tests / diagnostics): thresh[B] logits.
PENNY_API int penny_topk_topp_threshold(const void* logits, int is_fp32, long row_stride, const float* temps,
                                        const int* top_k, const float* top_p, float* thresh, int B, int V,
                                        hipStream_t stream) {
  if (B <= 0) return 0;
  if (is_fp32) {
    hipLaunchKernelGGL((topk_topp_threshold_kernel<float, false>), dim3(B), dim3(1024), 0, stream, (const float*)logits,
                       row_stride, temps, top_k, top_p, thresh, V, FsmMask{});
  } else {
    hipLaunchKernelGGL((topk_topp_threshold_kernel<bf16, false>), dim3(B), dim3(1024), 0, stream, (const bf16*)logits,
                       row_stride, temps, top_k, top_p, thresh, V, FsmMask{});
  }
  PENNY_RETURN_LAUNCH();
}

// Log-probability of one chosen token per row of logits the step already holds (top-k / top-p rows,
// constrained rows, the unfused LM head): logprob[row] = log softmax(l)[ids[row]] over the raw
// logits at temperature 1 -- what the fused LM heads' log-probability forms report.  One pass: every
// thread keeps an online (max, sum of exp(l - max)) over its 8-logit chunks, merged across the
// 1024-thread workgroup; then the gather.  -inf logits add nothing, a NaN logit makes the row NaN,
// and an id outside [0, V) reports NaN without a read.
__device__ __forceinline__ float lse_scale(float from, float to) { return from == to ? 1.f : __expf(from - to); }
__device__ __forceinline__ void lse_merge(float& m, float& s, float om, float os) {
  const float nm = fmaxf(m, om);
  s = s * lse_scale(m, nm) + os * lse_scale(om, nm);
  m = nm;
}

// The row's (max, sum exp): lse_thread leaves each thread's own pair over its chunks, lse_waves the 16
// per-wave partials in sm / ss (thread 0 keeps wave 0's in m, s), lse_finish merges them on thread 0:
// one code path, one order, for every kernel that reports a log-probability off a logits row -- their
// values for the same row and id are bit-equal.
template <typename T>
__device__ __forceinline__ void lse_thread(const T* __restrict__ lr, int V, float& m, float& s) {
  const int tid = threadIdx.x;
  m = -INFINITY;
  s = 0.f;
  const int nch = V >> 3;
  for (int c = tid; c < nch; c += 1024) {
    float f[8];
    load8<T>(lr + c * 8, f);
    float cm = f[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) cm = fmaxf(cm, f[k]);
    const float nm = fmaxf(m, cm);          // fmaxf drops a NaN: it reaches s through its exp below
    s *= lse_scale(m, nm);
#pragma unroll
    for (int k = 0; k < 8; ++k) s += f[k] == -INFINITY ? 0.f : __expf(f[k] - nm);
    m = nm;
  }
  for (int loc = (V & ~7) + tid; loc < V; loc += 1024) {   // tail (V not a multiple of 8)
    const float l = (float)lr[loc];
    const float nm = fmaxf(m, l);
    s = s * lse_scale(m, nm) + (l == -INFINITY ? 0.f : __expf(l - nm));
    m = nm;
  }
}
__device__ __forceinline__ void lse_waves(float* sm, float* ss, float& m, float& s) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(m, o, 64), os = __shfl_xor(s, o, 64);
    lse_merge(m, s, om, os);
  }
  if (lane == 0) {
    sm[wid] = m;
    ss[wid] = s;
  }
  __syncthreads();
}
__device__ __forceinline__ void lse_finish(float& m, float& s, const float* sm, const float* ss) {
  for (int w = 1; w < 16; ++w) lse_merge(m, s, sm[w], ss[w]);
}
template <typename T>
__device__ __forceinline__ float row_logprob(const T* __restrict__ lr, int id, int V, float m, float s) {
  return id >= 0 && id < V ? (float)lr[id] - m - logf(s) : NAN;
}

template <typename T>
__global__ void __launch_bounds__(1024) token_logprob_kernel(const T* __restrict__ logits, long row_stride,
                                                             const int* __restrict__ ids,
                                                             float* __restrict__ logprob, int V) {
  __shared__ float sm[16], ss[16];
  const int row = blockIdx.x, tid = threadIdx.x;
  const T* lr = logits + row * row_stride;
  float m, s;
  lse_thread<T>(lr, V, m, s);
  lse_waves(sm, ss, m, s);
  if (tid == 0) {
    lse_finish(m, s, sm, ss);
    logprob[row] = row_logprob<T>(lr, ids[row], V, m, s);
  }
}

// logits [B, V] bf16 / f32 with 16-B aligned rows (as penny_sample), ids [B] int32 -> logprob [B] f32.
PENNY_API int penny_token_logprob(const void* logits, int is_fp32, long row_stride, const int* ids, float* logprob,
                                  int B, int V, hipStream_t stream) {
  if (B <= 0) return 0;
  if (!logits || !ids || !logprob || V <= 0) return (int)hipErrorInvalidValue;
  if (is_fp32) {
    hipLaunchKernelGGL(token_logprob_kernel<float>, dim3(B), dim3(1024), 0, stream, (const float*)logits, row_stride,
                       ids, logprob, V);
  } else {
    hipLaunchKernelGGL(token_logprob_kernel<bf16>, dim3(B), dim3(1024), 0, stream, (const bf16*)logits, row_stride,
                       ids, logprob, V);
  }
  PENNY_RETURN_LAUNCH();
}

// Top-N alternatives: per row with n = topn[row] > 0, the chosen token's log-probability (the value
// token_logprob_kernel reports, by the same code) and the n largest logits of the row in descending
// order, equal logits by ascending token id (+0 and -0 are equal), each with its log-probability
// from the same (m, s).  Raw logits at temperature 1: no mask, penalty or filter.  No sort of the
// vocabulary and no workspace: a radix select over order-preserving integer keys finds the n-th
// largest key, how many keys lie strictly above it and how many equal it; one more pass collects
// the keys above and the first members (in index order) of the threshold's plateau -- gathered
// unordered and ranked by index when the plateau fits LDS, by workgroup scans over sweeps in index
// order when it does not; at most TOPN_MAX candidates are then ranked in LDS.  Rows with n <= 0 leave
// after reading their parameter and write nothing.
//
// The select only counts keys at or above a floor: the smallest of the 32 half-wave maxima the
// log-sum-exp pass leaves behind.  32 different elements reach it, so the n-th largest (n <= 20) does
// too, and of a 128k-entry row a few hundred keys do -- without it every element lands an LDS atomic
// on the two or three bins of the first digit (sign + exponent), 64 lanes to one address.
#define TOPN_MAX 20
static_assert(TOPN_MAX <= 32, "the select's floor counts on 32 half-wave maxima");
#define TOPN_EQ_CAP 2048   // plateau members gathered unordered (<= the 16 x 256 histogram words)

__device__ __forceinline__ uint32_t tkey(float f) { return fkey(f == 0.f ? 0.f : f); }   // -0 -> +0

// every (index, element) of the row once, 16 B per lane then the tail (V not a multiple of 8)
template <typename T, typename F>
__device__ __forceinline__ void row_foreach(const T* __restrict__ lr, int V, F&& fn) {
  const int nch = V >> 3;
  for (int c = threadIdx.x; c < nch; c += 1024) {
    float f[8];
    load8<T>(lr + c * 8, f);
#pragma unroll
    for (int k = 0; k < 8; ++k) fn(c * 8 + k, f[k]);
  }
  for (int loc = (V & ~7) + threadIdx.x; loc < V; loc += 1024) fn(loc, (float)lr[loc]);
}

// 256 integer bins (ascending digit) -> the digit whose bin holds the `want`-th key counting from
// the TOP (1 <= want <= the bins' total), the count above that bin and the count in it.  One wave,
// as find_from_top.
__device__ __forceinline__ void find_kth_from_top(const uint32_t* bins, uint32_t want, int& digit, uint32_t& above,
                                                  uint32_t& inbin) {
  const int lane = threadIdx.x & 63;
  const uint32_t b0 = bins[4 * lane], b1 = bins[4 * lane + 1], b2 = bins[4 * lane + 2], b3 = bins[4 * lane + 3];
  const uint32_t seg = b0 + b1 + b2 + b3;
  uint32_t suf = seg;                                // inclusive suffix sum over lanes >= l
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t v = __shfl_down(suf, o, 64);
    if (lane + o < 64) suf += v;
  }
  const uint32_t abv = suf - seg;
  unsigned long long hit = __ballot(abv < want && want <= suf);
  if (hit == 0) hit = __ballot(seg > 0u);            // want beyond the total: the lowest nonzero bin
  const int src = hit ? (int)__ffsll((long long)hit) - 1 : 0;
  uint32_t a = __shfl(abv, src, 64);
  const uint32_t c3 = __shfl(b3, src, 64), c2 = __shfl(b2, src, 64), c1 = __shfl(b1, src, 64);
  uint32_t c = __shfl(b0, src, 64);
  int d = 4 * src;
  if (a + c3 >= want) d += 3, c = c3;
  else if ((a += c3, a + c2 >= want)) d += 2, c = c2;
  else if ((a += c2, a + c1 >= want)) d += 1, c = c1;
  else a += c1;
  digit = d;
  above = a;
  inbin = c;
}

template <typename T>
__global__ void __launch_bounds__(1024) topn_logprob_kernel(const T* __restrict__ logits, long row_stride,
                                                            const int* __restrict__ ids,
                                                            const int* __restrict__ topn, int max_n,
                                                            float* __restrict__ logprob, int* __restrict__ top_ids,
                                                            float* __restrict__ top_lp, int V) {
  __shared__ uint32_t hist[16][256];     // per-wave digit counts
  __shared__ uint32_t bins[256];
  __shared__ float sm[16], ss[16];
  __shared__ float s_ms[2];              // the row's (m, s)
  __shared__ float s_hmax[32];           // half-wave maxima
  __shared__ uint32_t s_prefix, s_want, s_inbin, s_ngt, s_neq;
  __shared__ uint32_t wsum[2][16];
  __shared__ uint32_t ckey[TOPN_MAX];
  __shared__ int cid[TOPN_MAX];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  int n = topn[row];
  if (n <= 0) return;
  n = min(n, max_n);                     // the entry point checked max_n <= min(TOPN_MAX, V)
  const T* lr = logits + row * row_stride;
  float m, s;
  lse_thread<T>(lr, V, m, s);
  float hmax = m;                        // never NaN: fmaxf drops one
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) hmax = fmaxf(hmax, __shfl_xor(hmax, o, 64));
  if ((lane & 31) == 0) s_hmax[tid >> 5] = hmax;
  lse_waves(sm, ss, m, s);               // its barrier publishes s_hmax too
  float lo = s_hmax[0];
#pragma unroll
  for (int i = 1; i < 32; ++i) lo = fminf(lo, s_hmax[i]);
  // a half wave without an element (short rows) holds -inf, no element's value: no floor then
  const uint32_t kfloor = lo == -INFINITY ? 0u : tkey(lo);
  if (tid == 0) {
    lse_finish(m, s, sm, ss);
    logprob[row] = row_logprob<T>(lr, ids[row], V, m, s);
    s_ms[0] = m;
    s_ms[1] = s;
    s_ngt = 0u;
    s_neq = 0u;
  }
  if (tid < TOPN_MAX) {
    ckey[tid] = 0u;
    cid[tid] = 0;
  }
  // ---- radix select: the n-th largest key and the count strictly above it ----------------------
  // bf16 logits widen to keys whose low 16 bits follow from the sign: two digits decide
  constexpr int LAST_SHIFT = sizeof(T) == 2 ? 16 : 0;
  uint32_t prefix = 0, pmask = 0, want = (uint32_t)n;
  for (int shift = 24; shift >= LAST_SHIFT; shift -= 8) {
    for (int i = tid; i < 16 * 256; i += 1024) (&hist[0][0])[i] = 0u;
    __syncthreads();
    row_foreach<T>(lr, V, [&](int, float v) {
      const uint32_t key = tkey(v);
      if (key >= kfloor && (key & pmask) == prefix) atomicAdd(&hist[wid][(key >> shift) & 255], 1u);
    });
    __syncthreads();
    if (tid < 256) {
      uint32_t t = 0;
#pragma unroll
      for (int w = 0; w < 16; ++w) t += hist[w][tid];
      bins[tid] = t;
    }
    __syncthreads();
    if (wid == 0) {
      int d;
      uint32_t above, inbin;
      find_kth_from_top(bins, want, d, above, inbin);
      if (lane == 0) {
        s_prefix = prefix | ((uint32_t)d << shift);
        s_want = want - above;
        s_inbin = inbin;
      }
    }
    __syncthreads();
    prefix = s_prefix;
    want = s_want;
    pmask |= 255u << shift;
  }
  if (LAST_SHIFT == 16 && !(prefix & 0x80000000u)) prefix |= 0xffffu;   // a negative value's key
  // ---- collect: every key above the threshold, and the first `need` of its plateau by index -----
  const uint32_t thr = prefix;
  const uint32_t need = min(max(want, 1u), (uint32_t)n), ngt = (uint32_t)n - need;
  // the last digit's bin holds exactly the plateau: every key equal to the threshold
  const uint32_t neq = s_inbin;
  if (neq <= TOPN_EQ_CAP) {
    // a plateau that fits the (now free) histogram memory: one pass without a barrier gathers its
    // indices in any order, then each is ranked among them and the `need` smallest are taken
    uint32_t* s_eq = &hist[0][0];
    row_foreach<T>(lr, V, [&](int idx, float v) {
      const uint32_t key = tkey(v);
      if (key > thr) {
        const uint32_t slot = atomicAdd(&s_ngt, 1u);
        if (slot < ngt) {
          ckey[slot] = key;
          cid[slot] = idx;
        }
      } else if (key == thr) {
        const uint32_t slot = atomicAdd(&s_neq, 1u);
        if (slot < TOPN_EQ_CAP) s_eq[slot] = (uint32_t)idx;
      }
    });
    __syncthreads();
    const uint32_t got = min(neq, s_neq);       // == neq: the select counted the same keys
    for (uint32_t i = tid; i < got; i += 1024) {
      const uint32_t mine = s_eq[i];
      uint32_t r = 0;
      if (neq > need)
        for (uint32_t j = 0; j < got; ++j) r += s_eq[j] < mine ? 1u : 0u;
      else
        r = i;                           // all of it is taken: the final ranking orders it
      if (r < need) {
        ckey[ngt + r] = thr;
        cid[ngt + r] = (int)mine;
      }
    }
  }
  // a larger plateau: sweeps in index order, a workgroup scan in each giving every member its rank
  const int nch = V >> 3, nsw = neq <= TOPN_EQ_CAP ? -1 : (nch + 1023) >> 10;
  uint32_t base = 0;                     // plateau members in the sweeps before this one
  for (int sw = 0; sw <= nsw; ++sw) {    // sweep nsw is the tail, one element per thread
    float f[8];
    int i0 = 0, nv = 0;
    if (sw < nsw) {
      const int c = sw * 1024 + tid;
      if (c < nch) {
        load8<T>(lr + c * 8, f);
        i0 = c * 8;
        nv = 8;
      }
    } else {
      const int loc = (V & ~7) + tid;
      if (loc < V) {
        f[0] = (float)lr[loc];
        i0 = loc;
        nv = 1;
      }
    }
    uint32_t eq = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (k < nv) {
        const uint32_t key = tkey(f[k]);
        if (key > thr) {
          const uint32_t slot = atomicAdd(&s_ngt, 1u);
          if (slot < ngt) {
            ckey[slot] = key;
            cid[slot] = i0 + k;
          }
        } else if (key == thr) {
          eq |= 1u << k;
        }
      }
    }
    if (base < need) {                   // uniform: base is the same in every thread
      const uint32_t cnt = __popc(eq);
      uint32_t incl = cnt;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o, 64);
        if (lane >= o) incl += v;
      }
      if (lane == 63) wsum[sw & 1][wid] = incl;
      __syncthreads();
      uint32_t off = base + incl - cnt, tot = 0;
#pragma unroll
      for (int w = 0; w < 16; ++w) {
        const uint32_t v = wsum[sw & 1][w];
        if (w < wid) off += v;
        tot += v;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if ((eq >> k) & 1u) {
          if (off < need) {
            ckey[ngt + off] = thr;
            cid[ngt + off] = i0 + k;
          }
          ++off;
        }
      }
      base += tot;
    }
  }
  __syncthreads();
  // ---- rank the n candidates: (key descending, id ascending) -----------------------------------
  if (tid < n) {
    const uint32_t key = ckey[tid];
    const int id = cid[tid];
    int rank = 0;
    for (int i = 0; i < n; ++i) {
      const uint32_t ki = ckey[i];
      rank += (i != tid && (ki > key || (ki == key && cid[i] < id))) ? 1 : 0;
    }
    top_ids[(size_t)row * TOPN_MAX + rank] = id;
    top_lp[(size_t)row * TOPN_MAX + rank] = row_logprob<T>(lr, id, V, s_ms[0], s_ms[1]);
  }
}

// logits [B, V] bf16 / f32 with 16-B aligned rows (as penny_sample), ids [B], topn [B] int32 (<= 0:
// the row is skipped) -> logprob [B] f32, top_ids / top_lp [B, TOPN_MAX]; columns >= topn[row] are
// not written.  max_n: the host's bound on topn (the kernel caps every row at it); max_n > TOPN_MAX
// or max_n > V is refused.
PENNY_API int penny_topn_logprob(const void* logits, int is_fp32, long row_stride, const int* ids, const int* topn,
                                 int max_n, float* logprob, int* top_ids, float* top_lp, int B, int V,
                                 hipStream_t stream) {
  if (B <= 0) return 0;
  if (!logits || !ids || !topn || !logprob || !top_ids || !top_lp || V <= 0 || max_n < 0 || max_n > TOPN_MAX ||
      max_n > V)
    return (int)hipErrorInvalidValue;
  if (is_fp32) {
    hipLaunchKernelGGL(topn_logprob_kernel<float>, dim3(B), dim3(1024), 0, stream, (const float*)logits, row_stride,
                       ids, topn, max_n, logprob, top_ids, top_lp, V);
  } else {
    hipLaunchKernelGGL(topn_logprob_kernel<bf16>, dim3(B), dim3(1024), 0, stream, (const bf16*)logits, row_stride,
                       ids, topn, max_n, logprob, top_ids, top_lp, V);
  }
  PENNY_RETURN_LAUNCH();
}
