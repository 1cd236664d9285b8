// K15: filtered exact top-k similarity search over an HBM-resident corpus (replaces Qdrant's
// filtered HNSW query, tools/qdrant_tool.py:98-153).
//
// Filters are the reference's: user_id == u (always) AND date >= t (optional).  Such filters are
// very selective (one user's rows out of ~1M), so the search is organised around the filter, not
// the vectors:
//   1. filter_compact: one pass over the int32 user codes + int64 dates (12 B/row, ~12 MB for
//      1M rows) evaluates every query's filter and appends matching row ids to a per-query
//      candidate list (wave-aggregated atomics).  Vectors of non-matching rows are never read.
//   2. score: one wave per candidate row computes <corpus_row, query> (768-d bf16, 16 B/lane).
//   3. select: one workgroup per query bitonic-sorts up to SORT_CAP (score, row) pairs in LDS,
//      descending by score, ties by row id, and writes the first k.
// Queries with more candidates than SORT_CAP are finished by the caller (ops/retrieval.py, in the
// same order, from the device-side score list), which the host detects from the returned counts.
#include "common.h"

#define SORT_CAP 8192

__global__ void filter_compact_kernel(const int* __restrict__ user_codes, const long long* __restrict__ dates, long N,
                                      const int* __restrict__ q_user, const long long* __restrict__ q_floor, int nq,
                                      int* __restrict__ counts, int* __restrict__ cand, int cap) {
  __shared__ int su[64];
  __shared__ long long sf[64];
  for (int i = threadIdx.x; i < nq; i += blockDim.x) {
    su[i] = q_user[i];
    sf[i] = q_floor[i];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  for (long base = (long)blockIdx.x * blockDim.x; base < N; base += (long)gridDim.x * blockDim.x) {
    const long n = base + threadIdx.x;
    const bool in = n < N;
    const int code = in ? user_codes[n] : -2;
    const long long d = in ? dates[n] : 0;
    for (int qi = 0; qi < nq; ++qi) {
      const bool hit = in && code == su[qi] && d >= sf[qi];
      const unsigned long long mask = __ballot(hit);
      if (mask == 0ull) continue;
      int start = 0;
      if (lane == __ffsll((long long)mask) - 1) start = atomicAdd(&counts[qi], __popcll(mask));
      start = __shfl(start, __ffsll((long long)mask) - 1, 64);
      if (hit) {
        const int pos = start + __popcll(mask & ((1ull << lane) - 1ull));
        if (pos < cap) cand[(long)qi * cap + pos] = (int)n;
      }
    }
  }
}

// one wave per (query, candidate); D multiple of 8, D <= 1024
__global__ void score_kernel(const bf16* __restrict__ corpus, int D, const bf16* __restrict__ queries,
                             const int* __restrict__ counts, const int* __restrict__ cand, int cap,
                             float* __restrict__ scores) {
  const int qi = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int waves = (gridDim.x * blockDim.x) >> 6;
  const int wid = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int cnt = min(counts[qi], cap);
  const int nch = D >> 3;
  float qv[2][8];
  for (int r = 0; r < 2; ++r) {
    const int c = lane + 64 * r;
    if (c < nch) unpack8(reinterpret_cast<const uint4*>(queries + (long)qi * D)[c], qv[r]);
  }
  for (int i = wid; i < cnt; i += waves) {
    const int row = cand[(long)qi * cap + i];
    const uint4* cr = reinterpret_cast<const uint4*>(corpus + (long)row * D);
    float acc = 0.f;
    for (int r = 0; r < 2; ++r) {
      const int c = lane + 64 * r;
      if (c < nch) {
        float f[8];
        unpack8(cr[c], f);
#pragma unroll
        for (int k = 0; k < 8; ++k) acc += f[k] * qv[r][k];
      }
    }
    acc = wave_sum(acc);
    if (lane == 0) scores[(long)qi * cap + i] = acc;
  }
}

__device__ __forceinline__ bool before(float sa, int ia, float sb, int ib) {  // a ranks before b
  return sa > sb || (sa == sb && ia < ib);
}

__global__ void __launch_bounds__(1024) select_kernel(const int* __restrict__ counts, const int* __restrict__ cand,
                                                      const float* __restrict__ scores, int cap,
                                                      const int* __restrict__ ks, int kmax, int* __restrict__ out_ids,
                                                      float* __restrict__ out_scores, int* __restrict__ out_count) {
  extern __shared__ __attribute__((aligned(16))) char dyn[];
  float* ss = reinterpret_cast<float*>(dyn);
  int* si = reinterpret_cast<int*>(dyn + SORT_CAP * sizeof(float));
  const int qi = blockIdx.x;
  const int total = counts[qi];
  const int cnt = min(total, cap);
  const int k = min(ks[qi], min(cnt, kmax));
  if (total > SORT_CAP) {  // host finishes this query
    if (threadIdx.x == 0) out_count[qi] = -total;
    return;
  }
  int n = 1;
  while (n < cnt) n <<= 1;
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const bool v = i < cnt;
    ss[i] = v ? scores[(long)qi * cap + i] : -INFINITY;
    si[i] = v ? cand[(long)qi * cap + i] : 0x7fffffff;
  }
  __syncthreads();
  for (int size = 2; size <= n; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int j = i ^ stride;
        if (j > i) {
          const bool desc = (i & size) == 0;  // this run sorted "best first"
          const bool swap = desc ? before(ss[j], si[j], ss[i], si[i]) : before(ss[i], si[i], ss[j], si[j]);
          if (swap) {
            const float t = ss[i]; ss[i] = ss[j]; ss[j] = t;
            const int u = si[i]; si[i] = si[j]; si[j] = u;
          }
        }
      }
      __syncthreads();
    }
  }
  for (int i = threadIdx.x; i < k; i += blockDim.x) {
    out_ids[(long)qi * kmax + i] = si[i];
    out_scores[(long)qi * kmax + i] = ss[i];
  }
  if (threadIdx.x == 0) out_count[qi] = k;
}

PENNY_API int penny_filtered_topk(const void* corpus, const int* user_codes, const long long* dates, long N, int D,
                                  const void* queries, const int* q_user, const long long* q_floor, const int* ks,
                                  int nq, int kmax, int* counts, int* cand, float* scores, int cap, int* out_ids,
                                  float* out_scores, int* out_count, hipStream_t stream) {
  if (nq <= 0) return 0;
  if (nq > 64 || D % 8 || D > 1024) return (int)hipErrorInvalidValue;
  hipMemsetAsync(counts, 0, sizeof(int) * nq, stream);
  long g = (N + 255) / 256;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  hipLaunchKernelGGL(filter_compact_kernel, dim3((int)g), dim3(256), 0, stream, user_codes, dates, N, q_user, q_floor,
                     nq, counts, cand, cap);
  hipLaunchKernelGGL(score_kernel, dim3(64, nq), dim3(256), 0, stream, (const bf16*)corpus, D, (const bf16*)queries,
                     counts, cand, cap, scores);
  const size_t lds = SORT_CAP * (sizeof(float) + sizeof(int));
  hipLaunchKernelGGL(select_kernel, dim3(nq), dim3(1024), lds, stream, counts, cand, scores, cap, ks, kmax, out_ids,
                     out_scores, out_count);
  PENNY_RETURN_LAUNCH();
}

// ---- hybrid retrieval: BM25 term scores fused into the score pass --------------------------------
// Each corpus row carries LEX_DOC_TERMS int32 term hashes (128 B, zero = empty slot, distinct within
// a row) beside its vector; each query carries LEX_QUERY_TERMS hashes with prepared weights
// (ops/retrieval.py, hybrid_query_weights):
//   score(q, d) = dw * <q, v_d> + r[n_d] * sum_{j : t_j in terms(d)} u_j,   n_d = non-zero slots of d.
// All logs and divisions are done by the caller; the device multiplies and adds only.
#define LEX_DOC_TERMS 32
#define LEX_QUERY_TERMS 16
#define LEX_DF_MASK 0xFFFFF

// one wave per (query, candidate), as score_kernel; lanes 0-7 also take 16 B of the row's terms each
__global__ void hybrid_score_kernel(const bf16* __restrict__ corpus, int D, const int* __restrict__ terms,
                                    const bf16* __restrict__ queries, const int* __restrict__ q_terms,
                                    const float* __restrict__ q_u, const float* __restrict__ q_dw,
                                    const float* __restrict__ rtab, const int* __restrict__ counts,
                                    const int* __restrict__ cand, int cap, float* __restrict__ scores) {
  const int qi = blockIdx.y;
  const int lane = threadIdx.x & 63;
  const int waves = (gridDim.x * blockDim.x) >> 6;
  const int wid = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int cnt = min(counts[qi], cap);
  const int nch = D >> 3;
  const float dw = q_dw[qi];
  const bool dense = dw != 0.f;  // uniform per block: a purely lexical query reads no vector bytes
  int qt[LEX_QUERY_TERMS];
  float qu[LEX_QUERY_TERMS];
#pragma unroll
  for (int j = 0; j < LEX_QUERY_TERMS; ++j) {
    qt[j] = q_terms[qi * LEX_QUERY_TERMS + j];
    qu[j] = q_u[qi * LEX_QUERY_TERMS + j];
  }
  // The scalar loads above are waited for once; then the query vector (which needs dw), the first
  // candidate id and the r table are asked for together, so the chain to the first row is as deep as
  // in score_kernel.  The barriers keep the compiler from interleaving the groups with waits.
  __builtin_amdgcn_sched_barrier(0);
  // a lane without a chunk (c >= nch) loads chunk 0 and drops it: no branch, so no wait, between loads
  uint4 qraw[2] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
  if (dense) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int c = lane + 64 * r;
      qraw[r] = reinterpret_cast<const uint4*>(queries + (long)qi * D)[c < nch ? c : 0];
    }
  }
  int next_row = wid < cnt ? cand[(long)qi * cap + wid] : 0;
  const float rv = lane <= LEX_DOC_TERMS ? rtab[lane] : 0.f;  // r[n] sits in lane n: no load behind the terms
  __builtin_amdgcn_sched_barrier(0);
  float qv[2][8];
  for (int r = 0; r < 2; ++r) unpack8(qraw[r], qv[r]);
  for (int i = wid; i < cnt; i += waves) {
    const int row = next_row;
    if (i + waves < cnt) next_row = cand[(long)qi * cap + i + waves];
    // the terms go first so that their compares run while the vector chunks are still in flight
    int4 t = make_int4(0, 0, 0, 0);
    if (lane < LEX_DOC_TERMS / 4) t = reinterpret_cast<const int4*>(terms + (long)row * LEX_DOC_TERMS)[lane];
    float acc = 0.f;
    if (dense) {
      const uint4* cr = reinterpret_cast<const uint4*>(corpus + (long)row * D);
      uint4 raw[2];
#pragma unroll
      for (int r = 0; r < 2; ++r) raw[r] = cr[lane + 64 * r < nch ? lane + 64 * r : 0];
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        if (lane + 64 * r < nch) {  // score_kernel's sum, term for term
          float f[8];
          unpack8(raw[r], f);
#pragma unroll
          for (int k = 0; k < 8; ++k) acc += f[k] * qv[r][k];
        }
      }
    }
    const int n_d = __popcll(__ballot(t.x != 0)) + __popcll(__ballot(t.y != 0)) + __popcll(__ballot(t.z != 0)) +
                    __popcll(__ballot(t.w != 0));
    const float rn = __shfl(rv, n_d, 64);
    const int ts[4] = {t.x, t.y, t.z, t.w};
    float ps[4];  // one sum per slot, query terms in order, then (s0 + s1) + (s2 + s3): a fixed order
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      ps[s] = 0.f;
#pragma unroll
      for (int j = 0; j < LEX_QUERY_TERMS; ++j)
        if (ts[s] != 0 && ts[s] == qt[j]) ps[s] += qu[j];
    }
    const float lex = wave_sum((ps[0] + ps[1]) + (ps[2] + ps[3]));
    if (dense) acc = wave_sum(acc);
    if (lane == 0) scores[(long)qi * cap + i] = dw * acc + rn * lex;
  }
}

// Adds the rows' terms to the document-frequency buckets.  A wave takes 64 rows, one per lane, and
// walks the 32 slots; lanes whose terms fall in one bucket (the field labels of every row do) elect
// a leader that adds their count with one atomic, the ballot / leader style of filter_compact_kernel.
__global__ void lex_df_add_kernel(const int* __restrict__ terms, long n_rows, int* __restrict__ df) {
  const int lane = threadIdx.x & 63;
  for (long base = (long)blockIdx.x * blockDim.x; base < n_rows; base += (long)gridDim.x * blockDim.x) {
    const long n = base + threadIdx.x;
    const bool in = n < n_rows;
    for (int c = 0; c < LEX_DOC_TERMS / 4; ++c) {
      int4 t = make_int4(0, 0, 0, 0);
      if (in) t = reinterpret_cast<const int4*>(terms + n * LEX_DOC_TERMS)[c];
      const int ts[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int bucket = ts[s] & LEX_DF_MASK;
        unsigned long long todo = __ballot(ts[s] != 0);
        while (todo != 0ull) {
          const int leader = __ffsll((long long)todo) - 1;
          const int b = __shfl(bucket, leader, 64);
          const unsigned long long same = __ballot(ts[s] != 0 && bucket == b);
          if (lane == leader) atomicAdd(&df[b], __popcll(same));
          todo &= ~same;
        }
      }
    }
  }
}

PENNY_API int penny_filtered_topk_hybrid(const void* corpus, const int* user_codes, const long long* dates, long N,
                                         int D, const int* terms, const void* queries, const int* q_user,
                                         const long long* q_floor, const int* ks, const int* q_terms,
                                         const float* q_u, const float* q_dw, const float* rtab, int nq, int kmax,
                                         int* counts, int* cand, float* scores, int cap, int* out_ids,
                                         float* out_scores, int* out_count, hipStream_t stream) {
  if (nq <= 0) return 0;
  if (nq > 64 || D % 8 || D > 1024) return (int)hipErrorInvalidValue;
  hipMemsetAsync(counts, 0, sizeof(int) * nq, stream);
  long g = (N + 255) / 256;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  hipLaunchKernelGGL(filter_compact_kernel, dim3((int)g), dim3(256), 0, stream, user_codes, dates, N, q_user, q_floor,
                     nq, counts, cand, cap);
  hipLaunchKernelGGL(hybrid_score_kernel, dim3(64, nq), dim3(256), 0, stream, (const bf16*)corpus, D, terms,
                     (const bf16*)queries, q_terms, q_u, q_dw, rtab, counts, cand, cap, scores);
  const size_t lds = SORT_CAP * (sizeof(float) + sizeof(int));
  hipLaunchKernelGGL(select_kernel, dim3(nq), dim3(1024), lds, stream, counts, cand, scores, cap, ks, kmax, out_ids,
                     out_scores, out_count);
  PENNY_RETURN_LAUNCH();
}

PENNY_API int penny_lex_df_add(const int* terms, long n_rows, int* df, hipStream_t stream) {
  if (n_rows <= 0) return 0;
  long g = (n_rows + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(lex_df_add_kernel, dim3((int)g), dim3(256), 0, stream, terms, n_rows, df);
  PENNY_RETURN_LAUNCH();
}
