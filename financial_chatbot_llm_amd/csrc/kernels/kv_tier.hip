// Host-memory KV tier (ops/kv_tier.py, engine/kv_host_tier.py): whole KV blocks move between the paged
// pool and a dense staging buffer, which a plain hipMemcpyAsync carries over PCIe.
//
// The pool [L, 2, num_blocks, Hkv, 64*D] (models/common.py KVCache.buf) seen as bytes is `planes` = 2 L
// planes, `plane_stride` bytes apart, of num_blocks chunks of `plane_bytes` = Hkv * 64 * D * elt bytes;
// the staging buffer is [n, planes, plane_bytes], dense.
//   gather   staging[i, p, :] = pool[p, ids[i], :]
//   scatter  pool[p, ids[i], :] = staging[i, p, :]
// An id outside [0, num_blocks) is skipped: its staging rows (gather) or nothing at all (scatter) stay
// as they were, and no address is formed from it.  Two equal ids in one scatter are the caller's error
// (the last writer is not defined).
//
// A workgroup owns one (block, plane) pair -- blockIdx.x = i * planes + p -- and every gridDim.y-th
// 16 KiB segment of it: 256 lanes x 4 x 16 B, the four loads issued before the four stores.  Every byte
// offset is 64-bit (the production pool is ~250 GB).  Gather reads are non-temporal (a block leaves HBM
// once); the device sees device memory only, on both sides.  No LDS, no atomics, scratch 0.
#include "common.h"

static constexpr int KVT_THREADS = 256;
static constexpr int KVT_UNROLL = 4;
static constexpr long KVT_SEG_VECS = (long)KVT_THREADS * KVT_UNROLL;      // 16-B vectors per segment

typedef unsigned kvt_u32x4 __attribute__((ext_vector_type(4)));

template <bool GATHER>
__global__ void __launch_bounds__(KVT_THREADS) kv_tier_copy_kernel(char* __restrict__ pool, long plane_stride,
                                                                   long plane_bytes, int planes, int num_blocks,
                                                                   const int* __restrict__ ids, int n,
                                                                   char* __restrict__ staging) {
  const long row = blockIdx.x;                       // i * planes + p
  const int i = (int)(row / planes), p = (int)(row - (long)i * planes);
  PENNY_DASSERT(i < n);
  const int id = ids[i];
  if (id < 0 || id >= num_blocks) return;            // the same for the whole workgroup
  const long nvec = plane_bytes >> 4;
  PENNY_DASSERT((long)id * plane_bytes + plane_bytes <= plane_stride);
  kvt_u32x4* pv = reinterpret_cast<kvt_u32x4*>(pool + (long)p * plane_stride + (long)id * plane_bytes);
  kvt_u32x4* sv = reinterpret_cast<kvt_u32x4*>(staging + row * plane_bytes);
  const kvt_u32x4* src = GATHER ? pv : sv;
  kvt_u32x4* dst = GATHER ? sv : pv;
  for (long v0 = (long)blockIdx.y * KVT_SEG_VECS + threadIdx.x; v0 < nvec; v0 += (long)gridDim.y * KVT_SEG_VECS) {
    kvt_u32x4 r[KVT_UNROLL];
#pragma unroll
    for (int k = 0; k < KVT_UNROLL; ++k) {
      const long v = v0 + (long)k * KVT_THREADS;
      if (v < nvec) r[k] = GATHER ? __builtin_nontemporal_load(src + v) : src[v];
    }
#pragma unroll
    for (int k = 0; k < KVT_UNROLL; ++k) {
      const long v = v0 + (long)k * KVT_THREADS;
      if (v < nvec) {
        PENNY_DASSERT(v * 16 + 16 <= plane_bytes);
        dst[v] = r[k];
      }
    }
  }
}

static int kv_tier_launch(bool gather, void* pool, long plane_stride, long plane_bytes, int planes, int num_blocks,
                          const int* ids, int n, void* staging, hipStream_t stream) {
  if (n == 0) return 0;
  if (!pool || !ids || !staging || n < 0 || planes <= 0 || num_blocks <= 0 || plane_bytes <= 0 || plane_bytes % 16 ||
      plane_stride % 16 || plane_stride / plane_bytes < num_blocks || ((uintptr_t)pool & 15) ||
      ((uintptr_t)staging & 15) || ((uintptr_t)ids & 3) || (long)n * planes > 0x7fffffffL)
    return (int)hipErrorInvalidValue;
  const long segs = ((plane_bytes >> 4) + KVT_SEG_VECS - 1) / KVT_SEG_VECS;
  const dim3 grid((unsigned)((long)n * planes), (unsigned)(segs < 64 ? segs : 64));
  if (gather)
    hipLaunchKernelGGL(kv_tier_copy_kernel<true>, grid, dim3(KVT_THREADS), 0, stream, (char*)pool, plane_stride,
                       plane_bytes, planes, num_blocks, ids, n, (char*)staging);
  else
    hipLaunchKernelGGL(kv_tier_copy_kernel<false>, grid, dim3(KVT_THREADS), 0, stream, (char*)pool, plane_stride,
                       plane_bytes, planes, num_blocks, ids, n, (char*)staging);
  PENNY_RETURN_LAUNCH();
}

// staging [n, planes, plane_bytes] <- blocks ids[0..n) (device int32) of the pool: plane p of block b at
// pool + p * plane_stride_bytes + b * plane_bytes.  Everything 16-byte aligned.
PENNY_API int penny_kv_gather_blocks(const void* pool, long plane_stride_bytes, long plane_bytes, int planes,
                                     int num_blocks, const int* ids, int n, void* staging, hipStream_t stream) {
  return kv_tier_launch(true, const_cast<void*>(pool), plane_stride_bytes, plane_bytes, planes, num_blocks, ids, n,
                        staging, stream);
}

// the inverse: blocks ids[0..n) of the pool <- staging [n, planes, plane_bytes]
PENNY_API int penny_kv_scatter_blocks(void* pool, long plane_stride_bytes, long plane_bytes, int planes, int num_blocks,
                                      const int* ids, int n, const void* staging, hipStream_t stream) {
  return kv_tier_launch(false, pool, plane_stride_bytes, plane_bytes, planes, num_blocks, ids, n,
                        const_cast<void*>(staging), stream);
}
