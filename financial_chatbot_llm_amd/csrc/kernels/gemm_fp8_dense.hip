// Dense fp8 (OCP e4m3) x fp8 weight-streaming GEMM for decode-size steps of the Llama MLP
// (1 <= M <= 256 rows): Y = (Xq x Wq^T) * xs[m] * ws[n], W8A8 with f32 accumulation -- the Mixtral
// expert arithmetic (moe.hip) for ONE bucket of up to 256 rows.
//
// moe_gemm_kernel is shaped for many small buckets: one workgroup per weight slice (down at
// N = 4096 fills 64-128 of 256 CUs) and a walk over the rows in chunks of 64 that re-reads the slice
// per chunk.  Here:
//   * grid = (N / (16 NTF) row groups) x (S K-slices); a workgroup streams its 16 NTF weight rows of
//     its K-slice from HBM exactly ONCE, for all M rows: the accumulators of all ceil(M / 16) row
//     tiles (up to 16) x NTF weight fragments stay in registers;
//   * the 4 waves of a workgroup take the slice's 128-column chunks round-robin (together they walk
//     the rows front to back) and meet in LDS once, at the end, summed in wave order: no atomics, no
//     workspace, bitwise repeatable;
//   * W is the row-major [N, K] e4m3 weight the prefill tile kernel reads too (one copy): lane
//     16 g + r loads 16 contiguous bytes of row r at k = 64 p + 16 g, and the two loads of a 128-column
//     chunk fetch whole 128-B lines of 16 rows.  The activation lane does the same on its token row,
//     so both operands carry the same k permutation (as moe_gemm_kernel): bytes 0-7 feed the first
//     MFMA of the pair, bytes 8-15 the second.  X is at most 256 x K bytes and stays in L2;
//   * MFMA: v_mfma_f32_16x16x32_fp8_fp8.  Its 8-byte-per-lane operands come straight out of the
//     16-byte loads; the block-scaled 16x16x128 form wants 32 B per lane and operand, twice the
//     activation registers next to 16 row tiles of accumulators, and at these M the kernel waits for
//     HBM either way.
// Epilogues (s = the f32 sum over the workgroup's waves):
//   SILU   gate|up with the 16-row interleave: g = bf16(s_g xs ws_g), u = bf16(s_u xs ws_u),
//          Y[m, N/2] = bf16(bf16(silu(g)) * u)   -- ops.silu_mul(interleave16) of the bf16 gate|up
//   BF16   Y[m, N] = bf16(s xs ws)
//   SLABS  P[slice, m, N] = s xs ws in f32, unreduced (ops.gemm.Slabs consumers sum them)
// Rows >= M are never read (tile lanes past the last row re-read row M - 1 and are dropped) and
// never written.
#include "common.h"

#define DF8_EPI_SILU 1
#define DF8_EPI_BF16 2
#define DF8_EPI_SLABS 3
#define DF8_NW 4
#define DF8_MAX_S 16

template <int MT, int NTF, int EPI>
__global__ void __launch_bounds__(DF8_NW * 64) dense_fp8_kernel(
    const unsigned char* __restrict__ Xq, int ldx, const float* __restrict__ xs,
    const unsigned char* __restrict__ Wq, const float* __restrict__ ws, void* __restrict__ Yv, int ldy, int M, int N,
    int K, int kslice) {
  constexpr int NR = 16 * NTF;
  extern __shared__ __attribute__((aligned(16))) float red[];  // [DF8_NW][NR][64]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, col = lane & 15;
  const int n0 = blockIdx.x * NR;
  const int slice = blockIdx.y;
  const int mt = (M + 15) >> 4;  // row tiles in use (<= MT)
  f32x4 acc[NTF][MT];
#pragma unroll
  for (int f = 0; f < NTF; ++f)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[f][m] = f32x4{0.f, 0.f, 0.f, 0.f};
  const long kb = (long)slice * kslice + 16 * g;
  const unsigned char* xr[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int row = min(16 * m + col, M - 1);
    PENNY_DASSERT(row >= 0 && row < M);
    xr[m] = Xq + (long)row * ldx + kb;
  }
  const unsigned char* wr[NTF];
#pragma unroll
  for (int f = 0; f < NTF; ++f) {
    PENNY_DASSERT(n0 + 16 * f + col < N);
    wr[f] = Wq + (long)(n0 + 16 * f + col) * K + kb;
  }
  // this wave's 128-column chunks of the slice: w, w + NW, ...
  const int nch = kslice >> 7;
  const int mych = w < nch ? (nch - w + DF8_NW - 1) / DF8_NW : 0;
  uint4 wc[2][NTF], wn[2][NTF], xc[MT], xn[MT];
  auto load_w = [&](uint4 (&dst)[2][NTF], int c) {
    const int k = (w + c * DF8_NW) * 128;
    PENNY_DASSERT(k + 128 <= kslice);
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int f = 0; f < NTF; ++f) dst[h][f] = *reinterpret_cast<const uint4*>(wr[f] + k + 64 * h);
  };
  auto load_x = [&](uint4 (&dst)[MT], int c, int h) {
    const int k = (w + c * DF8_NW) * 128 + 64 * h;
#pragma unroll
    for (int m = 0; m < MT; ++m)
      if (m < mt) dst[m] = *reinterpret_cast<const uint4*>(xr[m] + k);
  };
  if (mych > 0) {
    load_w(wc, 0);
    load_x(xc, 0, 0);
  }
  for (int c = 0; c < mych; ++c) {
    const bool more = c + 1 < mych;
    if (more) load_w(wn, c + 1);  // the whole next chunk of W in flight under this one's MFMAs
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (h == 0) load_x(xn, c, 1);
      else if (more) load_x(xn, c + 1, 0);
#pragma unroll
      for (int f = 0; f < NTF; ++f) {
        const long a0 = ((long)wc[h][f].y << 32 | wc[h][f].x), a1 = ((long)wc[h][f].w << 32 | wc[h][f].z);
#pragma unroll
        for (int m = 0; m < MT; ++m) {
          if (m < mt) {
            const long b0 = ((long)xc[m].y << 32 | xc[m].x), b1 = ((long)xc[m].w << 32 | xc[m].z);
            acc[f][m] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a0, b0, acc[f][m], 0, 0, 0);
            acc[f][m] = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a1, b1, acc[f][m], 0, 0, 0);
          }
        }
      }
#pragma unroll
      for (int m = 0; m < MT; ++m) xc[m] = xn[m];
    }
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int f = 0; f < NTF; ++f) wc[h][f] = wn[h][f];
  }
  // the waves' partial sums meet in LDS, 64 rows (4 row tiles) at a time: acc[f][m][r] is weight row
  // 16 f + 4 g + r of the group, token row 16 m + col
  float* mine = red + w * NR * 64;
  constexpr int OUTN = (EPI == DF8_EPI_SILU) ? NR / 2 : NR;
#pragma unroll
  for (int c = 0; c < (MT + 3) / 4; ++c) {
    if (64 * c >= M) break;
#pragma unroll
    for (int f = 0; f < NTF; ++f)
#pragma unroll
      for (int mm = 0; mm < 4; ++mm)
        if (4 * c + mm < MT) {
#pragma unroll
          for (int r = 0; r < 4; ++r) mine[(16 * f + 4 * g + r) * 64 + 16 * mm + col] = acc[f][4 * c + mm][r];
        }
    __syncthreads();
    const int nrow = min(64, M - 64 * c);
    for (int idx = threadIdx.x; idx < 64 * (OUTN / 8); idx += DF8_NW * 64) {
      const int m = idx / (OUTN / 8), c8 = (idx % (OUTN / 8)) * 8;
      if (m >= nrow) continue;  // rows >= M: never written
      const int row = 64 * c + m;
      const float sx = xs[row];
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (EPI == DF8_EPI_SILU) {
          const int cc = c8 + j, pair = cc >> 4, jj = cc & 15;
          const int rg = 32 * pair + jj, ru = rg + 16;
          float gs = 0.f, us = 0.f;
#pragma unroll
          for (int ww = 0; ww < DF8_NW; ++ww) {
            gs += red[(ww * NR + rg) * 64 + m];
            us += red[(ww * NR + ru) * 64 + m];
          }
          const float gv = (float)(bf16)(gs * sx * ws[n0 + rg]);
          const float uv = (float)(bf16)(us * sx * ws[n0 + ru]);
          // SiLU in the activation dtype, as silu_mul_kernel: bf16(silu(g)) * u, rounded by pack8
          o[j] = (float)(bf16)(gv / (1.f + __expf(-gv))) * uv;
        } else {
          float s = 0.f;
#pragma unroll
          for (int ww = 0; ww < DF8_NW; ++ww) s += red[(ww * NR + c8 + j) * 64 + m];
          o[j] = s * sx * ws[n0 + c8 + j];
        }
      }
      if (EPI == DF8_EPI_SLABS) {
        float* p = (float*)Yv + ((long)slice * M + row) * ldy + n0 + c8;
        *reinterpret_cast<f32x4*>(p) = f32x4{o[0], o[1], o[2], o[3]};
        *reinterpret_cast<f32x4*>(p + 4) = f32x4{o[4], o[5], o[6], o[7]};
      } else {
        const int ncol = (EPI == DF8_EPI_SILU) ? (n0 / 2 + c8) : (n0 + c8);
        *reinterpret_cast<uint4*>((bf16*)Yv + (long)row * ldy + ncol) = pack8(o);
      }
    }
    __syncthreads();
  }
}

template <int MT, int NTF>
static int dense_fp8_launch(const void* Xq, int ldx, const float* xs, const void* Wq, const float* ws, void* Y,
                            int ldy, int M, int N, int K, int epi, int S, hipStream_t stream) {
  const dim3 grid(N / (16 * NTF), S);
  const size_t lds = (size_t)DF8_NW * 16 * NTF * 64 * sizeof(float);
#define DF8_GO(EPI_)                                                                                          \
  hipLaunchKernelGGL((dense_fp8_kernel<MT, NTF, EPI_>), grid, dim3(DF8_NW * 64), lds, stream,                 \
                     (const unsigned char*)Xq, ldx, xs, (const unsigned char*)Wq, ws, Y, ldy, M, N, K, K / S)
  if (epi == DF8_EPI_SILU) DF8_GO(DF8_EPI_SILU);
  else if (epi == DF8_EPI_BF16) DF8_GO(DF8_EPI_BF16);
  else DF8_GO(DF8_EPI_SLABS);
#undef DF8_GO
  PENNY_RETURN_LAUNCH();
}

// Xq [M, K] e4m3 (row stride ldx bytes), xs [M] f32 row scales, Wq [N, K] e4m3 row-major, ws [N] f32.
//   epi 1 SILU:  Y bf16 [M, N/2] (row stride ldy elements), Wq with the 16-row gate|up interleave
//   epi 2 BF16:  Y bf16 [M, N]
//   epi 3 SLABS: Y f32 [S, M, N] (row stride ldy, slab stride M * ldy), slab s = K-slice s
// ntf: 16-row weight groups per workgroup (2 or 4).  Contract (checked, hipErrorInvalidValue, nothing
// launched): 1 <= M <= 256; K % 128 == 0; N % (16 ntf) == 0; ldx % 16 == 0, ldx >= K; ldy % 8 == 0
// (bf16) / % 4 == 0 (f32) and >= the output width; Xq, Wq, Y 16-byte aligned; xs, ws non-null;
// S == 1 for SILU / BF16, 1 <= S <= 16 with K % (128 S) == 0 for SLABS.
PENNY_API int penny_dense_fp8_gemm(const void* Xq, int ldx, const float* xs, const void* Wq, const float* ws, void* Y,
                                   int ldy, int M, int N, int K, int epi, int S, int ntf, hipStream_t stream) {
  const int bad = (int)hipErrorInvalidValue;
  if (M < 1 || M > 256 || N <= 0 || K <= 0 || K % 128) return bad;
  if (!Xq || !xs || !Wq || !ws || !Y) return bad;
  if ((ntf != 2 && ntf != 4) || N % (16 * ntf)) return bad;
  if (ldx % 16 || ldx < K) return bad;
  if (((uintptr_t)Xq | (uintptr_t)Wq | (uintptr_t)Y) & 15) return bad;
  if (epi == DF8_EPI_SLABS) {
    if (S < 1 || S > DF8_MAX_S || K % (128 * S) || ldy % 4 || ldy < N) return bad;
  } else if (epi == DF8_EPI_SILU || epi == DF8_EPI_BF16) {
    if (S != 1 || ldy % 8 || ldy < (epi == DF8_EPI_SILU ? N / 2 : N)) return bad;
  } else {
    return bad;
  }
  const int mt = (M + 15) / 16;
#define DF8_CASE(MT_)                                                                                         \
  if (mt <= MT_) {                                                                                            \
    if (ntf == 4) return dense_fp8_launch<MT_, 4>(Xq, ldx, xs, Wq, ws, Y, ldy, M, N, K, epi, S, stream);      \
    return dense_fp8_launch<MT_, 2>(Xq, ldx, xs, Wq, ws, Y, ldy, M, N, K, epi, S, stream);                    \
  }
  DF8_CASE(1) DF8_CASE(2) DF8_CASE(4) DF8_CASE(8) DF8_CASE(16)
#undef DF8_CASE
  return bad;
}
