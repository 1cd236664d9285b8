// Dense weight-streaming GEMM for decode-size steps of the Llama MLP (1 <= M <= 256 rows), in two weight
// formats against dynamic per-row e4m3 activations: Y = (Xq x W^T) * xs[m] * ws[n] with f32 accumulation.
//   fp8    W8A8: W[N, K] row-major OCP e4m3 codes -- the Mixtral expert arithmetic (moe.hip) for ONE bucket
//          of up to 256 rows;
//   MXFP4  W4A8: OCP e2m1 codes with E8M0 block exponents (below),
// and penny_mxfp4_expand, which turns an MXFP4 weight into the e4m3 codes every fp8 kernel reads.
// One kernel template holds both formats' main loops; the grid, the reduction, the epilogues and the output
// layouts are written once and are the same for both.
//
// moe_gemm_kernel is shaped for many small buckets: one workgroup per weight slice (down at N = 4096 fills
// 64-128 of 256 CUs) and a walk over the rows in chunks of 64 that re-reads the slice per chunk.  Here:
//   * grid = (N / (16 NTF) row groups) x (S K-slices); a workgroup streams its 16 NTF weight rows of its
//     K-slice from HBM exactly ONCE, for all M rows: the accumulators of all ceil(M / 16) row tiles (up to
//     16) x NTF weight fragments stay in registers;
//   * the 4 waves of a workgroup take the slice's chunks (128 columns fp8, 256 MXFP4) round-robin (together
//     they walk the rows front to back) and meet in LDS once, at the end, summed in wave order: no atomics,
//     no workspace, bitwise repeatable;
//   * X is at most 256 x K bytes and stays in L2.
//
// fp8 operands:
//   * W is the row-major [N, K] e4m3 weight the prefill tile kernel reads too (one copy): lane 16 g + r loads
//     16 contiguous bytes of row r at k = 64 p + 16 g, and the two loads of a 128-column chunk fetch whole
//     128-B lines of 16 rows.  The activation lane does the same on its token row, so both operands carry
//     the same k permutation (as moe_gemm_kernel): bytes 0-7 feed the first MFMA of the pair, bytes 8-15 the
//     second;
//   * MFMA: v_mfma_f32_16x16x32_fp8_fp8.  Its 8-byte-per-lane operands come straight out of the 16-byte
//     loads; the block-scaled 16x16x128 form wants 32 B per lane and operand, twice the activation registers
//     next to 16 row tiles of accumulators, and at these M the kernel waits for HBM either way.
//
// MXFP4 operands.  The weight W[N, K] is three tensors (ops/mxfp4_dense.py):
//   codes [N, K/2] uint8   e2m1 (magnitudes 0, .5, 1, 1.5, 2, 3, 4, 6; bit 3 the sign), element 2j in the
//                          low nibble of byte j, element 2j + 1 in the high nibble
//   exps  [N, K/32] uint8  E8M0 127 + e of each 32-column block, e in -8 .. 0
//   ws    [N] f32          row scale;  w[n, k] = ws[n] 2^e[n, k/32] e2m1(code[n, k])
// For e in -8 .. 0 every e2m1 2^e is an e4m3fn value, so the expansion is exact and both formats' kernels
// compute the same mathematical product.
//   * MFMA: v_mfma_scale_f32_16x16x128_f8f6f4 with A = the weights in fp4 (cbsz 4: the low 4 registers of
//     the operand) and B = the activations in e4m3 at unit scale.  Measured on the hardware with one-hot
//     activations (tests/test_dense_mxfp4_gpu.py pins it):
//       - fp4 operand: lane l feeds row l & 15, k = 32 (l >> 4) .. + 31 in natural order, the low nibble of
//         a byte the even k; its scale operand (byte 0 of the word at op_sel 0) scales exactly those 32;
//       - e4m3 operand: lane l feeds row l & 15, registers 0-3 k = 16 (l >> 4) .. + 15 and registers 4-7
//         k = 64 + 16 (l >> 4) .. + 15 -- two 64-wide halves, as the fp8 loop's pair of loads.
//     So a lane loads 16 B of codes at byte 64 h + 16 g of the row's 128 per chunk (h = 0, 1: whole 128-B
//     lines of 16 rows), its one E8M0 byte of that (row, block) out of one 8-B load of
//     exps[row][k0 / 32 .. + 8], and 2 x 16 B of activations at columns 128 h + 16 g and + 64: the MX block
//     is the lane's share, no cross-lane work;
//   * the activations need 8 VGPRs per row tile, so the row tiles are walked in groups of 4 with the next
//     group's loads in flight (a 64-VGPR ring).
//
// Epilogues (s = the f32 sum over the workgroup's waves):
//   SILU   gate|up with the 16-row interleave: g = bf16(s_g xs ws_g), u = bf16(s_u xs ws_u),
//          Y[m, N/2] = bf16(bf16(silu(g)) * u)   -- ops.silu_mul(interleave16) of the bf16 gate|up
//   BF16   Y[m, N] = bf16(s xs ws)
//   SLABS  P[slice, m, N] = s xs ws in f32, unreduced (ops.gemm.Slabs consumers sum them)
// Rows >= M are never read (tile lanes past the last row re-read row M - 1 and are dropped) and never
// written.
//
// MXFP4 registers (hipcc -O3, gfx950, 256 threads = one wave per SIMD; VGPR / AGPR, the largest of the three
// epilogues; no instantiation uses scratch -- the build's -Rpass-analysis=kernel-resource-usage shows
// ScratchSize 0 for all 33 MXFP4 kernels and the expander, 29 / 0):
//   row tiles      1          2          4          8          12         16
//   NTF = 2     80 / 8    94 / 16   118 / 32   166 / 96   208 / 136  252 / 180
//   NTF = 4    116 / 16  132 / 32   174 / 84   214 / 164  256 / 256      --
// hipcc does not keep the accumulators of the scaled MFMA in place (the instruction has no tied form, as
// gemm_prefill.hip found), so beyond 4 row tiles they move between the two register files and the counts
// exceed 4 MT NTF accumulators + 2 W buffers + the X ring.  16 row tiles x 4 fragments (256 accumulators)
// spilled 60-100 registers in every form tried (in-place asm "uses", 2-tile groups, 32-bit offsets), so the
// launcher runs MXFP4 ntf = 4 above 192 rows as 32-row groups: the same arithmetic per output element.
#include "common.h"

#define DS_FP8 0
#define DS_MXFP4 1
#define DS_EPI_SILU 1
#define DS_EPI_BF16 2
#define DS_EPI_SLABS 3
#define DS_NW 4
#define DS_MAX_S 16

typedef int ds_i32x8 __attribute__((ext_vector_type(8)));
typedef const unsigned char* __restrict__ ds_exps;

// Wq: the e4m3 codes [N, K] (fp8) or the e2m1 codes [N, K/2] (MXFP4).  WE: empty for fp8, ds_exps for MXFP4,
// whose E8M0 exponents [N, K/32] are then the one argument in its place: each format's kernel takes exactly
// its own arguments (an unused pointer in fp8's list moved its kernarg loads and address arithmetic).
template <int FMT, int MT, int NTF, int EPI, class... WE>
__global__ void __launch_bounds__(DS_NW * 64) dense_stream_kernel(
    const unsigned char* __restrict__ Xq, int ldx, const float* __restrict__ xs,
    const unsigned char* __restrict__ Wq, WE... We_, const float* __restrict__ ws, void* __restrict__ Yv, int ldy,
    int M, int N, int K, int kslice) {
  static_assert(sizeof...(WE) == (FMT == DS_MXFP4), "MXFP4 alone has the exponent pointer");
  constexpr int NR = 16 * NTF;
  extern __shared__ __attribute__((aligned(16))) float red[];  // [DS_NW][NR][64]
  const int lane = threadIdx.x & 63;
  // the wave: MXFP4's loop was tuned with it declared wave-uniform, fp8's with the plain vector value
  const int w = FMT == DS_MXFP4 ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : (int)(threadIdx.x >> 6);
  const int g = lane >> 4, col = lane & 15;
  const int n0 = blockIdx.x * NR;
  const int slice = blockIdx.y;
  const int mt = (M + 15) >> 4;  // row tiles in use (<= MT)
  f32x4 acc[NTF][MT];
#pragma unroll
  for (int f = 0; f < NTF; ++f)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[f][m] = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (FMT == DS_FP8) {
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
    const int mych = w < nch ? (nch - w + DS_NW - 1) / DS_NW : 0;
    uint4 wc[2][NTF], wn[2][NTF], xc[MT], xn[MT];
    auto load_w = [&](uint4 (&dst)[2][NTF], int c) {
      const int k = (w + c * DS_NW) * 128;
      PENNY_DASSERT(k + 128 <= kslice);
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int f = 0; f < NTF; ++f) dst[h][f] = *reinterpret_cast<const uint4*>(wr[f] + k + 64 * h);
    };
    auto load_x = [&](uint4 (&dst)[MT], int c, int h) {
      const int k = (w + c * DS_NW) * 128 + 64 * h;
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
  } else {
    constexpr int GS = MT < 4 ? MT : 4;  // row tiles per activation group: a 64-VGPR ring
    constexpr int NG = MT / GS;
    static_assert(MT == GS * NG, "row tiles: whole groups");
    const unsigned char* Wc = Wq;
    ds_exps We = (We_, ...);
    const long k0 = (long)slice * kslice;  // first column of the slice
    // Addresses are a uniform 64-bit base plus a 32-bit lane offset (the launcher bounds ldx, so
    // 256 ldx and 64 K fit): one VGPR per pointer; sixteen 64-bit row pointers held across the loop spilled.
    // Activations: this lane's 2 x 16 bytes of row tile m, chunk column k, half h: xbase + k + 128 h + xoff(m)
    // and 64 bytes on (the e4m3 operand's k order, see the header).
    // Row 16 m + col, clamped to M - 1 in the last tile in use; the tiles of the instantiation past it (MT is
    // the next of 1, 2, 4, 8, 12, 16, so they share its group of 4) are loaded and multiplied the same way
    // and never stored: the main loop has no branch on M
    const unsigned char* xbase = Xq + k0;
    const unsigned xl = (unsigned)(col * ldx + 16 * g), xlast = (unsigned)(min(16 * (mt - 1) + col, M - 1) * ldx + 16 * g);
    PENNY_DASSERT(16 * (mt - 1) < M && M <= 16 * MT);
    auto xoff = [&](int m) -> unsigned { return m >= mt - 1 ? xlast : xl + (unsigned)(m * 16 * ldx); };
    // codes: 16 bytes at wbase + f 16 (K / 2) + k / 2 + 64 h + wl; exponents: 8 bytes at ebase + f 16 (K / 32) + k / 32 + el
    PENNY_DASSERT(n0 + NR <= N);
    const unsigned char* wbase = Wc + (long)n0 * (K >> 1) + (k0 >> 1);
    const unsigned char* ebase = We + (long)n0 * (K >> 5) + (k0 >> 5);
    const unsigned wl = (unsigned)(col * (K >> 1) + 16 * g), el = (unsigned)(col * (K >> 5));
    // this wave's 256-column chunks of the slice: w, w + NW, ...
    const int nch = kslice >> 8;
    const int mych = w < nch ? (nch - w + DS_NW - 1) / DS_NW : 0;
    // W: the current chunk and the next one; X: two buffers alternated statically (a chunk has 2 NG groups,
    // so every chunk starts on buffer 0).  The main loop has no branch: the prefetch of the last chunk re-reads
    // that chunk (an L2 hit) -- a branch round a prefetch made hipcc wait for every load in flight before each
    // group's MFMAs
    uint4 wc[2][NTF], wn[2][NTF];
    uint2 ec[NTF], en[NTF];
    uint4 x[2][GS][2];
    auto load_w = [&](uint4 (&dst)[2][NTF], uint2 (&de)[NTF], int c) {
      const int k = (w + c * DS_NW) * 256;
      PENNY_DASSERT(k >= 0 && k + 256 <= kslice);
#pragma unroll
      for (int f = 0; f < NTF; ++f)
        de[f] = *reinterpret_cast<const uint2*>(ebase + ((long)f * 16 * (K >> 5) + (k >> 5)) + el);
#pragma unroll
      for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int f = 0; f < NTF; ++f)
          dst[h][f] = *reinterpret_cast<const uint4*>(wbase + ((long)f * 16 * (K >> 1) + (k >> 1) + 64 * h) + wl);
    };
    auto load_x = [&](uint4 (&dst)[GS][2], int c, int h, int gi) {
      const int k = (w + c * DS_NW) * 256 + 128 * h;
      PENNY_DASSERT(k >= 0 && k + 128 <= kslice);
#pragma unroll
      for (int j = 0; j < GS; ++j) {
        const unsigned char* p = xbase + k + xoff(gi * GS + j);
        dst[j][0] = *reinterpret_cast<const uint4*>(p);
        dst[j][1] = *reinterpret_cast<const uint4*>(p + 64);
      }
    };
    if (mych > 0) {
      load_w(wc, ec, 0);
      load_x(x[0], 0, 0, 0);
    }
    for (int c = 0; c < mych; ++c) {
      const int cn = min(c + 1, mych - 1);
      load_w(wn, en, cn);  // the whole next chunk of W in flight under this one's MFMAs
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        ds_i32x8 a[NTF];
        int sc[NTF];
#pragma unroll
        for (int f = 0; f < NTF; ++f) {
          a[f] = ds_i32x8{(int)wc[h][f].x, (int)wc[h][f].y, (int)wc[h][f].z, (int)wc[h][f].w, 0, 0, 0, 0};
          sc[f] = (int)(((h ? ec[f].y : ec[f].x) >> (8 * g)) & 0xffu);  // E8M0 of (row, k-block 4 h + g)
        }
#pragma unroll
        for (int gi = 0; gi < NG; ++gi) {
          const int p = (h * NG + gi) & 1;
          // the next group's activations in flight under this group's MFMAs
          if (gi + 1 < NG) load_x(x[p ^ 1], c, h, gi + 1);
          else if (h == 0) load_x(x[p ^ 1], c, 1, 0);
          else load_x(x[p ^ 1], cn, 0, 0);
#pragma unroll
          for (int j = 0; j < GS; ++j) {
            const uint4 lo = x[p][j][0], hi = x[p][j][1];
            const ds_i32x8 b =
                ds_i32x8{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
#pragma unroll
            for (int f = 0; f < NTF; ++f)
              acc[f][gi * GS + j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[f], b, acc[f][gi * GS + j], 4,
                                                                                     0, 0, sc[f], 0, 127);
          }
          // one group's loads and MFMAs per scheduling region
          __builtin_amdgcn_sched_barrier(0);
        }
      }
#pragma unroll
      for (int f = 0; f < NTF; ++f) {
        ec[f] = en[f];
#pragma unroll
        for (int h = 0; h < 2; ++h) wc[h][f] = wn[h][f];
      }
    }
  }
  // the waves' partial sums meet in LDS, 64 rows (4 row tiles) at a time: acc[f][m][r] is weight row
  // 16 f + 4 g + r of the group, token row 16 m + col
  float* mine = red + w * NR * 64;
  constexpr int OUTN = (EPI == DS_EPI_SILU) ? NR / 2 : NR;
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
    for (int idx = threadIdx.x; idx < 64 * (OUTN / 8); idx += DS_NW * 64) {
      const int m = idx / (OUTN / 8), c8 = (idx % (OUTN / 8)) * 8;
      if (m >= nrow) continue;  // rows >= M: never written
      const int row = 64 * c + m;
      const float sx = xs[row];
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (EPI == DS_EPI_SILU) {
          const int cc = c8 + j, pair = cc >> 4, jj = cc & 15;
          const int rg = 32 * pair + jj, ru = rg + 16;
          float gs = 0.f, us = 0.f;
#pragma unroll
          for (int ww = 0; ww < DS_NW; ++ww) {
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
          for (int ww = 0; ww < DS_NW; ++ww) s += red[(ww * NR + c8 + j) * 64 + m];
          o[j] = s * sx * ws[n0 + c8 + j];
        }
      }
      if (EPI == DS_EPI_SLABS) {
        float* p = (float*)Yv + ((long)slice * M + row) * ldy + n0 + c8;
        *reinterpret_cast<f32x4*>(p) = f32x4{o[0], o[1], o[2], o[3]};
        *reinterpret_cast<f32x4*>(p + 4) = f32x4{o[4], o[5], o[6], o[7]};
      } else {
        const int ncol = (EPI == DS_EPI_SILU) ? (n0 / 2 + c8) : (n0 + c8);
        *reinterpret_cast<uint4*>((bf16*)Yv + (long)row * ldy + ncol) = pack8(o);
      }
    }
    __syncthreads();
  }
}

template <int FMT, int MT, int NTF>
static int dense_stream_launch(const void* Xq, int ldx, const float* xs, const void* Wq, const void* We,
                               const float* ws, void* Y, int ldy, int M, int N, int K, int epi, int S,
                               hipStream_t stream) {
  const dim3 grid(N / (16 * NTF), S), block(DS_NW * 64);
  const size_t lds = (size_t)DS_NW * 16 * NTF * 64 * sizeof(float);
  const unsigned char *x = (const unsigned char*)Xq, *wq = (const unsigned char*)Wq, *we = (const unsigned char*)We;
#define DS_GO(EPI_)                                                                                          \
  if constexpr (FMT == DS_MXFP4)                                                                             \
    hipLaunchKernelGGL((dense_stream_kernel<FMT, MT, NTF, EPI_, ds_exps>), grid, block, lds, stream, x, ldx, \
                       xs, wq, we, ws, Y, ldy, M, N, K, K / S);                                              \
  else                                                                                                       \
    hipLaunchKernelGGL((dense_stream_kernel<FMT, MT, NTF, EPI_>), grid, block, lds, stream, x, ldx, xs, wq,  \
                       ws, Y, ldy, M, N, K, K / S)
  if (epi == DS_EPI_SILU) {
    DS_GO(DS_EPI_SILU);
  } else if (epi == DS_EPI_BF16) {
    DS_GO(DS_EPI_BF16);
  } else {
    DS_GO(DS_EPI_SLABS);
  }
#undef DS_GO
  PENNY_RETURN_LAUNCH();
}

// The contract of both entry points (checked, hipErrorInvalidValue, nothing launched), then the row-tile
// dispatch.  CHUNK = the columns of one wave step, 128 (fp8) or 256 (MXFP4): 1 <= M <= 256; K % CHUNK == 0;
// ntf 2 or 4, N % (16 ntf) == 0; ldx % 16 == 0, ldx >= K; ldy % 8 == 0 (bf16) / % 4 == 0 (f32) and >= the
// output width; Xq, xs, Wq, ws, Y non-null; Xq, Wq, Y 16-byte aligned; S == 1 for SILU / BF16, 1 <= S <= 16
// with K % (CHUNK S) == 0 for SLABS.  MXFP4 alone: We non-null, ldx < 2^23, and xs, We, ws 16-byte aligned
// too.  fp8 passes no We.
template <int FMT>
static int dense_stream_gemm(const void* Xq, int ldx, const float* xs, const void* Wq, const void* We,
                             const float* ws, void* Y, int ldy, int M, int N, int K, int epi, int S, int ntf,
                             hipStream_t stream) {
  constexpr int CHUNK = FMT == DS_MXFP4 ? 256 : 128;
  const int bad = (int)hipErrorInvalidValue;
  if (M < 1 || M > 256 || N <= 0 || K <= 0 || K % CHUNK) return bad;
  if (!Xq || !xs || !Wq || !ws || !Y) return bad;
  if ((ntf != 2 && ntf != 4) || N % (16 * ntf)) return bad;
  if (ldx % 16 || ldx < K) return bad;
  if (((uintptr_t)Xq | (uintptr_t)Wq | (uintptr_t)Y) & 15) return bad;
  if constexpr (FMT == DS_MXFP4) {
    if (!We || ldx >= (1 << 23)) return bad;  // 256 ldx: the kernel's 32-bit lane offsets
    if (((uintptr_t)xs | (uintptr_t)We | (uintptr_t)ws) & 15) return bad;
  }
  if (epi == DS_EPI_SLABS) {
    if (S < 1 || S > DS_MAX_S || K % (CHUNK * S) || ldy % 4 || ldy < N) return bad;
  } else if (epi == DS_EPI_SILU || epi == DS_EPI_BF16) {
    if (S != 1 || ldy % 8 || ldy < (epi == DS_EPI_SILU ? N / 2 : N)) return bad;
  } else {
    return bad;
  }
  const int mt = (M + 15) / 16;
  // Row-tile steps: fp8 1, 2, 4, 8, 16; MXFP4 also 12, and no 16 x 4: 256 accumulator registers beside the W
  // buffers and the X ring spilled 60-100 registers to scratch in every form tried (see the header), so MXFP4
  // ntf = 4 above 192 rows runs as 32-row groups on twice the workgroups: the same arithmetic per output
  // element, bit for bit.
#define DS_CASE(MT_)                                                                                          \
  if (mt <= MT_) {                                                                                            \
    if constexpr (FMT == DS_FP8 || MT_ < 16) {                                                                \
      if (ntf == 4)                                                                                           \
        return dense_stream_launch<FMT, MT_, 4>(Xq, ldx, xs, Wq, We, ws, Y, ldy, M, N, K, epi, S, stream);    \
    }                                                                                                         \
    return dense_stream_launch<FMT, MT_, 2>(Xq, ldx, xs, Wq, We, ws, Y, ldy, M, N, K, epi, S, stream);        \
  }
  DS_CASE(1) DS_CASE(2) DS_CASE(4) DS_CASE(8)
  if constexpr (FMT == DS_MXFP4) {
    DS_CASE(12)
  }
  DS_CASE(16)
#undef DS_CASE
  return bad;
}

// Xq [M, K] e4m3 (row stride ldx bytes), xs [M] f32 row scales, ws [N] f32 row scales of the weight, which
// is Wq [N, K] e4m3 row-major (fp8) or Wc [N, K/2] e2m1 pairs + We [N, K/32] E8M0 (MXFP4).
//   epi 1 SILU:  Y bf16 [M, N/2] (row stride ldy elements), W with the 16-row gate|up interleave
//   epi 2 BF16:  Y bf16 [M, N]
//   epi 3 SLABS: Y f32 [S, M, N] (row stride ldy, slab stride M * ldy), slab s = K-slice s
// ntf: 16-row weight groups per workgroup (2 or 4).  The contract: dense_stream_gemm, CHUNK = 128.
PENNY_API int penny_dense_fp8_gemm(const void* Xq, int ldx, const float* xs, const void* Wq, const float* ws, void* Y,
                                   int ldy, int M, int N, int K, int epi, int S, int ntf, hipStream_t stream) {
  return dense_stream_gemm<DS_FP8>(Xq, ldx, xs, Wq, nullptr, ws, Y, ldy, M, N, K, epi, S, ntf, stream);
}

// As penny_dense_fp8_gemm on the MXFP4 weight.  The contract: dense_stream_gemm, CHUNK = 256.
PENNY_API int penny_dense_mxfp4_gemm(const void* Xq, int ldx, const float* xs, const void* Wc, const void* We,
                                     const float* ws, void* Y, int ldy, int M, int N, int K, int epi, int S,
                                     int ntf, hipStream_t stream) {
  return dense_stream_gemm<DS_MXFP4>(Xq, ldx, xs, Wc, We, ws, Y, ldy, M, N, K, epi, S, ntf, stream);
}

// codes + exponents -> e4m3fn codes [N, K] row-major (row stride K), exactly: one lane per 32-column
// block (16 B of codes, one exponent byte, 32 B out) through a 9 x 16 table in LDS.  An exponent byte
// outside 119 .. 127 is clamped into the table (the format never holds one), so no NaN code (0x7f /
// 0xff) is ever written; -0 (code 8) becomes e4m3 -0 (0x80).
__global__ void __launch_bounds__(256) mxfp4_expand_kernel(const unsigned char* __restrict__ Wc,
                                                           const unsigned char* __restrict__ We,
                                                           unsigned char* __restrict__ out, long nblk) {
  __shared__ __attribute__((aligned(16))) unsigned char lut[9 * 16];
  if (threadIdx.x < 9 * 16) {
    const int e = (int)(threadIdx.x >> 4) - 8, code = threadIdx.x & 15, mag = code & 7;
    // e2m1 magnitude in units of 1/2: 0, 1, 2, 3, 4, 6, 8, 12;  v = units * 2^(e - 1) = units * 2^(e + 8) * 2^-9
    const int units = mag < 2 ? mag : ((2 | (mag & 1)) << ((mag >> 1) - 1));
    const int q = units << (e + 8);  // v in e4m3's subnormal step 2^-9: 0 .. 12 * 256
    int c;
    if (q < 8) {
      c = q;  // zero and the subnormals
    } else {
      const int msb = 31 - __builtin_clz(q);  // v = 1.mmm * 2^(msb - 9): at most 2 significant bits, exact
      c = ((msb - 9 + 7) << 3) | ((q >> (msb - 3)) & 7);
    }
    lut[threadIdx.x] = (unsigned char)(c | ((code & 8) << 4));
  }
  __syncthreads();
  const long i = (long)blockIdx.x * 256 + threadIdx.x;  // (row, block) in row-major order
  if (i >= nblk) return;
  const uint4 cw = *reinterpret_cast<const uint4*>(Wc + 16 * i);
  const unsigned char* row = lut + 16 * min(max((int)We[i] - 119, 0), 8);
  const unsigned cin[4] = {cw.x, cw.y, cw.z, cw.w};
  unsigned o[8];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const unsigned v = cin[j] >> (16 * hh);  // 2 bytes = 4 elements, low nibble first
      o[2 * j + hh] = (unsigned)row[v & 15] | (unsigned)row[(v >> 4) & 15] << 8 | (unsigned)row[(v >> 8) & 15] << 16 |
                      (unsigned)row[(v >> 12) & 15] << 24;
    }
  }
  uint4* dst = reinterpret_cast<uint4*>(out + 32 * i);
  dst[0] = uint4{o[0], o[1], o[2], o[3]};
  dst[1] = uint4{o[4], o[5], o[6], o[7]};
}

// Wc [N, K/2], We [N, K/32] -> out [N, K] e4m3 codes.  Contract (checked, hipErrorInvalidValue, nothing
// launched): N >= 1, K >= 32, K % 32 == 0, all three non-null, Wc and out 16-byte aligned.
PENNY_API int penny_mxfp4_expand(const void* Wc, const void* We, void* out, int N, int K, hipStream_t stream) {
  const int bad = (int)hipErrorInvalidValue;
  if (N < 1 || K < 32 || K % 32 || !Wc || !We || !out) return bad;
  if (((uintptr_t)Wc | (uintptr_t)out) & 15) return bad;
  const long nblk = (long)N * (K / 32);
  const long grid = (nblk + 255) / 256;
  if (grid > 0x7fffffffL) return bad;
  hipLaunchKernelGGL(mxfp4_expand_kernel, dim3((unsigned)grid), dim3(256), 0, stream, (const unsigned char*)Wc,
                     (const unsigned char*)We, (unsigned char*)out, nblk);
  PENNY_RETURN_LAUNCH();
}
