"""Exact reference for the decode GEMM kernels (gemm_splitk.hip, gemm_skinny.hip; plain torch, no GPU).

The kernels take bf16 inputs and accumulate in f32.  With inputs that are small integers times a power
of two the reference needs no tolerance:

* x and w entries are integers in [-8, 8] times 2^-ex / 2^-ew -- all exact in bf16;
* every product and every partial sum is then an integer multiple of 2^-(ex+ew) of magnitude at most
  64 * K in those units.  ``ExactGemm`` asserts 64 * K < 2^24 for the K it is built for, so an f32
  accumulation is exact in any order, MFMA or not, and so is the f32 sum of split-K slabs;
* the integer products are computed in int64, per 64-column block (the kernels' BK = 64 stage) with
  prefix sums over the blocks: any K slice [k0, k0 + kc), any M and N prefix is then one subtraction.

Expected values: f32 slabs exact; a bf16 output is the exact value rounded once, to nearest even
(integer sums hit ties often, so this pins the tie rule too); reduce + residual is
``bf16(f32(bf16(sum)) + f32(residual))`` with the add in f32 (one IEEE add, the same on CPU and GPU);
the fused SiLU forms are ``ops.silu_mul`` of the exact bf16 gate|up (their documented contract).
"""
from __future__ import annotations

import functools
import math
from typing import Tuple

import torch

BK = 64            # columns per block: the kernels' stage width
AMAX = 8           # |integer entry| <= AMAX
MMAX, NMAX = 257, 256
KMAX = 28672       # the Llama-3-70B down projection: the largest K any decode table holds
EX, EW = 3, 4      # default scales: x = int * 2^-3, w = int * 2^-4


class ExactGemm:
    """Integer X [M, K] and W [N, K] (|entries| <= 8) with block prefix sums of X @ W.T.

    ``prefix[b]`` = X[:, :64 b] @ W[:, :64 b].T, int32 on the CPU.  ``to(device)`` gives a copy whose
    prefix is f32 on that device (exact: every entry is below 2^24)."""

    def __init__(self, X: torch.Tensor, W: torch.Tensor):
        assert X.dtype == torch.int64 and W.dtype == torch.int64 and X.shape[1] == W.shape[1]
        K = X.shape[1]
        assert K % BK == 0
        amax = int(max(X.abs().max(), W.abs().max()))
        assert amax <= AMAX
        # the exactness bound: max |integer sum| < 2^24 for the largest K used
        assert amax * amax * K < (1 << 24), f"K = {K} too deep for exact f32 accumulation"
        nb = K // BK
        M, N = X.shape[0], W.shape[0]
        self.X, self.W, self.K = X.to(torch.int8), W.to(torch.int8), K
        prefix = torch.zeros((nb + 1, M, N), dtype=torch.int32)
        acc = torch.zeros((M, N), dtype=torch.int64)
        # a 64-column block product is at most 64 * 64 in magnitude: the f64 BLAS product is exact and
        # (unlike torch's int64 matmul) takes well under a second; the sums over blocks are int64
        xb = X.view(M, nb, BK).transpose(0, 1).to(torch.float64)   # [nb, M, 64]
        wb = W.view(N, nb, BK).permute(1, 2, 0).to(torch.float64)  # [nb, 64, N]
        for b0 in range(0, nb, 32):
            blocks = torch.bmm(xb[b0:b0 + 32], wb[b0:b0 + 32]).to(torch.int64)
            cs = blocks.cumsum(0) + acc
            prefix[b0 + 1:b0 + 1 + cs.shape[0]] = cs.to(torch.int32)
            acc = cs[-1]
        assert int(prefix.abs().max()) < (1 << 24)
        self.prefix = prefix

    def to(self, device) -> "ExactGemm":
        o = object.__new__(ExactGemm)
        o.X, o.W, o.K = self.X.to(device), self.W.to(device), self.K
        o.prefix = self.prefix.to(device).to(torch.float32)
        return o

    # ---- inputs -------------------------------------------------------------------------------
    def x(self, M: int, K: int, ex: int = EX, k0: int = 0) -> torch.Tensor:
        """bf16 [M, K]: integer rows 0..M-1, columns k0..k0+K-1, times 2^-ex (exact)."""
        return (self.X[:M, k0:k0 + K].to(torch.float32) * 2.0 ** -ex).to(torch.bfloat16)

    def w(self, N: int, K: int, ew: int = EW, k0: int = 0) -> torch.Tensor:
        return (self.W[:N, k0:k0 + K].to(torch.float32) * 2.0 ** -ew).to(torch.bfloat16)

    # ---- expected outputs ---------------------------------------------------------------------
    def product(self, M: int, N: int, k0: int, kc: int) -> torch.Tensor:
        """X[:M, k0:k0+kc] @ W[:N, k0:k0+kc].T in integer units (int32 on the CPU, f32 on a device)."""
        assert k0 % BK == 0 and kc % BK == 0 and k0 + kc <= self.K
        return self.prefix[(k0 + kc) // BK, :M, :N] - self.prefix[k0 // BK, :M, :N]

    def slabs(self, M: int, N: int, K: int, S: int, e: int = EX + EW) -> torch.Tensor:
        """Exact f32 split-K slabs [S, M, N] of x(M, K, ex) @ w(N, K, ew).T with e = ex + ew."""
        assert K % (BK * S) == 0
        kc = K // S
        P = torch.stack([self.product(M, N, s * kc, kc) for s in range(S)])
        return P.to(torch.float32) * 2.0 ** -e

    def f32(self, M: int, N: int, K: int, e: int = EX + EW) -> torch.Tensor:
        return self.product(M, N, 0, K).to(torch.float32) * 2.0 ** -e

    def bf16(self, M: int, N: int, K: int, e: int = EX + EW) -> torch.Tensor:
        """The exact product rounded once to bf16 (round to nearest even)."""
        return self.f32(M, N, K, e).to(torch.bfloat16)


def add_residual(y: torch.Tensor, residual: torch.Tensor) -> torch.Tensor:
    """bf16(f32(y) + f32(residual)) for a bf16 y: the GEMM-then-add rounding of the residual epilogues."""
    assert y.dtype == torch.bfloat16 and residual.dtype == torch.bfloat16
    return (y.to(torch.float32) + residual.to(torch.float32)).to(torch.bfloat16)


def silu_exponents(K: int) -> Tuple[int, int]:
    """(ex, ew) for a gate|up GEMM of depth K: entries uniform on -8..8 have variance 24, so a gate
    value has standard deviation 24 sqrt(K) 2^-(ex+ew); this puts it in [2, 4) -- SiLU's curved range."""
    e = int(math.floor(math.log2(24.0 * math.sqrt(K)))) - 1
    return e // 2, e - e // 2


def random_ints(rows: int, K: int, seed: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-AMAX, AMAX + 1, (rows, K), generator=g, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def master(kmax: int = KMAX, M: int = MMAX, N: int = NMAX) -> ExactGemm:
    """One X [M, kmax] / W [N, kmax] pair per (session, size); every test case is a slice of it."""
    return ExactGemm(random_ints(M, kmax, 1234), random_ints(N, kmax, 4321))


def silu_mul_f64(gu: torch.Tensor, interleave16: bool) -> torch.Tensor:
    """silu(gate) * up in f64 from a bf16 gate|up [T, 2F] (no intermediate rounding)."""
    F = gu.shape[-1] // 2
    g64 = gu.to(torch.float64)
    if interleave16:
        v = g64.reshape(*gu.shape[:-1], F // 16, 2, 16)
        g, u = v[..., 0, :].reshape(*gu.shape[:-1], F), v[..., 1, :].reshape(*gu.shape[:-1], F)
    else:
        g, u = g64[..., :F], g64[..., F:]
    return g / (1.0 + torch.exp(-g)) * u
