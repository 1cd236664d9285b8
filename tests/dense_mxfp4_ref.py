"""Host-side cases and references for the dense MXFP4 GEMM (``gemm_dense_stream.hip``,
``ops.mxfp4_dense.dense_mxfp4_gemm``), on top of ``dense_fp8_ref``: its sentinel buffers, NaN-padded X
rows, ``pow2``, ``OutBuf``, ``untouched`` and ``bits``.

The weight of a case is codes [N, K/2] (e2m1, even k in the low nibble), exps [N, K/32] (E8M0, 127 + e,
e in -8 .. 0) and ws [N].  A product of an e2m1 value, a power of two and an e4m3 value is exact in f32,
so the fp8 file's two exact families carry over:

* one-hot rows: row m of Xq is zero except a power of two at column k(m); W random -- all 16 codes, -0
  included, exponents over the full -8 .. 0;
* few-term sums: at most 4 non-zeros per row in distinct 256-column chunks (distinct K slices where the
  config has that many), integers of magnitude <= 8 in X, integers of magnitude <= 6 in W (e2m1 values
  times a block scale of 1 or 1/2): |sum| <= 192 < 2^9.

``w_values`` unpacks a weight without the code under test; every case carries the e4m3 codes of the same
values (``wq``: the conversion is checked to be exact), so ``exact_product``, ``expected``, ``emulate``
and ``reference_f64`` are ``dense_fp8_ref``'s, applied to the unpacked values.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Tuple

import torch

import dense_fp8_ref as D
from dense_fp8_ref import (NAN_CODE, SENTINEL, XPAD_COLS, XPAD_ROWS, OutBuf, bits, codes_of, out_buffer, pow2, result,  # noqa: F401
                           untouched, values_of)

E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0])
CHUNK = 256


def required_columns(K: int, S: int) -> List[int]:
    """The columns k(m) the one-hot cases must hit: every column of the first and the last 256-column
    chunk (both nibbles of every byte of a lane's 16, every lane group, both MFMAs of a chunk), and one
    column either side of every boundary between K slices and between the chunks the waves alternate on."""
    cols = set(range(0, CHUNK)) | set(range(K - CHUNK, K))
    for b in list(range(CHUNK, K, CHUNK)) + [s * (K // S) for s in range(1, S)]:
        cols |= {b - 1, b}
    return sorted(cols)


def pack(codes: torch.Tensor) -> torch.Tensor:
    """4-bit codes [N, K] (uint8) -> [N, K/2]: element 2j in the low nibble of byte j."""
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()


def unpack(wc: torch.Tensor) -> torch.Tensor:
    out = torch.empty((wc.shape[0], wc.shape[1] * 2), dtype=torch.uint8, device=wc.device)
    out[:, 0::2], out[:, 1::2] = wc & 15, wc >> 4
    return out


def w_values(wc: torch.Tensor, we: torch.Tensor) -> torch.Tensor:
    """f32 [N, K]: e2m1(code) * 2^(exp - 127)."""
    v = E2M1.to(wc.device)[unpack(wc).long()]
    return v * torch.exp2(we.float() - 127.0).repeat_interleave(32, dim=1)


def w_fp8(wc: torch.Tensor, we: torch.Tensor) -> torch.Tensor:
    """The e4m3 codes of the same values (exact for exponents -8 .. 0: asserted)."""
    v = w_values(wc, we)
    q = v.to(D.FP8)
    assert torch.equal(q.float(), v), "e2m1 * 2^e not exact in e4m3"
    return q.view(torch.uint8)


def all_codes_and_exponents() -> Tuple[torch.Tensor, torch.Tensor]:
    """A [9 * 16, 32] weight: row 16 b + c holds code c in every even column (beside every other code in the
    odd ones) at exponent -b.  Returns (codes [144, 16], exps [144, 1])."""
    codes = torch.empty((144, 32), dtype=torch.uint8)
    for b in range(9):
        for c in range(16):
            codes[16 * b + c, 0::2] = c
            codes[16 * b + c, 1::2] = torch.arange(16, dtype=torch.uint8)
    exps = (127 - torch.arange(9).repeat_interleave(16)).to(torch.uint8)[:, None]
    return pack(codes), exps.contiguous()


class Case(NamedTuple):
    M: int
    N: int
    K: int
    xq: torch.Tensor          # uint8 [M + XPAD_ROWS, K + XPAD_COLS]; rows >= M and columns >= K are NaN codes
    xs: torch.Tensor          # f32 [>= M + XPAD_ROWS] (16-byte aligned); rows >= M NaN
    wc: torch.Tensor          # uint8 [N, K/2]
    we: torch.Tensor          # uint8 [N, K/32]
    ws: torch.Tensor          # f32 [N]
    wq: torch.Tensor          # uint8 [N, K]: the e4m3 codes of the unpacked weight (for the references)

    def to(self, dev) -> "Case":
        return Case(self.M, self.N, self.K, *(t.to(dev) for t in (self.xq, self.xs, self.wc, self.we, self.ws, self.wq)))

    def x_view(self) -> torch.Tensor:
        return self.xq[:, :self.K]

    def fp8(self) -> D.Case:
        """The same case for ``dense_fp8_ref``'s references (and the fp8 kernel)."""
        return D.Case(self.M, self.N, self.K, self.xq, self.xs, self.wq, self.ws)


def _xs_rows(M: int) -> int:
    return (M + XPAD_ROWS + 3) // 4 * 4          # whole 16-byte groups: xs of every call stays aligned


def _wrap(M, N, K, x, xs, wc, we, ws) -> Case:
    xq = torch.full((M + XPAD_ROWS, K + XPAD_COLS), NAN_CODE, dtype=torch.uint8)
    xq[:M, :K] = x
    xsf = torch.full((_xs_rows(M),), float("nan"), dtype=torch.float32)
    xsf[:M] = xs
    return Case(M, N, K, xq, xsf, wc.contiguous(), we.contiguous(), ws.contiguous(), w_fp8(wc, we))


def random_w(N: int, K: int, g: torch.Generator, dev="cpu") -> Tuple[torch.Tensor, torch.Tensor]:
    """Random codes (all 16, -0 included) and random exponents over the full -8 .. 0."""
    wc = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.int32, device=dev).to(torch.uint8)
    we = torch.randint(119, 128, (N, K // 32), generator=g, dtype=torch.int32, device=dev).to(torch.uint8)
    return wc, we


def int_w(N: int, K: int, g: torch.Generator, dev="cpu") -> Tuple[torch.Tensor, torch.Tensor]:
    """Integer weights of magnitude <= 6: blocks at scale 1 hold 0, 1, 2, 3, 4, 6, blocks at scale 1/2 the
    codes of 2, 4, 6 (values 1, 2, 3), either sign."""
    we = torch.randint(126, 128, (N, K // 32), generator=g, dtype=torch.int32, device=dev).to(torch.uint8)
    full = torch.tensor([0, 2, 4, 5, 6, 7], dtype=torch.uint8, device=dev)       # 0 1 2 3 4 6
    half = torch.tensor([0, 4, 6, 7], dtype=torch.uint8, device=dev)             # 0 2 4 6, times 1/2
    a = full[torch.randint(0, 6, (N, K), generator=g, device=dev)]
    b = half[torch.randint(0, 4, (N, K), generator=g, device=dev)]
    mag = torch.where(we.repeat_interleave(32, dim=1) == 127, a, b)
    sign = torch.randint(0, 2, (N, K), generator=g, device=dev).to(torch.uint8) << 3
    return pack(mag | sign), we


def onehot_cases(M: int, N: int, K: int, S: int, seed: int, dev="cpu",
                 w: Optional[Tuple[torch.Tensor, torch.Tensor]] = None) -> List[Case]:
    """The one-hot calls that together hit every column of :func:`required_columns` (K, S): call c, row m
    has +-2^a (a in -2 .. 2) at the (c M + m)-th required column (wrapping round).  Built at once and moved
    to ``dev`` once; the cases are views sharing W (``w``: codes and exponents already on ``dev``) and ws."""
    g = torch.Generator().manual_seed(seed)
    cols = required_columns(K, S)
    C = -(-len(cols) // M)
    idx = torch.tensor((cols * (M + 1))[:C * M]).view(C, M)
    val = pow2((C, M), -2, 2, g) * (1.0 - 2.0 * torch.randint(0, 2, (C, M), generator=g).float())
    xq = torch.full((C, M + XPAD_ROWS, K + XPAD_COLS), NAN_CODE, dtype=torch.uint8)
    xq[:, :M, :K] = 0
    xq[torch.arange(C)[:, None], torch.arange(M)[None, :], idx] = codes_of(val)
    xs = torch.full((C, _xs_rows(M)), float("nan"), dtype=torch.float32)
    xs[:, :M] = pow2((C, M), -3, 3, g)
    wc, we = random_w(N, K, g) if w is None else w
    ws = pow2((N,), -3, 3, g)
    xq, xs, wc, we, ws = xq.to(dev), xs.to(dev), wc.to(dev).contiguous(), we.to(dev).contiguous(), ws.to(dev)
    wq = w_fp8(wc, we)
    return [Case(M, N, K, xq[c], xs[c], wc, we, ws, wq) for c in range(C)]


def few_term_case(M: int, N: int, K: int, S: int, seed: int, w: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                  silu: bool = False) -> Case:
    """Row m: up to 4 integers (1 .. 8, either sign) in distinct 256-column chunks -- spread over the K
    slices first -- and integer W (:func:`int_w`).  ``silu``: scales that put the gate values in SiLU's
    curved range."""
    g = torch.Generator().manual_seed(seed)
    nch = K // CHUNK
    J = min(4, nch)
    per = nch // S                                   # chunks per slice
    x = torch.zeros((M, K), dtype=torch.float32)
    for m in range(M):
        order = torch.randperm(S, generator=g).tolist()
        chunks: List[int] = []
        while len(chunks) < J:                       # round-robin over the slices, a fresh chunk each time
            for s in order:
                c = s * per + int(torch.randint(0, per, (1,), generator=g))
                if c not in chunks and len(chunks) < J:
                    chunks.append(c)
        for c in chunks:
            k = c * CHUNK + int(torch.randint(0, CHUNK, (1,), generator=g))
            v = int(torch.randint(1, 9, (1,), generator=g)) * (1 if int(torch.randint(0, 2, (1,), generator=g)) else -1)
            x[m, k] = v
    wc, we = int_w(N, K, torch.Generator().manual_seed(seed + 1)) if w is None else w
    lo, hi = (-4, -2) if silu else (-3, 3)
    xs, ws = pow2((M,), lo, hi, g), pow2((N,), -2 if silu else -3, 0 if silu else 3, g)
    dev = wc.device
    case = _wrap(M, N, K, codes_of(x), xs, wc.cpu(), we.cpu(), ws) if dev.type == "cpu" else None
    if case is None:                                 # W already on the device: move the rest there
        xq = torch.full((M + XPAD_ROWS, K + XPAD_COLS), NAN_CODE, dtype=torch.uint8)
        xq[:M, :K] = codes_of(x)
        xsf = torch.full((_xs_rows(M),), float("nan"), dtype=torch.float32)
        xsf[:M] = xs
        case = Case(M, N, K, xq.to(dev), xsf.to(dev), wc, we, ws.to(dev), w_fp8(wc, we))
    return case


def random_case(M: int, N: int, K: int, seed: int) -> Case:
    """N(0, 1) activations rounded to e4m3, random W codes and exponents, random positive f32 scales."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((M, K), generator=g).clamp(-400, 400).to(D.FP8).view(torch.uint8)
    wc, we = random_w(N, K, g)
    xs = torch.rand((M,), generator=g) * 0.02 + 0.001
    ws = torch.rand((N,), generator=g) * 0.02 + 0.001
    return _wrap(M, N, K, x, xs, wc, we, ws)


# expectations: dense_fp8_ref's, on the unpacked values
def exact_product(case: Case, S: int) -> torch.Tensor:
    return D.exact_product(case.fp8(), S)


def expected(case: Case, epilogue: str, S: int, silu_mul) -> torch.Tensor:
    return D.expected(case.fp8(), epilogue, S, silu_mul)


def emulate(case: Case, epilogue: str, S: int, silu_mul) -> torch.Tensor:
    return D.emulate(case.fp8(), epilogue, S, silu_mul)


def reference_f64(case: Case, epilogue: str, S: int) -> D.F64Ref:
    return D.reference_f64(case.fp8(), epilogue, S)


def table_splits(N: int, K: int) -> List[Tuple[int, int]]:
    """(S, ntf) of every table entry for (N, K) in ``ops.mxfp4_dense.DENSE_MXFP4`` (the default config
    where the shape has none), plus S = 1."""
    from financial_chatbot_llm_amd.ops.mxfp4_dense import DENSE_MXFP4, _default_config
    rows = [(S, ntf) for _, S, ntf in DENSE_MXFP4.get((N, K), ())]
    if not rows and _default_config(N, K) is not None:
        rows = [_default_config(N, K)]
    out = []
    for S, ntf in rows:
        for c in ((S, ntf), (1, ntf)):
            if c not in out:
                out.append(c)
    return out
