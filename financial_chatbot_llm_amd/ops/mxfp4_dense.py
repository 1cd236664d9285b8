"""MXFP4 weights for the dense Llama MLP: gate|up and down as W4A8 GEMMs.

The format -- one contract for the quantiser, the kernels and every oracle.  A weight ``W[N, K]``
(K a multiple of 32) is three tensors:

* ``codes`` uint8 ``[N, K/2]``: OCP e2m1 (magnitudes 0, 0.5, 1, 1.5, 2, 3, 4, 6; bit 3 the sign);
  element ``k = 2j`` in the low nibble of byte j, ``k = 2j + 1`` in the high nibble;
* ``exps`` uint8 ``[N, K/32]``: E8M0, ``127 + e`` with the block exponent e restricted to -8 .. 0;
* ``ws`` f32 ``[N]``: the row scale;  ``w[n, k] ~= ws[n] * 2^e[n, k/32] * e2m1(code[n, k])``.

With e in -8 .. 0 every ``e2m1 * 2^e`` is an e4m3fn value (down to 2^-9, up to 6), so the 4-bit
weight expands to e4m3 codes with the same row scale and no error (``expand_mxfp4``), and every fp8
kernel computes on the expansion the same mathematical product as the 4-bit kernel.

Activations, accumulation and epilogues are ``ops/fp8_dense.py``'s: dynamic per-row e4m3
(``penny_quant_rows_fp8``), f32 accumulation, ``xs[m] * ws[n]`` in the epilogue, gate and up rounded
to bf16 once before ``silu_mul(interleave16=True)``, down rounded to bf16 once or left as unreduced
f32 :class:`~.gemm.Slabs`.

``mlp_mxfp4`` takes, on the GPU: "stream" -- up to 256 rows, ``penny_dense_mxfp4_gemm``
(``csrc/kernels/gemm_dense_stream.hip``) reads the codes; "expand" -- above that (or where K is a
multiple of 128 and not of 256), each projection is expanded into a persistent e4m3 scratch
(``penny_mxfp4_expand``) and ``mlp_fp8`` runs on a :class:`~.fp8_dense.DenseFp8MLP` view of it;
"torch" -- CPU tensors and whatever neither accepts, in the kernels' operation order.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple, Union

import torch

from . import _native as N
from . import fp8_dense
from .fp8_dense import DenseFp8MLP, EPI, MAX_M, MAX_S, _quant, dense_fp8_reference, mlp_fp8
from .gemm import Slabs

CHUNK = 256            # columns of one wave step: two 16x16x128 MFMAs
E_MIN, E_MAX = -8, 0   # block exponents the format holds (every e2m1 * 2^e an e4m3 value)
E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
FP8 = torch.float8_e4m3fn

_LUT: Dict[torch.device, torch.Tensor] = {}


def _lut(dev: torch.device) -> torch.Tensor:
    t = _LUT.get(dev)
    if t is None:
        t = _LUT[dev] = torch.tensor(list(E2M1) + [-v for v in E2M1], dtype=torch.float32, device=dev)
    return t


class DenseMxfp4MLP:
    """One layer's quantised MLP: ``gate_up_c`` [2F, H/2] / ``gate_up_e`` [2F, H/32] / ``gate_up_s`` [2F]
    (16-row gate|up interleave) and ``down_c`` [H, F/2] / ``down_e`` [H, F/32] / ``down_s`` [H].
    ``scratch``: the e4m3 expansion buffer of the "expand" path, shared by all layers of a model."""

    __slots__ = ("gate_up_c", "gate_up_e", "gate_up_s", "down_c", "down_e", "down_s", "scratch")

    def __init__(self, gate_up_c, gate_up_e, gate_up_s, down_c, down_e, down_s, scratch: Optional["ExpandScratch"] = None):
        self.gate_up_c, self.gate_up_e, self.gate_up_s = gate_up_c, gate_up_e, gate_up_s
        self.down_c, self.down_e, self.down_s = down_c, down_e, down_s
        self.scratch = scratch

    @property
    def H(self) -> int:
        return self.down_c.shape[0]

    @property
    def F(self) -> int:
        return self.down_c.shape[1] * 2

    def named_tensors(self) -> Dict[str, torch.Tensor]:
        """Weight-dict key suffix -> tensor, in the constructor's order."""
        return {"gate_up_c": self.gate_up_c, "gate_up_e": self.gate_up_e, "gate_up_scale": self.gate_up_s,
                "down_c": self.down_c, "down_e": self.down_e, "down_scale": self.down_s}

    def tensors(self) -> Tuple[torch.Tensor, ...]:
        return tuple(self.named_tensors().values())

    def num_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.tensors())


class ExpandScratch:
    """One layer's e4m3 MLP (3 F H bytes) for the "expand" path: allocated once per model when it is
    quantised (before the KV pool is sized), overwritten by every layer's call."""

    __slots__ = ("gate_up", "down")

    def __init__(self, H: int, F_: int, device):
        self.gate_up = torch.empty((2 * F_, H), dtype=FP8, device=device)
        self.down = torch.empty((H, F_), dtype=FP8, device=device)

    def num_bytes(self) -> int:
        return self.gate_up.numel() + self.down.numel()


# ---------------------------------------------------------------------------------------------
# quantiser, unpack, expand
# ---------------------------------------------------------------------------------------------
def pack_codes(codes: torch.Tensor) -> torch.Tensor:
    """[N, K] 4-bit codes (uint8) -> [N, K/2]: even k in the low nibble."""
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).contiguous()


def unpack_codes(packed: torch.Tensor) -> torch.Tensor:
    """[N, K/2] -> [N, K] 4-bit codes."""
    return torch.stack((packed & 15, packed >> 4), dim=-1).reshape(packed.shape[0], -1)


def _pow2_f64(e: torch.Tensor) -> torch.Tensor:
    """2^e as f64 from the exponent field: exact on every device (a device exp2 need not be)."""
    return ((e.to(torch.int64) + 1023) << 52).view(torch.float64)


def _quantize_rows(w: torch.Tensor, row_amax: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """No device division or exp2 (neither need be correctly rounded on a GPU): f64 products of an f32 scale,
    a power of two and a 3-bit threshold are exact, so the CPU and the GPU give the same bits."""
    Nr, K = w.shape
    wf = w.double()                                            # bf16 / f32 values, exact
    amax = wf.abs().amax(dim=1) if row_amax is None else row_amax.double()
    ws = torch.where(amax > 0, (amax * (1.0 / 6.0)).float(), torch.ones_like(amax, dtype=torch.float32))
    top = 6.0 * ws.double()                                    # exact: the value a block amax is compared with
    blk = wf.view(Nr, K // 32, 32)
    bmax = blk.abs().amax(dim=2)
    # the smallest e with bmax <= top * 2^e, from the mantissas and exponents (no log2: exact at the boundary)
    mb, eb = torch.frexp(bmax)
    mt, et = torch.frexp(top)
    e = (eb - et[:, None]) + (mb > mt[:, None]).to(eb.dtype)
    e = torch.where(bmax > 0, e, torch.full_like(e, E_MIN)).clamp(E_MIN, E_MAX)
    a = blk.abs()
    t = (ws.double()[:, None] * _pow2_f64(e))[:, :, None]      # the block's unit: |w| / t is rounded to e2m1
    # round to nearest e2m1, ties to the even code; everything above 5 saturates at 6 (code 7)
    code = ((a > 0.25 * t).to(torch.uint8) + (a >= 0.75 * t).to(torch.uint8) + (a > 1.25 * t).to(torch.uint8)
            + (a >= 1.75 * t).to(torch.uint8) + (a > 2.5 * t).to(torch.uint8) + (a >= 3.5 * t).to(torch.uint8)
            + (a > 5.0 * t).to(torch.uint8))
    code = code | (((blk < 0) & (code > 0)).to(torch.uint8) << 3)          # -0 is never produced
    return pack_codes(code.view(Nr, K)), (e + 127).to(torch.uint8).contiguous(), ws.contiguous()


def quantize_mxfp4_rowwise(w: torch.Tensor, rows_per_pass: int = 2048,
                           row_amax: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``w`` [N, K] (K a multiple of 32) -> (codes [N, K/2] uint8, exps [N, K/32] uint8, ws [N] f32), on
    ``w``'s device.  ``ws[n] = amax_n / 6`` (1 for an all-zero row); per 32-block the smallest e in -8 .. 0
    with ``amax_block <= 6 ws 2^e`` (an all-zero block: -8); the code is the nearest e2m1 value of
    ``w / (ws 2^e)``, ties to the even code, saturating at +-6.  Run once at load, ``rows_per_pass`` rows
    at a time (the f64 intermediates of a 70B projection would not fit otherwise).

    ``row_amax`` [N]: the amax of the whole rows where ``w`` holds a column shard of them (``down`` under
    tensor parallelism: the maximum over the ranks' shards).  The 32-blocks of a shard are blocks of the whole
    row, so with the whole row's scale a shard gets exactly the codes and exponents the unsharded weight has
    in those columns; it must be >= the shard's own amax, which would otherwise saturate."""
    if w.dim() != 2 or w.shape[1] % 32 or w.shape[1] == 0:
        raise ValueError(f"quantize_mxfp4_rowwise: [N, K] with K a multiple of 32, got {tuple(w.shape)}")
    if row_amax is not None:
        if row_amax.shape != (w.shape[0],):
            raise ValueError(f"quantize_mxfp4_rowwise: row_amax {tuple(row_amax.shape)} for {w.shape[0]} rows")
        if w.numel() and bool((row_amax.double() < w.double().abs().amax(dim=1)).any()):
            raise ValueError("quantize_mxfp4_rowwise: row_amax below a row's own amax")
    parts = [_quantize_rows(w[i:i + rows_per_pass], None if row_amax is None else row_amax[i:i + rows_per_pass])
             for i in range(0, w.shape[0], rows_per_pass)]
    if not parts:
        dev = w.device
        return (torch.empty((0, w.shape[1] // 2), dtype=torch.uint8, device=dev),
                torch.empty((0, w.shape[1] // 32), dtype=torch.uint8, device=dev), torch.empty(0, dtype=torch.float32, device=dev))
    return tuple(torch.cat([p[i] for p in parts]) for i in range(3))


def quantize_dense_mlp_mxfp4(gate_up: torch.Tensor, down: torch.Tensor, scratch: Optional[ExpandScratch] = None,
                             down_row_amax: Optional[torch.Tensor] = None) -> DenseMxfp4MLP:
    """bf16 ``gate_up`` [2F, H] (interleave16, as the model shards it) and ``down`` [H, F] ->
    :class:`DenseMxfp4MLP`.  Row-wise, so the interleave is untouched.  ``down_row_amax``: the whole rows'
    amax where ``down`` is a column shard (see :func:`quantize_mxfp4_rowwise`)."""
    if (gate_up.dim() != 2 or down.dim() != 2 or gate_up.shape[0] != 2 * down.shape[1] or gate_up.shape[1] != down.shape[0]
            or gate_up.shape[1] % 32 or down.shape[1] % 32):
        raise ValueError(f"gate_up {tuple(gate_up.shape)} / down {tuple(down.shape)} are no [2F, H] / [H, F] pair "
                         "with H and F multiples of 32")
    return DenseMxfp4MLP(*quantize_mxfp4_rowwise(gate_up), *quantize_mxfp4_rowwise(down, row_amax=down_row_amax),
                         scratch=scratch)


def unpack_mxfp4(codes: torch.Tensor, exps: torch.Tensor) -> torch.Tensor:
    """(codes [N, K/2], exps [N, K/32]) -> f32 [N, K]: ``e2m1(code) * 2^(exp - 127)``, without ``ws``."""
    v = _lut(codes.device)[unpack_codes(codes).long()]
    sc = (exps.to(torch.int32).clamp_min(1) << 23).view(torch.float32)      # an E8M0 byte is an f32 exponent field
    return (v.view(v.shape[0], -1, 32) * sc[:, :, None]).view(v.shape[0], -1)


def expand_mxfp4(codes: torch.Tensor, exps: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The weight as e4m3fn codes [N, K] (exact for exponents -8 .. 0): ``penny_mxfp4_expand`` on the GPU,
    torch on the CPU, bit-equal.  ``out``: a contiguous [N, K] one-byte tensor to write into."""
    Nr, K = codes.shape[0], codes.shape[1] * 2
    if exps.shape != (Nr, K // 32) or not codes.is_contiguous() or not exps.is_contiguous():
        raise ValueError("expand_mxfp4: contiguous codes [N, K/2] and exps [N, K/32]")
    if out is None:
        out = torch.empty((Nr, K), dtype=FP8, device=codes.device)
    elif out.shape != (Nr, K) or out.element_size() != 1 or not out.is_contiguous():
        raise ValueError("expand_mxfp4: out must be a contiguous one-byte [N, K] tensor")
    if Nr == 0:
        return out
    if N.use_native(codes):
        N.call("penny_mxfp4_expand", N.ptr(codes), N.ptr(exps), N.ptr(out), Nr, K, N.stream())
    else:
        e = exps.clamp(127 + E_MIN, 127 + E_MAX)               # as the kernel: the table has no other row
        out.view(torch.uint8).copy_(unpack_mxfp4(codes, e).to(FP8).view(torch.uint8))
    return out


# ---------------------------------------------------------------------------------------------
# the streaming kernel
# ---------------------------------------------------------------------------------------------
# (N, K) -> [(max M, S, ntf), ...] for penny_dense_mxfp4_gemm, shaped like fp8_dense.DENSE_FP8: S K-slices
# (slabs only; SiLU and bf16 outputs run S = 1), 16 * ntf weight rows per workgroup, grid = N / (16 ntf) x S.
# Chosen from bench/kernels.py --only dense_mxfp4_sweep (profiles/dense_mxfp4_sweep.jsonl): per shape and row band
# (1-16, 64-256) the candidate with the smallest summed time relative to each row count's best; the chosen configs
# against bf16 and fp8: --only dense_mxfp4_mlp (profiles/dense_mxfp4_mlp.jsonl).  Shapes without an entry take
# ``_default_config``.
DENSE_MXFP4: fp8_dense.Table = {
    # Llama-3-8B
    (28672, 4096): [(256, 1, 4)],                    # gate|up: 448 workgroups
    (4096, 14336): [(16, 2, 2), (256, 4, 4)],        # down: 128 x 2 to 16 rows, 64 x 4 above
    # Llama-3-70B TP=1
    (57344, 8192): [(16, 1, 2), (256, 1, 4)],        # gate|up: 32-row groups to 16 rows, 64-row groups above
    (8192, 28672): [(16, 2, 2), (256, 2, 4)],        # down: 256 x 2 to 16 rows, 128 x 2 above
    # Llama-3-70B TP=8 per-rank shards: 32-row groups
    (7168, 8192): [(256, 1, 2)],
    (8192, 3584): [(256, 1, 2)],
}


def _default_config(N_: int, K: int) -> Optional[Tuple[int, int]]:
    """(S, ntf) for an unmeasured shape: 32-row groups, K slices until the grid covers the 256 CUs."""
    return fp8_dense._default_config(N_, K, CHUNK)


def dense_mxfp4_config(M: int, N_: int, K: int, epilogue: str) -> Optional[Tuple[int, int]]:
    """(S, ntf) for the streaming kernel at this shape and epilogue, or None where its contract
    (1 <= M <= 256, K % (256 S) == 0, N % (16 ntf) == 0) does not hold."""
    if K <= 0:
        return None
    return fp8_dense._config(DENSE_MXFP4, CHUNK, M, N_, K, epilogue)


def dense_mxfp4_gemm(xq: torch.Tensor, xs: torch.Tensor, wc: torch.Tensor, we: torch.Tensor, ws: torch.Tensor,
                     epilogue: str, S: int = 1, ntf: int = 2, out: Optional[torch.Tensor] = None,
                     M: Optional[int] = None) -> torch.Tensor:
    """``penny_dense_mxfp4_gemm``: ``xq`` [M, K] e4m3 codes (row stride a multiple of 16), ``xs`` [M],
    ``wc`` [N, K/2] / ``we`` [N, K/32] / ``ws`` [N] -> "silu": bf16 [M, N/2]; "bf16": [M, N]; "slabs": f32
    [S, M, N].  ``out`` / ``M`` as :func:`~.fp8_dense.dense_fp8_gemm`.  The kernel's contract violations
    raise (``hipErrorInvalidValue``) before anything is launched."""
    M = xq.shape[0] if M is None else M
    K = xq.shape[1]
    N_ = wc.shape[0]
    if (wc.shape[1] * 2 != K or we.shape != (N_, K // 32) or not wc.is_contiguous() or not we.is_contiguous()
            or xq.stride(1) != 1):
        raise ValueError("dense_mxfp4_gemm: wc [N, K/2] and we [N, K/32] contiguous, xq rows contiguous")
    if out is None:
        out = fp8_dense._alloc_out(xq, M, N_, epilogue, S)
    N.call("penny_dense_mxfp4_gemm", N.ptr(xq), xq.stride(0), N.ptr(xs), N.ptr(wc), N.ptr(we), N.ptr(ws), N.ptr(out),
           out.stride(-2), M, N_, K, EPI[epilogue], S, ntf, N.stream())
    return out


# ---------------------------------------------------------------------------------------------
# the MLP
# ---------------------------------------------------------------------------------------------
def _stream_ok(M: int, w: DenseMxfp4MLP) -> bool:
    return fp8_dense._stream_ok(M, w, dense_mxfp4_config)


def _expanded(w: DenseMxfp4MLP, fill: bool) -> DenseFp8MLP:
    """The :class:`DenseFp8MLP` view of the scratch + the row scales; ``fill``: expand this layer into it."""
    sc = w.scratch
    if sc is None or sc.gate_up.device != w.gate_up_c.device or sc.gate_up.shape != (2 * w.F, w.H):
        sc = w.scratch = ExpandScratch(w.H, w.F, w.gate_up_c.device)
    if fill:
        expand_mxfp4(w.gate_up_c, w.gate_up_e, out=sc.gate_up)
        expand_mxfp4(w.down_c, w.down_e, out=sc.down)
    return DenseFp8MLP(sc.gate_up, w.gate_up_s, sc.down, w.down_s)


def mlp_mxfp4_path(h: torch.Tensor, w: DenseMxfp4MLP) -> str:
    """Which path :func:`mlp_mxfp4` takes for ``h``: "stream" | "expand" | "torch"."""
    M = h.shape[0]
    if N.use_native(h) and h.dtype == torch.bfloat16 and M > 0:
        if _stream_ok(M, w):
            return "stream"
        if fp8_dense._stream_ok(M, w) or fp8_dense._tiles_ok(M, w):     # the fp8 kernels' own rules (H and F only)
            return "expand"
    return "torch"


def mlp_mxfp4(h: torch.Tensor, w: DenseMxfp4MLP, slabs: bool = False) -> Tuple[Union[torch.Tensor, Slabs], torch.Tensor]:
    """The MXFP4 MLP of ``h`` [M, H] bf16 -> (down output, bf16 intermediate ``a`` [M, F]), as
    :func:`~.fp8_dense.mlp_fp8`: bf16 [M, H], or with ``slabs`` at decode sizes the unreduced f32
    :class:`~.gemm.Slabs` of the down GEMM."""
    path = mlp_mxfp4_path(h, w)
    if path == "torch":
        return _mlp_torch(h, w)
    if path == "expand":
        # the expansion is exact, so the fp8 kernels (streaming or tiles, by mlp_fp8's own rules) compute the
        # product of the same weights
        return mlp_fp8(h, _expanded(w, fill=True), slabs=slabs)
    if h.stride(1) != 1 or h.stride(0) % 8:
        h = h.contiguous()
    return fp8_dense._mlp_stream(h, slabs, dense_mxfp4_config, dense_mxfp4_gemm,
                                 (w.gate_up_c, w.gate_up_e, w.gate_up_s), (w.down_c, w.down_e, w.down_s))


def _as_fp8(w: DenseMxfp4MLP) -> DenseFp8MLP:
    """A fresh :class:`DenseFp8MLP` holding the exact expansion (oracles and the torch path)."""
    return DenseFp8MLP(expand_mxfp4(w.gate_up_c, w.gate_up_e), w.gate_up_s, expand_mxfp4(w.down_c, w.down_e), w.down_s)


def _mlp_torch(h: torch.Tensor, w: DenseMxfp4MLP) -> Tuple[torch.Tensor, torch.Tensor]:
    """The kernels' operation order in torch: ``fp8_dense._mlp_torch`` on the unpacked weights."""
    return fp8_dense._mlp_torch(h, _as_fp8(w))


def dense_mxfp4_reference(h: torch.Tensor, w: DenseMxfp4MLP, quant_act: bool = True) -> torch.Tensor:
    """fp32 reference of the MXFP4 MLP, quantising for itself: :func:`~.fp8_dense.dense_fp8_reference` on
    the unpacked weights.  ``quant_act=False`` keeps the activations unquantised (the weight-only error)."""
    return dense_fp8_reference(h, _as_fp8(w), quant_act=quant_act)
