"""fp8 e4m3 (OCP) weights for the dense Llama MLP: gate|up and down as W8A8 GEMMs.

One fp8 contract with the Mixtral experts (``ops/moe.py``):

* weights: e4m3fn codes with one f32 scale per output row (``quantize_fp8_rowwise``), made once
  from the rank's own bf16 shard; gate|up keeps its 16-row interleave;
* activations: dynamic per-row e4m3 (``penny_quant_rows_fp8``, scale = amax / 448) in front of each
  of the two GEMMs;
* f32 accumulation, dequantised in the epilogue by ``xs[m] * ws[n]``; gate and up rounded to bf16
  once, then ``silu_mul(interleave16=True)``; down rounded to bf16 once, or left as unreduced f32
  split-K :class:`~.gemm.Slabs` for ``ops.rms_norm``.

``mlp_fp8`` takes, on the GPU: up to 256 rows the weight-streaming kernel of
``csrc/kernels/gemm_dense_stream.hip`` (``penny_dense_fp8_gemm``), above that the grouped fp8 tile GEMM
of ``gemm_prefill.hip`` with a single bucket; shapes outside both kernels' contracts, and CPU
tensors, take the torch path (same operation order).  One copy of each weight: both kernels read
the row-major ``[N, K]`` codes.

The streaming kernel has a second weight format (``ops/mxfp4_dense.py``); what the two share on the host
is written here once and takes the format's table, chunk width and functions: ``_config``,
``_default_config``, ``_alloc_out``, ``_stream_ok`` and ``_mlp_stream``.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Tuple, Union

import torch

from . import _native as N
from .activation import silu_mul
from .gemm import Slabs
from .moe import _fake_quant_rows, moe_fp8_reference, quantize_fp8_rowwise, TILE_SCHED

EPI = {"silu": 1, "bf16": 2, "slabs": 3}
MAX_M = 256            # the streaming kernel's row range (ops.gemm.linear's decode-size steps)
MAX_S = 16             # K slices the kernel supports (slabs only)
CHUNK = 128            # columns of one wave step: two pairs of 16x16x32 MFMAs
Table = Dict[Tuple[int, int], List[Tuple[int, int, int]]]


class DenseFp8MLP:
    """One layer's quantised MLP: ``gate_up_q`` [2F, H] e4m3 (16-row gate|up interleave) with
    ``gate_up_s`` [2F] f32, ``down_q`` [H, F] e4m3 with ``down_s`` [H] f32 (row-major, one copy)."""

    __slots__ = ("gate_up_q", "gate_up_s", "down_q", "down_s")

    def __init__(self, gate_up_q, gate_up_s, down_q, down_s):
        self.gate_up_q, self.gate_up_s, self.down_q, self.down_s = gate_up_q, gate_up_s, down_q, down_s

    @property
    def H(self) -> int:
        return self.down_q.shape[0]

    @property
    def F(self) -> int:
        return self.down_q.shape[1]

    def named_tensors(self) -> Dict[str, torch.Tensor]:
        """Weight-dict key suffix -> tensor, in the constructor's order."""
        return {"gate_up_q": self.gate_up_q, "gate_up_scale": self.gate_up_s, "down_q": self.down_q, "down_scale": self.down_s}

    def tensors(self) -> Tuple[torch.Tensor, ...]:
        return tuple(self.named_tensors().values())

    def num_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in self.tensors())


def quantize_dense_mlp(gate_up: torch.Tensor, down: torch.Tensor) -> DenseFp8MLP:
    """bf16 ``gate_up`` [2F, H] (interleave16, as the model shards it) and ``down`` [H, F] ->
    :class:`DenseFp8MLP`.  Row-wise, so the interleave is untouched."""
    if gate_up.dim() != 2 or down.dim() != 2 or gate_up.shape[0] != 2 * down.shape[1] or gate_up.shape[1] != down.shape[0]:
        raise ValueError(f"gate_up {tuple(gate_up.shape)} / down {tuple(down.shape)} are no [2F, H] / [H, F] pair")
    gq, gs = quantize_fp8_rowwise(gate_up)
    dq, ds = quantize_fp8_rowwise(down)
    return DenseFp8MLP(gq.contiguous(), gs.float().contiguous(), dq.contiguous(), ds.float().contiguous())


# (N, K) -> [(max M, S, ntf), ...] for penny_dense_fp8_gemm: S K-slices (the slab epilogue; SiLU and
# bf16 outputs always run S = 1, their K split is the workgroup's four waves), 16 * ntf weight rows per
# workgroup.  Grid = N / (16 ntf) x S workgroups.  Chosen from the interleaved candidate sweep of
# bench/kernels.py --only dense_fp8_sweep at M = 1, 16, 64, 128, 256 (profiles/dense_fp8_sweep.jsonl);
# the chosen configs against bf16: --only dense_fp8_mlp (profiles/dense_fp8_mlp.jsonl).  64-row groups
# halve the activation bytes a workgroup pulls from L2 per weight byte and win wherever the grid still
# covers the CUs (8B gate|up at 128 rows: 63 vs 85 us); the narrow TP=8 shards keep 32-row groups.
# Shapes without an entry take ``_default_config``.
DENSE_FP8: Table = {
    # Llama-3-8B (profiles/dense_fp8_sweep.jsonl)
    (28672, 4096): [(256, 1, 4)],                    # gate|up: 448 workgroups; 28.5 us at 1 row, 63 at 128
    (4096, 14336): [(16, 8, 4), (256, 4, 4)],        # down: 64 x 8 to 16 rows (12.9-14.3 us), 64 x 4 above
    # Llama-3-70B TP=1 (profiles/dense_fp8_sweep.jsonl)
    (57344, 8192): [(256, 1, 4)],                    # gate|up: 896 workgroups; 100 us at 1 row, 220 at 128
    (8192, 28672): [(16, 4, 4), (256, 2, 4)],        # down: 128 x 4 to 16 rows (48 us), 128 x 2 above
    # Llama-3-70B TP=8 per-rank shards (profiles/dense_fp8_sweep.jsonl): 32-row groups, 22-26 % ahead of 64
    (7168, 8192): [(256, 1, 2)],                     # gate|up shard: 224 workgroups
    (8192, 3584): [(256, 1, 2)],                     # down shard (bf16 into the all-reduce): 256 workgroups
}


def _default_config(N_: int, K: int, chunk: int = CHUNK) -> Optional[Tuple[int, int]]:
    """(S, ntf) for an unmeasured shape: 32-row groups, K slices until the grid covers the 256 CUs."""
    if N_ % 32 or K % chunk:
        return None
    S = 1
    while S < 8 and (N_ // 32) * S < 256 and K % (2 * chunk * S) == 0:
        S *= 2
    return S, 2


def _config(table: Table, chunk: int, M: int, N_: int, K: int, epilogue: str) -> Optional[Tuple[int, int]]:
    """(S, ntf) of a streaming kernel with ``chunk``-column wave steps from its ``table``, or None where its
    contract (1 <= M <= 256, K % (chunk S) == 0, N % (16 ntf) == 0) does not hold."""
    if not 1 <= M <= MAX_M or K % chunk:
        return None
    cfg = None
    for max_m, S, ntf in table.get((N_, K), ()):
        if M <= max_m:
            cfg = (S, ntf)
            break
    if cfg is None:
        cfg = _default_config(N_, K, chunk)
    if cfg is None:
        return None
    S, ntf = cfg
    if epilogue != "slabs":
        S = 1
    if N_ % (16 * ntf) or K % (chunk * S) or not 1 <= S <= MAX_S:
        return None
    return S, ntf


def dense_fp8_config(M: int, N_: int, K: int, epilogue: str) -> Optional[Tuple[int, int]]:
    """(S, ntf) for the streaming kernel at this shape and epilogue, or None where its contract
    (1 <= M <= 256, K % (128 S) == 0, N % (16 ntf) == 0) does not hold."""
    return _config(DENSE_FP8, CHUNK, M, N_, K, epilogue)


def _alloc_out(xq: torch.Tensor, M: int, N_: int, epilogue: str, S: int) -> torch.Tensor:
    """The output of one streaming GEMM: "slabs" f32 [S, M, N]; "silu" bf16 [M, N/2]; "bf16" [M, N]."""
    if epilogue == "slabs":
        return torch.empty((S, M, N_), dtype=torch.float32, device=xq.device)
    return torch.empty((M, N_ // 2 if epilogue == "silu" else N_), dtype=torch.bfloat16, device=xq.device)


def dense_fp8_gemm(xq: torch.Tensor, xs: torch.Tensor, wq: torch.Tensor, ws: torch.Tensor, epilogue: str,
                   S: int = 1, ntf: int = 2, out: Optional[torch.Tensor] = None, M: Optional[int] = None) -> torch.Tensor:
    """``penny_dense_fp8_gemm``: ``xq`` [M, K] e4m3 codes (row stride a multiple of 16), ``xs`` [M],
    ``wq`` [N, K] e4m3 row-major, ``ws`` [N] -> "silu": bf16 [M, N/2]; "bf16": [M, N]; "slabs": f32
    [S, M, N].  ``out``: the output buffer (its row stride is passed on; slabs: [S, M, >= N] with
    slab stride M rows).  ``M``: rows to compute where ``xq`` / ``out`` hold more.  The kernel's
    contract violations raise (``hipErrorInvalidValue``) before anything is launched."""
    M = xq.shape[0] if M is None else M
    K = xq.shape[1]
    N_ = wq.shape[0]
    if wq.shape[1] != K or not wq.is_contiguous() or xq.stride(1) != 1:
        raise ValueError("dense_fp8_gemm: wq must be contiguous [N, K], xq rows contiguous")
    if out is None:
        out = _alloc_out(xq, M, N_, epilogue, S)
    N.call("penny_dense_fp8_gemm", N.ptr(xq), xq.stride(0), N.ptr(xs), N.ptr(wq), N.ptr(ws), N.ptr(out),
           out.stride(-2), M, N_, K, EPI[epilogue], S, ntf, N.stream())
    return out


def _quant(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    M, K = x.shape
    q = torch.empty((M, K), dtype=torch.uint8, device=x.device)
    s = torch.empty(M, dtype=torch.float32, device=x.device)
    N.call("penny_quant_rows_fp8", N.ptr(x), x.stride(0), M, K, N.ptr(q), N.ptr(s), N.stream())
    return q, s


_BUCKETS: Dict[Tuple[torch.device, int], torch.Tensor] = {}
_ONES: Dict[torch.device, torch.Tensor] = {}


def _bucket(dev: torch.device, M: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The tile GEMM's single bucket: device offsets [0, M] and unit routing weights (made once per M)."""
    off = _BUCKETS.get((dev, M))
    if off is None:
        off = _BUCKETS[(dev, M)] = torch.tensor([0, M], dtype=torch.int32, device=dev)
    ones = _ONES.get(dev)
    if ones is None or ones.numel() < M:
        ones = _ONES[dev] = torch.ones(max(M, 4096), dtype=torch.float32, device=dev)
    return off, ones


def _stream_ok(M: int, w, config: Callable = dense_fp8_config) -> bool:
    """Both GEMMs of ``w`` (anything with ``H`` and ``F``) are in the contract of ``config``'s streaming kernel."""
    H, F_ = w.H, w.F
    return config(M, 2 * F_, H, "silu") is not None and config(M, H, F_, "slabs") is not None


def _mlp_stream(h: torch.Tensor, slabs: bool, config: Callable, gemm: Callable, gate_up: Tuple[torch.Tensor, ...],
                down: Tuple[torch.Tensor, ...]) -> Tuple[Union[torch.Tensor, Slabs], torch.Tensor]:
    """The streaming MLP of either format: quantise, gate|up SiLU GEMM, quantise, down GEMM as slabs or
    bf16.  ``config`` / ``gemm``: the format's ``dense_*_config`` / ``dense_*_gemm``; ``gate_up`` / ``down``:
    the weight tensors ``gemm`` takes after ``xq, xs``."""
    M, H = h.shape
    F_ = gate_up[0].shape[0] // 2
    xq, xs = _quant(h)
    _, ntf = config(M, 2 * F_, H, "silu")
    a = gemm(xq, xs, *gate_up, "silu", 1, ntf)
    aq, as_ = _quant(a)
    S, ntf = config(M, H, F_, "slabs" if slabs else "bf16")
    if slabs:
        return Slabs(gemm(aq, as_, *down, "slabs", S, ntf)), a
    return gemm(aq, as_, *down, "bf16", 1, ntf), a


def _tiles_ok(M: int, w: DenseFp8MLP) -> bool:
    H, F_ = w.H, w.F
    return M > MAX_M and H % 256 == 0 and F_ % 128 == 0      # N % 256 and K % 128 of both tile GEMMs


def mlp_fp8_path(h: torch.Tensor, w: DenseFp8MLP) -> str:
    """Which path :func:`mlp_fp8` takes for ``h``: "stream" | "tiles" | "torch"."""
    M = h.shape[0]
    if N.use_native(h) and h.dtype == torch.bfloat16 and M > 0:
        if _stream_ok(M, w):
            return "stream"
        if _tiles_ok(M, w):
            return "tiles"
    return "torch"


def mlp_fp8(h: torch.Tensor, w: DenseFp8MLP, slabs: bool = False) -> Tuple[Union[torch.Tensor, Slabs], torch.Tensor]:
    """The fp8 MLP of ``h`` [M, H] bf16 -> (down output, bf16 intermediate ``a`` [M, F]).  The output is
    bf16 [M, H], or with ``slabs`` at decode sizes the unreduced f32 :class:`~.gemm.Slabs` of the down
    GEMM.  ``a`` = silu(gate) * up is what the down GEMM's quantiser read (LoRA's down delta needs it)."""
    M, H = h.shape
    F_ = w.F
    path = mlp_fp8_path(h, w)
    if path == "torch":
        return _mlp_torch(h, w)
    if h.stride(1) != 1 or h.stride(0) % 8:
        h = h.contiguous()
    if path == "stream":
        return _mlp_stream(h, slabs, dense_fp8_config, dense_fp8_gemm, (w.gate_up_q, w.gate_up_s), (w.down_q, w.down_s))
    xq, xs = _quant(h)
    # prefill sizes: the grouped fp8 tile GEMM with one bucket [0, M) (epi 7: SiLU; epi 8: x route_w = 1)
    dev = h.device
    st = N.stream()
    offsets, ones = _bucket(dev, M)
    a = torch.empty((M, F_), dtype=torch.bfloat16, device=dev)
    N.call("penny_moe_gemm_prefill_fp8", N.ptr(xq), H, None, N.ptr(xs), N.ptr(offsets), N.ptr(w.gate_up_q),
           N.ptr(w.gate_up_s), None, N.ptr(a), F_, M, 1, 2 * F_, H, 7 + TILE_SCHED, st)
    aq, as_ = _quant(a)
    y = torch.empty((M, H), dtype=torch.bfloat16, device=dev)
    N.call("penny_moe_gemm_prefill_fp8", N.ptr(aq), F_, None, N.ptr(as_), N.ptr(offsets), N.ptr(w.down_q),
           N.ptr(w.down_s), N.ptr(ones), N.ptr(y), H, M, 1, H, F_, 8 + TILE_SCHED, st)
    return y, a


def _mlp_torch(h: torch.Tensor, w: DenseFp8MLP) -> Tuple[torch.Tensor, torch.Tensor]:
    """The kernels' operation order in torch (f32): quantise rows, GEMM, dequantise, gate|up rounded to
    bf16, ``silu_mul``, quantise rows, GEMM, dequantise, one bf16 rounding."""
    w13 = w.gate_up_q.float() * w.gate_up_s[:, None]
    w2 = w.down_q.float() * w.down_s[:, None]
    x = _fake_quant_rows(h.float())
    a = silu_mul((x @ w13.t()).to(torch.bfloat16), interleave16=True)
    y = _fake_quant_rows(a.float()) @ w2.t()
    return y.to(h.dtype), a.to(h.dtype)


def dense_fp8_reference(h: torch.Tensor, w: DenseFp8MLP, quant_act: bool = True) -> torch.Tensor:
    """fp32 reference of the fp8 MLP, quantising for itself: ``moe_fp8_reference`` with one expert and
    routing weight 1.  ``quant_act`` rounds both GEMM inputs through dynamic per-row e4m3, as the
    kernels do; False keeps the activations unquantised (the weight-only error)."""
    T = h.shape[0]
    routing = (torch.ones((T, 1), dtype=torch.float32), torch.zeros((T, 1), dtype=torch.int32))
    return moe_fp8_reference(h, None, w.gate_up_q[None], w.gate_up_s[None], w.down_q[None], w.down_s[None], 1,
                             quant_act=quant_act, routing=routing)
