"""Multi-LoRA: per-row low-rank deltas on a shared base projection (``csrc/kernels/lora.hip``).

:class:`LoRATable` holds ``slots`` adapters for the projection groups of a Llama decoder.  A group is
one input ``x`` and the projections that read it: ``"qkv"`` (``q_proj``, ``k_proj``, ``v_proj``: three
column segments of the fused QKV output), ``"o"`` (``o_proj``) and ``"down"`` (``down_proj``).  Per
group and layer the table keeps, zero-padded to the table rank ``R`` (a multiple of 32)::

    A       [L, slots, nseg * R, K]   the segments' lora_A matrices stacked
    B       [L, slots, N, R]          the segments' lora_B matrices stacked (rows = output columns)
    present [L, slots] int32          bit g: the slot's adapter targets segment g
    scale   [slots] f32               lora_alpha / r

:func:`lora_delta` adds the delta to a step's projection output, for a row ``m`` with slot
``a = row_slot[m]`` in ``[0, slots)``::

    t[m, :] = round_to_x_dtype( sum_k x[m, k] * A_a[:, k] )            f32 accumulation, ONE rounding
    y[m, n] = base[m, n] + scale_a * sum_j t[m, g R + j] * B_a[n, j]   n in segment g; f32, scale in f32

``base`` is a bf16 ``[M, N]`` tensor rewritten in place (``float(base) + delta`` in f32, then one
round-to-nearest-even) or slab 0 of a split-K GEMM's f32 :class:`~.gemm.Slabs` (the f32 delta is
added; the consumer's slab sum does the rest).  Rows with another slot value (``-1``: the base model),
and the segments an adapter does not target, keep every bit.  A row's bits do not depend on the step
size, its position or its batch mates.  CPU tensors take the torch path below: the same operations in
the same order (on f32 tensors the rounding of ``t`` is the identity), the numerics reference.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional, Sequence, Tuple, Union

import torch

from . import _native as N
from .gemm import Slabs

GROUPS: Dict[str, Tuple[str, ...]] = {"qkv": ("q_proj", "k_proj", "v_proj"), "o": ("o_proj",),
                                      "down": ("down_proj",)}
MODULE_GROUP = {m: (g, i) for g, ms in GROUPS.items() for i, m in enumerate(ms)}
MAX_RANK = 64
K_GRAIN = 128          # the shrink kernel's k per wave: K is a multiple of it
K_SLAB = 512           # k per shrink workgroup: ceil(K / K_SLAB) partial slabs, a function of K alone


def padded_rank(rank: int) -> int:
    """The table rank for adapters of at most ``rank``: the 16x16x32 MFMA's k step."""
    if not 1 <= int(rank) <= MAX_RANK:
        raise ValueError(f"LoRA rank {rank} outside 1..{MAX_RANK}")
    return (int(rank) + 31) // 32 * 32


class _Group:
    def __init__(self, layers: int, slots: int, R: int, seg_sizes: Sequence[int], K: int, device, dtype):
        self.seg_sizes = tuple(int(s) for s in seg_sizes)
        if not 1 <= len(self.seg_sizes) <= 3 or any(s <= 0 or s % 16 for s in self.seg_sizes) or K <= 0 or K % K_GRAIN:
            raise ValueError(f"LoRA group of segments {self.seg_sizes} x K = {K}: segments must be multiples of 16 "
                             f"columns (at most 3) and K a multiple of {K_GRAIN}")
        self.nseg, self.K, self.N = len(self.seg_sizes), int(K), sum(self.seg_sizes)
        ends, e = [], 0
        for s in self.seg_sizes:
            e += s
            ends.append(e)
        self.seg_end = tuple(ends)
        self.c_seg_end = (ctypes.c_int * self.nseg)(*ends)
        self.A = torch.zeros((layers, slots, self.nseg * R, self.K), dtype=dtype, device=device)
        self.B = torch.zeros((layers, slots, self.N, R), dtype=dtype, device=device)
        self.present = torch.zeros((layers, slots), dtype=torch.int32, device=device)
        self.scale = torch.zeros((slots,), dtype=torch.float32, device=device)

    def num_bytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self.A, self.B, self.present, self.scale))


class LoRATable:
    """``slots`` adapters of rank <= ``rank`` over ``layers`` layers.  ``shapes`` maps each group name to
    ``(segment sizes, K)``: the output columns of its projections and their shared input width."""

    def __init__(self, slots: int, rank: int, layers: int, shapes: Dict[str, Tuple[Sequence[int], int]], device,
                 dtype=torch.bfloat16):
        if slots <= 0 or layers <= 0:
            raise ValueError(f"LoRA table of {slots} slots x {layers} layers")
        self.slots, self.layers, self.rank, self.R = int(slots), int(layers), int(rank), padded_rank(rank)
        self.device, self.dtype = torch.device(device), dtype
        self.groups: Dict[str, _Group] = {g: _Group(layers, slots, self.R, segs, K, device, dtype)
                                          for g, (segs, K) in shapes.items()}

    def num_bytes(self) -> int:
        return sum(g.num_bytes() for g in self.groups.values())

    def bytes_per_slot(self) -> int:
        return self.num_bytes() // self.slots

    def _check_slot(self, slot: int) -> int:
        if not 0 <= int(slot) < self.slots:
            raise ValueError(f"slot {slot} outside the table's {self.slots}")
        return int(slot)

    def clear(self, slot: int) -> None:
        slot = self._check_slot(slot)
        for g in self.groups.values():
            g.A[:, slot].zero_()
            g.B[:, slot].zero_()
            g.present[:, slot].zero_()
            g.scale[slot] = 0.0

    def set(self, slot: int, layer_tensors: Dict[Tuple[int, str], Tuple[torch.Tensor, torch.Tensor]],
            scale: float) -> None:
        """Replace ``slot`` by the adapter ``{(layer, module): (lora_A [r, K], lora_B [n, r])}`` with
        ``scale`` = lora_alpha / r; modules it does not name are absent (their columns keep their bits)."""
        slot = self._check_slot(slot)
        for (layer, module), (a, b) in layer_tensors.items():      # everything is checked before a write
            if module not in MODULE_GROUP or MODULE_GROUP[module][0] not in self.groups:
                raise ValueError(f"LoRA target {module!r} is not supported")
            if not 0 <= layer < self.layers:
                raise ValueError(f"layer {layer} outside the model's {self.layers}")
            g, i = MODULE_GROUP[module]
            G = self.groups[g]
            r = a.shape[0]
            if a.dim() != 2 or b.dim() != 2 or not 1 <= r <= self.R or r > self.rank:
                raise ValueError(f"layers.{layer}.{module}: rank {r} above the table's {self.rank}")
            if tuple(a.shape) != (r, G.K) or tuple(b.shape) != (G.seg_sizes[i], r):
                raise ValueError(f"layers.{layer}.{module}: lora_A {tuple(a.shape)} / lora_B {tuple(b.shape)} do not "
                                 f"fit a [{G.seg_sizes[i]}, {G.K}] projection")
            if not (bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all())):
                raise ValueError(f"layers.{layer}.{module}: non-finite adapter weights")
        self.clear(slot)
        R = self.R
        for (layer, module), (a, b) in layer_tensors.items():
            g, i = MODULE_GROUP[module]
            G = self.groups[g]
            r = a.shape[0]
            n0 = G.seg_end[i] - G.seg_sizes[i]
            G.A[layer, slot, i * R:i * R + r].copy_(a.to(self.dtype))
            G.B[layer, slot, n0:G.seg_end[i], :r].copy_(b.to(self.dtype))
            G.present[layer, slot] |= 1 << i
        for G in self.groups.values():
            G.scale[slot] = float(scale)


def _target(out_or_slabs: Union[torch.Tensor, Slabs]) -> torch.Tensor:
    t = out_or_slabs.P[0] if isinstance(out_or_slabs, Slabs) else out_or_slabs
    if t.dim() != 2:
        raise ValueError(f"lora_delta target of shape {tuple(t.shape)}")
    return t


def _delta_ref(x: torch.Tensor, out: torch.Tensor, G: _Group, R: int, layer: int, row_slot: torch.Tensor,
               slots: int) -> None:
    rs = row_slot.long()
    rs = torch.where((rs >= 0) & (rs < slots), rs, torch.full_like(rs, -1))
    for s in torch.unique(rs).tolist():
        if s < 0:
            continue
        rows = torch.nonzero(rs == s).reshape(-1)
        t = (x[rows].float() @ G.A[layer, s].float().t()).to(x.dtype).float()
        pres, scale = int(G.present[layer, s]), G.scale[s]
        for g in range(G.nseg):
            if not (pres >> g) & 1:
                continue
            n0, n1 = G.seg_end[g] - G.seg_sizes[g], G.seg_end[g]
            delta = scale * (t[:, g * R:(g + 1) * R] @ G.B[layer, s, n0:n1].float().t())
            out[rows, n0:n1] = (out[rows, n0:n1].float() + delta).to(out.dtype)


def lora_delta(x: torch.Tensor, out_or_slabs: Union[torch.Tensor, Slabs], table: LoRATable, layer: int, group: str,
               row_slot: torch.Tensor) -> Union[torch.Tensor, Slabs]:
    """Add the rows' adapter deltas of projection ``group`` of ``layer`` to its output (module
    docstring), in place: the shrink, then the expand.  ``x`` [M, K], ``row_slot`` [M] int32."""
    G = table.groups[group]
    out = _target(out_or_slabs)
    M, K = x.shape
    if K != G.K or tuple(out.shape) != (M, G.N):
        raise ValueError(f"lora_delta({group}): x {tuple(x.shape)} / output {tuple(out.shape)} against a "
                         f"[{G.N}, {G.K}] projection")
    if row_slot.shape != (M,):
        raise ValueError(f"row_slot of shape {tuple(row_slot.shape)}, expected ({M},)")
    if not 0 <= layer < table.layers:
        raise ValueError(f"layer {layer} outside the table's {table.layers}")
    if M == 0:
        return out_or_slabs
    if not N.use_native(x):
        _delta_ref(x, out, G, table.R, layer, row_slot, table.slots)
        return out_or_slabs
    if x.dtype != torch.bfloat16 or table.dtype != torch.bfloat16 or out.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError(f"lora_delta takes bf16 x and tables and a bf16 or f32 output, not {x.dtype} / {out.dtype}")
    if out.stride(1) != 1:
        raise ValueError("lora_delta writes its output in place: its rows must be contiguous")
    if x.stride(1) != 1 or x.stride(0) % 8 or x.data_ptr() % 16:
        x = x.contiguous()
    row_slot = row_slot.to(torch.int32).contiguous()
    C = G.nseg * table.R
    S = (K + K_SLAB - 1) // K_SLAB
    part = torch.empty((S, M, C), dtype=torch.float32, device=x.device)
    st = N.stream()
    N.call("penny_lora_shrink", N.ptr(x), x.stride(0), N.ptr(row_slot), N.ptr(G.A[layer]), table.slots, G.nseg, table.R,
           N.ptr(part), M, K, st)
    N.call("penny_lora_expand", N.ptr(part), S, N.ptr(row_slot), N.ptr(G.B[layer]), N.ptr(G.present[layer]),
           N.ptr(G.scale), table.slots, G.c_seg_end, G.nseg, table.R, N.ptr(out), int(out.dtype == torch.float32),
           out.stride(0), M, G.N, st)
    return out_or_slabs
