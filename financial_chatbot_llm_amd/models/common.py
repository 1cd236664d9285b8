"""Shared model plumbing: attention metadata, paged KV cache, deterministic weight init."""
from __future__ import annotations

import zlib
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import torch

from ..ops.attention import FP8, KV_BS, DecodeWorkspace, KVScales


@dataclass
class AttentionMetadata:
    """Per-step batch layout: ``num_prefill_tokens`` prefill tokens first, then one token per
    decoding sequence.  All tensors live on the model's device."""

    slots: torch.Tensor                      # [T] int32 KV slot per token (-1: no write)
    num_prefill_tokens: int = 0
    cu_q: Optional[torch.Tensor] = None      # [Sp+1] int32
    ctx_lens_p: Optional[torch.Tensor] = None  # [Sp] int32 total KV length after this step
    block_tables_p: Optional[torch.Tensor] = None  # [Sp, max_blocks] int32
    max_q_len: int = 0
    num_decode: int = 0
    ctx_lens_d: Optional[torch.Tensor] = None  # [Bd]
    block_tables_d: Optional[torch.Tensor] = None
    decode_ws: Optional[DecodeWorkspace] = None
    causal: bool = True
    prefill_work: Optional[torch.Tensor] = None  # [n, 2] int32 (ops.attention.prefill_work_list) or lean [., 6]
    prefill_lean: Optional[tuple] = None          # lean list counts (items, merges, slots), host ints
    row_slot: Optional[torch.Tensor] = None       # [T] int32 LoRA table slot per row (-1: base model); None: no row has one
    lora: Optional[object] = None                 # the ops.LoRATable those slots index (None: the model's own)


class KVCache:
    """All layers' paged K/V in ONE HBM allocation: [L, 2, num_blocks, Hkv, 64*D] bf16.

    ``k(l)`` / ``v(l)`` are [num_blocks, Hkv, 64*D] tiles in MFMA-fragment-native order
    (csrc/kernels/kv_layout.h).

    ``kv_dtype="fp8"``: the pool holds OCP e4m3fn codes, one byte per element (head dim 128 only),
    with per-(layer, kv head) scales ``k_scale`` / ``v_scale`` [L, Hkv] (default 1): ``value = code *
    scale``.  ``scales(l)`` is the layer's :class:`~..ops.attention.KVScales` (None for bf16).
    """

    def __init__(self, num_layers: int, num_blocks: int, num_kv_heads: int, head_dim: int,
                 dtype=torch.bfloat16, device="cuda", kv_dtype: str = "bf16", k_scale=None, v_scale=None):
        self.num_layers, self.num_blocks = num_layers, num_blocks
        self.num_kv_heads, self.head_dim = num_kv_heads, head_dim
        if kv_dtype not in ("bf16", "fp8"):
            raise ValueError(f"unknown kv_dtype {kv_dtype!r} (bf16 | fp8)")
        self.kv_dtype = kv_dtype
        self.scale = self.inv_scale = None
        shape = (num_layers, 2, num_blocks, num_kv_heads, KV_BS * head_dim)
        if kv_dtype == "fp8":
            if head_dim != 128:
                raise ValueError(f"fp8 KV cache needs head dim 128, got {head_dim}")
            # allocated as bytes and viewed: zero bytes are the code of +0
            self.buf = torch.zeros(shape, dtype=torch.uint8, device=device).view(FP8)
            sc = torch.ones((num_layers, 2, num_kv_heads), dtype=torch.float32)
            for i, t in enumerate((k_scale, v_scale)):
                if t is not None:
                    t = torch.as_tensor(t, dtype=torch.float32).cpu()
                    if tuple(t.shape) != (num_layers, num_kv_heads):
                        raise ValueError(f"kv scales must be [{num_layers}, {num_kv_heads}], got {tuple(t.shape)}")
                    sc[:, i] = t
            if not bool((sc > 0).all()) or not bool(torch.isfinite(sc).all()):
                raise ValueError("kv scales must be positive and finite")
            self.scale = sc.to(device)                  # [L, 2, Hkv] f32
            self.inv_scale = (1.0 / sc).to(device)      # computed once, on the host
        else:
            self.buf = torch.zeros(shape, dtype=dtype, device=device)

    @property
    def is_fp8(self) -> bool:
        return self.kv_dtype == "fp8"

    @property
    def elt(self) -> int:
        return self.buf.element_size()

    def scales(self, layer: int) -> Optional[KVScales]:
        return KVScales(self.scale[layer], self.inv_scale[layer]) if self.is_fp8 else None

    def k(self, layer: int) -> torch.Tensor:
        return self.buf[layer, 0]

    def v(self, layer: int) -> torch.Tensor:
        return self.buf[layer, 1]

    @staticmethod
    def bytes_per_block(num_layers: int, num_kv_heads: int, head_dim: int, elt: int = 2) -> int:
        return num_layers * 2 * num_kv_heads * KV_BS * head_dim * elt


def param_seed(base: int, name: str) -> int:
    return (base * 1_000_003 + zlib.crc32(name.encode())) & 0x7FFFFFFF


def random_tensor(name: str, shape, seed: int, device, dtype=torch.bfloat16, std: float = 0.02,
                  kind: str = "normal") -> torch.Tensor:
    """Deterministic per-name init, identical on every rank (so TP shards agree)."""
    if kind == "ones":
        return torch.ones(shape, dtype=dtype, device=device)
    if kind == "zeros":
        return torch.zeros(shape, dtype=dtype, device=device)
    g = torch.Generator(device=device)
    g.manual_seed(param_seed(seed, name))
    t = torch.randn(shape, generator=g, device=device, dtype=torch.float32 if device == "cpu" else dtype)
    return t.mul_(std).to(dtype)
