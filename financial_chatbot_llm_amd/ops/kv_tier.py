"""Whole KV blocks between the paged pool and a dense staging buffer (``csrc/kernels/kv_tier.hip``).

The pool is ``KVCache.buf`` ``[L, 2, num_blocks, Hkv, 64*D]`` (bf16 or fp8 bytes), or any contiguous
``[planes, num_blocks, ...]`` tensor; seen as bytes it is ``planes`` planes of ``num_blocks`` chunks of
``plane_bytes`` bytes.  ``staging`` is a contiguous uint8 ``[cap, planes, plane_bytes]`` tensor on the
pool's device and ``ids`` ``n <= cap`` int32 block ids::

    gather_blocks    staging[i, p, :] = pool[p, ids[i], :]      i < n; rows >= n keep their bytes
    scatter_blocks   pool[p, ids[i], :] = staging[i, p, :]      every other block keeps its bytes

An id outside ``[0, num_blocks)`` is skipped in both directions.  The bytes are moved as they are: bf16
and fp8 pools need nothing special.  CPU tensors take the torch path below (``index_select`` /
``index_copy_``), the oracle of the kernels' tests.
"""
from __future__ import annotations

from typing import Sequence, Union

import torch

from . import _native as N


def pool_planes(kv_buf: torch.Tensor) -> torch.Tensor:
    """``kv_buf`` as a uint8 ``[planes, num_blocks, plane_bytes]`` view (no copy)."""
    if not kv_buf.is_contiguous():
        raise ValueError("the KV pool must be contiguous")
    if kv_buf.dim() == 5:
        L, two, nb = kv_buf.shape[:3]
        planes = L * two
    elif kv_buf.dim() >= 3:
        planes, nb = kv_buf.shape[:2]
    else:
        raise ValueError(f"KV pool of shape {tuple(kv_buf.shape)}: expected [L, 2, num_blocks, Hkv, 64*D] or "
                         "[planes, num_blocks, ...]")
    b = kv_buf.reshape(planes, nb, -1)
    b = b if b.dtype == torch.uint8 else b.view(torch.uint8)
    if b.shape[2] % 16:
        raise ValueError(f"plane_bytes = {b.shape[2]} is not a multiple of 16")
    return b


def _check(kv_buf: torch.Tensor, ids: Union[torch.Tensor, Sequence[int]], staging: torch.Tensor):
    pool = pool_planes(kv_buf)
    if not torch.is_tensor(ids):
        ids = torch.tensor(list(ids), dtype=torch.int32, device=pool.device)
    ids = ids.to(torch.int32).contiguous()
    planes, _, pb = pool.shape
    if staging.dtype != torch.uint8 or staging.dim() != 3 or not staging.is_contiguous() \
            or tuple(staging.shape[1:]) != (planes, pb):
        raise ValueError(f"staging {tuple(staging.shape)} {staging.dtype}: expected contiguous uint8 "
                         f"[cap, {planes}, {pb}]")
    if ids.dim() != 1 or ids.numel() > staging.shape[0]:
        raise ValueError(f"{tuple(ids.shape)} block ids for a staging buffer of {staging.shape[0]} blocks")
    if ids.device != pool.device or staging.device != pool.device:
        raise ValueError(f"pool on {pool.device}, ids on {ids.device}, staging on {staging.device}: the kernels "
                         "see one device's memory only")
    return pool, ids, staging


def _valid_rows(pool: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    return torch.nonzero((ids >= 0) & (ids < pool.shape[1])).reshape(-1)


def gather_blocks(kv_buf: torch.Tensor, ids, staging: torch.Tensor) -> torch.Tensor:
    """``staging[i, p, :] = pool[p, ids[i], :]`` (module docstring); returns ``staging``."""
    pool, ids, staging = _check(kv_buf, ids, staging)
    n = ids.numel()
    if n == 0:
        return staging
    if not N.use_native(pool):
        rows = _valid_rows(pool, ids)
        staging[rows] = pool.index_select(1, ids[rows].long()).transpose(0, 1)
        return staging
    N.call("penny_kv_gather_blocks", N.ptr(pool), pool.stride(0), pool.shape[2], pool.shape[0], pool.shape[1],
           N.ptr(ids), n, N.ptr(staging), N.stream())
    return staging


def scatter_blocks(kv_buf: torch.Tensor, ids, staging: torch.Tensor) -> torch.Tensor:
    """``pool[p, ids[i], :] = staging[i, p, :]`` (module docstring); returns ``kv_buf``."""
    pool, ids, staging = _check(kv_buf, ids, staging)
    n = ids.numel()
    if n == 0:
        return kv_buf
    if not N.use_native(pool):
        rows = _valid_rows(pool, ids)
        pool.index_copy_(1, ids[rows].long(), staging[rows].transpose(0, 1))
        return kv_buf
    N.call("penny_kv_scatter_blocks", N.ptr(pool), pool.stride(0), pool.shape[2], pool.shape[0], pool.shape[1],
           N.ptr(ids), n, N.ptr(staging), N.stream())
    return kv_buf
