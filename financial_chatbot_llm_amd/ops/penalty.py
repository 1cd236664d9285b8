"""Repetition, presence and frequency penalties (``csrc/kernels/penalty.hip``).

:class:`PenaltyTable` is the device table of token counts, one row ("slot") per penalised sequence:
``[slots, Vs]`` int16 with ``Vs`` = V rounded up to 8; bit 15 of an entry says the token occurs in the
slot's prompt, bits 0-14 count how often the sequence has emitted it (at most 32767).
:func:`reset` hands a slot to a new sequence, :func:`add` counts emitted tokens and
:func:`apply_penalties` rewrites a step's logits in front of the sampler.  Per logit ``l`` of a row
with ``slot >= 0``, in f32 and in this order::

    c    = count (+ 1 where the token is the row's pending token)
    seen = c > 0 or the prompt bit
    q    = (l / rep if l > 0 else l * rep) if seen and rep != 1 else l
    pen  = fma(freq, float(c), pres if c > 0 else 0)
    l'   = q - pen, rounded once to the logits' dtype

Repetition covers prompt and output, presence and frequency the output only.  A row with ``rep = 1,
pres = 0, freq = 0`` and every row with ``slot < 0`` keep their bits.  CPU tensors take the torch path
below: the same operations in the same order, except that torch does not fuse the ``fma``.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _native as N
from .sampling import _aligned_rows

MAX_COUNT = 0x7FFF
PROMPT_BIT = -0x8000           # bit 15 of an int16 entry


class PenaltyTable:
    """``slots`` rows of token counts over a ``V``-token vocabulary, zero-initialised."""

    def __init__(self, slots: int, V: int, device):
        if slots <= 0 or V <= 0:
            raise ValueError(f"penalty table of {slots} slots x {V} tokens")
        self.slots, self.V, self.Vs = int(slots), int(V), (int(V) + 7) // 8 * 8
        self.device = torch.device(device)
        self.table = torch.zeros((self.slots, self.Vs), dtype=torch.int16, device=self.device)

    def _native(self) -> bool:
        return N.use_native(self.table)


def _ids(x, device) -> torch.Tensor:
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x, np.int32)))
    return x.to(device=device, dtype=torch.int32).contiguous()


def reset(t: PenaltyTable, slot: int, prompt_ids) -> None:
    """Zero ``slot``'s row and set the prompt bit of every id of ``prompt_ids`` (a sequence of ints or
    an integer tensor; duplicates are fine)."""
    if not 0 <= int(slot) < t.slots:
        raise ValueError(f"slot {slot} outside the table's {t.slots}")
    ids = _ids(prompt_ids, t.device).reshape(-1)
    if t._native():
        N.call("penny_pen_reset", N.ptr(t.table), t.slots, t.V, t.Vs, int(slot), N.ptr(ids), ids.numel(), N.stream())
        return
    if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= t.V):
        raise ValueError("prompt id outside the vocabulary")
    row = t.table[int(slot)]
    row.zero_()
    row[ids.long()] = PROMPT_BIT


def add(t: PenaltyTable, pairs) -> None:
    """count[slot, token] += 1 for every (slot, token) row of ``pairs`` [n, 2]; duplicates within one
    call all land."""
    pairs = _ids(pairs, t.device).reshape(-1, 2)
    n = pairs.shape[0]
    if n == 0:
        return
    if t._native():
        N.call("penny_pen_add", N.ptr(t.table), t.slots, t.V, t.Vs, N.ptr(pairs), n, N.stream())
        return
    s, v = pairs[:, 0].long(), pairs[:, 1].long()
    if int(s.min()) < 0 or int(s.max()) >= t.slots or int(v.min()) < 0 or int(v.max()) >= t.V:
        raise ValueError("(slot, token) pair outside the table")
    # int32 accumulation, then back: bit 15 and the neighbours stay as they are
    flat = t.table.view(-1)
    idx, cnt = torch.unique(s * t.Vs + v, return_counts=True)
    flat[idx] = (flat[idx].to(torch.int32) + cnt.to(torch.int32)).to(torch.int16)


def _apply_ref(logits: torch.Tensor, slot: torch.Tensor, pending_tok: torch.Tensor, rep: torch.Tensor,
               pres: torch.Tensor, freq: torch.Tensor, t: PenaltyTable) -> torch.Tensor:
    S, V = logits.shape
    slot = slot.long()
    on = slot >= 0
    rows = t.table[slot.clamp(min=0)][:, :V].to(torch.int32)
    c = rows & MAX_COUNT
    pend = pending_tok.long()
    hit = (pend >= 0) & (pend < V)
    c[torch.nonzero(hit).reshape(-1), pend[hit]] += 1
    seen = (c > 0) | ((rows & 0x8000) != 0)
    l = logits.float()
    rep, pres, freq = (x.float().reshape(S, 1) for x in (rep, pres, freq))
    q = torch.where(seen & (rep != 1), torch.where(l > 0, l / rep, l * rep), l)
    pen = freq * c.float() + torch.where(c > 0, pres, torch.zeros_like(pres))
    res = (q - pen).to(logits.dtype)
    neutral = ~on | ((rep == 1) & (pres == 0) & (freq == 0)).reshape(S)
    return torch.where(neutral.reshape(S, 1), logits, res)


def apply_penalties(logits: torch.Tensor, slot: torch.Tensor, pending_tok: torch.Tensor, rep: torch.Tensor,
                    pres: torch.Tensor, freq: torch.Tensor, table: PenaltyTable,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Penalise ``logits`` [S, V] (bf16 or f32) row by row: ``slot`` [S] int32 names each row's table
    row (< 0: the row is left alone), ``pending_tok`` [S] int32 a token that counts as one more
    occurrence for this call only (< 0: none; the table is never written), ``rep`` / ``pres`` /
    ``freq`` [S] f32 the row's parameters.  In place, or into ``out`` (rows with ``slot < 0`` are
    copied through) leaving ``logits`` as it was; returns the penalised tensor.  The slots of one
    call's rows must be distinct from each other."""
    S, V = logits.shape
    if V != table.V:
        raise ValueError(f"logits of {V} columns, penalty table for {table.V}")
    if logits.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"apply_penalties takes bf16 or f32 logits, not {logits.dtype}")
    if out is not None and (out.shape != logits.shape or out.dtype != logits.dtype):
        raise ValueError("out must match the logits' shape and dtype")
    for x in (slot, pending_tok, rep, pres, freq):
        if x.shape != (S,):
            raise ValueError(f"per-row argument of shape {tuple(x.shape)}, expected ({S},)")
    if not N.use_native(logits):
        res = _apply_ref(logits, slot, pending_tok, rep, pres, freq, table)
        dst = logits if out is None else out
        dst.copy_(res)
        return dst
    i32 = lambda x: x.to(torch.int32).contiguous()         # noqa: E731
    f32 = lambda x: x.to(torch.float32).contiguous()       # noqa: E731
    slot, pending_tok, rep, pres, freq = i32(slot), i32(pending_tok), f32(rep), f32(pres), f32(freq)
    src = _aligned_rows(logits)
    dst = out
    if out is not None and not (out.stride(1) == 1 and out.stride(0) == src.stride(0) and out.data_ptr() % 16 == 0):
        dst = torch.empty_strided(src.shape, src.stride(), dtype=src.dtype, device=src.device)
    N.call("penny_pen_apply", N.ptr(src), int(src.dtype == torch.float32), src.stride(0), N.ptr(slot),
           N.ptr(pending_tok), N.ptr(rep), N.ptr(pres), N.ptr(freq), N.ptr(table.table), table.slots, table.Vs,
           N.ptr(dst), S, V, N.stream())
    if out is None:
        if src is not logits:            # the rows went through the aligned copy: bring them back
            logits.copy_(src)
        return logits
    if dst is not out:
        out.copy_(dst)
    return out
