"""Token-automaton constrained sampling (``csrc/kernels/constrain.hip`` + the MASKED sampler kernels).

:class:`FsmTables` is the device table set the engine stacks its automata into (``agent.automaton``):
byte transitions, accepting flags, per-state token masks and the tokens' bytes.  It is allocated
once at a fixed capacity, so the pointers captured in decode hipGraphs stay valid while automata are
added.  :func:`sample_constrained` is ``ops.sample`` with a state per row: disallowed tokens count
as -inf (before top-k / top-p) and the row's next state comes back beside the sampled id.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _native as N
from .sampling import SPLITS, _aligned_rows, apply_top_k_top_p, sample

DEAD = 0xFFFF


def mask_words(V: int) -> int:
    """Mask words per state: ceil(V / 32) rounded up to a multiple of 4 (16-byte rows)."""
    return (-(-V // 32) + 3) // 4 * 4


class FsmTables:
    """Device (and host mirror) tables of ``capacity`` automaton states over a ``V``-token vocabulary.

    ``tok_off`` [nt + 1] / ``tok_bytes`` are the tokenizer's token bytes; ids nt .. V-1 (logit
    columns past the tokenizer's vocabulary) get no bytes and are never allowed.  Unused states admit
    nothing."""

    def __init__(self, capacity: int, V: int, tok_off: np.ndarray, tok_bytes: np.ndarray, eot: int, device):
        if not 0 < capacity < DEAD:
            raise ValueError(f"fsm capacity {capacity} outside 1..{DEAD - 1}")
        nt = len(tok_off) - 1
        if nt > V:                                           # logits narrower than the tokenizer: cut
            tok_off = tok_off[:V + 1]
        elif nt < V:
            tok_off = np.concatenate([tok_off, np.full(V - nt, tok_off[-1], tok_off.dtype)])
        self.capacity, self.V, self.W, self.eot = int(capacity), int(V), mask_words(V), int(eot)
        self.device = torch.device(device)
        self.used = 0
        self.h_byte_next = np.full((capacity, 256), DEAD, np.uint16)
        self.h_accept = np.zeros(capacity, np.uint8)
        self.h_done_of = np.arange(capacity, dtype=np.int32)
        self.h_tok_off = np.ascontiguousarray(tok_off, np.int32)
        self.h_tok_bytes = np.ascontiguousarray(tok_bytes, np.uint8)
        dev = self.device
        self.byte_next = torch.from_numpy(self.h_byte_next.view(np.int16).copy()).to(dev)
        self.accept = torch.zeros(capacity, dtype=torch.uint8, device=dev)
        self.done_of = torch.from_numpy(self.h_done_of.copy()).to(dev)
        self.masks = torch.zeros((capacity, self.W), dtype=torch.int32, device=dev)
        self.tok_off = torch.from_numpy(self.h_tok_off).to(dev)
        self.tok_bytes = torch.from_numpy(self.h_tok_bytes).to(dev)

    def add(self, byte_next: np.ndarray, accept: np.ndarray, done: int) -> int:
        """Stack an automaton (local state ids) behind the ones present; returns its state offset."""
        n = byte_next.shape[0]
        off = self.used
        if off + n > self.capacity:
            raise ValueError(f"{n} automaton states do not fit: {off} of {self.capacity} in use")
        g = byte_next.astype(np.uint16).copy()
        g[g != DEAD] += np.uint16(off)
        self.h_byte_next[off:off + n] = g
        self.h_accept[off:off + n] = accept
        self.h_done_of[off:off + n] = off + int(done)
        self.byte_next[off:off + n].copy_(torch.from_numpy(g.view(np.int16)))
        self.accept[off:off + n].copy_(torch.from_numpy(np.ascontiguousarray(accept, np.uint8)))
        self.done_of[off:off + n].fill_(off + int(done))
        self.used = off + n
        build_masks(self, off, n)
        return off


def build_masks(t: FsmTables, s0: int, n: int) -> None:
    """Fill ``t.masks[s0 : s0 + n]`` from the transition tables: the HIP kernel on a GPU table set,
    ``agent.automaton.build_masks_ref`` on a CPU one."""
    if not (0 <= s0 and s0 + n <= t.capacity):
        raise ValueError("state range outside the table")
    if t.device.type == "cuda" and not N._FORCE_TORCH_OPS:
        N.call("penny_fsm_build_masks", N.ptr(t.byte_next), N.ptr(t.accept), N.ptr(t.tok_off), N.ptr(t.tok_bytes),
               N.ptr(t.masks), t.capacity, int(s0), int(n), t.V, t.W, t.eot, N.stream())
        return
    from ..agent.automaton import build_masks_ref
    m = build_masks_ref(t.h_byte_next, t.h_accept, t.h_tok_off, t.h_tok_bytes, t.eot, states=range(s0, s0 + n))
    t.masks[s0:s0 + n].copy_(torch.from_numpy(m.view(np.int32)))


def advance_ref(t: FsmTables, state: int, tok: int) -> int:
    """Host replica of the device state update for an ALLOWED token."""
    if state < 0:
        return -1
    if state >= t.capacity:
        return state
    if tok == t.eot:
        return int(t.h_done_of[state])
    cur = state
    for b in t.h_tok_bytes[t.h_tok_off[tok]:t.h_tok_off[tok + 1]]:
        cur = int(t.h_byte_next[cur, b])
        if cur == DEAD:
            return int(t.h_done_of[state])
    return cur


def masked_logits(logits: torch.Tensor, state: torch.Tensor, t: FsmTables) -> torch.Tensor:
    """Reference: ``logits`` with -inf at every token the row's state does not allow."""
    B, V = logits.shape
    st = state.to("cpu").tolist()
    masks = t.masks.to("cpu").numpy().view(np.uint32)
    out = logits.clone()
    for b, s in enumerate(st):
        if s < 0:
            continue
        if s >= t.capacity:
            out[b] = float("-inf")
            continue
        bits = np.unpackbits(masks[s].view(np.uint8), bitorder="little")[:V].astype(bool)
        out[b, torch.from_numpy(~bits).to(out.device)] = float("-inf")
    return out


def sample_constrained(logits: torch.Tensor, temperatures: torch.Tensor, seeds: torch.Tensor, state: torch.Tensor,
                       tables: FsmTables, out: Optional[torch.Tensor] = None,
                       state_out: Optional[torch.Tensor] = None, top_k: Optional[torch.Tensor] = None,
                       top_p: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """:func:`ops.sample` under a token automaton: ``state`` [B] int32 is each row's automaton state
    (-1: unconstrained).  Tokens the state's mask does not allow count as -inf, BEFORE the top-k /
    top-p threshold; the choice among the rest is ``sample``'s (same noise, same tie rule).  Returns
    (tokens [B] int32, next state [B] int32): the state advanced over the chosen token's bytes, eot
    -> the automaton's done state, -1 for unconstrained rows.  A row whose mask admits nothing emits
    ``tables.eot`` and goes to done.  ``state_out`` may alias ``state``."""
    B, V = logits.shape
    if V > tables.V:
        raise ValueError(f"logits of {V} columns, automaton tables for {tables.V}")
    filt = top_k is not None and top_p is not None
    if N.use_native(logits):
        out = torch.empty((B,), dtype=torch.int32, device=logits.device) if out is None else out
        state_out = torch.empty((B,), dtype=torch.int32, device=logits.device) if state_out is None else state_out
        if state.dtype != torch.int32 or not state.is_contiguous():
            state = state.to(torch.int32).contiguous()
        logits = _aligned_rows(logits)
        ws = torch.empty((B * SPLITS * 2 + B,), dtype=torch.float32, device=logits.device)
        tk = top_k.to(torch.int32).contiguous() if filt else None
        tp = top_p.to(torch.float32).contiguous() if filt else None
        N.call("penny_sample_fsm", N.ptr(logits), int(logits.dtype == torch.float32), logits.stride(0),
               N.ptr(temperatures), N.ptr(seeds), N.ptr(tk) if filt else None, N.ptr(tp) if filt else None,
               N.ptr(out), N.ptr(ws), B, V, N.ptr(state), N.ptr(state_out), N.ptr(tables.masks), tables.W,
               tables.capacity, N.ptr(tables.byte_next), N.ptr(tables.tok_off), N.ptr(tables.tok_bytes), tables.V,
               N.ptr(tables.done_of), tables.eot, N.stream())
        return out, state_out
    ml = masked_logits(logits, state, tables)
    toks = sample(ml, temperatures, seeds, top_k=top_k if filt else None, top_p=top_p if filt else None)
    st = state.tolist()
    none = torch.isneginf(ml.float()).all(-1).tolist()
    res, nxt = toks.tolist(), []
    for b in range(B):
        if st[b] >= 0 and none[b]:
            res[b] = tables.eot
        nxt.append(advance_ref(tables, st[b], res[b]))
    toks = torch.tensor(res, dtype=torch.int32)
    ns = torch.tensor(nxt, dtype=torch.int32)
    if out is not None:
        out.copy_(toks)
        toks = out
    if state_out is not None:
        state_out.copy_(ns)
        ns = state_out
    return toks, ns
