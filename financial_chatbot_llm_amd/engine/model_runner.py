"""Executes scheduled batches on the GPU: input prep, forward, logits, sampling, hipGraph decode.

Per step the host packs one int32 staging buffer (token ids, positions, KV slots, context
lengths, block tables, sampling seeds) and ships it with ONE pinned H2D copy; the forward then
runs without further host round-trips, and the only D2H sync is the sampled ids.

Pure-decode steps (the hot loop: one token per running sequence) replay a hipGraph captured
per batch-size bucket (``torch.cuda.graph`` records hipGraph on ROCm): the ~10 kernels x L
layers of a decode step become one launch, removing ~1.5 us x 300+ launch gaps per token
(SURVEY §7.4).  Padding rows of a bucket write no KV (slot -1) and their outputs are dropped.
"""
from __future__ import annotations

import itertools
import math
import os
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from .. import ops
from ..models.common import AttentionMetadata, KVCache
from ..ops import attention as _attn
from ..ops.attention import KV_BS, DecodeWorkspace, mark_shared_blocks, prefill_plan
from ..ops.sampling import TOPN_MAX
from ..parallel import comm
from ..utils.logging import get_logger
from ..utils.profiling import marker
from .scheduler import ScheduledBatch
from .sequence import Sequence

logger = get_logger(__name__)


# prefill-step GEMM M histogram bucket upper bounds (engine stats / bench record)
PREFILL_M_BUCKETS = (256, 512, 1024, 2048, 3072, 4096, 1 << 30)


@dataclass
class StepInputs:
    """Host-side description of one forward (also what the TP leader broadcasts, C4)."""

    ids: np.ndarray                 # [T]
    positions: np.ndarray           # [T]
    slots: np.ndarray               # [T]
    cu_q: np.ndarray                # [Sp+1]
    ctx_p: np.ndarray               # [Sp]
    bt_p: np.ndarray                # [Sp, W]
    max_q_len: int
    ctx_d: np.ndarray               # [Bd]
    bt_d: np.ndarray                # [Bd, W]
    logits_idx: np.ndarray          # [S] rows whose next token is sampled
    temps: np.ndarray               # [S] f32
    seeds: np.ndarray               # [S] int64
    top_k: np.ndarray               # [S]
    top_p: np.ndarray               # [S]
    src: Optional[np.ndarray] = None  # [Bd] row of the previous step's sampled vector (-1: ids[] is real)
    pwork: Optional[np.ndarray] = None  # prefill attention work list (filled by the runner): [n, 2] or lean [., 6]
    # [S] automaton state per sampled row (constrained decoding; None: no row is constrained):
    # >= 0 an explicit global state, -1 unconstrained, <= -2 carry row (-2 - v) of the previous
    # step's state_out (the row's last token is still on the device)
    fsm_state: Optional[np.ndarray] = None
    # some sampled row's request asked for log-probabilities: the step samples through the
    # log-probability form of whatever path it takes and every row's value rides back with the ids
    # (rows that did not ask discard theirs).  Not on the C4 wire: TP / CP engines refuse the request.
    want_logprobs: bool = False
    # penalties (ops.penalty; None: no sampled row is penalised).  pen [S, 2] int32: the row's slot of
    # the count table (-1: not penalised) and the row of the previous step's sampled vector that holds
    # its still-pending previous token (-1: that token is counted already); pen_params [S, 3] f32:
    # repetition, presence, frequency; pen_add [n, 2] int32: (slot, token) pairs counted before the
    # step's rows read the table.  Not on the C4 wire: TP / CP engines refuse the request.
    pen: Optional[np.ndarray] = None
    pen_params: Optional[np.ndarray] = None
    pen_add: Optional[np.ndarray] = None
    # [S] int32 top-N alternatives asked for per sampled row (SamplingParams.top_logprobs; None: no row
    # asks).  Such a step samples as it would without them, then reads the alternatives -- and those
    # rows' log-probabilities -- off the step's raw logits (``ModelRunner._sample``).  Not on the C4 wire.
    topn: Optional[np.ndarray] = None
    # [T] int32 LoRA table slot per row (SamplingParams.adapter; -1: the base model; None: no row of the
    # step has one): every row of a sequence -- prompt chunks, known and jump-forward runs, prompt-lookup
    # verification rows, decode rows -- carries its sequence's slot.  Not on the C4 wire: TP / CP
    # engines refuse the request.
    row_slot: Optional[np.ndarray] = None

    @property
    def num_prefill_tokens(self) -> int:
        return int(self.cu_q[-1]) if len(self.cu_q) else 0

    # -- C4 wire format: one flat byte buffer (no pickling) ------------------------------------
    _ARRAYS = ("ids", "positions", "slots", "cu_q", "ctx_p", "bt_p", "ctx_d", "bt_d", "logits_idx", "temps",
               "seeds", "top_k", "top_p", "src", "pwork", "fsm_state")
    _LOCAL = ("pen", "pen_params", "pen_add", "topn", "row_slot")     # staged with the step's arrays, never sent

    def pack(self) -> np.ndarray:
        """[header int64: max_q_len, then (dtype code, rows, cols) per array] + raw array bytes."""
        arrs = [getattr(self, n) for n in self._ARRAYS]
        head = [self.max_q_len]
        body = []
        for a in arrs:
            if a is None:
                head += [-1, 0, 0]
                continue
            a = np.ascontiguousarray(a)
            head += [_DT_CODE[a.dtype.str], a.shape[0], a.shape[1] if a.ndim == 2 else -1]
            body.append(a.view(np.uint8).reshape(-1))
        h = np.asarray(head, np.int64).view(np.uint8)
        return np.concatenate([h] + body)

    @classmethod
    def unpack(cls, buf: np.ndarray) -> "StepInputs":
        n = len(cls._ARRAYS)
        head = buf[:8 * (1 + 3 * n)].view(np.int64)
        off = 8 * (1 + 3 * n)
        vals = {}
        for i, name in enumerate(cls._ARRAYS):
            code, rows, cols = (int(x) for x in head[1 + 3 * i: 4 + 3 * i])
            if code < 0:
                vals[name] = None
                continue
            dt = np.dtype(_DT_NAME[code])
            count = rows * (cols if cols >= 0 else 1)
            a = buf[off: off + count * dt.itemsize].view(dt)
            off += count * dt.itemsize
            vals[name] = a.reshape(rows, cols) if cols >= 0 else a
        return cls(max_q_len=int(head[0]), **vals)

    @property
    def num_decode(self) -> int:
        return len(self.ctx_d)

    # -- control messages on the C4 channel (max_q_len < 0, no arrays) -------------------------
    CTRL_RCCL_FALLBACK = -2          # every TP rank: retire the custom all-reduce, RCCL from here on

    @classmethod
    def control(cls, code: int) -> "StepInputs":
        e = np.zeros(0, np.int32)
        return cls(e, e, e, np.zeros(1, np.int32), e, np.zeros((0, 1), np.int32), code, e, np.zeros((0, 1), np.int32),
                   np.zeros(0, np.int64), np.zeros(0, np.float32), np.zeros(0, np.int64), e, np.zeros(0, np.float32))

    @property
    def control_code(self) -> int:
        return self.max_q_len if self.max_q_len < 0 else 0


_DT_NAME = ("<i4", "<i8", "<f4")
_DT_CODE = {n: i for i, n in enumerate(_DT_NAME)}


def _slots(seq: Sequence, start: int, n: int) -> List[int]:
    bt = seq.block_table
    return [bt[p // KV_BS] * KV_BS + p % KV_BS for p in range(start, start + n)]


def sample_rows(seq, n: int) -> int:
    """Sampled positions at the end of a sequence's final chunk of n tokens: the whole draft + 1
    for a speculative chunk (engine.speculative), else the last token only."""
    return max(1, min(seq.spec_rows, n))


def fsm_code(seq, k: int) -> int:
    """``StepInputs.fsm_state`` entry of the row that samples output token k of ``seq``."""
    if seq.fsm_off is None or seq.params.forced_output is not None:
        return -1
    if k > 0 and seq.output_ids[k - 1] < 0:          # PENDING: its state is on the device too
        return -2 - seq.pending_src if seq.pending_src >= 0 else -1
    s = seq.fsm_state_before(k)
    return seq.fsm_off + s if s >= 0 else -1


def penalised(params) -> bool:
    """Does a request with these ``SamplingParams`` sample under penalties?  Any of the three off its
    neutral value; scripted outputs sample nothing and ignore them."""
    return params.forced_output is None and (params.repetition_penalty != 1.0 or params.presence_penalty != 0.0
                                             or params.frequency_penalty != 0.0)


class _PenRows:
    """The penalty columns of a step under construction (``StepInputs.pen*``)."""

    def __init__(self):
        self.rows: List[Tuple[int, int]] = []
        self.params: List[Tuple[float, float, float]] = []
        self.adds: List[Tuple[int, int]] = []
        self.any = False

    def row(self, seq, k: int) -> None:
        """The row that samples output token k of ``seq``: count the known tokens the table lacks
        (``output_ids[pen_counted : first PENDING]``) and name a PENDING predecessor's device row."""
        slot = seq.pen_slot
        if slot < 0:
            self.rows.append((-1, -1))
            self.params.append((1.0, 0.0, 0.0))
            return
        self.any = True
        out = seq.output_ids
        i = seq.pen_counted
        while i < k and out[i] >= 0:
            self.adds.append((slot, out[i]))
            i += 1
        seq.pen_counted = i
        pend = seq.pending_src if (i < k and out[i] < 0) else -1
        p = seq.params
        self.rows.append((slot, pend))
        self.params.append((p.repetition_penalty, p.presence_penalty, p.frequency_penalty))

    def arrays(self):
        if not self.any:
            return None, None, None
        return (np.asarray(self.rows, np.int32).reshape(-1, 2), np.asarray(self.params, np.float32).reshape(-1, 3),
                np.asarray(self.adds, np.int32).reshape(-1, 2))


def _table(rows: List[List[int]]) -> np.ndarray:
    """Ragged block tables -> zero-padded [len(rows), max len] int32, in one vectorised scatter."""
    lens = np.fromiter((len(r) for r in rows), np.int64, len(rows))
    w = max(int(lens.max()) if len(rows) else 1, 1)
    out = np.zeros((len(rows), w), np.int32)
    if len(rows):
        flat = np.fromiter(itertools.chain.from_iterable(rows), np.int32, int(lens.sum()))
        mask = np.arange(w)[None, :] < lens[:, None]
        out[mask] = flat
    return out


def build_step_inputs(batch: ScheduledBatch, lora: bool = False) -> StepInputs:
    """The host arrays of one step.  Per-token work is numpy (a prefill step carries ~2-4k tokens:
    a per-token Python list build cost ~1 ms of the host's critical path between GPU steps).
    ``lora``: the engine holds adapters, so the rows' slots are collected (``StepInputs.row_slot``)."""
    ids_parts: List[np.ndarray] = []
    pos_parts: List[np.ndarray] = []
    slot_parts: List[np.ndarray] = []
    cu = [0]
    ctx_p, tables_p = [], []
    logits_idx, temps, seeds, tk, tp, fsm, tn = [], [], [], [], [], [], []
    want_lp = want_tn = False
    pen = _PenRows()
    max_q = 0
    rs_parts: List[np.ndarray] = []
    for seq, start, n in batch.prefill:
        if lora:
            rs_parts.append(np.full(n, seq.lora_slot, np.int32))
        np_ = len(seq.prompt_ids)
        if start + n <= np_:
            ids_parts.append(np.asarray(seq.prompt_ids[start:start + n], np.int32))
        else:
            ids_parts.append(np.asarray(seq.all_ids[start:start + n], np.int32))
        p = np.arange(start, start + n, dtype=np.int32)
        pos_parts.append(p)
        bt = np.asarray(seq.block_table, np.int32)
        slot_parts.append(bt[p // KV_BS] * KV_BS + p % KV_BS)
        cu.append(cu[-1] + n)
        ctx_p.append(start + n)
        tables_p.append(seq.block_table)
        max_q = max(max_q, n)
        if start + n == seq.num_tokens:
            # a speculative chunk samples its last spec_rows positions (verification), others one
            r = sample_rows(seq, n)
            k0 = len(seq.output_ids) - r + 1
            want_lp = want_lp or seq.params.logprobs
            want_tn = want_tn or seq.params.top_logprobs > 0
            for i in range(r):
                logits_idx.append(cu[-1] - r + i)
                temps.append(seq.params.temperature)
                seeds.append(seq.step_seed_at(k0 + i))
                tk.append(seq.params.top_k)
                tp.append(seq.params.top_p)
                fsm.append(fsm_code(seq, k0 + i))
                tn.append(seq.params.top_logprobs)
                pen.row(seq, k0 + i)
    Tp = cu[-1]
    ids_d, pos_d, slots_d = [], [], []
    ctx_d, tables_d, src = [], [], []
    for j, seq in enumerate(batch.decode):
        p = seq.num_tokens - 1
        if seq.pending_src >= 0:      # token sampled by the step still in flight: device gather
            ids_d.append(0)
            src.append(seq.pending_src)
        else:
            ids_d.append(seq.output_ids[-1] if seq.output_ids else seq.prompt_ids[-1])
            src.append(-1)
        pos_d.append(p)
        slots_d.append(seq.block_table[p // KV_BS] * KV_BS + p % KV_BS)
        ctx_d.append(p + 1)
        tables_d.append(seq.block_table)
        logits_idx.append(Tp + j)
        temps.append(seq.params.temperature)
        seeds.append(seq.step_seed())
        tk.append(seq.params.top_k)
        tp.append(seq.params.top_p)
        fsm.append(fsm_code(seq, len(seq.output_ids)))
        tn.append(seq.params.top_logprobs)
        pen.row(seq, len(seq.output_ids))
        want_lp = want_lp or seq.params.logprobs
        want_tn = want_tn or seq.params.top_logprobs > 0

    i32 = lambda x: np.asarray(x, np.int32)  # noqa: E731
    cat = lambda parts, tail: np.concatenate(parts + [i32(tail)]) if parts else i32(tail)  # noqa: E731
    src_a = i32(src) if any(x >= 0 for x in src) else None
    row_slot = None
    if lora:
        row_slot = cat(rs_parts, [seq.lora_slot for seq in batch.decode])
        row_slot = row_slot if bool((row_slot >= 0).any()) else None
    bt_d = _table(tables_d)
    if _attn.LEAN_FLAGS & 1 and _attn.DECODE_LEAN and len(ctx_d) >= _attn.LEAN_NT_MIN_B:
        # the lean kernel's cache policy per block -- only where ops.decode keeps the NT bit
        mark_shared_blocks(bt_d, ctx_d)
    return StepInputs(cat(ids_parts, ids_d), cat(pos_parts, pos_d), cat(slot_parts, slots_d), i32(cu), i32(ctx_p),
                      _table(tables_p), max_q, i32(ctx_d), bt_d, np.asarray(logits_idx, np.int64),
                      np.asarray(temps, np.float32), np.asarray(seeds, np.int64), i32(tk), np.asarray(tp, np.float32),
                      src_a, None, i32(fsm) if any(x != -1 for x in fsm) else None, bool(want_lp), *pen.arrays(),
                      i32(tn) if want_tn else None, row_slot)


def prefill_step_inputs(seq: Sequence, start: int, n: int) -> StepInputs:
    """A prefill-only step of prompt tokens [start, start + n) of one sequence that samples nothing
    (prompt scoring): its rows attend to the sequence's first start + n tokens through its block
    table, like a scheduled prefill chunk."""
    p = np.arange(start, start + n, dtype=np.int32)
    bt = np.asarray(seq.block_table, np.int32)
    e = np.zeros(0, np.int32)
    return StepInputs(np.asarray(seq.prompt_ids[start:start + n], np.int32), p, bt[p // KV_BS] * KV_BS + p % KV_BS,
                      np.asarray([0, n], np.int32), np.asarray([start + n], np.int32), _table([seq.block_table]), n,
                      e, _table([]), np.zeros(0, np.int64), np.zeros(0, np.float32), np.zeros(0, np.int64), e,
                      np.zeros(0, np.float32), None,
                      row_slot=np.full(n, seq.lora_slot, np.int32) if seq.lora_slot >= 0 else None)


class CollectiveTimeout(RuntimeError):
    """A device-side collective (custom xGMI all-reduce) reported a missing peer."""


class PendingStep:
    """Sampled ids of a launched step (host copy in flight).  A step that sampled with
    log-probabilities carries them in the same host buffer, ``lp_off`` int32 slots in (f32 bits), or
    in ``cpu_lp`` on the CPU: ``result()`` leaves them in ``logprobs`` ([n] floats, else None).  A step
    with top-N rows (``topn``: its [n] per-row counts) carries their [n, TOPN_MAX] ids and values behind
    them, ``tn_off`` slots in (``cpu_topn`` on the CPU): ``top_logprobs`` is then one list of
    (token id, log-probability) pairs per row, None for a row that asked for none."""

    def __init__(self, cpu_out: Optional[torch.Tensor], n: int, host: Optional[torch.Tensor], event,
                 start_event=None, stats: Optional[Dict] = None, key: str = "", check_err: bool = False,
                 lp_off: int = -1, cpu_lp: Optional[torch.Tensor] = None, topn: Optional[np.ndarray] = None,
                 tn_off: int = -1, cpu_topn=None):
        self._cpu, self.n, self._host, self._event = cpu_out, n, host, event
        self._start, self._stats, self._key = start_event, stats, key
        self._check_err = check_err
        self._lp_off, self._cpu_lp = lp_off, cpu_lp
        self._topn, self._tn_off, self._cpu_topn = topn, tn_off, cpu_topn
        self.logprobs: Optional[List[float]] = None
        self.top_logprobs: Optional[List[Optional[List[Tuple[int, float]]]]] = None

    def _pairs(self, ids: torch.Tensor, lps: torch.Tensor) -> None:
        il, vl = ids.tolist(), lps.tolist()
        self.top_logprobs = [list(zip(il[r][:k], vl[r][:k])) if k > 0 else None
                             for r, k in enumerate(self._topn.tolist())]

    def result(self) -> List[int]:
        if self.n == 0:
            return []
        if self._cpu_lp is not None:
            self.logprobs = self._cpu_lp.tolist()
        if self._cpu_topn is not None:
            self._pairs(*self._cpu_topn)
        if self._cpu is not None:
            return self._cpu.tolist()
        if self._event is not None:
            self._event.synchronize()
        if self._start is not None:   # device time of the step (PENNY_STEP_GPU_TIMING=1)
            st = self._stats
            st[self._key] += self._start.elapsed_time(self._event) / 1e3
            # device idle between consecutive steps: this step's start - the previous step's end
            prev_end = st.get("_prev_end_ev")
            if prev_end is not None:
                gap = prev_end.elapsed_time(self._start) / 1e3
                if gap > 0:
                    st["gpu_idle_s"] += gap
                    st["gpu_idle_gaps"] += 1
            st["_prev_end_ev"] = self._event
        if self._check_err and int(self._host[self.n]):
            raise CollectiveTimeout("custom all-reduce: a TP peer missed the bounded wait; this step's "
                                    "hidden states are stale")
        if self._lp_off >= 0:
            self.logprobs = self._host[self._lp_off:self._lp_off + self.n].view(torch.float32).tolist()
        if self._tn_off >= 0:
            w = self.n * TOPN_MAX
            self._pairs(self._host[self._tn_off:self._tn_off + w].view(self.n, TOPN_MAX),
                        self._host[self._tn_off + w:self._tn_off + 2 * w].view(torch.float32).view(self.n, TOPN_MAX))
        return self._host[:self.n].tolist()


class Sampled(NamedTuple):
    """What the sampling stage leaves on the device: the token per row, the next automaton states
    (sampler "fsm" only), the tokens' log-probabilities (only when asked for) and the top-N rows'
    alternatives ([rows, TOPN_MAX] ids and values; only in a step that holds such a row)."""
    out: torch.Tensor
    state_out: Optional[torch.Tensor] = None
    logprob: Optional[torch.Tensor] = None
    top_ids: Optional[torch.Tensor] = None
    top_lp: Optional[torch.Tensor] = None


class _DecodeGraph:
    def __init__(self, graph, B: int, out: torch.Tensor, fused: bool = False,
                 state_out: Optional[torch.Tensor] = None, logprob: Optional[torch.Tensor] = None,
                 top_ids: Optional[torch.Tensor] = None, top_lp: Optional[torch.Tensor] = None):
        # fused: the graph samples inside the LM head (no top-k / top-p support)
        # state_out: the constrained twin's next automaton states (beside ``out``)
        # logprob: a log-probability twin's [B] f32 values (beside ``out``)
        # top_ids, top_lp: a top-N twin's [B, TOPN_MAX] alternatives
        self.graph, self.B, self.out, self.fused, self.state_out = graph, B, out, fused, state_out
        self.logprob, self.top_ids, self.top_lp = logprob, top_ids, top_lp


# Which sampler a step runs, and which captured graph holds it, decided from booleans alone.  Samplers:
# "fsm" logits -> masked threshold -> masked sampler + automaton state update, "shard" the TP
# vocabulary-parallel sampler, "fused" inside the LM head (no logits, no top-k / top-p), "logits"
# logits -> threshold -> sampler, "pen" logits -> penalties -> threshold -> sampler.
def sampler_kind(fsm: bool, filters: bool, shard: bool, fused: bool, pen: bool = False) -> str:
    """Sampler of an eager step: constrained rows, else penalised rows, else the shard / fused LM-head
    sampler where the model has one and no row carries top-k / top-p, else the logits sampler.  A step
    with constrained AND penalised rows is "fsm": the penalties run on its logits first."""
    if fsm:
        return "fsm"
    if pen:
        return "pen"
    if not filters and (shard or fused):
        return "shard" if shard else "fused"
    return "logits"


def default_graph_kind(shard: bool, fused: bool) -> str:
    """Sampler of a bucket's up-front graph; "shard" and "fused" make it a fused graph
    (``_DecodeGraph.fused``), "logits" has the threshold kernel in the graph for every row."""
    return "shard" if shard else "fused" if fused else "logits"


DEFAULT_GRAPH, EAGER = "default", "eager"
TOPN_TWIN = "+topn"      # suffix of a twin's sampler name: the same sampling stage, then the alternatives
LORA_TWIN = "+lora"      # last suffix of a twin's sampler name: the same graph with the rows' adapter deltas


def graph_plan(fsm: bool, filters: bool, lp: bool, bucket_fused: bool, tp: bool, pen: bool = False,
               topn: bool = False, lora: bool = False):
    """What runs a pure-decode step whose bucket's default graph is ``bucket_fused`` or not:
    DEFAULT_GRAPH, EAGER, or the (sampler, lp) of the bucket's twin graph, captured on the first step
    that needs it.  The default graph has no automaton, no penalties, no log-probabilities and, when
    fused, no top-k / top-p; twins exist at TP = 1 only, and none holds penalties and the automaton
    together (such a step runs eagerly).  ``topn`` (a row asks for alternatives, which implies ``lp``)
    picks the twin the step would replay without it, with ``TOPN_TWIN`` appended to the sampler's name:
    a graph of its own, so the plain twins stay as they are.  ``lora`` (a row runs on an adapter):
    whatever graph the step would replay without it -- the default graph included -- has a twin of its
    own with ``LORA_TWIN`` appended last; what runs eagerly without it still does."""
    lp = lp or topn
    if not (fsm or pen or lp or (filters and bucket_fused)):
        if not lora:
            return DEFAULT_GRAPH
        return EAGER if tp else (("fused" if bucket_fused else "logits") + LORA_TWIN, False)
    if tp or (fsm and pen):
        return EAGER
    kind = "fsm" if fsm else "pen" if pen else "logits" if filters or not bucket_fused else "fused"
    return kind + (TOPN_TWIN if topn else "") + (LORA_TWIN if lora else ""), lp


class ModelRunner:
    def __init__(self, model, kv: KVCache, max_model_len: int, max_decode_batch: int = 256,
                 use_graphs: bool = True, graph_sizes: Tuple[int, ...] = (1, 2, 4, 8, 16, 32, 64, 128, 256),
                 fsm_max_states: int = 4096):
        self.model = model
        self.kv = kv
        self.device = model.device
        self.max_model_len = max_model_len
        self.max_blocks = (max_model_len + KV_BS - 1) // KV_BS
        self.on_gpu = self.device.type == "cuda"
        self.use_graphs = use_graphs and self.on_gpu
        self.G = model.hq // model.hkv
        self.graph_sizes = tuple(sorted(s for s in graph_sizes if s <= max_decode_batch))
        self.max_decode_batch = max(self.graph_sizes) if self.graph_sizes else max_decode_batch
        cfg = model.cfg
        self.decode_ws = DecodeWorkspace.create(max(max_decode_batch, 1), model.hq, model.D, max_model_len,
                                                self.device) if self.on_gpu else None
        # TP decode as two micro-batch chains on two streams (DecoderModel.forward_decode_dual): their
        # all-reduces hide under the other chain's compute; needs the second custom-AR channel
        # (decided at the first graph capture: the engine enables the AR channels after building us)
        self._dual: Optional[bool] = None
        self.dual_min_batch = int(os.environ.get("PENNY_TP_DUAL_MIN_BATCH", "2"))
        self._max_decode_ws = max(max_decode_batch, 1)
        self.decode_ws2 = None
        self.graphs: Dict[int, _DecodeGraph] = {}         # the default graph of every bucket, captured up front
        # twins of the buckets, captured by the first step that needs one (graph_plan): keyed (bucket,
        # sampler, log-probabilities); a key that could not be captured runs eagerly from then on
        self.twins: Dict[Tuple[int, str, bool], _DecodeGraph] = {}
        self._twin_failed: set = set()
        # constrained decoding (ops.constrain): the device automaton tables are allocated at the first
        # registration, at a fixed capacity -- the decode graphs capture their pointers
        self.fsm_max_states = int(fsm_max_states)
        self.fsm: Optional[ops.FsmTables] = None
        self._fsm_known: Dict[str, int] = {}              # automaton key -> state offset
        self._fsm_tok_key = None
        self.last_fsm_state: Optional[torch.Tensor] = None   # state_out of the latest step, beside last_sampled
        # penalties (ops.penalty): the count table, allocated by the engine at the first penalised
        # request (``ensure_penalty_table``), and the static inputs of the "pen" graph twins
        self.pen_table: Optional[ops.PenaltyTable] = None
        self._pen_static = None
        self._topn_static = None                          # per-row N of the top-N graph twins
        # LoRA (ops.lora): the adapter table, allocated by the engine at the first load_adapter
        # (``ensure_lora_table``) and handed to the model with a step's row slots, and the per-row slots of the LoRA graph twins
        self.lora_table: Optional[ops.LoRATable] = None
        self._lora_static = None
        self._static = None
        self.graph_pool = None
        self.stats = {"steps": 0, "graph_steps": 0, "tokens": 0, "prefill_steps": 0, "prefill_step_tokens": 0,
                      "prefill_tile_pad_rows": 0, "prefill_m_hist": [0] * len(PREFILL_M_BUCKETS), "gpu_graph_s": 0.0, "gpu_eager_s": 0.0,
                      "gpu_idle_s": 0.0, "gpu_idle_gaps": 0, "_prev_end_ev": None, "overlap_steps": 0,
                      "constrained_steps": 0, "constrained_tokens": 0, "logprob_steps": 0,
                      "penalty_steps": 0, "penalty_rows": 0, "top_logprob_steps": 0, "lora_steps": 0, "lora_rows": 0}
        # TP prefill steps of >= overlap_min_rows rows run as two micro-batches whose all-reduces
        # overlap the other half's compute (PENNY_TP_OVERLAP=0 disables)
        self.tp_overlap = os.environ.get("PENNY_TP_OVERLAP", "1") == "1"
        self.overlap_min_rows = int(os.environ.get("PENNY_TP_OVERLAP_MIN_ROWS", "1024"))
        # device time of every step and the device idle between steps (two events per step: on by
        # default so every bench run reports where the non-busy GPU time is; =0 turns it off)
        self._gpu_timing = self.on_gpu and os.environ.get("PENNY_STEP_GPU_TIMING", "1") == "1"
        # sampled ids of the latest step stay on the device: the next step gathers its decode ids
        # from here when it was launched before this one's ids reached the host (overlap mode)
        # a speculative chunk samples draft + 1 rows (engine.speculative: drafts <= 16 tokens)
        self.max_samplers = 17 * max(self.max_decode_batch, max_decode_batch) + 1024
        self.last_sampled = torch.zeros(self.max_samplers, dtype=torch.int32, device=self.device)
        # one slot past the sampled ids carries the custom all-reduce's timeout flag back with them, and
        # the slots from _lp_off on the step's log-probabilities (f32 bits): one buffer, one event
        self._lp_off = self.max_samplers + 1
        self._tn_off = 2 * self.max_samplers + 1      # top-N alternatives: allocated with the first such step
        self._pinned_out = ([torch.zeros(2 * self.max_samplers + 1, dtype=torch.int32).pin_memory() for _ in range(2)]
                            if self.on_gpu else None)
        self._out_flip = 0
        self._ev_ring: Optional[List[Tuple[torch.cuda.Event, torch.cuda.Event]]] = None
        self._ev_i = 0
        # eager-step inputs: one pinned staging ring slot -> ONE H2D copy per step (see _stage_inputs)
        self._staged: Optional[Dict[int, torch.Tensor]] = None
        self._stage_ring: List[Optional[torch.Tensor]] = [None] * 4
        self._stage_events: List[Optional[torch.cuda.Event]] = [None] * 4
        self._stage_flip = 0
        self._stage_enabled = os.environ.get("PENNY_STAGE_INPUTS", "1") == "1"

    # ------------------------------------------------------------------------------------
    # eager path
    # ------------------------------------------------------------------------------------
    _STAGE_DTYPES = {np.dtype(np.int32): torch.int32, np.dtype(np.int64): torch.int64,
                     np.dtype(np.float32): torch.float32}

    def _stage_inputs(self, si: StepInputs) -> None:
        """Upload every array of an eager step with ONE H2D copy: the arrays are packed (16-B
        aligned) into a pinned staging slot, copied as one byte buffer and handed out as typed
        device views by ``_to_dev``.  One copy per array meant ~12 blit kernels and pinned
        allocations per step on the compute stream."""
        self._staged = None
        if not self.on_gpu or not self._stage_enabled:
            return
        arrs = []
        total = 0
        for name in StepInputs._ARRAYS + StepInputs._LOCAL:
            a = getattr(si, name)
            if a is None or a.dtype not in self._STAGE_DTYPES:
                continue
            arrs.append((a, np.ascontiguousarray(a), total))
            total += (a.nbytes + 15) // 16 * 16
        if total == 0:
            return
        k = self._stage_flip
        self._stage_flip = (k + 1) % len(self._stage_ring)
        if self._stage_events[k] is not None:
            self._stage_events[k].synchronize()     # the copy that last read this slot is done
        buf = self._stage_ring[k]
        if buf is None or buf.numel() < total:
            buf = torch.empty(max(total, 1 << 20), dtype=torch.uint8).pin_memory()
            self._stage_ring[k] = buf
        host = buf.numpy()
        for _, c, off in arrs:
            host[off:off + c.nbytes] = c.reshape(-1).view(np.uint8)
        dev = torch.empty(total, dtype=torch.uint8, device=self.device)
        dev.copy_(buf[:total], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._stage_events[k] = ev
        self._staged = {id(a): dev[off:off + c.nbytes].view(self._STAGE_DTYPES[c.dtype]).view(c.shape)
                        for a, c, off in arrs}

    def _to_dev(self, a: np.ndarray, dtype=None) -> torch.Tensor:
        t = self._staged.get(id(a)) if self._staged is not None else None
        if t is None:
            t = torch.from_numpy(np.ascontiguousarray(a))
            if self.on_gpu:
                t = t.pin_memory().to(self.device, non_blocking=True)
        return t if dtype is None else t.to(dtype)

    def _meta(self, si: StepInputs, slots: torch.Tensor) -> AttentionMetadata:
        m = AttentionMetadata(slots=slots, num_prefill_tokens=si.num_prefill_tokens, num_decode=si.num_decode,
                              decode_ws=self.decode_ws)
        if si.num_prefill_tokens:
            m.cu_q = self._to_dev(si.cu_q)
            m.ctx_lens_p = self._to_dev(si.ctx_p)
            m.block_tables_p = self._to_dev(si.bt_p)
            m.max_q_len = si.max_q_len
            if self.on_gpu:   # LPT-ordered prefill attention tiles (staged with the step when precomputed)
                work = si.pwork if si.pwork is not None else prefill_plan(si.cu_q, si.ctx_p, self.G, self.model.hkv)
                m.prefill_work = self._to_dev(work) if work is not None else None
                if work is not None and work.shape[1] == 6:        # lean split-KV list: its counts
                    m.prefill_lean = (int(work[0, 1]), int(work[0, 2]), int(work[0, 3]))
        if si.num_decode:
            m.ctx_lens_d = self._to_dev(si.ctx_d)
            m.block_tables_d = self._to_dev(si.bt_d)
        if si.row_slot is not None:
            m.row_slot, m.lora = self._to_dev(si.row_slot), self.lora_table
        return m

    def register_automaton(self, a) -> int:
        """Stack a ``TokenAutomaton`` into the device tables (once per automaton) and return the
        offset of its states: state ids are global, so one step can carry rows of different tool
        sets.  Raises ValueError when it does not fit ``fsm_max_states`` or was compiled for another
        tokenizer than the automata already present."""
        off = self._fsm_known.get(a.key)
        if off is not None:
            return off
        tok_key = (len(a.tok_off), int(a.tok_off[-1]), a.eot_id)
        if self.fsm is None:
            self.fsm = ops.FsmTables(self.fsm_max_states, self.model.cfg.vocab_size, a.tok_off, a.tok_bytes,
                                     a.eot_id, self.device)
            self._fsm_tok_key = tok_key
            self.last_fsm_state = torch.full((self.max_samplers,), -1, dtype=torch.int32, device=self.device)
        elif tok_key != self._fsm_tok_key:
            raise ValueError("automaton compiled for another tokenizer than the tables hold")
        off = self.fsm.add(a.byte_next, a.accept, a.done)
        self._fsm_known[a.key] = off
        logger.info(f"automaton registered: {a.num_states} states at offset {off} "
                    f"({self.fsm.used}/{self.fsm.capacity} in use)")
        return off

    def _resolve_fsm(self, code: torch.Tensor) -> torch.Tensor:
        """Step-local automaton states: carry codes (<= -2) read the previous step's ``state_out``
        (``last_fsm_state``) -- before any kernel of this step writes it."""
        return torch.where(code <= -2, self.last_fsm_state[(-2 - code).clamp(min=0).long()], code)

    def ensure_penalty_table(self, slots: int) -> "ops.PenaltyTable":
        """The count table of the penalised sequences, allocated at the first call: its pointer is
        captured by the "pen" graph twins, so it is never replaced."""
        if self.pen_table is None:
            self.pen_table = ops.PenaltyTable(slots, self.model.cfg.vocab_size, self.device)
            logger.info(f"penalty table: {slots} slots x {self.pen_table.Vs} tokens "
                        f"({self.pen_table.table.numel() * 2 / 1e6:.1f} MB)")
        return self.pen_table

    def ensure_lora_table(self, slots: int, max_rank: int) -> "ops.LoRATable":
        """The adapter table of the model's QKV / O / down projections, allocated at the first call: the
        LoRA graph twins capture its pointers, so it is never replaced."""
        if self.lora_table is None:
            m, c = self.model, self.model.cfg
            shapes = {"qkv": ((m.hq * m.D, m.hkv * m.D, m.hkv * m.D), c.hidden_size),
                      "o": ((c.hidden_size,), m.hq * m.D), "down": ((c.hidden_size,), c.intermediate_size)}
            self.lora_table = ops.LoRATable(slots, max_rank, c.num_layers, shapes, self.device,
                                            dtype=getattr(m, "dtype", torch.bfloat16))
            logger.info(f"LoRA table: {slots} slots x rank {self.lora_table.R} "
                        f"({self.lora_table.bytes_per_slot() / 1e6:.1f} MB per slot)")
        return self.lora_table

    def _count_lora_step(self, si: StepInputs) -> None:
        self.stats["lora_steps"] += 1
        self.stats["lora_rows"] += int((si.row_slot >= 0).sum())

    def _resolve_pending_tok(self, row: torch.Tensor) -> torch.Tensor:
        """Pending rows (of the previous step's sampled vector, -1: none) -> the tokens they hold, read
        from ``last_sampled`` before any kernel of this step writes it."""
        return torch.where(row >= 0, self.last_sampled[row.clamp(min=0).long()], row)

    def _pen_inputs(self, si: StepInputs):
        """Count ``si.pen_add`` into the table and return the step's (slot, pending token, params
        [3, S]) on the device -- at the point of the step where the pending ids are gathered."""
        if self.pen_table is None:
            raise RuntimeError("a penalised step without a penalty table")
        if len(si.pen_add):
            ops.penalty.add(self.pen_table, self._to_dev(si.pen_add))
        pen = self._to_dev(si.pen)
        return (pen[:, 0].contiguous(), self._resolve_pending_tok(pen[:, 1]),
                self._to_dev(si.pen_params).t().contiguous())

    def _count_penalty_step(self, si: StepInputs) -> None:
        self.stats["penalty_steps"] += 1
        self.stats["penalty_rows"] += int((si.pen[:, 0] >= 0).sum())

    def _gather_pending(self, ids: torch.Tensor, src: torch.Tensor, offset: int) -> None:
        """ids[offset + r] <- last_sampled[src[r]] where src[r] >= 0 (device-side, no host sync)."""
        rows = ids[offset:offset + src.shape[0]]
        rows.copy_(torch.where(src >= 0, self.last_sampled[src.clamp(min=0).long()], rows))

    def _overlap_split(self, si: StepInputs) -> Optional[int]:
        """Row at which a TP prefill step is cut into two micro-batches (None: no overlap)."""
        m = self.model
        if (getattr(m, "tp_size", 1) == 1 or not self.tp_overlap or si.num_prefill_tokens < self.overlap_min_rows
                or (hasattr(m, "uses_sp") and m.uses_sp(len(si.ids))) or not hasattr(m, "forward_overlap")):
            return None
        half = len(si.ids) // 2
        t = half // 128 * 128 if half >= 512 else half       # GEMM-friendly halves on real steps
        return max(1, min(t, si.num_prefill_tokens))

    def _split_inputs(self, si: StepInputs, t: int):
        """Two StepInputs for rows [0, t) (prefill only) and [t, T) (rest of the prefill + the
        decodes); the sequence containing row t appears in both, its first part with the
        context length it has after those rows."""
        cu = si.cu_q
        s = int(np.searchsorted(cu, t, side="right")) - 1          # sequence holding row t
        cut = t > cu[s]                                              # row t is inside sequence s
        na = s + (1 if cut else 0)
        cu_a = np.concatenate([cu[:s + 1], [t]]) if cut else cu[:s + 1]
        ctx_a = si.ctx_p[:na].copy()
        if cut:
            ctx_a[-1] = si.ctx_p[s] - (cu[s + 1] - t)
        cu_b = np.concatenate([[0], cu[s + 1:] - t]) if cut else cu[s:] - t
        empty_i = np.zeros(0, np.int32)
        a = StepInputs(si.ids[:t], si.positions[:t], si.slots[:t], cu_a.astype(np.int32), ctx_a,
                       si.bt_p[:na], si.max_q_len, empty_i, np.zeros((0, 1), np.int32), si.logits_idx[:0],
                       si.temps[:0], si.seeds[:0], si.top_k[:0], si.top_p[:0], None)
        b = StepInputs(si.ids[t:], si.positions[t:], si.slots[t:], cu_b.astype(np.int32), si.ctx_p[s:],
                       si.bt_p[s:], si.max_q_len, si.ctx_d, si.bt_d, si.logits_idx, si.temps, si.seeds,
                       si.top_k, si.top_p, None)
        return a, b

    def _hidden(self, si: StepInputs) -> torch.Tensor:
        """Final hidden states of every row of the step."""
        ids = self._to_dev(si.ids)
        if si.src is not None:
            self._gather_pending(ids, self._to_dev(si.src), si.num_prefill_tokens)
        pos = self._to_dev(si.positions)
        slots = self._to_dev(si.slots)
        t = self._overlap_split(si)
        if t is not None:    # TP prefill: micro-batch pipeline overlapping the all-reduces
            a, b = self._split_inputs(si, t)
            metas = (self._meta(a, slots[:t]), self._meta(b, slots[t:]))
            self.stats["overlap_steps"] += 1
            return self.model.forward_overlap(ids, pos, metas, t, self.kv)
        return self.model.forward(ids, pos, self._meta(si, slots), self.kv)

    def forward_logits(self, si: StepInputs) -> torch.Tensor:
        h = self._hidden(si)
        idx = self._to_dev(si.logits_idx)
        return self.model.logits(h.index_select(0, idx))

    def _fused_sampling(self, h: torch.Tensor) -> bool:
        """Does sampling the rows ``h`` run inside the LM head (fused K11 + K12)?  TP=1 only: under TP
        the vocabulary is sharded and the logits are all-gathered before sampling."""
        m = self.model
        return getattr(m, "tp_size", 1) == 1 and hasattr(m, "lm_weight") and ops.fused_lm_head_ok(h, m.lm_weight())

    def _lm_tiled(self):
        f = getattr(self.model, "lm_tiled", None)
        return f() if f is not None else None

    def _shard_sampling(self) -> bool:
        """TP: rows without top-k / top-p are sampled vocab-parallel (``sample_vocab_parallel``:
        [B, 2] candidates all-gathered instead of the [B, V] logits); ``PENNY_VOCAB_PARALLEL_SAMPLE=0``
        restores logits all-gather + sampler."""
        m = self.model
        return (getattr(m, "tp_size", 1) > 1 and hasattr(m, "sample_vocab_parallel")
                and os.environ.get("PENNY_VOCAB_PARALLEL_SAMPLE", "1") != "0")

    @staticmethod
    def _has_filters(si: StepInputs) -> bool:
        return bool((si.top_k > 0).any() or (si.top_p < 1).any())

    def logits_and_sample(self, si: StepInputs) -> Sampled:
        """Forward the step, then sample one token per ``si.logits_idx`` row: fused into the LM head
        where it applies (no top-k / top-p rows), else logits -> sampler."""
        state = None
        if si.fsm_state is not None:       # resolved where the pending ids are gathered: before any write
            state = self._resolve_fsm(self._to_dev(si.fsm_state))
        pen = self._pen_inputs(si) if si.pen is not None else None
        h = self._hidden(si)
        hs = h.index_select(0, self._to_dev(si.logits_idx))
        filt = self._has_filters(si)
        kind = sampler_kind(state is not None, filt, self._shard_sampling(), self._fused_sampling(hs),
                            pen is not None)
        if kind == "shard":
            self.stats["vocab_parallel_sample_steps"] = self.stats.get("vocab_parallel_sample_steps", 0) + 1
        elif kind == "fused":
            self.stats["fused_lm_head_steps"] = self.stats.get("fused_lm_head_steps", 0) + 1
        return self._sample(hs, kind, self._to_dev(si.temps), self._to_dev(si.seeds),
                            self._to_dev(si.top_k) if filt else None, self._to_dev(si.top_p) if filt else None,
                            state, si.want_logprobs, pen, self._to_dev(si.topn) if si.topn is not None else None)

    def _sample(self, hs: torch.Tensor, kind: str, temps: torch.Tensor, seeds: torch.Tensor,
                top_k: Optional[torch.Tensor] = None, top_p: Optional[torch.Tensor] = None,
                state: Optional[torch.Tensor] = None, lp: bool = False, pen=None,
                topn: Optional[torch.Tensor] = None) -> Sampled:
        """The one sampling stage, of eager steps and captured graphs alike: one token per hidden row
        ``hs`` through the sampler ``kind`` (see ``sampler_kind``).  ``lp``: the log-probability form
        -- the same tokens, the fused LM head still without logits, a step that holds its logits
        reading the values off them right after the (untouched) sampler.  ``topn`` ([rows] int32, > 0
        where a row asks for alternatives; implies ``lp``): the stage runs as without it, then
        ``ops.topn_logprobs`` reads the raw logits -- the ones the stage holds, else (the fused LM head)
        the LM-head logits GEMM's, computed after the sampler -- and replaces those rows'
        log-probabilities by the value from that same row of logits; the other rows keep theirs."""
        m = self.model
        lp = lp or topn is not None
        if kind == "shard":
            return Sampled(m.sample_vocab_parallel(hs, temps, seeds))
        if kind == "fused":
            if lp:
                out, logprob = ops.lm_head_sample_logprob(hs, m.lm_weight(), temps, seeds, wt=self._lm_tiled())
                return self._with_topn(Sampled(out, None, logprob), hs, None, topn)
            return Sampled(ops.lm_head_sample(hs, m.lm_weight(), temps, seeds, wt=self._lm_tiled()))
        logits = m.logits(hs).contiguous()
        state_out = None
        chosen = logits                  # what the sampler reads: the penalised logits of a "pen" step
        if pen is not None:
            # penalties first (then the automaton mask, then top-k / top-p): in place, unless the step
            # reports log-probabilities -- those stay the raw model distribution
            slot, ptok, par = pen
            chosen = ops.apply_penalties(logits, slot, ptok, par[0], par[1], par[2], self.pen_table,
                                         out=torch.empty_like(logits) if lp else None)
        elif kind == "pen":
            raise RuntimeError("a penalised step without its penalty inputs")
        if kind == "fsm":
            if self.fsm is None:
                raise RuntimeError("a constrained step without a registered automaton")
            out, state_out = ops.sample_constrained(chosen, temps, seeds, state, self.fsm, top_k=top_k, top_p=top_p)
        else:                       # device-side top-k / top-p threshold when given
            out = ops.sample(chosen, temps, seeds, top_k=top_k, top_p=top_p)
        return self._with_topn(Sampled(out, state_out, ops.token_logprobs(logits, out) if lp else None), hs, logits,
                               topn)

    def _with_topn(self, sampled: Sampled, hs: torch.Tensor, logits: Optional[torch.Tensor],
                   topn: Optional[torch.Tensor]) -> Sampled:
        """The alternatives of a step's top-N rows, after its sampling stage: off ``logits`` (raw, as
        the stage holds them) or, None, the LM-head logits of ``hs``."""
        if topn is None:
            return sampled
        if logits is None:
            logits = self.model.logits(hs).contiguous()
        n = hs.shape[0]
        top_ids = torch.empty((n, TOPN_MAX), dtype=torch.int32, device=hs.device)
        top_lp = torch.empty((n, TOPN_MAX), dtype=torch.float32, device=hs.device)
        logprob = sampled.logprob.float().contiguous()      # the kernel writes the top-N rows' entries only
        ops.topn_logprobs(logits, sampled.out, topn, out=(logprob, top_ids, top_lp))
        return sampled._replace(logprob=logprob, top_ids=top_ids, top_lp=top_lp)

    def execute(self, si: StepInputs) -> List[int]:
        """Run one step; returns the sampled token per entry of ``si.logits_idx``."""
        return self.launch(si).result()

    def launch(self, si: StepInputs) -> "PendingStep":
        """Enqueue one step on the current stream and return without waiting for the GPU; the
        sampled ids reach the host through ``PendingStep.result()`` (pinned D2H + event)."""
        self.stats["steps"] += 1
        self.stats["tokens"] += len(si.ids)
        if si.num_prefill_tokens:   # GEMM M of the steps that run the prefill (library) GEMMs
            M = len(si.ids)
            self.stats["prefill_steps"] += 1
            self.stats["prefill_step_tokens"] += M
            # rows the 256-row prefill tiles pad (M > 256: the tile kernels' M quantisation) and the
            # step-size histogram, for the bench record
            self.stats["prefill_tile_pad_rows"] += (-M) % 256 if M > 256 else 0
            b = next(i for i, hi in enumerate(PREFILL_M_BUCKETS) if M <= hi)
            self.stats["prefill_m_hist"][b] += 1
        if len(si.logits_idx) == 0:
            self._stage_inputs(si)
            try:
                self._forward_only(si)
            finally:
                self._staged = None
            return PendingStep(None, 0, None, None)
        start_ev = end_ev = None
        if self.on_gpu:
            # a small ring of reused events (creating two timing events per step cost ~30 us of
            # host time between launches); 4 pairs cover the step in flight, the one being collected and
            # the previous step's end event the idle-gap measurement still reads
            if self._ev_ring is None:
                self._ev_ring = [(torch.cuda.Event(enable_timing=self._gpu_timing),
                                  torch.cuda.Event(enable_timing=self._gpu_timing)) for _ in range(4)]
            start_ev, end_ev = self._ev_ring[self._ev_i]
            self._ev_i = (self._ev_i + 1) % len(self._ev_ring)
            if self._gpu_timing:
                start_ev.record()
            else:
                start_ev = None
        G = None
        if self.use_graphs and si.num_prefill_tokens == 0 and 0 < si.num_decode <= self.max_decode_batch:
            G = self._decode_graph(si)
        graph = G is not None
        if graph:
            with marker(f"decode.graph[{si.num_decode}]"):
                out, so, lpv, tid, tlp = self._graph_decode(si, G)
        else:
            with marker(f"forward.eager[{len(si.ids)}]"):
                if si.num_prefill_tokens and si.pwork is None and self.on_gpu:
                    si.pwork = prefill_plan(si.cu_q, si.ctx_p, self.G, self.model.hkv)
                self._stage_inputs(si)
                try:
                    out, so, lpv, tid, tlp = self.logits_and_sample(si)
                finally:
                    self._staged = None
        n = len(si.logits_idx)
        self.last_sampled[:n].copy_(out[:n].to(torch.int32), non_blocking=True)
        if si.want_logprobs:
            self.stats["logprob_steps"] += 1
        if si.topn is not None:
            self.stats["top_logprob_steps"] += 1
        if si.pen is not None:
            self._count_penalty_step(si)
        if si.row_slot is not None:
            self._count_lora_step(si)
        if si.fsm_state is not None:
            self.last_fsm_state[:n].copy_(so[:n], non_blocking=True)
            self.stats["constrained_steps"] += 1
            self.stats["constrained_tokens"] += int((si.fsm_state != -1).sum())
        ar = comm.custom_all_reduce()
        if not self.on_gpu:
            cpu = out[:n].clone()
            cpu_lp = lpv[:n].float().clone() if lpv is not None else None
            tn = dict(topn=si.topn, cpu_topn=(tid[:n], tlp[:n])) if si.topn is not None else {}
            if ar is not None:           # a host-side stand-in (tests): its flag is host memory
                return PendingStep(None, n, torch.cat([cpu.to(torch.int32), ar.err.to(torch.int32)[:1]]), None,
                                   check_err=True, cpu_lp=cpu_lp, **tn)
            return PendingStep(cpu, n, None, None, cpu_lp=cpu_lp, **tn)
        if si.topn is not None and self._pinned_out[0].numel() < self._tn_off + 2 * TOPN_MAX * self.max_samplers:
            # the first step with top-N rows: the host buffers grow by the alternatives' region (a step
            # in flight keeps the buffer it was given)
            self._pinned_out = [torch.zeros(self._tn_off + 2 * TOPN_MAX * self.max_samplers,
                                            dtype=torch.int32).pin_memory() for _ in range(2)]
        host = self._pinned_out[self._out_flip]
        self._out_flip ^= 1
        host[:n].copy_(out[:n], non_blocking=True)
        if lpv is not None:
            host[self._lp_off:self._lp_off + n].view(torch.float32).copy_(lpv[:n], non_blocking=True)
        if si.topn is not None:        # [n, TOPN_MAX] ids then values, sized by this step's rows
            w = n * TOPN_MAX
            host[self._tn_off:self._tn_off + w].view(n, TOPN_MAX).copy_(tid[:n], non_blocking=True)
            host[self._tn_off + w:self._tn_off + 2 * w].view(torch.float32).view(n, TOPN_MAX).copy_(
                tlp[:n], non_blocking=True)
        if ar is not None:
            # the xGMI all-reduce never raises from the device: a peer that missed its bounded wait
            # sets ar.err and the step's sums are stale, so the flag rides the per-step host sync
            host[n:n + 1].copy_(ar.err, non_blocking=True)
        ev = end_ev
        ev.record()
        return PendingStep(None, n, host, ev, start_ev, self.stats, "gpu_graph_s" if graph else "gpu_eager_s",
                           check_err=ar is not None, lp_off=self._lp_off if lpv is not None else -1,
                           topn=si.topn, tn_off=self._tn_off if si.topn is not None else -1)

    def _forward_only(self, si: StepInputs) -> None:
        self._hidden(si)

    def score_chunk(self, si: StepInputs, targets: np.ndarray) -> Tuple[List[float], List[int]]:
        """Prompt scoring: forward a prefill-only step and return, for every row whose ``targets``
        entry ([T] int32, < 0: none) names the token that follows it, log p(target | row) and the
        row's argmax token (``model.token_logprobs``: no [T, V] logits).  Synchronous, on the current
        stream after whatever step is in flight; apart from the KV slots the step names it touches
        no runner state (no ``launch()``, output ring, ``last_sampled`` or decode graph)."""
        if si.num_decode or si.src is not None or len(si.logits_idx):
            raise ValueError("score_chunk takes a prefill-only step without sampled rows")
        rows = np.flatnonzero(np.asarray(targets) >= 0)
        if si.row_slot is not None:
            self._count_lora_step(si)
        if si.pwork is None and self.on_gpu:
            si.pwork = prefill_plan(si.cu_q, si.ctx_p, self.G, self.model.hkv)
        self._stage_inputs(si)
        try:
            h = self._hidden(si)
        finally:
            self._staged = None
        if len(rows) == 0:
            return [], []
        tg = torch.from_numpy(np.ascontiguousarray(np.asarray(targets, np.int32)[rows])).to(self.device)
        if len(rows) < len(si.ids):
            h = h.index_select(0, torch.from_numpy(rows).to(self.device))
        lp, top1 = self.model.token_logprobs(h, tg)
        return lp.float().cpu().tolist(), top1.cpu().tolist()

    def drop_graphs(self) -> None:
        """Forget every captured decode graph (they bake in the custom all-reduce kernels and its
        buffers): after a runtime fallback to RCCL (comm.fallback_to_rccl) decode runs eagerly."""
        if self.on_gpu:
            torch.cuda.synchronize(self.device)
        self.graphs.clear()
        self.twins.clear()
        self.use_graphs = False
        self._dual = False

    # ------------------------------------------------------------------------------------
    # hipGraph decode
    # ------------------------------------------------------------------------------------
    def _alloc_static(self) -> None:
        B, W = self.max_decode_batch, self.max_blocks
        # ids | pos | slots | ctx | block tables | gather rows | top-k live in ONE device buffer fed
        # by ONE pinned H2D copy
        self._src_off = 4 * B + B * W          # pending-token gather rows (-1: host id)
        self._topk_off = self._src_off + B     # per-row top-k (0: off)
        self._fsm_off = self._topk_off + B     # per-row automaton state / carry code (-1: unconstrained)
        self._dev_i32 = torch.zeros(self._fsm_off + B, dtype=torch.int32, device=self.device)
        d = self._dev_i32
        self._static = {
            "ids": d[0:B], "pos": d[B:2 * B], "slots": d[2 * B:3 * B], "ctx": d[3 * B:4 * B],
            "bt": d[4 * B:self._src_off].view(B, W),
            "src": d[self._src_off:self._topk_off],
            "top_k": d[self._topk_off:self._topk_off + B],
            "fsm": d[self._fsm_off:self._fsm_off + B],
            "f32": torch.zeros(2 * B, dtype=torch.float32, device=self.device),     # temps | top_p
            "seeds": torch.zeros(B, dtype=torch.int64, device=self.device),
        }
        self._static["slots"].fill_(-1)
        self._static["ctx"].fill_(1)
        self._static["src"].fill_(-1)
        self._static["fsm"].fill_(-1)
        self._static["temps"], self._static["top_p"] = self._static["f32"][:B], self._static["f32"][B:]
        self._static["top_p"].fill_(1.0)
        # two pinned staging sets, alternated per graph step: in overlap mode the host packs step
        # N+1 while step N's H2D copy may still be queued behind step N-1 on the stream, so a
        # single buffer could be overwritten before the DMA reads it
        self._pinned_sets = [(torch.zeros(self._fsm_off + B, dtype=torch.int32).pin_memory(),
                              torch.zeros(2 * B, dtype=torch.float32).pin_memory(),
                              torch.zeros(B, dtype=torch.int64).pin_memory()) for _ in range(2)]
        self._pin_flip = 0
        self._pinned_i32, self._pinned_f, self._pinned_l = self._pinned_sets[0]

    @property
    def dual_decode(self) -> bool:
        if self._dual is None:
            m = self.model
            self._dual = bool(self.on_gpu and getattr(m, "tp_size", 1) > 1 and hasattr(m, "forward_decode_dual")
                              and getattr(m.cfg, "arch", "") == "llama" and comm.custom_all_reduce() is not None
                              and getattr(comm, "_CUSTOM_AR_2", None) is not None
                              and os.environ.get("PENNY_TP_DUAL_DECODE", "1") != "0")
            if self._dual:
                # each chain's all-reduce must fit ITS custom instance: a half batch falling back to
                # RCCL would put two streams' RCCL collectives on one communicator inside one graph
                need = ((self.max_decode_batch + 1) // 2) * m.cfg.hidden_size * 2
                cap = min(comm.custom_all_reduce().max_bytes, comm._CUSTOM_AR_2.max_bytes)
                if need > cap:
                    logger.warning(f"TP dual decode disabled: a half batch all-reduces {need} B > the custom "
                                   f"all-reduce's {cap} B")
                    self._dual = False
            if self._dual:
                self.decode_ws2 = DecodeWorkspace.create(self._max_decode_ws, m.hq, m.D, self.max_model_len,
                                                         self.device)
        return self._dual

    def _run_static(self, B: int, kind: Optional[str] = None, lp: bool = False) -> Tuple[str, Sampled]:
        """One decode step of bucket B on the static inputs, sampled by ``kind`` (None: the bucket's
        default sampler, decided here and returned)."""
        s = self._static
        topn = row_slot = None
        if kind is not None and kind.endswith(LORA_TWIN):
            kind, row_slot = kind[:-len(LORA_TWIN)], self._lora_static["slot"][:B]
        if kind is not None and kind.endswith(TOPN_TWIN):
            kind, topn = kind[:-len(TOPN_TWIN)], self._topn_static["n"][:B]
        fsm = kind == "fsm"
        pen = None
        if kind == "pen":     # pending rows -> tokens, before the sampler of this graph writes last_sampled
            ps = self._pen_static
            ps["tok"][:B].copy_(self._resolve_pending_tok(ps["i32"][1, :B]))
            pen = (ps["i32"][0, :B], ps["tok"][:B], ps["f32"][:, :B])
        self._gather_pending(s["ids"], s["src"][:B], 0)
        if fsm:      # carry codes -> states, in place, before the sampler of this graph writes state_out
            s["fsm"][:B].copy_(self._resolve_fsm(s["fsm"][:B]))
        if self.dual_decode and B >= self.dual_min_batch:
            k = B // 2                       # two chains: rows [0, k) and [k, B)
            metas = [AttentionMetadata(slots=s["slots"][a:b], num_prefill_tokens=0, num_decode=b - a,
                                       ctx_lens_d=s["ctx"][a:b], block_tables_d=s["bt"][a:b], decode_ws=ws)
                     for (a, b), ws in (((0, k), self.decode_ws), ((k, B), self.decode_ws2))]
            self.stats["dual_decode_graphs"] = self.stats.get("dual_decode_graphs", 0) + 1
            h = self.model.forward_decode_dual(s["ids"][:B], s["pos"][:B], metas, k, self.kv)
        else:
            meta = AttentionMetadata(slots=s["slots"][:B], num_prefill_tokens=0, num_decode=B,
                                     ctx_lens_d=s["ctx"][:B], block_tables_d=s["bt"][:B], decode_ws=self.decode_ws,
                                     row_slot=row_slot, lora=self.lora_table)
            h = self.model.forward(s["ids"][:B], s["pos"][:B], meta, self.kv)
        if kind is None:
            kind = default_graph_kind(self._shard_sampling(), self._fused_sampling(h))
        # the top-k / top-p threshold kernel is always in a graph that samples from logits: unfiltered
        # rows (k=0, p=1) exit after reading their parameters; under TP such rows replay eagerly
        filt = kind in ("fsm", "logits", "pen")
        return kind, self._sample(h, kind, s["temps"][:B], s["seeds"][:B], s["top_k"][:B] if filt else None,
                                  s["top_p"][:B] if filt else None, s["fsm"][:B] if fsm else None, lp, pen, topn)

    def _capture(self, B: int, kind: Optional[str] = None, lp: bool = False) -> _DecodeGraph:
        for _ in range(2):      # warm up (allocator + hipBLASLt heuristics) outside the capture
            self._run_static(B, kind, lp)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, pool=self.graph_pool):
            kind, sampled = self._run_static(B, kind, lp)
        if self.graph_pool is None:
            self.graph_pool = g.pool()
        return _DecodeGraph(g, B, sampled.out, kind in ("shard", "fused"), sampled.state_out, sampled.logprob,
                            sampled.top_ids, sampled.top_lp)

    def capture_graphs(self) -> None:
        if not self.use_graphs:
            return
        if self._static is None:
            self._alloc_static()
        torch.cuda.synchronize()
        for B in sorted(self.graph_sizes, reverse=True):
            self.graphs[B] = self._capture(B)
        torch.cuda.synchronize()
        logger.info(f"captured decode hipGraphs for batch sizes {sorted(self.graphs)}")

    def _decode_graph(self, si: StepInputs) -> Optional[_DecodeGraph]:
        """The captured graph that runs this pure-decode step (``graph_plan``), or None: eagerly.  A
        twin is captured by the first step that needs it; one that cannot be (e.g. out of memory after
        the KV pool took HBM) leaves its steps on the eager path for good."""
        if not self.graphs:
            self.capture_graphs()
        B = self._bucket(si.num_decode)
        G = self.graphs[B]
        plan = graph_plan(si.fsm_state is not None, self._has_filters(si), si.want_logprobs, G.fused,
                          getattr(self.model, "tp_size", 1) > 1, si.pen is not None, si.topn is not None,
                          si.row_slot is not None)
        if plan == DEFAULT_GRAPH:
            return G
        if plan == EAGER:
            return None
        key = (B, *plan)
        if key in self._twin_failed:
            return None
        if key not in self.twins:
            try:
                self._capture_twin(key)
            except Exception as e:  # noqa: BLE001
                logger.warning(f"decode graph twin {key} not captured ({e}); running its steps eagerly")
                self._twin_failed.add(key)
                torch.cuda.synchronize(self.device)
                return None
        return self.twins[key]

    def _capture_twin(self, key: Tuple[int, str, bool]) -> None:
        """Capture mid-serving: the static inputs still hold the step in flight, so the warm-up and
        capture passes run with every KV slot masked (< 0: no cache write), no pending-token
        gather and no automaton state -- they must not rewrite live sequences' KV -- and the inputs
        are restored after."""
        B, kind, lp = key
        s = self._static
        if kind.endswith(LORA_TWIN):
            self._alloc_lora_static()      # no row on an adapter (slot -1) until the replay fills them in
            kind = kind[:-len(LORA_TWIN)]
        if kind.endswith(TOPN_TWIN):
            self._alloc_topn_static()      # no row asks (N = 0) until the replay fills them in
            kind = kind[:-len(TOPN_TWIN)]
        if kind == "pen":
            self._alloc_pen_static()       # no row penalised (slot -1) until the replay fills them in
        saved = (s["slots"][:B].clone(), s["src"][:B].clone(), s["fsm"][:B].clone())
        s["slots"][:B].fill_(-1)
        s["src"][:B].fill_(-1)
        s["fsm"][:B].fill_(-1)
        try:
            self.twins[key] = self._capture(B, key[1], lp)
        finally:                                  # the step in flight keeps its inputs either way
            s["slots"][:B].copy_(saved[0])
            s["src"][:B].copy_(saved[1])
            s["fsm"][:B].copy_(saved[2])
            torch.cuda.synchronize()

    def _alloc_pen_static(self) -> None:
        """Static inputs of the "pen" twins, allocated with the first of them (the default graphs and
        their staging buffers stay as they are): slot | pending row [2, B] int32 and the parameters
        [3, B] f32, each fed by one pinned copy per penalised graph step; ``tok`` holds the pending
        tokens the graph resolves."""
        B = self.max_decode_batch
        if self._pen_static is None:
            self._pen_static = {
                "i32": torch.zeros((2, B), dtype=torch.int32, device=self.device),
                "tok": torch.full((B,), -1, dtype=torch.int32, device=self.device),
                "f32": torch.zeros((3, B), dtype=torch.float32, device=self.device),
                "pinned": [(torch.zeros((2, B), dtype=torch.int32).pin_memory(),
                            torch.zeros((3, B), dtype=torch.float32).pin_memory()) for _ in range(2)],
                "flip": 0,
            }
        self._pen_static["i32"].fill_(-1)

    def _alloc_topn_static(self) -> None:
        """Static per-row N of the top-N twins ([B] int32, one pinned copy per such graph step),
        allocated with the first of them."""
        B = self.max_decode_batch
        if self._topn_static is None:
            self._topn_static = {"n": torch.zeros(B, dtype=torch.int32, device=self.device),
                                 "pinned": [torch.zeros(B, dtype=torch.int32).pin_memory() for _ in range(2)],
                                 "flip": 0}
        self._topn_static["n"].zero_()

    def _alloc_lora_static(self) -> None:
        """Static per-row adapter slots of the LoRA twins ([B] int32, one pinned copy per such graph
        step), allocated with the first of them."""
        B = self.max_decode_batch
        if self._lora_static is None:
            self._lora_static = {"slot": torch.full((B,), -1, dtype=torch.int32, device=self.device),
                                 "pinned": [torch.zeros(B, dtype=torch.int32).pin_memory() for _ in range(2)],
                                 "flip": 0}
        self._lora_static["slot"].fill_(-1)

    def _stage_lora_static(self, si: StepInputs, B: int) -> None:
        ls = self._lora_static
        pin = ls["pinned"][ls["flip"]]
        ls["flip"] ^= 1
        a = pin.numpy()
        a[:B] = -1
        a[:si.num_decode] = si.row_slot
        ls["slot"].copy_(pin, non_blocking=True)

    def _stage_topn_static(self, si: StepInputs, B: int) -> None:
        ts = self._topn_static
        pin = ts["pinned"][ts["flip"]]
        ts["flip"] ^= 1
        a = pin.numpy()
        a[:B] = 0
        a[:si.num_decode] = si.topn
        ts["n"].copy_(pin, non_blocking=True)

    def _stage_pen_static(self, si: StepInputs, B: int) -> None:
        """The penalty inputs of a "pen" twin's replay; ``pen_add`` is counted eagerly in front of it."""
        ps = self._pen_static
        n = si.num_decode
        if len(si.pen_add):
            ops.penalty.add(self.pen_table, torch.from_numpy(si.pen_add).pin_memory().to(self.device, non_blocking=True))
        pi, pf = ps["pinned"][ps["flip"]]
        ps["flip"] ^= 1
        a, f = pi.numpy(), pf.numpy()
        a[:, :B] = -1
        a[:, :n] = si.pen.T
        f[:, :B] = np.asarray([[1.0], [0.0], [0.0]], np.float32)
        f[:, :n] = si.pen_params.T
        ps["i32"].copy_(pi, non_blocking=True)
        ps["f32"].copy_(pf, non_blocking=True)

    def _bucket(self, n: int) -> int:
        for b in self.graph_sizes:
            if b >= n:
                return b
        return self.graph_sizes[-1]

    def _graph_decode(self, si: StepInputs, G: _DecodeGraph) -> Sampled:
        n, B = si.num_decode, G.B
        S, W = self.max_decode_batch, self.max_blocks
        self._pinned_i32, self._pinned_f, self._pinned_l = self._pinned_sets[self._pin_flip]
        self._pin_flip ^= 1
        buf = self._pinned_i32.numpy()
        # layout: ids | pos | slots | ctx | bt  (each section sized for the largest bucket)
        buf[0:n] = si.ids
        buf[S:S + n] = si.positions
        buf[2 * S:2 * S + B] = -1
        buf[2 * S:2 * S + n] = si.slots
        buf[3 * S:3 * S + B] = 1
        buf[3 * S:3 * S + n] = si.ctx_d
        bt = buf[4 * S:4 * S + S * W].reshape(S, W)
        bt[:B] = 0
        bt[:n, :si.bt_d.shape[1]] = si.bt_d
        src = buf[self._src_off:self._src_off + S]
        src[:B] = -1
        if si.src is not None:
            src[:n] = si.src
        tk = buf[self._topk_off:self._topk_off + S]
        tk[:B] = 0
        tk[:n] = si.top_k
        fs = buf[self._fsm_off:self._fsm_off + S]
        fs[:B] = -1
        if si.fsm_state is not None:
            fs[:n] = si.fsm_state
        f = self._pinned_f.numpy()
        f[:n] = si.temps
        f[S:S + B] = 1.0
        f[S:S + n] = si.top_p
        self._pinned_l.numpy()[:n] = si.seeds
        self._dev_i32.copy_(self._pinned_i32, non_blocking=True)
        s = self._static
        s["f32"].copy_(self._pinned_f, non_blocking=True)
        s["seeds"].copy_(self._pinned_l, non_blocking=True)
        if si.pen is not None:             # only a "pen" twin is chosen for such a step (graph_plan)
            self._stage_pen_static(si, B)
        if si.topn is not None:            # likewise a top-N twin
            self._stage_topn_static(si, B)
        if si.row_slot is not None:        # likewise a LoRA twin
            self._stage_lora_static(si, B)
        G.graph.replay()
        self.stats["graph_steps"] += 1
        return Sampled(G.out[:n], G.state_out, G.logprob, G.top_ids, G.top_lp)
