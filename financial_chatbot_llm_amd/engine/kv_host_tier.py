"""Host-memory tier of the paged KV cache: full blocks are copied to pinned host DRAM before HBM
forgets them, and a later prompt that matches them gets the bytes back over PCIe instead of a prefill.

:class:`HostKVTier` owns the host store, the device staging chunks, the copy streams and an exact index;
:class:`TieredBlockManager` wraps either block manager behind the interface the scheduler uses, so the
scheduler and both managers are unchanged.  Off by default (``EngineConfig.host_kv_gb = 0``): the engine
then holds the plain manager and none of this is constructed.

Index.  An entry is one full 64-token block, keyed by ``(parent, token bytes)``: ``parent`` is the uid of
the entry of the block in front of it, or ``("root", cache_salt)`` for a sequence's first block (salt 0:
the base model; an adapter's salt starts its own chains, as in the block managers), and the token bytes
are the block's 64 int32 ids.  The dict compares the tokens themselves: there is no hash to collide, so
no prompt is ever served another prompt's KV.  The tier moves bytes: bf16 and fp8 pools need nothing
special (the fp8 scales are static per layer and head).

Slots.  ``slots = host_bytes // bytes_per_block`` blocks of pinned memory, LRU.  A chain that is hit (or
saved) is touched tail first, root last, so a prefix never leaves the tier before its extensions.  A slot
with a queued or unfinished copy in either direction is pinned against eviction, and a saved entry is
visible to lookups only once its device-to-host copy has completed (``event.query()``).

Ordering.  ``save`` and the wrapper's ``match_prefix`` only queue work; :meth:`HostKVTier.drain` runs it
on the compute stream immediately before every step launch: first the queued saves (gather kernel into a
staging chunk, event, D2H on the save stream), then the queued restores (H2D on the restore stream into a
staging chunk, the compute stream waits for it, scatter kernel into the pool).  Blocks released at
``free`` can only be re-allocated by a later ``schedule()``, whose step launches after this drain, and
restored blocks are read only by the step launched after it.  (The H2D copies of the first two restore
chunks are queued ahead of the saves: they touch no pool block.)  Nothing here runs inside a graph capture.
Saving never stalls a step: with both save chunks still in flight the remaining blocks are dropped
(``save_skipped``).
"""
from __future__ import annotations

import contextlib
from collections import OrderedDict
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from ..models.common import KVCache
from ..ops import kv_tier as K
from ..ops.attention import KV_BS
from .sequence import PENDING, Sequence

MAX_SWAP_WAITS = 256      # admission attempts a preempted sequence may be put off for its swap-in
STAT_KEYS = ("host_kv_slots", "host_kv_used", "host_kv_saved_blocks", "host_kv_save_skipped", "host_kv_lookups",
             "host_kv_hit_blocks", "host_kv_restored_blocks", "host_kv_restored_tokens", "host_kv_evictions")


class _DoneEvent:
    """Event of a device without streams (CPU tensors): every copy is complete when it returns."""

    def record(self, stream=None) -> None:
        pass

    def query(self) -> bool:
        return True

    def synchronize(self) -> None:
        pass


class _Entry:
    __slots__ = ("uid", "key", "slot", "ready", "pins")

    def __init__(self, uid: int, key, slot: int):
        self.uid, self.key, self.slot = uid, key, slot
        self.ready = False      # its D2H copy has completed: visible to lookups
        self.pins = 0           # queued or unfinished copies that read or write its slot


class _Chunk:
    """One device staging chunk with its event; ``entries``: the save in flight from it (None: free)."""

    def __init__(self, stage: torch.Tensor, event):
        self.stage, self.event = stage, event
        self.entries: Optional[List[_Entry]] = None
        self.used = False


def _runs(slots: List[int]) -> List[Tuple[int, int, int]]:
    """``slots`` as (first position, first slot, length) runs of consecutive slots: one copy each."""
    out: List[Tuple[int, int, int]] = []
    j = 0
    while j < len(slots):
        m = 1
        while j + m < len(slots) and slots[j + m] == slots[j] + m:
            m += 1
        out.append((j, slots[j], m))
        j += m
    return out


class HostKVTier:
    def __init__(self, kv: KVCache, host_bytes: int, chunk_blocks: int = 16,
                 event_factory: Optional[Callable[[], object]] = None):
        self.kv = kv
        pool = K.pool_planes(kv.buf)
        self.planes, self.num_blocks, self.plane_bytes = (int(x) for x in pool.shape)
        self.bytes_per_block = self.planes * self.plane_bytes
        self.slots = int(host_bytes) // self.bytes_per_block
        if self.slots < 1:
            raise ValueError(f"host KV tier of {int(host_bytes)} bytes holds no {self.bytes_per_block}-byte block")
        self.chunk_blocks = max(1, int(chunk_blocks))
        self.device = pool.device
        self.cuda = self.device.type == "cuda"
        self._new_event = event_factory or ((lambda: torch.cuda.Event()) if self.cuda else _DoneEvent)
        # an allocation failure (pinned memory is a limited resource) raises here, at engine construction
        self.store = torch.empty((self.slots, self.planes, self.plane_bytes), dtype=torch.uint8, pin_memory=self.cuda)
        shape = (self.chunk_blocks, self.planes, self.plane_bytes)
        self._save_chunks = [_Chunk(torch.empty(shape, dtype=torch.uint8, device=self.device), self._new_event())
                             for _ in range(2)]
        self._restore_chunks = [_Chunk(torch.empty(shape, dtype=torch.uint8, device=self.device), self._new_event())
                                for _ in range(2)]
        self._scattered = [self._new_event() for _ in range(2)]     # restore chunk i's last scatter
        self._gathered = [self._new_event() for _ in range(2)]      # save chunk i's last gather
        # one copy stream per direction: PCIe is full duplex, and on one stream the save of a sequence
        # that has just finished would delay the restore of the next one by its whole D2H time
        self._copy_stream = torch.cuda.Stream(self.device) if self.cuda else None       # D2H (saves)
        self._load_stream = torch.cuda.Stream(self.device) if self.cuda else None       # H2D (restores)
        # block ids of one drain, staged through pinned memory (two buffers, alternating: a buffer is
        # rewritten two drains after its copy was queued)
        cap = 2 * self.chunk_blocks + self.num_blocks
        self._ids_host = [torch.empty((cap,), dtype=torch.int32, pin_memory=self.cuda) for _ in range(2)]
        self._ids_dev = [torch.empty((cap,), dtype=torch.int32, device=self.device) for _ in range(2)]
        self._ids_event = [self._new_event() for _ in range(2)]
        self._ids_used = [False, False]
        self._ids_turn = 0
        self._index: Dict[tuple, _Entry] = {}
        self._lru: "OrderedDict[int, _Entry]" = OrderedDict()       # oldest first
        self._free_slots: List[int] = list(range(self.slots - 1, -1, -1))
        self._next_uid = 0
        self._save_q: List[Tuple[int, _Entry]] = []                 # (device block, entry)
        self._restore_q: List[Tuple[_Entry, int]] = []              # (entry, device block)
        self._restoring: List[Tuple[object, List[_Entry]]] = []     # (H2D event, entries it reads)
        self.saved_blocks = 0
        self.save_skipped = 0
        self.lookups = 0
        self.hit_blocks = 0
        self.restored_blocks = 0
        self.restored_tokens = 0
        self.evictions = 0
        self.swap_waits = 0                # admission attempts of preempted sequences put off (TieredBlockManager)
        self.lookup_pending = False        # the latest lookup's run ended at an entry whose copy is in flight

    # -- index ----------------------------------------------------------------------------------------
    @staticmethod
    def _root(seq: Sequence):
        return ("root", int(getattr(seq, "cache_salt", 0)))

    @staticmethod
    def _block_key(parent, tokens) -> Optional[tuple]:
        """The key of a full block, None for one that is short or holds the PENDING placeholder."""
        if len(tokens) != KV_BS or PENDING in tokens:
            return None
        return (parent, np.asarray(tokens, dtype=np.int32).tobytes())

    def _touch(self, chain: List[_Entry]) -> None:
        for e in reversed(chain):                      # tail first, root last: the root is the youngest
            if e.uid in self._lru:
                self._lru.move_to_end(e.uid)

    def _remove(self, e: _Entry) -> None:
        if self._index.get(e.key) is e:
            del self._index[e.key]
        self._lru.pop(e.uid, None)
        self._free_slots.append(e.slot)

    def _take_slot(self) -> Optional[int]:
        if self._free_slots:
            return self._free_slots.pop()
        for e in self._lru.values():                   # oldest first; pinned slots are passed over
            if e.pins == 0:
                self._remove(e)
                self.evictions += 1
                return self._free_slots.pop()
        return None

    def _poll(self) -> None:
        """Completed copies: saved entries become visible, restored entries lose their pin."""
        for c in self._save_chunks:
            if c.entries is not None and c.event.query():
                for e in c.entries:
                    e.ready = True
                    e.pins -= 1
                c.entries = None
        while self._restoring and self._restoring[0][0].query():
            for e in self._restoring.pop(0)[1]:
                e.pins -= 1

    # -- the block manager wrapper's calls --------------------------------------------------------
    def save(self, seq: Sequence) -> int:
        """Queue the sequence's full, computed, host-known blocks that the tier does not hold yet;
        returns how many were queued.  The blocks are read by the next :meth:`drain`."""
        self._poll()
        resolved = seq.num_computed
        if seq.spec_rows > 1:                          # an unverified draft's positions are not resolved
            resolved = min(resolved, seq.num_tokens - seq.spec_rows)
        full = min(max(resolved, 0) // KV_BS, len(seq.block_table))
        if seq.params.ephemeral_kv:                    # what it computed itself will not recur (evict_first)
            full = min(full, seq.num_cached_prompt // KV_BS)
        if full <= 0:
            return 0
        ids = seq.all_ids
        parent = self._root(seq)
        chain: List[_Entry] = []
        queued = 0
        for i in range(full):
            key = self._block_key(parent, ids[i * KV_BS:(i + 1) * KV_BS])
            if key is None:
                break
            e = self._index.get(key)
            if e is None:
                slot = self._take_slot()
                if slot is None:                       # every slot is pinned by a copy
                    self.save_skipped += full - i
                    break
                e = _Entry(self._next_uid, key, slot)
                self._next_uid += 1
                e.pins = 1
                self._index[key] = e
                self._lru[e.uid] = e
                self._save_q.append((int(seq.block_table[i]), e))
                queued += 1
            e.pins += 1                                # the chain's own entries are not evicted to extend it
            chain.append(e)
            parent = e.uid
        for e in chain:
            e.pins -= 1
        self._touch(chain)
        return queued

    def lookup(self, seq: Sequence, start_block: int) -> List[_Entry]:
        """The run of consecutive ready entries that continues the sequence's chain from block
        ``start_block`` on; at least one prompt token is always left to compute."""
        self._poll()
        ids = seq.all_ids
        max_full = (len(ids) - 1) // KV_BS
        self.lookup_pending = False
        if start_block >= max_full:
            return []
        self.lookups += 1
        parent = self._root(seq)
        chain: List[_Entry] = []
        self.lookup_pending = False
        for i in range(max_full):
            key = self._block_key(parent, ids[i * KV_BS:(i + 1) * KV_BS])
            e = self._index.get(key) if key is not None else None
            if e is None:
                break
            if i >= start_block and not e.ready:
                self.lookup_pending = True             # the run goes on once this copy has completed
                break
            chain.append(e)
            parent = e.uid
        self._touch(chain)
        run = chain[start_block:]
        self.hit_blocks += len(run)
        return run

    def queue_restore(self, entries: List[_Entry], blocks: List[int]) -> None:
        for e, b in zip(entries, blocks):
            e.pins += 1
            self._restore_q.append((e, int(b)))
        self.restored_blocks += len(entries)
        self.restored_tokens += len(entries) * KV_BS

    # -- device work ------------------------------------------------------------------------------
    def _on_stream(self, stream):
        return torch.cuda.stream(stream) if self.cuda else contextlib.nullcontext()

    def _stage_ids(self, ids: List[int]) -> torch.Tensor:
        t = self._ids_turn
        self._ids_turn ^= 1
        if self._ids_used[t]:
            self._ids_event[t].synchronize()           # queued two drains ago: complete long since
        n = len(ids)
        host, dev = self._ids_host[t], self._ids_dev[t]
        host[:n] = torch.tensor(ids, dtype=torch.int32)
        dev[:n].copy_(host[:n], non_blocking=True)
        self._ids_event[t].record()
        self._ids_used[t] = True
        return dev

    def drain(self) -> None:
        """Run the queued saves, then the queued restores, on the current (compute) stream; the
        engine calls this immediately before every step launch."""
        if not self._save_q and not self._restore_q:
            return
        self._poll()
        saves, self._save_q = self._save_q, []
        # one restore per device block: of two queued for one block (the first one's sequence gave the
        # block back before any step ran), the later is the owner's
        last: Dict[int, _Entry] = {}
        for e, b in self._restore_q:
            old = last.pop(b, None)
            if old is not None:
                old.pins -= 1
            last[b] = e
        restores = [(e, b) for b, e in last.items()]
        self._restore_q = []
        # saves that find no free staging chunk are dropped now: their blocks may be rewritten by the
        # step about to launch
        cb = self.chunk_blocks
        parts: List[Tuple[_Chunk, int, List[Tuple[int, _Entry]]]] = []
        free = [i for i, c in enumerate(self._save_chunks) if c.entries is None]
        pos = 0
        while pos < len(saves) and free:
            i = free.pop(0)
            parts.append((self._save_chunks[i], i, saves[pos:pos + cb]))
            pos += cb
        for _, e in saves[pos:]:
            e.pins -= 1
            self._remove(e)
            self.save_skipped += 1
        ids = [b for _, _, part in parts for b, _ in part] + [b for _, b in restores]
        if not ids:
            return
        ids_dev = self._stage_ids(ids)
        cur = torch.cuda.current_stream(self.device) if self.cuda else None
        copy, load = self._copy_stream, self._load_stream
        rparts = [restores[k:k + cb] for k in range(0, len(restores), cb)]

        def load_part(idx: int) -> _Chunk:             # H2D of restore part idx into its staging chunk
            c = self._restore_chunks[idx & 1]
            with self._on_stream(load):
                if c.used:                             # the chunk's previous scatter has read it
                    self._wait(load, self._scattered[idx & 1])
                for j, s0, m in _runs([e.slot for e, _ in rparts[idx]]):
                    c.stage[j:j + m].copy_(self.store[s0:s0 + m], non_blocking=True)
                self._record(c.event, load)
            return c
        # the H2D copies of the first two restore parts are queued first: they depend on nothing of
        # this drain, and the restore's latency then does not include the host time of queuing the saves
        for idx in range(min(2, len(rparts))):
            load_part(idx)
        off = 0
        for c, i, part in parts:
            n = len(part)
            K.gather_blocks(self.kv.buf, ids_dev[off:off + n], c.stage)
            off += n
            self._record(self._gathered[i], cur)
            with self._on_stream(copy):
                self._wait(copy, self._gathered[i])
                for j, s0, m in _runs([e.slot for _, e in part]):
                    self.store[s0:s0 + m].copy_(c.stage[j:j + m], non_blocking=True)
                self._record(c.event, copy)
            c.entries = [e for _, e in part]
            self.saved_blocks += n
        for idx, part_r in enumerate(rparts):
            n = len(part_r)
            c = load_part(idx) if idx >= 2 else self._restore_chunks[idx & 1]
            self._wait(cur, c.event)
            K.scatter_blocks(self.kv.buf, ids_dev[off:off + n], c.stage)
            off += n
            self._record(self._scattered[idx & 1], cur)
            c.used = True
        if restores:
            done = self._new_event()
            self._record(done, load)
            self._restoring.append((done, [e for e, _ in restores]))
        self._poll()

    def _record(self, event, stream) -> None:
        if self.cuda:
            event.record(stream)
        else:
            event.record()

    def _wait(self, stream, event) -> None:
        if self.cuda:
            stream.wait_event(event)

    def synchronize(self) -> None:
        """Wait for every copy in flight (tests, benchmarks): saved entries become visible."""
        if self.cuda:
            self._copy_stream.synchronize()
            self._load_stream.synchronize()
        self._poll()

    @property
    def used(self) -> int:
        return len(self._index)

    def stats(self) -> Dict[str, int]:
        return {"host_kv_slots": self.slots, "host_kv_used": self.used, "host_kv_saved_blocks": self.saved_blocks,
                "host_kv_save_skipped": self.save_skipped, "host_kv_lookups": self.lookups,
                "host_kv_hit_blocks": self.hit_blocks, "host_kv_restored_blocks": self.restored_blocks,
                "host_kv_restored_tokens": self.restored_tokens, "host_kv_evictions": self.evictions}


class TieredBlockManager:
    """``inner`` (either block manager) with a host tier behind it: the interface the scheduler uses.

    ``match_prefix`` extends the inner manager's HBM match by the tier's run of blocks -- as many as
    ``inner.grow`` accepts -- queues their restores and commits them, so they carry their hashes and
    later sequences hit them in HBM; restored tokens cost no step budget.  ``free`` saves the sequence's
    full blocks first, which makes a preemption a swap instead of a recompute (see ``match_prefix`` for
    how a preempted sequence waits for its swap-in); a sequence marked ``kv_discard`` (an abort: the
    engine sets it) saves nothing.  Everything else is the inner manager's.
    """

    def __init__(self, inner, tier: HostKVTier):
        self.inner, self.tier = inner, tier
        self.num_blocks, self.block_size = inner.num_blocks, inner.block_size
        self.enable_prefix_caching = inner.enable_prefix_caching
        self.can_grow, self.commit = inner.can_grow, inner.commit
        self.num_free, self.usage, self.blocks_needed, self.hit_rate = (inner.num_free, inner.usage,
                                                                        inner.blocks_needed, inner.hit_rate)

    def __getattr__(self, name):                       # hits, queries, evictions, ...: the inner manager's
        inner = self.__dict__.get("inner")
        if inner is None:
            raise AttributeError(name)
        return getattr(inner, name)

    def match_prefix(self, seq: Sequence) -> int:
        if seq.block_table:
            return 0
        seq.tier_wait = False
        self.inner.match_prefix(seq)
        start = len(seq.block_table)
        tier = self.tier
        run = tier.lookup(seq, start)
        # Swap-in of a preempted sequence.  The scheduler matches a waiting sequence once, at its first
        # admission attempt -- for a preempted one that is the step that preempted it, with the pool dry
        # and its save not even copied.  While the tier holds (or is about to hold) blocks of it and the
        # pool cannot take the sequence, the attempt is refused with nothing attached (``grow`` says no
        # until the next ``match_prefix``), so the scheduler asks again next step: the sequence comes back
        # whole, over PCIe, when there is room, and pins no HBM while it waits.  Bounded per sequence.
        if seq.num_preemptions and (run or tier.lookup_pending) and seq.tier_waits < MAX_SWAP_WAITS \
                and self.inner.num_free() < self.inner.blocks_needed(seq, seq.num_tokens):
            tier.lookups -= 1                          # counted when it is served
            tier.hit_blocks -= len(run)
            self.inner.free(seq)
            seq.num_computed = seq.num_cached_prompt = 0
            seq.tier_wait = True
            seq.tier_waits += 1
            tier.swap_waits += 1
            return 0
        k = min(len(run), self.inner.num_free())
        if k > 0 and self.inner.grow(seq, (start + k) * self.block_size):
            self.tier.queue_restore(run[:k], seq.block_table[start:start + k])
            seq.num_computed = (start + k) * self.block_size
            seq.num_cached_prompt = seq.num_computed
            self.inner.commit(seq)
        return seq.num_computed

    def grow(self, seq: Sequence, total_tokens: int) -> bool:
        if seq.tier_wait and not seq.block_table:
            return False                               # waiting for room to be swapped in (match_prefix)
        return self.inner.grow(seq, total_tokens)

    def free(self, seq: Sequence, evict_first: bool = False) -> None:
        if seq.block_table and not seq.kv_discard:
            self.tier.save(seq)
        self.inner.free(seq, evict_first)
