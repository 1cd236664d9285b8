"""Host-memory KV tier on CPU tensors: the exact chain index, the slot LRU with its pins, save / lookup
rules, the block-manager wrapper on both managers, the config refusals and the ops' torch paths."""
import pytest
import torch

from financial_chatbot_llm_amd.config import EngineConfig
from financial_chatbot_llm_amd.engine.block_manager import PyBlockManager
from financial_chatbot_llm_amd.engine.kv_host_tier import HostKVTier, TieredBlockManager
from financial_chatbot_llm_amd.engine.scheduler import Scheduler
from financial_chatbot_llm_amd.engine.sequence import PENDING, SamplingParams, Sequence
from financial_chatbot_llm_amd.models.common import KVCache
from financial_chatbot_llm_amd.ops import gather_blocks, scatter_blocks

BS = 64
L, HKV, D = 2, 2, 128           # llama-tiny: planes = 4, plane_bytes = 32 KiB bf16


def _managers():
    out = [PyBlockManager]
    try:
        from financial_chatbot_llm_amd.engine.native_block_manager import NativeBlockManager
        NativeBlockManager(4)
        out.append(NativeBlockManager)
    except Exception:  # noqa: BLE001 - native runtime not built
        pass
    return out


MANAGERS = _managers()


class FakeEvent:
    """An event the test completes by hand."""
    live = []

    def __init__(self):
        self.done = True
        self.recorded = False
        FakeEvent.live.append(self)

    def record(self, stream=None):
        self.done = False
        self.recorded = True

    def query(self):
        return self.done

    def synchronize(self):
        self.done = True

    @classmethod
    def complete_all(cls):
        for e in cls.live:
            e.done = True


def make(num_blocks=32, slots=16, chunk=16, events=None, kv_dtype="bf16"):
    kv = KVCache(L, num_blocks, HKV, D, device="cpu", kv_dtype=kv_dtype)
    g = torch.Generator().manual_seed(1)
    raw = torch.randint(0, 256, (kv.buf.numel() * kv.buf.element_size(),), dtype=torch.uint8, generator=g)
    kv.buf.view(torch.uint8).reshape(-1).copy_(raw)
    per_block = KVCache.bytes_per_block(L, HKV, D, elt=kv.elt)
    tier = HostKVTier(kv, slots * per_block, chunk_blocks=chunk, event_factory=events)
    assert tier.slots == slots and tier.planes == 2 * L and tier.plane_bytes == HKV * BS * D * kv.elt
    return kv, tier


def seq_of(tokens, computed=None, table=None, salt=0, **params):
    s = Sequence("r", list(tokens), SamplingParams(**params))
    s.cache_salt = salt
    s.num_computed = len(tokens) if computed is None else computed
    s.block_table = list(range((s.num_computed + BS - 1) // BS)) if table is None else list(table)
    return s


def prompt(n, base=0):
    return [base + i for i in range(n)]


def block_bytes(kv, b):
    return kv.buf.view(torch.uint8).reshape(2 * L, kv.num_blocks, -1)[:, b].clone()


def saved(tier, tokens, salt=0):
    """Ready blocks of the chain of ``tokens`` (a probe one token longer, so every full block counts)."""
    probe = seq_of(list(tokens) + [7], computed=0, table=[], salt=salt)
    return len(tier.lookup(probe, 0))


# -- index ---------------------------------------------------------------------------------------------
def test_equal_prompts_share_entries_and_a_differing_token_misses_from_its_block_on():
    kv, tier = make()
    a = prompt(4 * BS)
    assert tier.save(seq_of(a)) == 4
    tier.drain()
    assert tier.save(seq_of(a)) == 0 and tier.used == 4           # the same chain: nothing new
    assert saved(tier, a) == 4
    for i in range(4):
        b = list(a)
        b[i * BS + 5] += 1000                                      # one token of block i differs
        assert saved(tier, b) == i
        q = seq_of(b)
        assert tier.save(q) == 4 - i                               # blocks i.. are new entries, 0..i-1 shared
        tier.drain()
    assert tier.used == 4 + 4 + 3 + 2 + 1


def test_cache_salts_never_share_entries():
    kv, tier = make()
    a = prompt(3 * BS)
    assert tier.save(seq_of(a, salt=0)) == 3
    tier.drain()
    assert saved(tier, a, salt=0) == 3 and saved(tier, a, salt=12345) == 0
    assert tier.save(seq_of(a, salt=12345)) == 3                   # the adapter's own chain
    tier.drain()
    assert saved(tier, a, salt=12345) == 3 and saved(tier, a, salt=999) == 0 and tier.used == 6


def test_saved_run_is_visible_only_after_its_copy_completed():
    FakeEvent.live.clear()
    kv, tier = make(events=FakeEvent)
    a = prompt(3 * BS)
    tier.save(seq_of(a))
    assert saved(tier, a) == 0                                     # queued, not even gathered
    tier.drain()
    assert saved(tier, a) == 0                                     # D2H in flight
    FakeEvent.complete_all()
    assert saved(tier, a) == 3
    assert tier.stats()["host_kv_saved_blocks"] == 3


def test_saved_bytes_are_the_blocks_bytes():
    kv, tier = make()
    a = prompt(2 * BS)
    tier.save(seq_of(a, table=[9, 4]))
    tier.drain()
    run = tier.lookup(seq_of(a + [1], computed=0, table=[]), 0)
    assert [torch.equal(tier.store[e.slot], block_bytes(kv, b)) for e, b in zip(run, (9, 4))] == [True, True]


# -- LRU -----------------------------------------------------------------------------------------------
def test_tail_first_touch_a_chain_loses_its_last_block_first():
    kv, tier = make(slots=4)
    a = prompt(4 * BS)
    tier.save(seq_of(a))
    tier.drain()
    assert saved(tier, a) == 4                                     # a hit: touched tail first, root last

    def held():                                                    # the chain's entries, without touching them
        n, parent = 0, tier._root(seq_of(a))
        while n < 4 and tier._block_key(parent, a[n * BS:(n + 1) * BS]) in tier._index:
            parent = tier._index[tier._block_key(parent, a[n * BS:(n + 1) * BS])].uid
            n += 1
        return n
    for k, want in ((1, 3), (2, 2), (3, 1)):
        tier.save(seq_of(prompt(BS, base=10_000 * k)))             # one new block: one eviction
        tier.drain()
        assert held() == want and tier.evictions == k


def test_slots_exhausted_evicts_the_oldest_and_counts():
    kv, tier = make(slots=4)
    chains = [prompt(2 * BS, base=10_000 * k) for k in range(3)]
    for c in chains:
        tier.save(seq_of(c))
        tier.drain()
    assert tier.used == 4 and tier.stats()["host_kv_evictions"] == 2
    assert [saved(tier, c) for c in chains] == [0, 2, 2]
    assert tier.stats()["host_kv_slots"] == 4 and tier.stats()["host_kv_used"] == 4


def test_a_slot_with_a_queued_restore_survives_lru_pressure():
    kv, tier = make(slots=2)
    a = prompt(2 * BS)
    tier.save(seq_of(a))
    tier.drain()
    run = tier.lookup(seq_of(a + [1], computed=0, table=[]), 0)
    tier.queue_restore(run[:1], [20])                              # block 0 of the chain is pinned now
    want = tier.store[run[0].slot].clone()
    q = seq_of(prompt(2 * BS, base=50_000))
    assert tier.save(q) == 1                                       # one slot could be taken, not two
    assert tier.stats()["host_kv_save_skipped"] == 1 and run[0].slot not in tier._free_slots
    assert tier._index[run[0].key] is run[0] and run[1].key not in tier._index
    tier.drain()
    assert torch.equal(block_bytes(kv, 20), want)                  # the restore read the pinned slot
    assert run[0].pins == 0                                        # ... and released it


def test_save_never_waits_for_a_staging_chunk():
    FakeEvent.live.clear()
    kv, tier = make(slots=16, chunk=2, events=FakeEvent)
    tier.save(seq_of(prompt(6 * BS)))
    tier.drain()                                                   # 2 chunks x 2 blocks in flight, 2 dropped
    st = tier.stats()
    assert st["host_kv_saved_blocks"] == 4 and st["host_kv_save_skipped"] == 2 and st["host_kv_used"] == 4
    tier.save(seq_of(prompt(2 * BS, base=70_000)))
    tier.drain()                                                   # both chunks still busy: all dropped
    assert tier.stats()["host_kv_save_skipped"] == 4 and tier.used == 4
    FakeEvent.complete_all()
    assert saved(tier, prompt(6 * BS)) == 4


# -- what save covers ------------------------------------------------------------------------------------
def test_save_covers_full_computed_blocks_only():
    kv, tier = make()
    a = prompt(4 * BS)
    assert tier.save(seq_of(a, computed=3 * BS - 1, table=[0, 1, 2])) == 2     # block 2 is one token short
    assert tier.save(seq_of(prompt(4 * BS, base=9000), computed=4 * BS, table=[5, 6])) == 2   # table ends first


def test_ephemeral_kv_saves_nothing_past_num_cached_prompt():
    kv, tier = make()
    s = seq_of(prompt(4 * BS), ephemeral_kv=True)
    s.num_cached_prompt = BS + 10
    assert tier.save(s) == 1
    s2 = seq_of(prompt(4 * BS, base=9000), ephemeral_kv=True)
    assert tier.save(s2) == 0


def test_a_block_holding_pending_and_everything_after_it_is_not_saved():
    kv, tier = make()
    toks = prompt(2 * BS - 1)
    s = seq_of(toks)
    s.output_ids = [PENDING] + [5] * BS                           # PENDING is the last token of block 1
    s.num_computed = s.num_tokens
    s.block_table = [0, 1, 2]
    assert tier.save(s) == 1
    tier.drain()
    assert tier.used == 1


def test_an_unverified_draft_is_not_saved():
    kv, tier = make()
    s = seq_of(prompt(BS + 60))
    s.output_ids = [3, 4, 5, 6, 7]                                 # a last token + 4 draft tokens, in flight
    s.spec_rows = 5
    s.num_computed = s.num_tokens                                  # 129: two full blocks by count
    s.block_table = [0, 1, 2]
    assert tier.save(s) == 1                                       # positions < 124 are resolved


# -- the wrapper ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("BM", MANAGERS)
def test_match_prefix_restores_commits_and_leaves_a_token(BM):
    kv, tier = make(num_blocks=12)
    bm = TieredBlockManager(BM(12, BS, True), tier)
    a = prompt(4 * BS)                                             # 4 full blocks, none left to compute after them
    s1 = Sequence("a", a, SamplingParams())
    assert bm.match_prefix(s1) == 0 and bm.grow(s1, len(a))
    s1.num_computed = len(a)
    bm.commit(s1)
    table = list(s1.block_table)
    want = [block_bytes(kv, b) for b in table]
    bm.free(s1)                                                    # a finish: saved
    tier.drain()
    assert tier.stats()["host_kv_saved_blocks"] == 4
    # push the blocks out of HBM: a filler takes the whole pool
    f = Sequence("f", prompt(12 * BS - 1, base=100_000), SamplingParams())
    bm.match_prefix(f)
    assert bm.grow(f, len(f.prompt_ids))
    assert bm.evictions >= 4
    kv.buf.zero_()
    f.num_computed = 0
    f.kv_discard = True
    bm.free(f)
    # the same prompt again: the inner manager has nothing, the tier everything but the last block
    s2 = Sequence("a2", a, SamplingParams())
    lookups = tier.stats()["host_kv_lookups"]
    got = bm.match_prefix(s2)
    assert got == 3 * BS and s2.num_computed == 3 * BS and s2.num_cached_prompt == 3 * BS     # >= 1 token left
    assert len(s2.block_table) == 3
    st = tier.stats()
    assert st["host_kv_restored_blocks"] == 3 and st["host_kv_restored_tokens"] == 3 * BS
    assert st["host_kv_lookups"] == lookups + 1 and st["host_kv_hit_blocks"] == 3
    tier.drain()
    assert all(torch.equal(block_bytes(kv, b), w) for b, w in zip(s2.block_table, want))
    # committed: a third sequence, one block longer, hits the restored blocks in the inner manager and
    # gets the fourth from the tier
    hits = bm.hits
    s3 = Sequence("a3", a + prompt(10, base=5000), SamplingParams())
    assert bm.match_prefix(s3) == 4 * BS
    assert s3.block_table[:3] == s2.block_table and bm.hits == hits + 3
    assert tier.stats()["host_kv_restored_blocks"] == 4
    tier.drain()
    assert torch.equal(block_bytes(kv, s3.block_table[3]), want[3])


@pytest.mark.parametrize("BM", MANAGERS)
def test_match_prefix_adds_the_restored_tokens_to_the_inner_match(BM):
    kv, tier = make(num_blocks=16)
    bm = TieredBlockManager(BM(16, BS, True), tier)
    a = prompt(5 * BS + 3)
    s1 = Sequence("a", a, SamplingParams())
    bm.match_prefix(s1)
    bm.grow(s1, len(a))
    s1.num_computed = len(a)
    bm.commit(s1)
    bm.free(s1)
    tier.drain()
    # a sequence sharing only the first two blocks stays resident; the rest of the pool is recycled
    keep = Sequence("k", a[:2 * BS] + prompt(5, base=777), SamplingParams())
    assert bm.match_prefix(keep) == 2 * BS and bm.grow(keep, keep.num_tokens)
    f = Sequence("f", prompt(13 * BS, base=100_000), SamplingParams())
    bm.match_prefix(f)
    assert bm.grow(f, f.num_tokens)
    f.kv_discard = True
    bm.free(f)
    s2 = Sequence("a2", a, SamplingParams())
    inner_hits = bm.hits
    assert bm.match_prefix(s2) == 5 * BS
    assert bm.hits == inner_hits + 2                               # two blocks from HBM, three from the tier
    assert s2.num_computed == s2.num_cached_prompt == 5 * BS
    assert tier.stats()["host_kv_restored_blocks"] == 3 and tier.stats()["host_kv_hit_blocks"] == 3


@pytest.mark.parametrize("BM", MANAGERS)
def test_match_prefix_restores_fewer_blocks_or_none_when_grow_refuses(BM):
    kv, tier = make(num_blocks=8)
    bm = TieredBlockManager(BM(8, BS, True), tier)
    a = prompt(4 * BS + 1)
    tier.save(seq_of(a))
    tier.drain()
    hog = Sequence("h", prompt(6 * BS, base=100_000), SamplingParams())
    bm.match_prefix(hog)
    assert bm.grow(hog, hog.num_tokens) and bm.num_free() == 2
    s = Sequence("a", a, SamplingParams())
    assert bm.match_prefix(s) == 2 * BS and len(s.block_table) == 2          # the two blocks grow accepts
    assert tier.stats()["host_kv_restored_blocks"] == 2 and bm.num_free() == 0
    s2 = Sequence("b", a, SamplingParams())
    s2.cache_salt = 0
    hits = bm.hits
    assert bm.match_prefix(s2) == 2 * BS and bm.hits == hits + 2             # HBM only: no block is free
    assert tier.stats()["host_kv_restored_blocks"] == 2 and len(s2.block_table) == 2


@pytest.mark.parametrize("BM", MANAGERS)
def test_a_preempted_sequence_waits_unattached_for_its_swap_in(BM):
    FakeEvent.live.clear()
    kv, tier = make(num_blocks=8, events=FakeEvent)
    bm = TieredBlockManager(BM(8, BS, True), tier)
    a = prompt(3 * BS + 20)
    s = Sequence("a", a, SamplingParams())
    bm.match_prefix(s)
    assert bm.grow(s, len(a))
    s.num_computed = len(a) - 1
    bm.commit(s)
    bm.free(s)                                                     # the preemption's free: 3 blocks queued
    s.num_computed, s.num_preemptions = 0, 1
    hog = Sequence("h", prompt(6 * BS, base=100_000), SamplingParams())
    bm.match_prefix(hog)
    assert bm.grow(hog, hog.num_tokens)                            # recycles its last full block
    tier.drain()
    looked = tier.stats()["host_kv_lookups"]
    # its copy is in flight and the pool is dry: refused, nothing attached, asked again next step
    assert bm.match_prefix(s) == 0 and s.block_table == [] and not bm.grow(s, 64) and s.block_table == []
    FakeEvent.complete_all()
    assert bm.match_prefix(s) == 0 and s.block_table == [] and not bm.grow(s, 64)      # ready, but no room
    assert tier.swap_waits == 2 and tier.stats()["host_kv_lookups"] == looked and bm.num_free() == 2
    hog.kv_discard = True
    bm.free(hog)
    assert bm.match_prefix(s) == 3 * BS and len(s.block_table) == 3                    # room: back whole
    assert tier.stats()["host_kv_restored_blocks"] == 1 and tier.stats()["host_kv_hit_blocks"] == 1
    assert tier.stats()["host_kv_lookups"] == looked + 1 and bm.grow(s, len(a))
    # a sequence that was never preempted takes what fits at once
    fresh = Sequence("f", a, SamplingParams())
    assert bm.match_prefix(fresh) == 3 * BS


@pytest.mark.parametrize("BM", MANAGERS)
def test_abort_saves_nothing_finish_and_preemption_save(BM):
    from financial_chatbot_llm_amd.engine.scheduler import ScheduledBatch
    kv, tier = make(num_blocks=16)
    bm = TieredBlockManager(BM(16, BS, True), tier)
    sched = Scheduler(bm, max_num_seqs=8, max_num_batched_tokens=4096, max_model_len=4096)

    def run(name, base):
        s = Sequence(name, prompt(2 * BS + 5, base=base), SamplingParams())
        sched.add(s)
        batch = sched.schedule()
        assert [q for q, _, _ in batch.prefill] == [s]
        s.num_computed = s.num_tokens
        bm.commit(s)
        return s

    s = run("abort", 0)
    s.kv_discard = True                                            # what LLMEngine.abort sets
    sched.abort(s)
    assert tier.stats()["host_kv_saved_blocks"] == 0 and not tier._save_q
    s = run("finish", 10_000)
    sched.finish(s, "stop")
    assert len(tier._save_q) == 2
    s = run("preempt", 20_000)
    sched._preempt(s, ScheduledBatch())
    assert len(tier._save_q) == 4 and s.num_computed == 0
    tier.drain()
    assert tier.stats()["host_kv_saved_blocks"] == 4


def test_engine_abort_marks_the_sequence_and_the_tier_is_off_by_default():
    from financial_chatbot_llm_amd.engine import LLMEngine
    base = dict(model="llama-tiny", device="cpu", num_kv_blocks=16, max_model_len=512, max_num_batched_tokens=256,
                use_cuda_graph=False)
    off = LLMEngine(EngineConfig(**base))
    assert not isinstance(off.bm, TieredBlockManager) and off.tier is None and off.scheduler.bm is off.bm
    assert type(off.bm).__name__ in ("PyBlockManager", "NativeBlockManager")
    st = off.stats()
    assert st["host_kv_slots"] == 0 and st["host_kv_restored_blocks"] == 0
    per_block = KVCache.bytes_per_block(L, HKV, D)
    on = LLMEngine(EngineConfig(host_kv_gb=8 * per_block / 2 ** 30, **base), model=off.model, tokenizer=off.tokenizer)
    assert isinstance(on.bm, TieredBlockManager) and on.scheduler.bm is on.bm and on.stats()["host_kv_slots"] == 8
    p = SamplingParams(temperature=0.0, max_tokens=4, ignore_eos=True)
    s = on.add_request("x", prompt(2 * BS + 3, base=300), p)
    on.step()
    on.step()
    assert s.num_computed >= 2 * BS
    on.abort("x")
    assert s.kv_discard and on.stats()["host_kv_saved_blocks"] == 0 and not on.tier._save_q
    s = on.add_request("y", prompt(2 * BS + 3, base=300), p)
    while not s.finished:
        on.step()
    on.add_request("z", prompt(5, base=900), p)
    on.step()                                                      # the launch in front of which the saves run
    assert on.stats()["host_kv_saved_blocks"] == 2


def test_engine_config_refusals(monkeypatch):
    assert EngineConfig().host_kv_gb == 0 and EngineConfig().host_kv_chunk_blocks == 16
    for kw, word in ((dict(tp_size=2), "tensor parallel"), (dict(cp_size=2), "context parallel"),
                     (dict(enable_prefix_caching=False), "enable_prefix_caching")):
        with pytest.raises(ValueError, match=word):
            EngineConfig(host_kv_gb=1.0, **kw)
        EngineConfig(host_kv_gb=0.0, **kw)                         # off: nothing to refuse
    monkeypatch.setenv("PENNY_HOST_KV_GB", "2.5")
    assert EngineConfig().host_kv_gb == 2.5
    with pytest.raises(ValueError, match="holds no"):
        HostKVTier(KVCache(L, 4, HKV, D, device="cpu"), 1000)


# -- ops -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_gather_scatter_torch_paths_round_trip(kv_dtype):
    kv, tier = make(num_blocks=10, kv_dtype=kv_dtype)
    planes, pb = tier.planes, tier.plane_bytes
    before = kv.buf.view(torch.uint8).clone()
    ids = torch.tensor([9, 0, 4, -1, 10], dtype=torch.int32)       # first, last, and two out of range
    staging = torch.full((6, planes, pb), 0xAB, dtype=torch.uint8)
    gather_blocks(kv.buf, ids, staging)
    for i, b in enumerate((9, 0, 4)):
        assert torch.equal(staging[i], block_bytes(kv, b))
    assert bool((staging[3:] == 0xAB).all())                       # skipped ids and rows >= n: untouched
    assert torch.equal(kv.buf.view(torch.uint8), before)
    dst = torch.tensor([1, 2, 3, 10, -5], dtype=torch.int32)
    scatter_blocks(kv.buf, dst, staging)
    for b, src in ((1, 9), (2, 0), (3, 4)):
        assert torch.equal(block_bytes(kv, b), before.reshape(planes, 10, -1)[:, src])
    after = kv.buf.view(torch.uint8).reshape(planes, 10, -1)
    others = [b for b in range(10) if b not in (1, 2, 3)]
    assert torch.equal(after[:, others], before.reshape(planes, 10, -1)[:, others])
    with pytest.raises(ValueError):
        gather_blocks(kv.buf, ids, staging[:2])                    # more ids than staging rows
    with pytest.raises(ValueError):
        gather_blocks(kv.buf, ids, torch.zeros((6, planes, pb + 16), dtype=torch.uint8))
