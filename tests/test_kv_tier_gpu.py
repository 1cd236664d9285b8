"""Host-memory KV tier on the GPU: the gather / scatter kernels against the torch oracle, 64-bit offsets,
the round trip through pinned memory, and the engine restoring an evicted prefix, swapping a preempted
sequence and keeping its default decode graphs.

Every comparison in this file is bit-exact (``torch.equal`` on byte views): the tier moves bytes, no
tolerance is involved anywhere.
"""
import pytest
import torch

from financial_chatbot_llm_amd.config import EngineConfig
from financial_chatbot_llm_amd.engine import LLMEngine, SamplingParams
from financial_chatbot_llm_amd.engine.kv_host_tier import HostKVTier, TieredBlockManager
from financial_chatbot_llm_amd.models.common import KVCache
from financial_chatbot_llm_amd.ops import gather_blocks, scatter_blocks
from financial_chatbot_llm_amd.ops.kv_tier import pool_planes

pytestmark = pytest.mark.gpu
DEV = "cuda"
BS = 64
L, HKV, D = 2, 2, 128           # llama-tiny: planes = 4, plane_bytes = 32 KiB bf16 / 16 KiB fp8
CHUNK = 16


def _oracle_gather(pool, ids, staging):
    return gather_blocks(pool.cpu(), ids.cpu(), staging.cpu())


def _oracle_scatter(pool, ids, staging):
    return scatter_blocks(pool.cpu(), ids.cpu(), staging.cpu())


def _random_bytes(shape, seed, dtype=torch.uint8):
    g = torch.Generator().manual_seed(seed)
    n = 1
    for s in shape:
        n *= s
    raw = torch.randint(0, 256, (n * torch.empty((), dtype=dtype).element_size(),), dtype=torch.uint8, generator=g)
    return raw.view(dtype).reshape(shape).to(DEV)


def _ids(n, nb):
    """n distinct ids that hold block 0 and the last block (as far as n allows), in no order."""
    rest = [(7 * i + 3) % (nb - 2) + 1 for i in range(nb)]
    out = [nb - 1, 0] + list(dict.fromkeys(rest))
    return out[:n] if n > 1 else [nb - 1]


# -- kernels against the oracle -------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, CHUNK])
@pytest.mark.parametrize("dtype,tail", [(torch.bfloat16, 16 * 1024), (torch.uint8, 16 * 1024), (torch.uint8, 48),
                                        (torch.bfloat16, 24)])
def test_kernels_match_the_torch_oracle(n, dtype, tail):
    """bf16 and uint8 pools at plane_bytes 32 KiB (bf16 x 16 Ki elements), 16 KiB and 48 B -- a tail far
    smaller than one workgroup pass."""
    nb, planes = 40, 4
    pool = _random_bytes((planes, nb, tail), seed=n + tail, dtype=dtype)
    pb = tail * pool.element_size()
    assert pb in (32 * 1024, 16 * 1024, 48)
    before = pool.clone()
    for ids in [_ids(n, nb)] + ([[0]] if n == 1 else []):
        idt = torch.tensor(ids, dtype=torch.int32, device=DEV)
        staging = torch.full((CHUNK, planes, pb), 0x5A, dtype=torch.uint8, device=DEV)
        want = _oracle_gather(before, idt, staging.clone())
        gather_blocks(pool, idt, staging)
        assert torch.equal(staging.cpu(), want)
        assert bool((staging[n:] == 0x5A).all())                   # rows >= n: untouched
        assert torch.equal(pool.view(torch.uint8), before.view(torch.uint8))
        # scatter other bytes into the same ids: every other block keeps its bytes
        src = _random_bytes((CHUNK, planes, pb), seed=99 + n)
        want_pool = _oracle_scatter(before.clone(), idt, src)
        work = before.clone()
        scatter_blocks(work, idt, src)
        assert torch.equal(work.cpu().view(torch.uint8), want_pool.view(torch.uint8))
        others = [b for b in range(nb) if b not in ids]
        assert torch.equal(pool_planes(work)[:, others], pool_planes(before)[:, others])
        back = torch.zeros_like(staging)
        gather_blocks(work, idt, back)
        assert torch.equal(back[:n], src[:n])


@pytest.mark.parametrize("bad", [-1, 40, 2 ** 31 - 1, -2 ** 31])
def test_an_out_of_range_id_changes_nothing(bad):
    nb, planes, pb = 40, 4, 16 * 1024
    pool = _random_bytes((planes, nb, pb), seed=5)
    before = pool.clone()
    ids = torch.tensor([3, bad, 39], dtype=torch.int32, device=DEV)
    staging = torch.full((4, planes, pb), 0x77, dtype=torch.uint8, device=DEV)
    gather_blocks(pool, ids, staging)
    assert torch.equal(staging[0], before[:, 3]) and torch.equal(staging[2], before[:, 39])
    assert bool((staging[1] == 0x77).all()) and bool((staging[3] == 0x77).all())
    src = _random_bytes((4, planes, pb), seed=6)
    scatter_blocks(pool, ids, src)
    torch.cuda.synchronize()
    assert torch.equal(pool[:, 3], src[0]) and torch.equal(pool[:, 39], src[2])
    others = [b for b in range(nb) if b not in (3, 39)]
    assert torch.equal(pool[:, others], before[:, others])


def test_offsets_are_64_bit():
    """2 planes x 70,000 blocks x 32 KiB = 4.6 GB: block 69,999 of plane 1 lies beyond 2^32 bytes; an
    offset truncated to 32 bits would land in block 69,999 - 65,536 of the same plane."""
    planes, nb, pb = 2, 70_000, 32 * 1024
    pool = torch.empty((planes, nb, pb), dtype=torch.uint8, device=DEV)
    far, alias = nb - 1, nb - 1 - 65_536
    assert (nb + far) * pb >= 2 ** 32 and (far - alias) * pb == 2 ** 31
    pool[:, alias] = 0x11
    pool[:, far] = 0x22
    keep = pool[:, alias].clone()
    src = _random_bytes((1, planes, pb), seed=8)
    ids = torch.tensor([far], dtype=torch.int32, device=DEV)
    scatter_blocks(pool, ids, src)
    back = torch.zeros_like(src)
    gather_blocks(pool, ids, back)
    assert torch.equal(back, src) and torch.equal(pool[:, far], src[0])
    assert torch.equal(pool[:, alias], keep)
    for wrapped in (far - 2 ** 17, far - 2 ** 16):                 # offsets wrapped at 2^32 and 2^31 bytes
        assert not torch.equal(pool[1, wrapped], src[0, 1])
    del pool
    torch.cuda.empty_cache()


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_round_trip_through_pinned_memory(kv_dtype):
    from financial_chatbot_llm_amd.engine.sequence import Sequence
    nb = 48
    kv = KVCache(L, nb, HKV, D, device=DEV, kv_dtype=kv_dtype)
    pool = pool_planes(kv.buf)
    pool.copy_(_random_bytes(tuple(pool.shape), seed=11))
    tier = HostKVTier(kv, 64 * KVCache.bytes_per_block(L, HKV, D, elt=kv.elt), chunk_blocks=CHUNK)
    assert tier.store.is_pinned() and tier.plane_bytes == HKV * BS * D * kv.elt
    # 40 blocks: more than the two save chunks of one drain, so the save goes out in two drains
    table = [nb - 1, 0] + list(range(5, 43))
    toks = list(range(1000, 1000 + len(table) * BS))
    want = pool[:, table].clone()
    for queued in (len(table), len(table) - 2 * CHUNK):            # the first drain drops what two chunks cannot take
        s = Sequence("s", toks, SamplingParams())
        s.block_table, s.num_computed = table, len(toks)
        assert tier.save(s) == queued
        tier.drain()
        tier.synchronize()
    assert tier.stats()["host_kv_saved_blocks"] == len(table) and tier.stats()["host_kv_save_skipped"] == 8
    pool.zero_()                                                   # HBM forgets them
    probe = Sequence("p", toks + [1], SamplingParams())
    run = tier.lookup(probe, 0)
    assert len(run) == len(table)
    dest = list(reversed(table))                                   # restored somewhere else: 3 chunks, 2 stagings
    tier.queue_restore(run, dest)
    tier.drain()
    torch.cuda.synchronize()
    assert torch.equal(pool[:, dest], want)
    rest = [b for b in range(nb) if b not in dest]
    assert bool((pool[:, rest] == 0).all())
    tier.synchronize()
    assert all(e.pins == 0 for e in run)


# -- engine ----------------------------------------------------------------------------------------------
PROMPT_A = [1000 + (i * 7919) % 3000 for i in range(6 * BS + 10)]
FILLERS = [[5000 + k * 4000 + (i * 104729) % 3500 for i in range(10 * BS + 5)] for k in range(2)]
GREEDY = SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True, logprobs=True)
BLOCK_BYTES = KVCache.bytes_per_block(L, HKV, D)


def _engine(kv_dtype="bf16", blocks=128, host_slots=0, **kw):
    elt = 1 if kv_dtype == "fp8" else 2
    cfg = dict(model="llama-tiny", device=DEV, num_kv_blocks=blocks, max_model_len=2048, max_num_seqs=4,
               graph_batch_sizes=(1, 2, 4), kv_dtype=kv_dtype,
               host_kv_gb=host_slots * BLOCK_BYTES * elt // 2 / 2 ** 30)
    cfg.update(kw)
    return LLMEngine(EngineConfig(**cfg))


def _run(eng, name, prompt, params=GREEDY):
    """One request alone, to the end: (sequence, its block table while it ran, new prefill tokens)."""
    t0 = eng.runner.stats["prefill_step_tokens"]
    seq = eng.add_request(name, prompt, params)
    table = []
    while not seq.finished:
        eng.step()
        if len(seq.block_table) > len(table):
            table = list(seq.block_table)
    while eng.has_work():
        eng.step()
    return seq, table, eng.runner.stats["prefill_step_tokens"] - t0


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_engine_restores_an_evicted_prefix_bit_exactly(kv_dtype):
    full = (len(PROMPT_A) - 1) // BS
    assert full == 6
    outs = {}
    for which, eng in (("control", _engine(kv_dtype, blocks=128)),
                       ("tiered", _engine(kv_dtype, blocks=12, host_slots=64))):
        assert isinstance(eng.bm, TieredBlockManager) == (which == "tiered")
        first = _run(eng, "a1", PROMPT_A)
        assert first[0].num_cached_prompt == 0 and first[2] == len(PROMPT_A)
        for k, f in enumerate(FILLERS):
            _run(eng, f"f{k}", f)
        if eng.tier is not None:
            eng.tier.synchronize()
        before = eng.stats()
        seq, table, computed = _run(eng, "a2", PROMPT_A)
        torch.cuda.synchronize()
        outs[which] = (seq, table, computed, before, eng.stats(), eng)
    cs, ctable, ccomp, cb, ca, ceng = outs["control"]
    ts, ttable, tcomp, tb, ta, teng = outs["tiered"]
    # the control hit its whole prefix in HBM, the tiered engine lost it and got it back from the host
    assert ca["kv_evictions"] == 0 and cs.num_cached_prompt == full * BS and ccomp == len(PROMPT_A) - full * BS
    assert ta["kv_evictions"] > 0 and tb["kv_evictions"] > 0
    assert ta["host_kv_restored_blocks"] - tb["host_kv_restored_blocks"] == full
    assert ta["host_kv_restored_tokens"] - tb["host_kv_restored_tokens"] == full * BS
    assert ts.num_cached_prompt == full * BS and tcomp == len(PROMPT_A) - full * BS
    assert tb["host_kv_saved_blocks"] >= full and ta["host_kv_slots"] == 64
    # same step shapes, same bytes in: the same tokens and log-probabilities out
    assert ts.output_ids == cs.output_ids and len(ts.output_ids) == 8
    assert ts.output_logprobs == cs.output_logprobs and all(v is not None for v in ts.output_logprobs)
    tp, cp = pool_planes(teng.kv.buf), pool_planes(ceng.kv.buf)
    assert len(ttable) >= full and len(ctable) >= full
    assert torch.equal(tp[:, ttable[:full]], cp[:, ctable[:full]])
    assert bool(tp[:, ttable[:full]].any())


# one long-running request and three that cross a block boundary in the same step: the youngest is
# preempted, the others' growth recycles two of its full blocks in that very step
PREEMPT = dict(blocks=12, prompt_lens=(60, 200, 200, 200), max_tokens=(300, 120, 120, 120))


@pytest.mark.parametrize("overlap", [True, False])
def test_a_preempted_sequence_is_swapped_in_again(overlap):
    """The pool forces a preemption; the preempted sequence waits with nothing attached until the pool
    can take it, gets the blocks HBM recycled back from the host, and finishes.  (Its tokens are not
    compared with an engine that never preempted: the positions after its last full block are recomputed
    by a prefill chunk, whose f32 summation order differs from the decode steps'.)"""
    eng = _engine(blocks=PREEMPT["blocks"], host_slots=64, async_scheduling=overlap)
    params = [SamplingParams(temperature=0.0, max_tokens=m, ignore_eos=True) for m in PREEMPT["max_tokens"]]
    prompts = [[2000 + 50 * k + (i * 31) % 900 for i in range(n)] for k, n in enumerate(PREEMPT["prompt_lens"])]
    seqs = [eng.add_request(f"p{k}", p, q) for k, (p, q) in enumerate(zip(prompts, params))]
    steps = 0
    while eng.has_work():
        eng.step()
        steps += 1
        assert steps < 4000
    st = eng.stats()
    print({k: v for k, v in st.items() if k.startswith("host_kv") or k in ("preemptions", "kv_evictions")},
          eng.tier.swap_waits, steps)
    assert st["preemptions"] > 0 and st["host_kv_restored_blocks"] > 0 and eng.tier.swap_waits > 0, st
    assert st["host_kv_restored_blocks"] == st["host_kv_hit_blocks"]
    assert all(s.finished and s.finish_reason == "length" for s in seqs)
    assert [len(s.output_ids) for s in seqs] == list(PREEMPT["max_tokens"])
    assert all(-1 not in s.output_ids for s in seqs)
    swapped = [s for s in seqs if s.num_preemptions]
    assert sum(s.num_cached_prompt for s in swapped) >= st["host_kv_restored_tokens"] > 0
    assert eng.bm.num_free() == PREEMPT["blocks"]                  # every block back


def test_the_tier_adds_no_graph_twin():
    p = SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True)
    seen = []
    for slots in (0, 64):
        eng = _engine(blocks=32, host_slots=slots)
        eng.warmup()
        out = eng.generate([PROMPT_A[:150]], p)[0]
        seen.append((out, sorted(eng.runner.graphs), {b: g.fused for b, g in eng.runner.graphs.items()},
                     dict(eng.runner.twins), eng.runner.stats["graph_steps"], eng.runner.stats["steps"]))
    off, on = seen
    assert on == off and off[3] == {} and off[4] > 0
