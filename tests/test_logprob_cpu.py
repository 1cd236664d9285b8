"""Prompt scoring on CPU: the reference ``ops.lm_head_logprobs`` / ``merge_logprob_stats`` and
``LLMEngine.score`` with its async, process and CLI wrappers on the tiny Llama.

SCORE_TOL: the chunked-vs-unchunked drift of ``runner.forward_logits`` -> f32 log_softmax on this CPU
engine is 0.0 (measured on the prompts below with 64-token chunks: the f32 reference ops are
row-independent), so twice it is 0 and the bound left is the evaluation error of two f32
log-softmax formulas, 1e-5 (the bound of the first test below: |values| < 32, a few f32 ulps).
"""
import asyncio
import dataclasses
import json

import pytest
import torch

from financial_chatbot_llm_amd import ops
from financial_chatbot_llm_amd.config import EngineConfig
from financial_chatbot_llm_amd.engine import LLMEngine, SamplingParams, ScoreResult
from financial_chatbot_llm_amd.engine.async_engine import AsyncEngine
from financial_chatbot_llm_amd.engine.process_engine import ProcessAsyncEngine
from financial_chatbot_llm_amd.models.common import AttentionMetadata, KVCache
from financial_chatbot_llm_amd.ops.attention import KV_BS

CFG = dict(model="llama-tiny", device="cpu", max_model_len=1024, max_num_batched_tokens=256,
           use_cuda_graph=False, max_num_seqs=8, num_kv_blocks=64)
SCORE_TOL = 1e-5
NEG_INF = float("-inf")


def _ids(n, seed=2024):
    return torch.randint(0, 128256, (n,), generator=torch.Generator().manual_seed(seed)).tolist()


def _unpack(stats):
    return stats[:, 0], stats[:, 1], stats[:, 2], stats.contiguous().view(torch.int32)[:, 3]


# ------------------------------------------------------------------------------------------------
# ops
# ------------------------------------------------------------------------------------------------
def test_cpu_logprobs_match_f64_log_softmax():
    g = torch.Generator().manual_seed(0)
    M, V, K = 33, 1000, 96
    h, w = torch.randn(M, K, generator=g), torch.randn(V, K, generator=g) * 0.3
    tg = torch.randint(0, V, (M,), generator=g, dtype=torch.int32)
    tg[:4] = torch.tensor([0, V - 1, -1, 500], dtype=torch.int32)
    logits = torch.nn.functional.linear(h, w)
    want = torch.log_softmax(logits.double(), -1).gather(1, tg.clamp(min=0).long()[:, None])[:, 0]
    lp = ops.lm_head_logprobs(h, w, tg)
    has = tg >= 0
    assert lp.dtype == torch.float32 and lp.shape == (M,)
    assert (lp[has].double() - want[has]).abs().max().item() <= 1e-5
    assert lp[2].item() == NEG_INF
    stats = ops.lm_head_logprobs(h, w, tg, return_stats=True)
    mx, s, tl, top1 = _unpack(stats)
    assert stats.shape == (M, 4) and stats.dtype == torch.float32
    assert torch.equal(mx, logits.max(-1).values) and torch.equal(top1, logits.argmax(-1).to(torch.int32))
    assert torch.equal(tl[has], logits.gather(1, tg.clamp(min=0).long()[:, None])[:, 0][has])
    lp1, t1 = ops.merge_logprob_stats(stats[None])
    assert torch.allclose(lp1[has], lp[has], atol=1e-6, rtol=0) and torch.equal(t1, top1)
    # a vocabulary shard: padded weight rows are ignored, ids are global, outside targets give -inf
    st = ops.lm_head_logprobs(h, w, tg + 7000, vvalid=600, voff=7000, return_stats=True)
    mx, s, tl, top1 = _unpack(st)
    assert torch.equal(mx, logits[:, :600].max(-1).values)
    assert torch.equal(top1, logits[:, :600].argmax(-1).to(torch.int32) + 7000)
    inside = (tg >= 0) & (tg < 600)
    assert bool((tl[~inside] == NEG_INF).all()) and bool(torch.isfinite(tl[inside]).all())
    with pytest.raises(ValueError):
        ops.lm_head_logprobs(h, w, tg, vvalid=V + 1)


def test_top1_ties_go_to_the_smallest_id():
    h = torch.ones(2, 4)
    w = torch.zeros(16, 4)
    w[[3, 9, 12]] = 1.0
    _, _, _, top1 = _unpack(ops.lm_head_logprobs(h, w, torch.tensor([3, -1]), return_stats=True))
    assert top1.tolist() == [3, 3]
    # across shards too: equal maxima, the smaller global id wins whichever shard comes first
    a = torch.tensor([[2.0, 1.5, 2.0, 0.0]])
    b = a.clone()
    a.view(torch.int32)[0, 3], b.view(torch.int32)[0, 3] = 900, 40
    for st in (torch.stack([a, b]), torch.stack([b, a])):
        lp, top1 = ops.merge_logprob_stats(st)
        assert top1.tolist() == [40] and lp.item() == pytest.approx(-torch.log(torch.tensor(3.0)).item())


@pytest.mark.parametrize("seed", range(6))
def test_merge_logprob_stats_over_random_splits(seed):
    g = torch.Generator().manual_seed(seed)
    M, V, K = 17, 900, 64
    h, w = torch.randn(M, K, generator=g), torch.randn(V, K, generator=g) * 0.3
    tg = torch.randint(0, V, (M,), generator=g, dtype=torch.int32)
    tg[0] = -1
    R = 1 + seed % 4
    cuts = sorted(torch.randint(1, V, (R - 1,), generator=g).tolist())
    bounds = [0] + cuts + [V]
    parts = [ops.lm_head_logprobs(h, w[lo:hi], tg, voff=lo, return_stats=True)
             for lo, hi in zip(bounds[:-1], bounds[1:]) if hi > lo]
    empty = torch.tensor([NEG_INF, 0.0, NEG_INF, 0.0]).repeat(M, 1)        # a shard without columns
    empty.view(torch.int32)[:, 3] = 0x7FFFFFFF
    parts.insert(seed % (len(parts) + 1), empty)
    lp, top1 = ops.merge_logprob_stats(torch.stack(parts))
    logits = torch.nn.functional.linear(h, w)
    want = torch.log_softmax(logits.double(), -1).gather(1, tg.clamp(min=0).long()[:, None])[:, 0]
    has = tg >= 0
    assert (lp[has].double() - want[has]).abs().max().item() <= 1e-5
    assert lp[0].item() == NEG_INF and not torch.isnan(lp).any()
    assert top1.dtype == torch.int32 and torch.equal(top1, logits.argmax(-1).to(torch.int32))


# ------------------------------------------------------------------------------------------------
# engine
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng():
    return LLMEngine(EngineConfig(**CFG))


def _dense_logprobs(model, ids):
    """One dense forward of the whole prompt -> f32 log_softmax gathered at the next tokens."""
    T = len(ids)
    nb = (T + KV_BS - 1) // KV_BS
    kv = KVCache(model.cfg.num_layers, nb + 1, model.hkv, model.D, dtype=model.w["embed"].dtype, device="cpu")
    bt = torch.arange(1, nb + 1, dtype=torch.int32)[None]
    pos = torch.arange(T, dtype=torch.int32)
    slots = (bt[0, (pos // KV_BS).long()] * KV_BS + pos % KV_BS).to(torch.int32)
    meta = AttentionMetadata(slots=slots, num_prefill_tokens=T, cu_q=torch.tensor([0, T], dtype=torch.int32),
                             ctx_lens_p=torch.tensor([T], dtype=torch.int32), block_tables_p=bt, max_q_len=T)
    logits = model.logits(model.forward(torch.tensor(ids, dtype=torch.int32), pos, meta, kv))
    lp = torch.log_softmax(logits.float(), -1)
    nxt = torch.tensor(ids[1:])
    return lp[:-1].gather(1, nxt[:, None])[:, 0], logits[:-1].float().argmax(-1) == nxt


@pytest.mark.parametrize("native_bm", [True, False])
def test_engine_score_matches_dense_forward(eng, native_bm, monkeypatch):
    from financial_chatbot_llm_amd.engine import block_manager, llm_engine
    monkeypatch.setattr(llm_engine, "make_block_manager",
                        lambda n, bs, pc: block_manager.make_block_manager(n, bs, pc, prefer_native=native_bm))
    e = LLMEngine(EngineConfig(**CFG), model=eng.model, tokenizer=eng.tokenizer)
    assert (type(e.bm).__name__ == "PyBlockManager") == (not native_bm)
    ids = _ids(300)
    # a cached prefix, so that a prefix-cache lookup or commit by score() would show below
    e.generate([ids[:200]], SamplingParams(temperature=0.0, max_tokens=2, ignore_eos=True))
    free, hit, queries = e.bm.num_free(), e.bm.hit_rate(), e.bm.queries
    res = e.score(ids)                            # 299 rows: two chunks of <= 256
    assert isinstance(res, ScoreResult) and len(res.logprobs) == len(res.top1_match) == len(ids) - 1
    assert e.bm.num_free() == free and e.bm.hit_rate() == hit and e.bm.queries == queries
    assert e.stats()["scored_tokens"] == len(ids) - 1
    want, want_match = _dense_logprobs(e.model, ids)
    err = (torch.tensor(res.logprobs) - want).abs().max().item()
    print(f"max |score - dense log_softmax| = {err:.3e}")
    assert err <= SCORE_TOL
    assert res.top1_match == want_match.tolist()
    # >= 3 chunks agree with one chunk under the same bound
    e.cfg = dataclasses.replace(e.cfg, max_num_batched_tokens=64)
    many = e.score(ids)
    e.cfg = dataclasses.replace(e.cfg, max_num_batched_tokens=1024)
    one = e.score(ids)
    assert (torch.tensor(many.logprobs) - torch.tensor(one.logprobs)).abs().max().item() <= SCORE_TOL
    assert many.top1_match == one.top1_match
    assert e.bm.num_free() == free and e.bm.hit_rate() == hit


def test_engine_score_errors_leak_nothing(eng):
    free = eng.bm.num_free()
    with pytest.raises(ValueError):
        eng.score([5])
    with pytest.raises(ValueError):
        eng.score([])
    with pytest.raises(ValueError):
        eng.score(_ids(eng.cfg.max_model_len + 1))
    assert len(eng.score(_ids(eng.cfg.max_model_len)).logprobs) == eng.cfg.max_model_len - 1
    assert eng.bm.num_free() == free
    small = LLMEngine(EngineConfig(**{**CFG, "num_kv_blocks": 3}), model=eng.model, tokenizer=eng.tokenizer)
    with pytest.raises(RuntimeError):
        small.score(_ids(4 * KV_BS))              # 255 rows need 4 blocks, 3 exist
    assert small.bm.num_free() == 3
    assert len(small.score(_ids(3 * KV_BS)).logprobs) == 3 * KV_BS - 1
    assert small.bm.num_free() == 3
    small.cp = object()                           # a context-parallel engine
    with pytest.raises(NotImplementedError):
        small.score(_ids(10))


@pytest.mark.parametrize("async_scheduling", [True, False])
def test_score_between_steps_leaves_generation_unchanged(eng, async_scheduling):
    prompts = [_ids(90, seed=1), _ids(40, seed=2)]
    sp = SamplingParams(temperature=0.8, max_tokens=10, ignore_eos=True, seed=77)

    def run(interleave):
        e = LLMEngine(EngineConfig(**{**CFG, "async_scheduling": async_scheduling}), model=eng.model,
                      tokenizer=eng.tokenizer)
        seqs = [e.add_request(f"r{i}", p, sp) for i, p in enumerate(prompts)]
        scores = []
        while any(not s.finished for s in seqs):
            e.step()
            if interleave:
                scores.append(e.score(_ids(150, seed=3)).logprobs)
        assert not interleave or all(s == scores[0] for s in scores)
        return [list(s.output_ids) for s in seqs]
    assert run(True) == run(False)


async def _score_while_streaming(aeng, ids):
    stream = asyncio.ensure_future(aeng.generate_all(_ids(60, seed=5), SamplingParams(temperature=0.0, max_tokens=24,
                                                                                      ignore_eos=True)))
    await asyncio.sleep(0)
    res = await aeng.score(ids)
    with pytest.raises(ValueError):
        await aeng.score([1])
    out = await stream
    return res, out


@pytest.mark.timeout(240)
def test_async_and_process_engines_score_like_the_engine(eng):
    ids = _ids(120, seed=9)
    want = eng.score(ids)
    aeng = AsyncEngine(engine=LLMEngine(EngineConfig(**CFG), model=eng.model, tokenizer=eng.tokenizer), warmup=False)
    try:
        res, out = asyncio.run(_score_while_streaming(aeng, ids))
        assert res == want and out.finished and len(out.seq.output_ids) == 24
        assert aeng.stats()["scored_tokens"] == len(ids) - 1
    finally:
        aeng.shutdown()
    peng = ProcessAsyncEngine(EngineConfig(**CFG))
    try:
        res, out = asyncio.run(_score_while_streaming(peng, ids))
        assert res == want and out.finished and len(out.seq.output_ids) == 24
        assert peng.stats()["scored_tokens"] == len(ids) - 1
    finally:
        peng.shutdown()


def test_engine_llm_score_text(eng):
    from financial_chatbot_llm_amd.engine.backend import EngineLLM
    aeng = AsyncEngine(engine=LLMEngine(EngineConfig(**CFG), model=eng.model, tokenizer=eng.tokenizer), warmup=False)
    try:
        text = "rent was paid on the first of the month, groceries twice a week"
        got = asyncio.run(EngineLLM(aeng, max_model_len=1024).score(text))
    finally:
        aeng.shutdown()
    ids = eng.tokenizer.encode(text, allow_special=False)
    want = eng.score(ids)
    assert set(got) == {"tokens", "logprobs", "nll_mean", "perplexity", "top1_accuracy"}
    assert got["tokens"] == len(ids) and got["logprobs"] == want.logprobs
    assert got["nll_mean"] == pytest.approx(-sum(want.logprobs) / len(want.logprobs))
    assert got["perplexity"] == pytest.approx(torch.tensor(got["nll_mean"]).exp().item(), rel=1e-5)
    assert got["top1_accuracy"] == sum(want.top1_match) / len(want.top1_match)


def test_bench_score_prints_one_json_line(tmp_path, capsys):
    from financial_chatbot_llm_amd.bench import score
    f = tmp_path / "t.txt"
    f.write_text("the quick brown fox jumps over the lazy dog. " * 12)
    assert score.main(["--model", "llama-tiny", "--device", "cpu", "--text-file", str(f), "--max-model-len", "64",
                       "--max-num-batched-tokens", "32"]) == 0
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    row = json.loads(lines[0])
    assert {"tokens", "nll_mean", "perplexity", "top1_accuracy", "path"} <= set(row)
    assert row["path"] == "reference" and row["tokens"] > 0 and row["windows"] >= 2
    assert row["perplexity"] == pytest.approx(torch.tensor(row["nll_mean"]).exp().item(), rel=1e-5)
