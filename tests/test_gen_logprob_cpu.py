"""Generation log-probabilities without a GPU: the ops fallbacks against the f64 reference, the input
condition of the GPU tests, the engine's alignment / None rules and unchanged tokens on the CPU
engine, ``LLMResult.mean_logprob``, the agent's decide-confidence metrics and the pass-through of the
process engine's wire tuples."""
import asyncio
import math

import pytest
import torch

from financial_chatbot_llm_amd import ops
from financial_chatbot_llm_amd.agent.agent import LLMAgent
from financial_chatbot_llm_amd.agent.automaton import compile_tool_automaton
from financial_chatbot_llm_amd.agent.llm import LLMResult, StubLLM, mean_logprob
from financial_chatbot_llm_amd.config import EngineConfig, ServingConfig
from financial_chatbot_llm_amd.engine import LLMEngine, SamplingParams
from financial_chatbot_llm_amd.tools import make_retrieval_tool
from financial_chatbot_llm_amd.utils.metrics import METRICS
import gen_logprob_ref as R
from test_constrain_cpu import PROBE

BASE = dict(model="llama-tiny", device="cpu", max_model_len=1024, max_num_batched_tokens=256,
            use_cuda_graph=False, max_num_seqs=8, num_kv_blocks=96)


# ------------------------------------------------------------------------------------------------
# ops
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("B,V", [(1, 8), (5, 1000), (3, 4099)])
def test_token_logprobs_cpu_matches_f64(B, V, dtype):
    logits, ids, want = R.token_logprob_rows(B, V, dtype)
    got = ops.token_logprobs(logits, ids)
    assert got.dtype == torch.float32 and got.shape == (B,)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    assert bool(nan[-1]) == (B >= 3)
    assert (got[~nan].double() - want[~nan]).abs().max().item() <= R.LOGPROB_TOL
    # a column slice of wider logits (unaligned view) and an id outside the vocabulary
    wide = torch.cat([torch.zeros(B, 3, dtype=dtype), logits], 1)
    assert torch.equal(ops.token_logprobs(wide[:, 3:], ids)[~nan], got[~nan])
    assert bool(torch.isnan(ops.token_logprobs(logits, torch.full((B,), V, dtype=torch.int32))).all())


@pytest.mark.parametrize("vvalid,voff", [(None, 0), (300, 1000)])
def test_lm_head_sample_logprob_cpu_fallback(vvalid, voff):
    """logits -> sample -> f32 log-softmax gather: greedy rows return the planted winners, every
    row its f64 log-probability, ids are global."""
    c = R.case(129, 512, vvalid, vvalid is None)
    ids, lp = ops.lm_head_sample_logprob(c.x, c.w, c.temps, c.seeds, vvalid=vvalid, voff=voff)
    assert ids.dtype == torch.int32 and lp.dtype == torch.float32
    for r, col in c.planted.items():
        assert int(ids[r]) == voff + col
    if c.tie_row is not None:
        assert int(ids[c.tie_row]) == voff + 5                 # two tied maxima: the smaller id
    plain = ops.lm_head_sample(c.x, c.w[:c.vvalid], c.temps, c.seeds)
    assert torch.equal(ids, plain + voff)
    assert (lp.double() - c.logprob_ref(ids, voff)).abs().max().item() <= R.LOGPROB_TOL


def test_inputs_exercise_the_sum():
    """The GPU tests' input condition: in every case at least half of the sampling rows have their
    most likely token below log p = -0.1 (so whatever they draw is), the logits' standard deviation
    is in the 1-3 range the tolerance derivation assumes, and greedy rows win by their plant."""
    for c in R.all_cases():
        assert c.spread_ok(), (c.M, c.V, c.vvalid)
        samp = ~c.greedy
        if bool(samp.any()):
            sd = float(c.logits[samp].float().std())
            assert 0.9 < sd < 3.0, sd
        for r, col in c.planted.items():
            assert int(c.logits[r].float().argmax()) == col and float(c.max_logprob()[r]) > -1e-3
        if c.tie_row is not None:
            row = c.logits[c.tie_row].float()
            assert float(row[5]) == float(row[c.vvalid - 40]) == float(row.max())


# ------------------------------------------------------------------------------------------------
# engine (CPU)
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def automaton():
    from financial_chatbot_llm_amd.engine.tokenizer import SyntheticLlamaTokenizer
    return compile_tool_automaton([PROBE], SyntheticLlamaTokenizer())


@pytest.mark.parametrize("overlap", [True, False], ids=["overlap", "sync"])
def test_engine_tokens_unchanged_and_logprobs_aligned(automaton, overlap):
    eng = LLMEngine(EngineConfig(async_scheduling=overlap, seed=0, **BASE))
    off, _ = R.run_scenario(eng, automaton, False, "a")
    state_off = R.pool_state(eng)
    assert eng.stats()["logprob_steps"] == 0
    assert all(s.output_logprobs == [] for s in off.values())
    eng2 = LLMEngine(EngineConfig(async_scheduling=overlap, seed=0, **BASE), model=eng.model)
    on, outs = R.run_scenario(eng2, automaton, True, "a")
    for n in R.NAMES:
        assert on[n].output_ids == off[n].output_ids, n
        assert on[n].finish_reason == off[n].finish_reason
    R.check_alignment(on, outs)
    assert eng2.stats()["logprob_steps"] > 0
    assert R.pool_state(eng2) == state_off
    # same model, same f32 CPU math on both paths: decode-time values equal score() up to f32 rounding
    assert R.score_drift(eng2, on) <= 1e-4


def test_refused_on_a_tp_engine_and_dropped_by_the_backend(caplog):
    """TP / CP engines refuse the request; EngineLLM drops the switch with one warning."""
    from types import SimpleNamespace
    from financial_chatbot_llm_amd.engine.backend import EngineLLM
    eng = LLMEngine(EngineConfig(seed=0, **BASE))
    eng.ps = SimpleNamespace(tp_size=2, rank=0, is_tp_leader=True, cp_size=1)
    with pytest.raises(NotImplementedError, match="log-probabilities"):
        eng.add_request("x", [1, 2, 3], SamplingParams(logprobs=True))
    assert "x" not in eng.requests

    seen = []

    class FakeAsync:
        tokenizer = eng.tokenizer
        engine = eng

        async def generate_all(self, ids, params):
            seen.append(params.logprobs)
            return SimpleNamespace(seq=SimpleNamespace(output_ids=[5, 6], output_logprobs=[-0.5, None],
                                                       num_prefilled=0, admit_time=None, first_token_time=None,
                                                       arrival=0.0))
    llm = EngineLLM(FakeAsync(), max_model_len=256)
    from financial_chatbot_llm_amd.wire import ChatMessage
    msgs = [ChatMessage(role="user", content="hello")]
    with caplog.at_level("WARNING"):
        r1 = asyncio.run(llm.agenerate(msgs, logprobs=True))
        r2 = asyncio.run(llm.agenerate(msgs, logprobs=True))
    assert seen == [False, False] and r1.logprobs is None and r1.mean_logprob is None and r2.logprobs is None
    assert sum("log-probabilities" in rec.getMessage() for rec in caplog.records) == 1
    eng.ps = SimpleNamespace(tp_size=1, rank=0, is_tp_leader=True, cp_size=1)
    llm2 = EngineLLM(FakeAsync(), max_model_len=256)
    r3 = asyncio.run(llm2.agenerate(msgs, logprobs=True))
    assert seen[-1] is True and r3.logprobs == [-0.5, None] and r3.mean_logprob == -0.5
    r4 = asyncio.run(llm2.agenerate(msgs))
    assert seen[-1] is False and r4.logprobs is None


# ------------------------------------------------------------------------------------------------
# LLMResult, agent metrics, process-engine wire
# ------------------------------------------------------------------------------------------------
def test_mean_logprob_skips_none():
    assert mean_logprob(None) is None and mean_logprob([]) is None and mean_logprob([None, None]) is None
    assert mean_logprob([-1.0, None, -3.0]) == -2.0
    r = LLMResult(text="x")
    assert r.logprobs is None and r.mean_logprob is None


class _ConfLLM(StubLLM):
    def __init__(self, means):
        super().__init__()
        self.means = list(means)
        self.asked = []

    async def agenerate(self, messages, tools=None, temperature=0.5, max_tokens=256, **kw):
        self.asked.append(bool(kw.get("logprobs")))
        res = await super().agenerate(messages, tools, temperature, max_tokens, **kw)
        m = self.means.pop(0)
        if kw.get("logprobs") and m is not None:
            res.logprobs, res.mean_logprob = [m, None], m
        return res


def _counters():
    c = METRICS.snapshot()
    return tuple(float(c.get(k) or 0.0) for k in ("decide_confidence_sum", "decide_confidence_count",
                                                "decide_low_confidence"))


def test_agent_records_decide_confidence(monkeypatch):
    monkeypatch.setenv("PENNY_DECIDE_LOGPROBS", "1")
    sv = ServingConfig.from_env()
    assert sv.decide_logprobs and sv.decide_confidence_threshold == 0.5
    monkeypatch.delenv("PENNY_DECIDE_LOGPROBS")
    assert not ServingConfig.from_env().decide_logprobs
    # two sampled decides (confidence 0.9 and 0.3) and a scripted one (nothing sampled: no mean)
    llm = _ConfLLM([math.log(0.9), math.log(0.3), None])
    agent = LLMAgent(llm, make_retrieval_tool(None), decide_logprobs=sv.decide_logprobs,
                     decide_confidence_threshold=sv.decide_confidence_threshold)
    before = _counters()
    for _ in range(3):
        asyncio.run(agent.query("How should I invest for retirement?", "u1"))
    after = _counters()
    assert llm.asked == [True, True, True]
    assert after[0] - before[0] == pytest.approx(1.2, abs=1e-9)
    assert after[1] - before[1] == 2 and after[2] - before[2] == 1
    # switched off: the decide call does not ask and nothing moves
    llm = _ConfLLM([math.log(0.9)])
    agent = LLMAgent(llm, make_retrieval_tool(None))
    asyncio.run(agent.query("How should I invest for retirement?", "u1"))
    assert llm.asked == [False] and _counters() == after


def test_process_engine_passes_logprobs_through():
    """The child's wire tuple carries new_logprobs; the parent rebuilds StepOutput and the RemoteSeq."""
    import queue
    from financial_chatbot_llm_amd.engine.process_engine import ProcessAsyncEngine, RemoteSeq

    class Loop:
        def call_soon_threadsafe(self, fn, *a):
            fn(*a)

    class Pipe:
        def __init__(self, msgs):
            self.msgs = list(msgs)

        def recv(self):
            if not self.msgs:
                raise EOFError
            return self.msgs.pop(0)
    pe = object.__new__(ProcessAsyncEngine)
    qa, qb = queue.Queue(), queue.Queue()
    pe._sinks = {"a": (Loop(), qa), "b": (Loop(), qb)}
    pe._seqs = {"a": RemoteSeq(), "b": RemoteSeq()}
    pe._score_waiters, pe._closed, pe.error = {}, True, None
    pe._out_r = Pipe([("out", [("a", [5, 6], False, None, [-0.25, None]), ("b", [7], False, None, None)]),
                      ("out", [("a", [9], True, "stop", [-1.5])]), ("stopped", None)])
    pe._read()
    o1, o2, ob = qa.get_nowait(), qa.get_nowait(), qb.get_nowait()
    assert o1.new_logprobs == [-0.25, None] and o2.new_logprobs == [-1.5] and o2.finished
    assert ob.new_logprobs is None and ob.seq.output_logprobs == []
    assert o2.seq.output_ids == [5, 6, 9] and o2.seq.output_logprobs == [-0.25, None, -1.5]
