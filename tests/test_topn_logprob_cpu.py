"""Top-N alternatives without a GPU: the certificate against hand-made wrong answers, the torch path
of ``ops.topn_logprobs`` against the f64 reference on the GPU tests' inputs, argument validation, the
engine's alignment rules and unchanged tokens on the CPU engine, and the plumbing above it
(``EngineLLM``, the agent's decide margin, the process engine's tuples)."""
import asyncio
import math

import pytest
import torch

from financial_chatbot_llm_amd import ops
from financial_chatbot_llm_amd.agent.agent import LLMAgent
from financial_chatbot_llm_amd.agent.automaton import compile_tool_automaton
from financial_chatbot_llm_amd.agent.llm import LLMResult, StubLLM
from financial_chatbot_llm_amd.config import EngineConfig, ServingConfig
from financial_chatbot_llm_amd.engine import LLMEngine, SamplingParams
from financial_chatbot_llm_amd.engine.model_runner import DEFAULT_GRAPH, EAGER, graph_plan
from financial_chatbot_llm_amd.tools import make_retrieval_tool
from financial_chatbot_llm_amd.utils.metrics import METRICS
import gen_logprob_ref as G
import topn_logprob_ref as R
from test_constrain_cpu import PROBE

BASE = dict(model="llama-tiny", device="cpu", max_model_len=1024, max_num_batched_tokens=256,
            use_cuda_graph=False, max_num_seqs=8, num_kv_blocks=96)
SENT_ID, SENT_LP = -7, 7.0


# ------------------------------------------------------------------------------------------------
# the certificate
# ------------------------------------------------------------------------------------------------
def test_certificate_rejects_wrong_answers():
    bf = torch.bfloat16
    row = torch.tensor([3.0, 1.0, 2.0, 2.0, 0.0, -0.0, 2.0, -1.0, 2.0, 0.5]).to(bf)
    good = [0, 2, 3, 6]                                   # 3, then the plateau of 2s in id order: 8 is left out
    assert R.reference(row[None], torch.tensor([0]), [4])[0][1] == good
    assert R.certificate(row, good) is None
    assert "tied ids" in R.certificate(row, [0, 3, 2, 6])             # two tied ids swapped
    assert "smaller id" in R.certificate(row, [0, 2, 3, 8])           # a later member of the same plateau
    assert "duplicate" in R.certificate(row, [0, 2, 2, 3])
    assert "range" in R.certificate(row, [0, 2, 3, 10])
    assert "larger" in R.certificate(row, [2, 3, 6, 8])               # the maximum left out
    # a logit one bf16 ulp off: the answer for the original row is not the answer any more
    up = row.clone()
    up[8] = (up[8].view(torch.int16) + 1).view(bf)                    # 2 -> 2 + 2^-6
    assert float(up[8]) == 2.0 + 2.0 ** -6
    assert R.certificate(up, good) is not None and R.certificate(up, [0, 8, 2, 3]) is None
    # -0 and +0 are one value: a selected -0 (id 5) ahead of the earlier +0 (id 4) is out of order
    full = [0, 2, 3, 6, 8, 1, 9, 4, 5]
    assert R.certificate(row, full) is None
    assert "tied ids" in R.certificate(row, [0, 2, 3, 6, 8, 1, 9, 5, 4])
    # a reported value one bf16 ulp off the f64 log-softmax
    want = torch.log_softmax(row.double(), -1)[torch.tensor(good)]
    assert R.values_ok(row, good, want.tolist(), G.LOGPROB_TOL) is None
    off = want.clone()
    off[1] = float((want[1].to(bf).view(torch.int16) + 1).view(bf))
    assert abs(float(off[1] - want[1])) > G.LOGPROB_TOL
    assert R.values_ok(row, good, off.tolist(), G.LOGPROB_TOL) is not None


# ------------------------------------------------------------------------------------------------
# ops: the torch path
# ------------------------------------------------------------------------------------------------
def _buffers(B, device="cpu"):
    return (torch.full((B,), SENT_LP, dtype=torch.float32, device=device),
            torch.full((B, R.TOPN_MAX), SENT_ID, dtype=torch.int32, device=device),
            torch.full((B, R.TOPN_MAX), SENT_LP, dtype=torch.float32, device=device))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_torch_path_matches_reference(dtype):
    assert ops.sampling.TOPN_MAX == R.TOPN_MAX
    for c in R.cases(dtype):
        bufs = _buffers(c.logits.shape[0])
        got = ops.topn_logprobs(c.logits, c.ids, c.topn, out=bufs)
        assert all(a is b for a, b in zip(got, bufs))
        R.check_case(c, *got, SENT_ID, SENT_LP, G.LOGPROB_TOL)
        # the chosen token's value is token_logprobs' for the same row and id
        want = ops.token_logprobs(c.logits, c.ids)
        for b, n in enumerate(c.topn.tolist()):
            if n > 0 and b not in c.nan_rows and not math.isnan(float(want[b])):
                assert float(got[0][b]) == float(want[b]), (c.name, b)


def test_cases_cover_what_they_claim():
    for dtype in (torch.bfloat16, torch.float32):
        cs = {c.name: c for c in R.cases(dtype)}
        assert {c.logits.shape[1] for c in cs.values()} >= set(R.VOCABS)
        assert cs["rand V=20 B=1"].topn.tolist() == [20]                       # n == V
        mixed = cs["rand V=8200 B=5"].topn.tolist()
        assert sorted(set(mixed)) == [0, 1, 5, 20]
        p = cs["plateau of 3000 maxima"]
        first = p.ref[0][1]                       # row 0: 3 larger values, then the plateau across the sweep edge
        assert first[:3] == [12799, 11, 12182] and first[3:] == list(range(R.SWEEP - 10, R.SWEEP + 7))
        assert p.ref[1][1][3:] == list(range(3 * R.WAVE - 7, 3 * R.WAVE + 10))
        assert p.ref[3][1] == [i for i in range(21) if i != 11]
        assert cs["all equal"].ref[0][1] == list(range(20))
        assert cs["mixed zeros"].ref[2][1][:5] == [0, 1, 2, 3, 4]
        sp = cs["-inf, NaN and +inf rows"]
        assert sp.ref[1][1] == [500, 7, 999, 0, 1] and sp.ref[1][2][3] == float("-inf")


def test_arguments_outside_the_contract_raise():
    lg = torch.zeros(2, 30, dtype=torch.bfloat16)
    ids = torch.zeros(2, dtype=torch.int32)
    ok = ops.topn_logprobs(lg, ids, 3)
    assert ok[1].shape == (2, 20) and ok[1][0, :3].tolist() == [0, 1, 2]
    with pytest.raises(ValueError, match="TOPN_MAX"):
        ops.topn_logprobs(lg, ids, torch.tensor([1, 21]))
    with pytest.raises(ValueError, match="V = 10"):
        ops.topn_logprobs(lg[:, :10], ids, torch.tensor([1, 11]))
    with pytest.raises(ValueError, match="topn must be"):
        ops.topn_logprobs(lg, ids, torch.tensor([1, 2, 3]))
    with pytest.raises(ValueError, match="topn must be"):
        ops.topn_logprobs(lg, ids, torch.tensor([1.0, 2.0]))
    with pytest.raises(ValueError, match="ids must be"):
        ops.topn_logprobs(lg, ids[:1], 3)
    with pytest.raises(ValueError, match="bf16 or f32"):
        ops.topn_logprobs(lg.half(), ids, 3)
    with pytest.raises(ValueError, match=r"\[B, V\]"):
        ops.topn_logprobs(lg[0], ids, 3)
    with pytest.raises(ValueError, match="out must be"):
        ops.topn_logprobs(lg, ids, 3, out=(torch.zeros(2), torch.zeros(2, 20), torch.zeros(2, 20)))


def test_graph_plan_topn_twins():
    """A top-N step replays a twin of its own, named after the twin the step would replay without it;
    what ran eagerly stays eager; without the argument nothing changes."""
    assert graph_plan(False, False, True, True, False, False, True) == ("fused+topn", True)
    assert graph_plan(False, False, False, True, False, topn=True) == ("fused+topn", True)      # implies lp
    assert graph_plan(False, True, True, True, False, topn=True) == ("logits+topn", True)
    assert graph_plan(False, False, True, False, False, topn=True) == ("logits+topn", True)
    assert graph_plan(True, False, True, True, False, topn=True) == ("fsm+topn", True)
    assert graph_plan(False, False, True, True, False, True, True) == ("pen+topn", True)
    assert graph_plan(True, False, True, True, False, True, True) == EAGER                      # fsm and pen
    assert graph_plan(False, False, True, True, True, topn=True) == EAGER                       # TP
    assert graph_plan(False, False, False, True, False) == DEFAULT_GRAPH
    assert graph_plan(False, False, True, True, False) == ("fused", True)


# ------------------------------------------------------------------------------------------------
# engine (CPU)
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def automaton():
    from financial_chatbot_llm_amd.engine.tokenizer import SyntheticLlamaTokenizer
    return compile_tool_automaton([PROBE], SyntheticLlamaTokenizer())


@pytest.mark.parametrize("overlap", [True, False], ids=["overlap", "sync"])
def test_engine_alignment_and_unchanged_tokens(automaton, overlap):
    eng = LLMEngine(EngineConfig(async_scheduling=overlap, seed=0, **BASE))
    off, _ = R.run_scenario(eng, automaton, 0, "c")
    state_off = G.pool_state(eng)
    assert eng.stats()["top_logprob_steps"] == 0
    assert all(s.output_top_logprobs == [] and s.output_logprobs == [] for s in off.values())
    eng2 = LLMEngine(EngineConfig(async_scheduling=overlap, seed=0, **BASE), model=eng.model)
    on, outs = R.run_scenario(eng2, automaton, 5, "c")
    for n in R.NAMES:
        assert on[n].output_ids == off[n].output_ids, n
        assert on[n].finish_reason == off[n].finish_reason, n
    R.check_alignment(on, outs, 5)
    assert eng2.stats()["top_logprob_steps"] > 0 and eng2.spec_stats["accepted"] > 0
    assert G.pool_state(eng2) == state_off
    # every listed value is the raw distribution's: score() of the prefix + the listed token agrees
    s = on["plain"]
    k = 3
    for tok, lp in s.output_top_logprobs[k][:2]:
        ref = eng2.score(s.prompt_ids + s.output_ids[:k] + [tok]).logprobs[-1]
        assert abs(ref - lp) <= 1e-4


def test_logprobs_only_mate_keeps_its_values(automaton):
    """A request with logprobs=True and no alternatives reports the same numbers beside a top-N batch
    mate as without one, and carries no lists."""
    runs = []
    for top in (0, 4):
        eng = LLMEngine(EngineConfig(seed=0, **BASE))
        a = eng.add_request("a", list(range(300, 340)), SamplingParams(temperature=0.8, max_tokens=6, seed=1,
                                                                       ignore_eos=True, logprobs=True))
        b = eng.add_request("b", list(range(400, 440)), SamplingParams(temperature=0.7, max_tokens=6, seed=2,
                                                                       ignore_eos=True, top_logprobs=top))
        while eng.has_work():
            eng.step()
        runs.append((a, b))
    (a0, b0), (a1, b1) = runs
    assert a1.output_ids == a0.output_ids and a1.output_logprobs == a0.output_logprobs
    assert a1.output_top_logprobs == [] and b0.output_logprobs == [] and b1.params.logprobs
    assert len(b1.output_top_logprobs) == len(b1.output_logprobs) == 6 and b1.output_ids == b0.output_ids


def test_validation_and_tp_refusal(automaton):
    from types import SimpleNamespace
    eng = LLMEngine(EngineConfig(seed=0, **BASE))
    for bad in (-1, 21, 2.0, True):
        with pytest.raises(ValueError, match="top_logprobs"):
            eng.add_request("v", [1, 2, 3], SamplingParams(top_logprobs=bad, constraint=automaton))
    assert "v" not in eng.requests and not eng.has_work()
    assert eng.runner.fsm is None and not eng.runner._fsm_known      # refused before anything was registered
    eng.ps = SimpleNamespace(tp_size=2, rank=0, is_tp_leader=True, cp_size=1)
    with pytest.raises(NotImplementedError, match="top_logprobs"):
        eng.add_request("x", [1, 2, 3], SamplingParams(top_logprobs=2))
    assert "x" not in eng.requests


# ------------------------------------------------------------------------------------------------
# EngineLLM, the agent's decide margin, the process engine
# ------------------------------------------------------------------------------------------------
def test_engine_llm_passes_top_logprobs_and_drops_them_under_tp(caplog):
    from types import SimpleNamespace
    from financial_chatbot_llm_amd.engine.backend import EngineLLM
    from financial_chatbot_llm_amd.wire import ChatMessage
    eng = LLMEngine(EngineConfig(seed=0, **BASE))
    seen = []
    tops = [[(5, -0.5), (9, -1.5)], None]

    class FakeAsync:
        tokenizer = eng.tokenizer
        engine = eng

        async def generate_all(self, ids, params):
            seen.append((params.logprobs, params.top_logprobs))
            return SimpleNamespace(seq=SimpleNamespace(output_ids=[5, 6], output_logprobs=[-0.5, None],
                                                       output_top_logprobs=list(tops), num_prefilled=0,
                                                       admit_time=None, first_token_time=None, arrival=0.0))
    msgs = [ChatMessage(role="user", content="hello")]
    llm = EngineLLM(FakeAsync(), max_model_len=256)
    r = asyncio.run(llm.agenerate(msgs, top_logprobs=2))
    assert seen[-1] == (True, 2) and r.top_logprobs == tops and r.logprobs == [-0.5, None] and r.token_ids == [5, 6]
    r = asyncio.run(llm.agenerate(msgs, logprobs=True))
    assert seen[-1] == (True, 0) and r.top_logprobs is None
    assert LLMResult(text="x").top_logprobs is None
    eng.ps = SimpleNamespace(tp_size=2, rank=0, is_tp_leader=True, cp_size=1)
    llm2 = EngineLLM(FakeAsync(), max_model_len=256)
    with caplog.at_level("WARNING"):
        r1 = asyncio.run(llm2.agenerate(msgs, top_logprobs=3))
        r2 = asyncio.run(llm2.agenerate(msgs, top_logprobs=3, logprobs=True))
    assert seen[-2:] == [(False, 0), (False, 0)] and r1.top_logprobs is None and r2.logprobs is None
    assert sum("log-probabilities" in rec.getMessage() for rec in caplog.records) == 1


class _TopLLM(StubLLM):
    def __init__(self, results):
        super().__init__()
        self.results = list(results)
        self.asked = []

    async def agenerate(self, messages, tools=None, temperature=0.5, max_tokens=256, **kw):
        self.asked.append((kw.get("top_logprobs"), bool(kw.get("logprobs"))))
        res = await super().agenerate(messages, tools, temperature, max_tokens, **kw)
        res.logprobs, res.top_logprobs, res.token_ids = self.results.pop(0)
        return res


def _margin():
    c = METRICS.snapshot()
    return float(c.get("decide_margin_sum") or 0.0), float(c.get("decide_margin_count") or 0.0)


def test_agent_records_decide_margin(monkeypatch):
    monkeypatch.setenv("PENNY_DECIDE_TOP_LOGPROBS", "5")
    assert ServingConfig.from_env().decide_top_logprobs == 5
    monkeypatch.delenv("PENNY_DECIDE_TOP_LOGPROBS")
    assert ServingConfig.from_env().decide_top_logprobs == 0
    llm = _TopLLM([
        ([-0.25, -0.1], [[(7, -0.25), (9, -1.75)], [(3, -0.1), (4, -3.0)]], [7, 3]),   # the likelier token: +1.5
        ([None, -2.0, None], [None, [(8, -0.5), (2, -2.0)], None], [1, 2, 3]),         # first SAMPLED token: -1.5
        ([None, None], [None, None], [1, 2]),                                          # scripted: nothing
        ([-0.75], [[(7, -0.75), (9, -0.75)]], [9]),            # tied logits, the later id drawn: 0, by its id
        ([-3.0], [[(7, -0.25), (9, -1.75)]], [5]),             # the drawn token is not listed: -2.75
        ([-0.25], [[(7, -0.25), (9, -1.75)]], None),           # a backend without token ids: nothing
    ])
    agent = LLMAgent(llm, make_retrieval_tool(None), decide_top_logprobs=1)       # at least two are asked for
    before = _margin()
    for _ in range(6):
        asyncio.run(agent.query("How should I invest for retirement?", "u1"))
    after = _margin()
    assert llm.asked == [(2, False)] * 6
    assert after[0] - before[0] == pytest.approx(-2.75, abs=1e-9) and after[1] - before[1] == 4
    llm = _TopLLM([([-0.25], [[(7, -0.25), (9, -1.75)]], [7])])
    agent = LLMAgent(llm, make_retrieval_tool(None), decide_top_logprobs=5)
    asyncio.run(agent.query("How should I invest for retirement?", "u1"))
    assert _margin()[0] - after[0] == pytest.approx(1.5) and llm.asked == [(5, False)]
    # off by default: the decide call does not ask and nothing moves
    now = _margin()
    llm = _TopLLM([([-0.25], [[(7, -0.25), (9, -1.75)]], [7])])
    asyncio.run(LLMAgent(llm, make_retrieval_tool(None)).query("How should I invest for retirement?", "u1"))
    assert llm.asked == [(None, False)] and _margin() == now


def test_process_engine_passes_top_logprobs_through():
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
    t1 = [[(5, -0.25), (8, -2.0)], None]
    pe._out_r = Pipe([("out", [("a", [5, 6], False, None, [-0.25, None], t1), ("b", [7], False, None, None, None)]),
                      ("out", [("a", [9], True, "stop", [-1.5], [[(9, -1.5), (1, -1.75)]])]), ("stopped", None)])
    pe._read()
    o1, o2, ob = qa.get_nowait(), qa.get_nowait(), qb.get_nowait()
    assert o1.new_top_logprobs == t1 and o2.new_top_logprobs == [[(9, -1.5), (1, -1.75)]]
    assert ob.new_top_logprobs is None and ob.seq.output_top_logprobs == []
    assert o2.seq.output_top_logprobs == t1 + [[(9, -1.5), (1, -1.75)]]
    assert o2.seq.output_logprobs == [-0.25, None, -1.5]
