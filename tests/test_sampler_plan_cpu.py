"""The sampling decisions of the model runner without a GPU: which sampler an eager step runs, which
one a bucket's default decode graph carries and which graph a pure-decode step replays -- every
combination of their boolean inputs against tables written out by hand -- and the runner's handling
of a twin graph that cannot be captured."""
import itertools

import pytest
import torch

from financial_chatbot_llm_amd.config import EngineConfig
from financial_chatbot_llm_amd.engine import LLMEngine, SamplingParams
from financial_chatbot_llm_amd.engine.model_runner import (DEFAULT_GRAPH, EAGER, _DecodeGraph, default_graph_kind,
                                                           graph_plan, sampler_kind)

# (fsm, filters, shard, fused) -> sampler of an eager step
EAGER_KIND = {
    (0, 0, 0, 0): "logits", (0, 0, 0, 1): "fused", (0, 0, 1, 0): "shard", (0, 0, 1, 1): "shard",
    (0, 1, 0, 0): "logits", (0, 1, 0, 1): "logits", (0, 1, 1, 0): "logits", (0, 1, 1, 1): "logits",
    (1, 0, 0, 0): "fsm", (1, 0, 0, 1): "fsm", (1, 0, 1, 0): "fsm", (1, 0, 1, 1): "fsm",
    (1, 1, 0, 0): "fsm", (1, 1, 0, 1): "fsm", (1, 1, 1, 0): "fsm", (1, 1, 1, 1): "fsm",
}

# (shard, fused) -> sampler of a bucket's default graph
DEFAULT_KIND = {(0, 0): "logits", (0, 1): "fused", (1, 0): "shard", (1, 1): "shard"}

D, E = DEFAULT_GRAPH, EAGER
# (fsm, filters, lp, bucket_fused, tp) -> the default graph, eager, or the twin's (sampler, lp)
PLAN = {
    # nothing the default graph lacks
    (0, 0, 0, 0, 0): D, (0, 0, 0, 0, 1): D, (0, 0, 0, 1, 0): D, (0, 0, 0, 1, 1): D,
    # log-probabilities only: the bucket's own sampler in its log-probability form
    (0, 0, 1, 0, 0): ("logits", True), (0, 0, 1, 0, 1): E, (0, 0, 1, 1, 0): ("fused", True), (0, 0, 1, 1, 1): E,
    # top-k / top-p only: a logits bucket has the threshold kernel, a fused one needs the twin
    (0, 1, 0, 0, 0): D, (0, 1, 0, 0, 1): D, (0, 1, 0, 1, 0): ("logits", False), (0, 1, 0, 1, 1): E,
    (0, 1, 1, 0, 0): ("logits", True), (0, 1, 1, 0, 1): E, (0, 1, 1, 1, 0): ("logits", True), (0, 1, 1, 1, 1): E,
    # constrained rows: always the masked sampler
    (1, 0, 0, 0, 0): ("fsm", False), (1, 0, 0, 0, 1): E, (1, 0, 0, 1, 0): ("fsm", False), (1, 0, 0, 1, 1): E,
    (1, 0, 1, 0, 0): ("fsm", True), (1, 0, 1, 0, 1): E, (1, 0, 1, 1, 0): ("fsm", True), (1, 0, 1, 1, 1): E,
    (1, 1, 0, 0, 0): ("fsm", False), (1, 1, 0, 0, 1): E, (1, 1, 0, 1, 0): ("fsm", False), (1, 1, 0, 1, 1): E,
    (1, 1, 1, 0, 0): ("fsm", True), (1, 1, 1, 0, 1): E, (1, 1, 1, 1, 0): ("fsm", True), (1, 1, 1, 1, 1): E,
}


def _bools(n):
    return list(itertools.product((False, True), repeat=n))


def test_eager_sampler_kind_table():
    assert len(EAGER_KIND) == 16
    for c in _bools(4):
        assert sampler_kind(*c) == EAGER_KIND[tuple(map(int, c))], c


def test_default_graph_kind_table():
    assert len(DEFAULT_KIND) == 4
    for c in _bools(2):
        assert default_graph_kind(*c) == DEFAULT_KIND[tuple(map(int, c))], c


def test_graph_plan_table_and_invariants():
    assert len(PLAN) == 32
    for c in _bools(5):
        fsm, filters, lp, bucket_fused, tp = c
        plan = graph_plan(*c)
        assert plan == PLAN[tuple(map(int, c))], c
        twin = plan not in (D, E)
        if tp:                                   # under TP no twin: the default graph or eager
            assert not twin
        if lp:                                   # an lp step never replays a graph without the values
            assert plan == E or (twin and plan[1] is True)
        elif twin:
            assert plan[1] is False
        if filters:                              # top-k / top-p rows never sample inside the LM head
            assert not (twin and plan[0] == "fused") and not (plan == D and bucket_fused)
        if fsm:                                  # constrained rows only ever meet the masked sampler
            assert plan == E or plan[0] == "fsm"


def test_twin_capture_failure_runs_eagerly_and_is_not_retried(monkeypatch):
    """A top-k decode step on a fused bucket needs the (8, "logits", False) twin; its capture raising
    leaves the step -- and every later one -- on the eager path with the same tokens, after ONE attempt."""
    eng = LLMEngine(EngineConfig(model="llama-tiny", device="cpu", max_model_len=256, max_num_batched_tokens=64,
                                 use_cuda_graph=False, max_num_seqs=8, num_kv_blocks=16, seed=0))
    prompts = [list(range(40, 60)), list(range(7, 19))]
    params = SamplingParams(temperature=0.0, top_k=5, max_tokens=4, ignore_eos=True)
    want = eng.generate(prompts, params)                # greedy: the same tokens on a second run
    r = eng.runner
    steps = r.stats["steps"]
    r.graphs = {8: _DecodeGraph(None, 8, None, fused=True)}
    r.graph_sizes, r.use_graphs = (8,), True
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)
    attempts = []

    def capture(key):
        attempts.append(key)
        raise RuntimeError("out of memory")
    monkeypatch.setattr(r, "_capture_twin", capture)
    monkeypatch.setattr(r, "_graph_decode", lambda *a: pytest.fail("replayed a graph"))
    assert eng.generate(prompts, params) == want
    assert attempts == [(8, "logits", False)] and r._twin_failed == {(8, "logits", False)}
    assert not r.twins and r.stats["graph_steps"] == 0 and r.stats["steps"] >= steps + 3    # several decode steps
