"""Constrained tool-call decoding on the CPU: the automaton against an independent checker
(``constrain_ref``), the numpy mask oracle against a Python byte walk, and the engine end to end --
a random-weight model under the constraint emits schema-valid decide outputs in both step modes.
All checks are exact.
"""
import json
import logging
import random
from typing import Literal, Optional

import numpy as np
import pytest
import torch
from pydantic import BaseModel, Field

from constrain_ref import check_output, complete_prefix
from financial_chatbot_llm_amd.agent.automaton import (DEAD, TokenAutomaton, build_masks_ref, compile_tool_automaton,
                                                       mask_words, token_bytes)
from financial_chatbot_llm_amd.agent.grammar import ToolCallGrammar
from financial_chatbot_llm_amd.config import EngineConfig
from financial_chatbot_llm_amd.engine import LLMEngine, SamplingParams
from financial_chatbot_llm_amd.engine.model_runner import StepInputs
from financial_chatbot_llm_amd.engine.tokenizer import SyntheticLlamaTokenizer
from financial_chatbot_llm_amd.tools import make_plot_tool, make_retrieval_tool
from financial_chatbot_llm_amd.tools.base import Tool

BASE = dict(model="llama-tiny", device="cpu", max_model_len=1024, max_num_batched_tokens=256,
            use_cuda_graph=False, max_num_seqs=8, num_kv_blocks=96)
TOK = SyntheticLlamaTokenizer()
EOT = TOK.special["<|eot_id|>"]
RET = make_retrieval_tool(None)
PLOT = make_plot_tool()


class ProbeArgs(BaseModel):
    count: int = Field(le=999)
    limit: Optional[int] = None
    flag: bool
    mode: Literal["a", "bb"] = "a"


class ListArgs(BaseModel):
    items: list[int]


PROBE = Tool("probe", "a finite language: no string field", ProbeArgs, lambda **kw: kw)
TOOLSETS = {"retrieval": [RET], "retrieval+plot": [RET, PLOT], "probe": [PROBE]}


@pytest.fixture(scope="module")
def automata():
    return {k: compile_tool_automaton(v, TOK) for k, v in TOOLSETS.items()}


def _random_walks(a: TokenAutomaton, n: int, seed: int, max_len: int = 400):
    """Random accepted strings: a byte walk that heads for the accepting state (shortest distance
    known per state) once it has wandered long enough."""
    rng = random.Random(seed)
    nxt = a.byte_next
    S = nxt.shape[0]
    live = [[(b, int(nxt[s, b])) for b in range(256) if nxt[s, b] != DEAD] for s in range(S)]
    dist = np.full(S, 1 << 30)
    dist[np.flatnonzero(a.accept)] = 0
    changed = True
    while changed:
        changed = False
        for s in range(S):
            for _, t in live[s]:
                if dist[t] + 1 < dist[s]:
                    dist[s] = dist[t] + 1
                    changed = True
    out = []
    for _ in range(n):
        s, data = a.start, bytearray()
        wander = rng.randrange(0, 120)
        while not (a.accept[s] and not live[s]):
            edges = live[s]
            if len(data) >= wander:
                edges = [e for e in edges if dist[e[1]] < dist[s]] or edges
            b, s = rng.choice(edges)
            data.append(b)
            assert len(data) < max_len
        out.append(bytes(data))
    return out, dist


# ---------------------------------------------------------------------------------------------
# 1. the automaton against the independent checker
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TOOLSETS))
def test_accepted_strings_parse_and_validate(automata, name):
    a = automata[name]
    assert a is not None and a.num_states <= 4096
    walks, dist = _random_walks(a, 300, seed=len(name))
    assert (dist[[s for s in range(a.num_states) if a.walk(a.start, b"") >= 0]] < (1 << 30)).all()
    kinds = set()
    for data in walks:
        text = data.decode("utf-8", "surrogateescape")
        check_output(text, TOOLSETS[name])
        assert a.accepts(data)
        kinds.add(text[:14])
    assert len(kinds) >= 2                       # both "No tool call" and calls were drawn


def test_no_reachable_dead_end(automata):
    """Every state reachable from the start can still reach the accepting state: a constrained row
    never finds itself with an empty mask."""
    for a in automata.values():
        nxt = a.byte_next
        reach, todo = {a.start}, [a.start]
        while todo:
            s = todo.pop()
            for t in set(int(x) for x in nxt[s] if x != DEAD):
                if t not in reach:
                    reach.add(t)
                    todo.append(t)
        _, dist = _random_walks(a, 0, 0)
        assert all(dist[s] < (1 << 30) for s in reach)


HEAD = '{"name": "probe", "parameters": {'
RHEAD = '{"name": "retrieve_transactions", "parameters": {'
GOOD = [
    "No tool call",
    HEAD + '"count": 7, "flag": true}}',
    HEAD + '"flag": false, "mode": "bb", "limit": null, "count": -999}}',
    HEAD + '"count": 0, "flag": true, "limit": 123456789}}',
    RHEAD + "}}",
    RHEAD + '"search_query": "rent \\"and\\" caf\\u00e9 \\n", "num_transactions": 20}}',
    RHEAD + '"time_period_days": -30, "user_id": "", "num_transactions": null}}',
]
NEAR_MISSES = [
    HEAD + '"count": 7, "count": 8, "flag": true}}',              # a repeated key
    HEAD + '"count": 7, "flag": true, "other": 1}}',               # an unknown key
    HEAD + '"count": 07, "flag": true}}',                          # a leading zero
    HEAD + '"count": 1000, "flag": true}}',                        # a digit more than le=999 allows
    HEAD + '"count": 7}}',                                         # '}' before the required "flag"
    HEAD + '"count": 7, "flag": true}} ',                          # trailing text
    HEAD + '"count": 7, "flag": true}}}',
    HEAD + '"count": 7,"flag": true}}',                            # not the canonical layout
    HEAD + '"count": 7, "flag": True}}',
    HEAD + '"count": 7, "flag": true, "mode": "b"}}',              # not in the Literal
    HEAD + '"count": 7.5, "flag": true}}',
    HEAD + '"count": 7, "flag": true, "limit": "3"}}',
    RHEAD + '"search_query": "a\nb"}}',                            # a raw newline in a string
    RHEAD + '"search_query": "a\\qb"}}',                           # an unknown escape
    RHEAD + '"num_transactions": 123456}}',                        # maximum 10000: five digits
    '{"name": "nope", "parameters": {}}',
    "No tool call.",
    "no tool call",
]


def test_good_strings_and_near_misses(automata):
    two = compile_tool_automaton([RET, PROBE], TOK)
    for s in GOOD:
        assert two.accepts(s), s
        check_output(s, [RET, PROBE])
    for s in NEAR_MISSES:
        assert not two.accepts(s), s
    for s in GOOD + NEAR_MISSES:                 # every prefix of a good string is viable
        for cut in range(len(s) + 1):
            if s in GOOD:
                assert two.viable(s[:cut]), s[:cut]
                check_output(complete_prefix(s[:cut], [RET, PROBE]), [RET, PROBE])
    assert not two.viable(HEAD + '"count": 7, "count')             # dies AT the repeated key
    assert not two.viable(HEAD + '"count": 07')
    assert not two.viable(RHEAD + '"search_query": "a\n')


def test_declared_order_above_four_properties(automata):
    a = automata["retrieval+plot"]
    head = '{"name": "create_financial_plot", "parameters": {"transactions_json": "[]", "plot_config": {'
    assert a.accepts(head + '"plot_type": "pie", "x_axis": "c", "title": "t", "group_by": null}}}')
    assert not a.viable(head + '"x_axis": "c", "plot_type')         # out of declared order
    assert not a.viable(head + '"plot_type": "pie", "x_axis": "c", "group_by')   # skips the required title
    assert not a.viable(head + '"plot_type": "donut')
    # at most four properties: any order
    assert a.accepts('{"name": "create_financial_plot", "parameters": {"plot_config": {"plot_type": "bar", '
                     '"x_axis": "d", "title": "x"}, "transactions_json": "[]"}}')


def test_refusals(caplog):
    arr = Tool("lister", "has an array", ListArgs, lambda **kw: kw)
    with caplog.at_level(logging.WARNING):
        assert compile_tool_automaton([arr], TOK) is None
        assert compile_tool_automaton([RET, PLOT], TOK, max_states=500) is None
    assert sum("constraint refused" in r.getMessage() for r in caplog.records) == 2

    class NoBytes(SyntheticLlamaTokenizer):        # a vocabulary without a single-byte '{' token
        def decode_bytes(self, ids):
            return b"".join(b"{{" if int(i) == ord("{") else SyntheticLlamaTokenizer.decode_bytes(self, [i])
                            for i in ids)

    with caplog.at_level(logging.WARNING):
        assert compile_tool_automaton([RET], NoBytes()) is None
    assert compile_tool_automaton([RET], TOK) is compile_tool_automaton([RET], TOK)      # cached


def test_hf_token_bytes_come_from_the_byte_level_alphabet():
    class FakeTk:
        def id_to_token(self, i):
            return {0: "Ġcaf", 1: "Ã", 2: "©", 3: "<|eot_id|>"}[i]

    class FakeHF:
        tk = FakeTk()
        special = {"<|eot_id|>": 3}

        def decode_bytes(self, ids):               # what decoding one id alone would give
            return "�".encode()

    t = FakeHF()
    assert token_bytes(t, 0) == b" caf"
    assert token_bytes(t, 1) + token_bytes(t, 2) == "é".encode()
    assert token_bytes(t, 3) == b""


# ---------------------------------------------------------------------------------------------
# 2. build_masks_ref and advance against a Python byte walk
# ---------------------------------------------------------------------------------------------
def test_masks_ref_equals_python_walk(automata):
    a = automata["retrieval+plot"]
    rng = np.random.default_rng(5)
    body = int(a.walk(a.start, RHEAD.encode() + b'"search_query": "x'))
    states = sorted(set([a.start, a.done, body, int(a.walk(a.start, b"No tool call"))]
                        + rng.choice(a.num_states, 12, replace=False).tolist()))
    masks = build_masks_ref(a.byte_next, a.accept, a.tok_off, a.tok_bytes, a.eot_id, states=states)
    V = a.vocab_size
    assert masks.shape == (len(states), mask_words(V)) and mask_words(V) % 4 == 0
    bits = np.unpackbits(masks.view(np.uint8), axis=1, bitorder="little").astype(bool)
    assert not bits[:, V:].any()
    pieces = [TOK.decode_bytes([t]) if t not in TOK.special.values() else b"" for t in range(V)]
    for r, s in enumerate(states):
        for t in range(V):
            want = (a.walk(s, pieces[t]) >= 0) if pieces[t] else (t == a.eot_id and bool(a.accept[s]))
            assert bits[r, t] == want, (s, t)
            assert (a.advance(s, t) >= 0) == want, (s, t)
    assert bits[states.index(body)].sum() > 100_000               # a string admits most of the vocabulary
    eot_ok = np.flatnonzero(build_masks_ref(a.byte_next, a.accept, a.tok_off, a.tok_bytes, a.eot_id)
                            [:, a.eot_id >> 5] >> np.uint32(a.eot_id & 31) & 1)
    assert eot_ok.tolist() == np.flatnonzero(a.accept).tolist() and a.done in eot_ok
    assert a.advance(int(a.walk(a.start, b"No tool call")), a.eot_id) == a.done
    assert a.advance(a.done, a.eot_id) == a.done and a.advance(a.start, a.eot_id) == -1


def test_step_inputs_pack_roundtrip_with_fsm_state():
    e = np.zeros(0, np.int32)
    base = (np.arange(3, dtype=np.int32), np.arange(3, dtype=np.int32), np.arange(3, dtype=np.int32),
            np.zeros(1, np.int32), e, np.zeros((0, 1), np.int32), 0, np.ones(3, np.int32), np.zeros((3, 1), np.int32),
            np.arange(3, dtype=np.int64), np.ones(3, np.float32), np.arange(3, dtype=np.int64), e[:0].repeat(3),
            np.ones(3, np.float32))
    plain = StepInputs(*base)                    # positional constructors keep working
    assert plain.fsm_state is None and StepInputs.unpack(plain.pack()).fsm_state is None
    si = StepInputs(*base, fsm_state=np.asarray([5, -1, -4], np.int32))
    assert StepInputs.unpack(si.pack()).fsm_state.tolist() == [5, -1, -4]
    assert len(si.pack()) - len(plain.pack()) == 12              # only the array itself is added


# ---------------------------------------------------------------------------------------------
# 3. the engine on the CPU
# ---------------------------------------------------------------------------------------------
def _text(seq):
    ids = [t for t in seq.output_ids if t != EOT]
    return TOK.decode_bytes(ids).decode("utf-8", "surrogateescape")


def _run(mode, params_list, prompts, **cfg):
    eng = LLMEngine(EngineConfig(async_scheduling=mode, seed=0, **{**BASE, **cfg}))
    seqs = [eng.add_request(f"r{i}", p, sp) for i, (p, sp) in enumerate(zip(prompts, params_list))]
    while any(not s.finished for s in seqs) or eng.has_work():
        eng.step()
    return seqs, eng


def _prompts(n):
    return [list(range(300 + 7 * i, 340 + 7 * i)) for i in range(n)]


@pytest.mark.parametrize("mode", [True, False], ids=["overlap", "sync"])
def test_engine_probe_outputs_are_valid(automata, mode):
    """Random weights, temperature 1: unconstrained, no sequence would even start a JSON object."""
    n = 32
    sps = [SamplingParams(temperature=1.0, max_tokens=96, seed=1000 + i, constraint=automata["probe"])
           for i in range(n)]
    seqs, eng = _run(mode, sps, _prompts(n))
    texts = set()
    for s in seqs:
        assert s.finish_reason == "stop" and s.output_ids[-1] == EOT, (s.finish_reason, _text(s))
        check_output(_text(s), [PROBE])
        if _text(s) != "No tool call":
            PROBE.validate(json.loads(_text(s))["parameters"])
        texts.add(_text(s))
    assert len(texts) > 8
    st = eng.stats()
    # every output token came from a constrained row; overlap mode also launches the row behind a
    # sequence's still unknown eot, which is sampled and dropped
    total = sum(len(s.output_ids) for s in seqs)
    assert st["constrained_steps"] > 0
    assert st["constrained_tokens"] >= total if mode else st["constrained_tokens"] == total


@pytest.mark.parametrize("mode", [True, False], ids=["overlap", "sync"])
def test_engine_retrieval_prefixes_viable_and_batch_mates_unchanged(automata, mode):
    n = 6
    free = [SamplingParams(temperature=1.0, max_tokens=12, seed=50 + i, ignore_eos=True) for i in range(2)]
    con = [SamplingParams(temperature=1.0, max_tokens=40, seed=2000 + i, constraint=automata["retrieval"])
           for i in range(n)]
    prompts = _prompts(n + 2)
    seqs, eng = _run(mode, con + free, prompts)
    stops = 0
    for s in seqs[:n]:
        text = _text(s)
        assert automata["retrieval"].viable(text.encode("utf-8", "surrogateescape"))
        check_output(complete_prefix(text, [RET]), [RET])
        if s.finish_reason == "stop":
            stops += 1
            check_output(text, [RET])
    alone, eng2 = _run(mode, free, prompts[n:])
    assert [s.output_ids for s in seqs[n:]] == [s.output_ids for s in alone]
    assert eng2.stats()["constrained_steps"] == 0 and eng2.runner.fsm is None


@pytest.mark.parametrize("mode", [True, False], ids=["overlap", "sync"])
def test_constraint_with_jump_forward_saves_steps(automata, mode):
    n = 8
    g = ToolCallGrammar([PROBE])
    mk = lambda jump: [SamplingParams(temperature=1.0, max_tokens=96, seed=3000 + i, constraint=automata["probe"],  # noqa: E731
                                      grammar=g if jump else None) for i in range(n)]
    plain, e0 = _run(mode, mk(False), _prompts(n))
    jumped, e1 = _run(mode, mk(True), _prompts(n))
    for s in plain + jumped:
        assert s.finish_reason == "stop"
        check_output(_text(s), [PROBE])
    assert e1.runner.stats["steps"] < e0.runner.stats["steps"]


@pytest.mark.parametrize("mode", [True, False], ids=["overlap", "sync"])
def test_constraint_with_prompt_lookup_drafts(automata, mode):
    """Drafts copied from a prompt that holds a valid call: cut where the automaton dies, verified
    with the explicit state behind each draft prefix."""
    call = '{"name": "probe", "parameters": {"count": 41, "flag": true, "mode": "bb"}}'
    prompt = TOK.encode("Example: " + call + " and again: " + call + " Now:", allow_special=False)
    n = 8
    sps = [SamplingParams(temperature=1.0, max_tokens=96, seed=4000 + i, constraint=automata["probe"],
                          prompt_lookup=8) for i in range(n)]
    seqs, eng = _run(mode, sps, [prompt] * n)
    for s in seqs:
        assert s.finish_reason == "stop"
        check_output(_text(s), [PROBE])
    assert eng.spec_stats["proposed"] > 0 and eng.spec_stats["accepted"] > 0
    plain, _ = _run(mode, [SamplingParams(temperature=1.0, max_tokens=96, seed=4000 + i, constraint=automata["probe"])
                           for i in range(n)], [prompt] * n)
    assert [s.output_ids for s in seqs] == [s.output_ids for s in plain]     # speculation changes no token


# ---------------------------------------------------------------------------------------------
# 4. refusals and the switch
# ---------------------------------------------------------------------------------------------
def test_add_request_refuses_constraint_under_tp(automata):
    eng = LLMEngine(EngineConfig(seed=0, **BASE))
    eng.model.tp_size = 2                        # a tensor-parallel model (tp_size=2)
    with pytest.raises(NotImplementedError):
        eng.add_request("c", [1, 2, 3], SamplingParams(constraint=automata["probe"]))
    eng.add_request("u", [1, 2, 3], SamplingParams(max_tokens=1))     # unconstrained requests pass
    eng.model.tp_size = 1
    eng.cp = object()                            # a context-parallel engine
    with pytest.raises(NotImplementedError):
        eng.add_request("c2", [1, 2, 3], SamplingParams(constraint=automata["probe"]))
    assert eng.runner.fsm is None


def test_tables_full_drops_the_constraint_with_a_warning(automata, caplog):
    seqs, eng = _run(True, [SamplingParams(temperature=1.0, max_tokens=4, seed=1, constraint=automata["retrieval"])],
                     _prompts(1), fsm_max_states=automata["retrieval"].num_states)
    assert seqs[0].fsm_off == 0 and eng.runner.fsm.used == eng.runner.fsm.capacity
    with caplog.at_level(logging.WARNING):
        s = eng.add_request("over", [5, 6, 7], SamplingParams(max_tokens=2, constraint=automata["probe"]))
    assert s.fsm_off is None and any("constraint dropped" in r.getMessage() for r in caplog.records)


def test_switch_off_changes_nothing():
    """Scripted run without the switch: no constrained step, no table, the same step counts."""
    forced = TOK.encode('{"name": "probe", "parameters": {"count": 1, "flag": true}}', allow_special=False) + [EOT]
    sp = SamplingParams(temperature=0.5, max_tokens=64, forced_output=forced)
    seqs, eng = _run(True, [sp], _prompts(1))
    assert seqs[0].output_ids == forced
    assert eng.runner.stats["constrained_steps"] == 0 and eng.runner.fsm is None
    # a scripted decide with the constraint attached samples nothing: still no constrained step
    a = compile_tool_automaton([PROBE], TOK)
    seqs2, eng2 = _run(True, [SamplingParams(temperature=0.5, max_tokens=64, forced_output=forced, constraint=a)],
                       _prompts(1))
    assert seqs2[0].output_ids == forced and eng2.runner.stats["constrained_steps"] == 0
    assert eng2.runner.stats["steps"] == eng.runner.stats["steps"]


def test_sample_constrained_cpu_reference(automata):
    from financial_chatbot_llm_amd import ops
    a = automata["probe"]
    t = ops.FsmTables(a.num_states + 8, a.vocab_size, a.tok_off, a.tok_bytes, a.eot_id, "cpu")
    off = t.add(a.byte_next, a.accept, a.done)
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(5, a.vocab_size, generator=g)
    temps = torch.tensor([0.0, 1.0, 0.0, 1.0, 0.0])
    seeds = torch.arange(5, dtype=torch.int64) + 11
    final = a.walk(a.start, b"No tool call")
    state = torch.tensor([off + a.start, off + a.start, -1, off + final, a.num_states + 3], dtype=torch.int32)
    tok, ns = ops.sample_constrained(logits, temps, seeds, state, t)
    assert TOK.decode_bytes([int(tok[0])]) in (b"{", b"N", b"No", b'{"') or a.advance(a.start, int(tok[0])) >= 0
    assert [int(ns[i]) for i in (0, 1)] == [off + a.advance(a.start, int(tok[i])) for i in (0, 1)]
    assert int(tok[2]) == int(torch.argmax(logits[2])) and int(ns[2]) == -1
    assert int(tok[3]) == a.eot_id and int(ns[3]) == off + a.done
    assert int(tok[4]) == a.eot_id                                   # an unused state admits nothing
