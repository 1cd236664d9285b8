"""Repetition / presence / frequency penalties without a GPU: the torch path of ops.penalty against the
float64 reference (tests/penalty_ref.py), the sampling-stage plan, and the engine end to end on the
CPU (eager, sync and overlap), where every path is deterministic."""
import pytest
import torch

from financial_chatbot_llm_amd import ops
from financial_chatbot_llm_amd.config import EngineConfig, ServingConfig
from financial_chatbot_llm_amd.engine.model_runner import (DEFAULT_GRAPH, EAGER, StepInputs, graph_plan,
                                                           sampler_kind)
from financial_chatbot_llm_amd.engine.sequence import SamplingParams, Sequence
import penalty_ref as R

SC = R

DEV = "cpu"


# ------------------------------------------------------------------------------------------------
# the new fields (fails on the parent)
# ------------------------------------------------------------------------------------------------
def test_fields_exist():
    p = SamplingParams()
    assert (p.repetition_penalty, p.presence_penalty, p.frequency_penalty) == (1.0, 0.0, 0.0)
    assert EngineConfig().penalty_slots == 64
    s = ServingConfig()
    assert (s.respond_repetition_penalty, s.respond_presence_penalty, s.respond_frequency_penalty) == (1.0, 0.0, 0.0)
    si = StepInputs.control(StepInputs.CTRL_RCCL_FALLBACK)
    assert si.pen is None and si.pen_params is None and si.pen_add is None
    assert not {"pen", "pen_params", "pen_add"} & set(StepInputs._ARRAYS)          # not on the C4 wire
    seq = Sequence("r", [1, 2], p)
    assert seq.pen_slot == -1 and seq.pen_counted == 0


def test_plan_with_penalties():
    for fsm in (False, True):
        for filt in (False, True):
            for shard in (False, True):
                for fused in (False, True):
                    assert sampler_kind(fsm, filt, shard, fused, False) == sampler_kind(fsm, filt, shard, fused)
                    assert sampler_kind(fsm, filt, shard, fused, True) == ("fsm" if fsm else "pen")
            for lp in (False, True):
                for bf in (False, True):
                    for tp in (False, True):
                        assert graph_plan(fsm, filt, lp, bf, tp, False) == graph_plan(fsm, filt, lp, bf, tp)
                        want = EAGER if tp or fsm else ("pen", lp)
                        assert graph_plan(fsm, filt, lp, bf, tp, True) == want
    assert graph_plan(False, False, False, True, False) == DEFAULT_GRAPH


# ------------------------------------------------------------------------------------------------
# table kernels (torch path)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", SC.RESET_V)
def test_reset(V):
    SC.check_reset(V, DEV)


def test_add():
    SC.check_add(DEV)


@pytest.mark.parametrize("S,V", SC.APPLY_SHAPES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
def test_apply(S, V, dtype, exact):
    SC.check_apply_all(S, V, dtype, exact, DEV)


def test_apply_then_sample_greedy():
    """Greedy rows are exact on the CPU sampler too: the argmax of the penalised logits."""
    c = R.apply_case(17, 1000, torch.float32, False, seed=3)
    c.logits = torch.nan_to_num(c.logits, nan=0.0, posinf=9.0, neginf=-9.0).clamp(-30, 30)
    t = SC.table_of(c, DEV)
    pl = ops.apply_penalties(c.logits.clone(), c.slot, c.pending, c.rep, c.pres, c.freq, t)
    temps, seeds = torch.zeros(17), torch.arange(17, dtype=torch.int64)
    tok = ops.sample(pl, temps, seeds)
    assert tok.tolist() == pl.double().argmax(1).tolist()
    raw = ops.sample(c.logits, temps, seeds)
    off = (c.slot < 0) | c.neutral
    assert torch.equal(tok[off], raw[off]) and not torch.equal(tok[~off], raw[~off])


def test_entry_points_refuse():
    SC.check_refusals(DEV)


# ------------------------------------------------------------------------------------------------
# engine (CPU: eager sync and eager overlap)
# ------------------------------------------------------------------------------------------------
MODES = {"eager-sync": (False, False), "eager-overlap": (False, True)}


@pytest.fixture(scope="module")
def world():
    return SC.World(DEV)


@pytest.mark.parametrize("mode", list(MODES))
def test_no_repeats_under_presence(world, mode):
    SC.check_no_repeats(world, *MODES[mode])


def test_mode_equality_and_recount(world):
    SC.check_mode_equality(world, MODES)


def test_table_after_every_step(world):
    SC.check_table_every_step(world)


def test_cpu_replay(world):
    SC.check_cpu_replay(world)


@pytest.mark.parametrize("mode", list(MODES))
def test_batch_mates(world, mode):
    SC.check_batch_mates(world, *MODES[mode])


@pytest.mark.parametrize("mode", list(MODES))
def test_slot_exhaustion(world, mode):
    SC.check_slot_exhaustion(world, *MODES[mode])


@pytest.mark.parametrize("mode", list(MODES))
def test_off_means_off(world, mode):
    SC.check_off(world, *MODES[mode])


@pytest.mark.parametrize("mode", list(MODES))
def test_scripted_and_speculative(world, mode):
    SC.check_scripted_and_spec(world, *MODES[mode])


def test_refusals(world):
    SC.check_engine_refusals(world)


# ------------------------------------------------------------------------------------------------
# serving
# ------------------------------------------------------------------------------------------------
def test_respond_switches_reach_respond_only(monkeypatch):
    SC.check_serving(monkeypatch)
