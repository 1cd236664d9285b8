"""Repetition / presence / frequency penalties on the GPU: the kernels of csrc/kernels/penalty.hip
against the float64 reference (tests/penalty_ref.py: the bounds are derived there), penalties in front
of the samplers against the fp64 sampler replica (tests/selection_ref.py), the sampling stage's
log-probabilities, and the engine in eager / hipGraph and sync / overlap mode."""
import numpy as np
import pytest
import torch

from financial_chatbot_llm_amd import ops
from financial_chatbot_llm_amd.ops import _native
import penalty_ref as R
from selection_ref import check_sampled, sample_ref
from test_selection_kernels_gpu import EPS, boundary_is_clear

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = {"eager-sync": (False, False), "eager-overlap": (False, True), "graph-sync": (True, False),
         "graph-overlap": (True, True)}


# ------------------------------------------------------------------------------------------------
# kernels
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", R.RESET_V)
def test_reset(V):
    R.check_reset(V, DEV)


def test_add():
    R.check_add(DEV)


@pytest.mark.parametrize("S,V", R.APPLY_SHAPES)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
def test_apply(S, V, dtype, exact):
    R.check_apply_all(S, V, dtype, exact, DEV)


def test_apply_runs_the_hip_kernel(monkeypatch):
    calls = []
    real = _native.call
    monkeypatch.setattr(_native, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    R.check_apply_all(3, 1000, torch.bfloat16, True, DEV)
    R.check_reset(8, DEV)
    R.check_add(DEV)
    assert {"penny_pen_apply", "penny_pen_reset", "penny_pen_add"} <= set(calls)


def test_entry_points_refuse():
    R.check_refusals(DEV)
    # the native checks themselves: hipErrorInvalidValue, nothing launched
    t = ops.PenaltyTable(2, 1000, DEV)
    lib = _native.load()
    ids = torch.tensor([1], dtype=torch.int32, device=DEV)
    st = _native.stream()
    assert lib.penny_pen_reset(_native.ptr(t.table), 2, 1000, 1000, 2, _native.ptr(ids), 1, st) == 1
    assert lib.penny_pen_reset(_native.ptr(t.table), 2, 1001, 1000, 0, _native.ptr(ids), 1, st) == 1
    assert lib.penny_pen_reset(_native.ptr(t.table) + 2, 2, 1000, 1000, 0, _native.ptr(ids), 1, st) == 1
    assert lib.penny_pen_add(_native.ptr(t.table) + 2, 2, 1000, 1000, _native.ptr(ids), 1, st) == 1
    torch.cuda.synchronize()
    assert not bool(t.table.any())


# ------------------------------------------------------------------------------------------------
# apply, then the samplers
# ------------------------------------------------------------------------------------------------
def _sampler_case(nucleus=True):
    """17 f32 rows at V = 2056 (finite logits): greedy rows, Gumbel rows and rows with top-k / top-p.
    A row under top-p is the first of a seeded sequence of N(0, 4T) rows whose PENALISED form (float64
    reference) keeps the nucleus cut 1e-3 of mass away from p, as in test_selection_kernels_gpu."""
    S, V = 17, 2056
    c = R.apply_case(S, V, torch.float32, False, seed=5)
    temps = torch.tensor([(0.0, 0.8, 1.0)[r % 3] for r in range(S)], dtype=torch.float32)
    seeds = torch.arange(S, dtype=torch.int64) * 7919 + 3
    top_k = torch.tensor([(0, 0, 20, 0)[r % 4] for r in range(S)], dtype=torch.int32)
    top_p = torch.tensor([(1.0, 1.0, 1.0, 0.8 if nucleus else 1.0)[r % 4] for r in range(S)], dtype=torch.float32)
    rows = []
    for r in range(S):
        tt = max(float(temps[r]), 0.5)
        for attempt in range(200):
            row = torch.randn(V, generator=torch.Generator().manual_seed(500 + 1000 * attempt + r)) * 4.0 * tt
            if float(top_p[r]) >= 1 or float(temps[r]) <= 0:
                break
            pen = row.double().numpy()[None, :]
            if int(c.slot[r]) >= 0:
                pen = R.penalise(pen, c.rows[r:r + 1], c.pending[r:r + 1], c.rep[r:r + 1], c.pres[r:r + 1],
                                 c.freq[r:r + 1])[0]
            if boundary_is_clear(pen[0], int(top_k[r]), float(top_p[r]), float(temps[r]))[0]:
                break
        rows.append(row)
    c.logits = torch.stack(rows)
    return c, temps, seeds, top_k, top_p


def _keep(pl, top_k, top_p, temps):
    """Survivors of top-k / top-p over ``pl`` (what the sampler reads), after checking that no cut
    sits on a tie or within rounding of p: an input condition, asserted on the kernel's own logits."""
    for b in range(pl.shape[0]):
        if float(temps[b]) <= 0:
            continue
        k, srt = int(top_k[b]), np.sort(pl[b].double().numpy())[::-1]
        if 0 < k < srt.size and np.isfinite(srt[k - 1]):
            assert srt[k - 1] != srt[k], f"row {b}: tie at the top-k boundary"
        if float(top_p[b]) < 1:
            ok, why = boundary_is_clear(pl[b], k, float(top_p[b]), float(temps[b]))
            assert ok, f"row {b}: {why}"
    return torch.isfinite(ops.apply_top_k_top_p(pl, top_k, top_p, temps))


def test_apply_then_sample():
    c, temps, seeds, top_k, top_p = _sampler_case()
    t = R.table_of(c, DEV)
    d = lambda x: x.to(DEV)              # noqa: E731
    raw = d(c.logits)
    pl = ops.apply_penalties(raw, d(c.slot), d(c.pending), d(c.rep), d(c.pres), d(c.freq), t,
                             out=torch.empty_like(raw))
    R.check_apply(pl.cpu(), c, False)
    off = (c.slot < 0) | c.neutral
    # no filters
    tok = ops.sample(pl, d(temps), d(seeds)).cpu()
    scores, _, _ = sample_ref(pl.cpu(), temps, seeds)
    check_sampled(tok, scores, EPS, greedy=temps <= 0)
    assert torch.equal(tok[off], ops.sample(raw, d(temps), d(seeds)).cpu()[off])
    assert not torch.equal(tok[~off], ops.sample(raw, d(temps), d(seeds)).cpu()[~off])
    # top-k / top-p behind the penalties
    keep = _keep(pl.cpu(), top_k, top_p, temps)
    tok = ops.sample(pl, d(temps), d(seeds), top_k=d(top_k), top_p=d(top_p)).cpu()
    scores, _, _ = sample_ref(pl.cpu(), temps, seeds, keep=keep)
    check_sampled(tok, scores, EPS, greedy=temps <= 0)
    assert torch.equal(tok[off], ops.sample(raw, d(temps), d(seeds), top_k=d(top_k), top_p=d(top_p)).cpu()[off])


def test_apply_then_sample_constrained():
    from financial_chatbot_llm_amd.ops.constrain import masked_logits
    world = R.World(DEV)
    a = world.automaton
    c, temps, seeds, top_k, top_p = _sampler_case(nucleus=False)
    V = 2056
    tables = ops.FsmTables(a.num_states + 8, V, a.tok_off, a.tok_bytes, a.eot_id, DEV)
    off0 = tables.add(a.byte_next, a.accept, a.done)
    state = torch.tensor([off0 + a.start if r % 2 == 0 else -1 for r in range(17)], dtype=torch.int32)
    t = R.table_of(c, DEV)
    d = lambda x: x.to(DEV)              # noqa: E731
    pl = ops.apply_penalties(d(c.logits), d(c.slot), d(c.pending), d(c.rep), d(c.pres), d(c.freq), t)
    tok, nxt = ops.sample_constrained(pl, d(temps), d(seeds), d(state), tables, top_k=d(top_k), top_p=d(top_p))
    ml = masked_logits(pl, d(state), tables).cpu()        # penalties, then the mask, then top-k / top-p
    assert bool(torch.isfinite(ml).any(1).all())
    keep = _keep(ml, top_k, top_p, temps) & torch.isfinite(ml)
    scores, _, _ = sample_ref(ml, temps, seeds, keep=keep)
    check_sampled(tok.cpu(), scores, EPS, greedy=temps <= 0)
    assert bool((nxt.cpu()[state < 0] == -1).all())


def test_sample_stage_logprobs_stay_raw():
    """ModelRunner._sample with lp=True and penalised rows: the tokens come from the penalised logits,
    the log-probabilities are ``ops.token_logprobs`` of the RAW logits, bit for bit."""
    world = R.World(DEV)
    eng = world.engine(False, False)
    run = eng.runner
    V = eng.model.cfg.vocab_size
    S = 5
    table = run.ensure_penalty_table(4)
    hot = torch.randint(0, V, (4, 4000), generator=torch.Generator().manual_seed(1))
    for s in range(4):
        ops.penalty.reset(table, s, hot[s, :100])
        ops.penalty.add(table, torch.stack([torch.full((3900,), s), hot[s, 100:]], 1).to(torch.int32))
    g = torch.Generator().manual_seed(2)
    hs = (torch.randn(S, eng.model.cfg.hidden_size, generator=g) * 0.5).to(eng.model.dtype).to(DEV)
    temps = torch.tensor([0.0, 0.8, 1.0, 0.0, 0.7], device=DEV)
    seeds = torch.arange(S, dtype=torch.int64, device=DEV) + 11
    slot = torch.tensor([0, -1, 2, 3, 1], dtype=torch.int32, device=DEV)
    pend = torch.tensor([-1, -1, 5, int(hot[3, 0]), -1], dtype=torch.int32, device=DEV)
    par = torch.tensor([[1.3, 1.0, 1.2, 1.0, 1.5], [0.5, 0.0, 0.2, 0.9, 0.0], [0.3, 0.0, 0.1, 0.0, 0.4]],
                       device=DEV)
    raw = eng.model.logits(hs).contiguous()
    keep = raw.clone()
    # the raw argmax of every slotted row has been emitted three times: its penalty moves the greedy rows
    top = raw.float().argmax(1).to(torch.int32)
    ops.penalty.add(table, torch.stack([slot, top], 1)[slot >= 0].repeat(3, 1))
    got = run._sample(hs, "pen", temps, seeds, None, None, None, True, (slot, pend, par))
    assert torch.equal(R.to_bits(eng.model.logits(hs).contiguous()), R.to_bits(keep))
    pl = ops.apply_penalties(raw.clone(), slot, pend, par[0], par[1], par[2], table)
    assert torch.equal(got.out, ops.sample(pl, temps, seeds))
    assert not torch.equal(got.out, ops.sample(raw, temps, seeds))
    want = ops.token_logprobs(raw, got.out)
    assert torch.equal(got.logprob.view(torch.int32), want.view(torch.int32))
    plain = run._sample(hs, "pen", temps, seeds, None, None, None, False, (slot, pend, par))
    assert torch.equal(plain.out, got.out) and plain.logprob is None


# ------------------------------------------------------------------------------------------------
# engine
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def world():
    return R.World(DEV)


@pytest.mark.parametrize("mode", list(MODES))
def test_no_repeats_under_presence(world, mode):
    R.check_no_repeats(world, *MODES[mode])


def test_mode_equality_and_recount(world):
    R.check_mode_equality(world, MODES)


def test_table_after_every_step(world):
    R.check_table_every_step(world)


@pytest.mark.parametrize("mode", list(MODES))
def test_batch_mates(world, mode):
    R.check_batch_mates(world, *MODES[mode])


@pytest.mark.parametrize("mode", ["eager-overlap", "graph-overlap"])
def test_slot_exhaustion(world, mode):
    R.check_slot_exhaustion(world, *MODES[mode])


@pytest.mark.parametrize("mode", list(MODES))
def test_off_means_off(world, mode):
    R.check_off(world, *MODES[mode])


@pytest.mark.parametrize("mode", ["eager-sync", "graph-overlap"])
def test_scripted_and_speculative(world, mode):
    R.check_scripted_and_spec(world, *MODES[mode])


def test_refusals(world):
    R.check_engine_refusals(world)
