"""Generation log-probabilities on the GPU: the log-probability forms of the fused LM heads
(gemm_prefill.hip EPI_SAMPLE_LP, gemm_splitk.hip SK_SAMPLE_LP, their shared merge kernel),
``penny_token_logprob`` for steps that hold logits, and the engine end to end.

Kernel tests use exact inputs (``gen_logprob_ref``): every logit is exact in f32 under any accumulation
order, so the chosen logit lc and the row maximum Mx equal the reference bit for bit and only log S
rounds.  LOGPROB_TOL = 1e-4 nats against the f64 log-softmax, re-derived for these kernels:

* a partial's sum: each lane adds its 4 * FW <= 32 terms (FW = 2, 4 or 8 row groups per wave: partials
  32, 64 or 128 columns wide), then two xor-shuffle additions -- at most 34 f32 additions on a path;
* the merge: a thread adds ceil(P / 256) of the row's P partials (P = 4008 for the streaming kernel
  at V = 128256, nf = 4: 16 terms; P = 4 .. 32 in these tests), then 6 shuffle additions and 3 to
  join the four waves -- at most 25;
* every addition of positive terms adds at most 2^-24 relative error: <= 59 * 2^-24 = 3.5e-6;
* each term passes two __expf (l - pm in the partial, pm - Mx in the merge): the argument's product
  with log2 e rounds to 2^-24 relative of |argument| <= 32, 2.8e-6 absolute in the exponent each,
  plus one ulp of v_exp_f32 each: <= 6e-6 relative together;
* logf is good to 2 ulp of |log S| <= 12 (1.4e-6); lc - Mx is exact (two bf16 values of magnitude
  below 32) and the final subtraction rounds once (<= 32 * 2^-24 = 1.9e-6).

Sum: below 1.3e-5 nats for any fan-in up to the production 4008 partials per row, so 1e-4 keeps the
margin of tests/test_logprob_gpu.py for the same reduction.  The order of the reduction is fixed
(lane, shuffle tree, strided thread sums, tree), so the figure does not depend on the launch.
"""

import pytest
import torch

from financial_chatbot_llm_amd import ops
from financial_chatbot_llm_amd.agent.automaton import compile_tool_automaton
from financial_chatbot_llm_amd.config import EngineConfig
from financial_chatbot_llm_amd.engine import LLMEngine
from financial_chatbot_llm_amd.ops import _native, gemm
import gen_logprob_ref as R
from test_constrain_cpu import PROBE

pytestmark = pytest.mark.gpu
DEV = "cuda"
INVALID = 1            # hipErrorInvalidValue


def _dev(c):
    return c.x.to(DEV), c.w.to(DEV), c.temps.to(DEV), c.seeds.to(DEV)


def _check(c, ids, lp, voff=0, what=""):
    """ids' planted winners / tie rule, the input condition on the drawn tokens, logprob vs f64."""
    ids_c, lp_c = ids.cpu(), lp.cpu()
    for r, col in c.planted.items():
        assert int(ids_c[r]) == voff + col, (what, r)
    if c.tie_row is not None:
        assert int(ids_c[c.tie_row]) == voff + 5, what          # tied maxima: the smaller id
    want = c.logprob_ref(ids_c, voff)
    samp = ~c.greedy
    if bool(samp.any()):
        assert int((want[samp] < -0.1).sum()) * 2 >= int(samp.sum()), what
    err = (lp_c.double() - want).abs().max().item()
    print(f"{what}: max |logprob - f64 log_softmax| = {err:.3e}")
    assert err <= R.LOGPROB_TOL, what
    return err


# ------------------------------------------------------------------------------------------------
# the tile kernel
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,V", R.TILE_SHAPES)
def test_tile_kernel_same_tokens_and_logprob(M, V, monkeypatch):
    monkeypatch.setenv("PENNY_FUSED_LM_HEAD", "force")       # the tile kernel below 128 rows too
    c = R.case(M, V, None, M > 12)
    x, w, temps, seeds = _dev(c)
    plain = ops.lm_head_sample(x, w, temps, seeds)
    ids, lp = ops.lm_head_sample_logprob(x, w, temps, seeds)
    assert ids.dtype == torch.int32 and lp.dtype == torch.float32
    assert torch.equal(ids, plain)                            # greedy and Gumbel rows, bit for bit
    _check(c, ids, lp, what=f"tile M={M} V={V}")
    if M > 1:    # batch invariance: row 1 alone is bit-equal to row 1 in the batch
        i1, l1 = ops.lm_head_sample_logprob(x[1:2].contiguous(), w, temps[1:2].contiguous(), seeds[1:2].contiguous())
        assert torch.equal(i1, ids[1:2]) and torch.equal(l1.view(torch.int32), lp[1:2].view(torch.int32))


# ------------------------------------------------------------------------------------------------
# the streaming kernel: both nf, both W forms, both rings
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", R.STREAM_M)
def test_stream_kernel_same_tokens_and_logprob(M):
    c = R.case(M, 512, None, M > 12)
    x, w, temps, seeds = _dev(c)
    wt = gemm.tile_weight(w)
    d_nf, d_r2 = ops.sampling.stream_cfg(M)
    first = None
    for nf in (4, 8):
        for rowmajor in (True, False):
            for ring2 in (d_r2, not d_r2):
                wk = w if rowmajor else wt
                kw = dict(nf=nf, rowmajor=rowmajor, ring2=ring2)
                plain = ops.lm_head_stream_sample(x, wk, temps, seeds, **kw)
                ids, lp = ops.lm_head_stream_sample_logprob(x, wk, temps, seeds, **kw)
                assert torch.equal(ids, plain), kw
                _check(c, ids, lp, what=f"stream M={M} {kw}")
                first = ids if first is None else first
                assert torch.equal(ids, first), kw            # exact logits: one token whatever the form
    # the routed entry point: the streaming kernel below 128 rows, with the table's nf and ring
    ids, lp = ops.lm_head_sample_logprob(x, w, temps, seeds, wt=wt)
    assert torch.equal(ids, ops.lm_head_sample(x, w, temps, seeds, wt=wt)) and torch.equal(ids, first)
    _check(c, ids, lp, what=f"routed M={M} nf={d_nf}")


# ------------------------------------------------------------------------------------------------
# vocabulary padding on both kernels
# ------------------------------------------------------------------------------------------------
def test_vocab_padding_both_kernels(monkeypatch):
    vvalid, voff = 300, 1000
    for M in (129, 17):
        c = R.case(M, 512, vvalid)
        x, w, temps, seeds = _dev(c)
        if M >= 128:
            pairs = ops.lm_head_sample_shard(x, w, vvalid, voff, temps, seeds)
        else:
            pairs = ops.lm_head_stream_sample(x, w, temps, seeds, vvalid=vvalid, voff=voff, pairs=True)
        ids, lp = ops.lm_head_sample_logprob(x, w, temps, seeds, vvalid=vvalid, voff=voff)
        assert torch.equal(ids, pairs[:, 1].contiguous())                 # global ids of the plain kernel
        assert int(ids.min()) >= voff and int(ids.max()) < voff + vvalid
        _check(c, ids, lp, voff, what=f"padding M={M}")
    monkeypatch.setenv("PENNY_FUSED_LM_HEAD", "force")                    # the tile kernel at 17 rows
    ids_t, lp_t = ops.lm_head_sample_logprob(x, w, temps, seeds, vvalid=vvalid, voff=voff)
    assert torch.equal(ids_t, ids)
    _check(c, ids_t, lp_t, voff, what="padding tile M=17")


def test_unfused_route_is_opt_in(monkeypatch):
    """PENNY_LOGPROB_UNFUSED=1 sends 17 rows (inside LOGPROB_UNFUSED_ROWS) through logits + sampler +
    token_logprobs; on exact inputs that is the same token and the same number.  Unset: fused."""
    c = R.case(17, 512, None, True)
    x, w, temps, seeds = _dev(c)
    calls = []
    real = _native.call
    monkeypatch.setattr(_native, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    fused = ops.lm_head_sample_logprob(x, w, temps, seeds)
    assert "penny_lm_head_stream_sample_logprob" in calls and "penny_token_logprob" not in calls
    monkeypatch.setenv("PENNY_LOGPROB_UNFUSED", "1")
    del calls[:]
    ids, lp = ops.lm_head_sample_logprob(x, w, temps, seeds)
    assert "penny_token_logprob" in calls and "penny_sample" in calls
    assert not any(n.startswith("penny_lm_head") for n in calls)
    assert torch.equal(ids, fused[0])
    _check(c, ids, lp, what="unfused route M=17")
    del calls[:]
    ops.lm_head_sample_logprob(*_dev(R.case(64, 512, None, True)))                # outside the ranges: fused
    assert calls == ["penny_lm_head_stream_sample_logprob"]


# ------------------------------------------------------------------------------------------------
# token_logprobs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("B,V", [(1, 8), (5, 1000), (3, 128256)])
def test_token_logprobs(B, V, dtype, monkeypatch):
    logits, ids, want = R.token_logprob_rows(B, V, dtype)
    ld, idd = logits.to(DEV), ids.to(DEV)
    got = ops.token_logprobs(ld, idd).cpu()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan) and bool(nan[-1]) == (B >= 3)
    err = (got[~nan].double() - want[~nan]).abs().max().item()
    print(f"token_logprobs B={B} V={V} {dtype}: {err:.3e}")
    assert err <= R.LOGPROB_TOL
    # a column-slice view (row stride V + 3, base off a 16-B boundary) takes the _aligned_rows copy
    wide = torch.cat([torch.zeros(B, 3, dtype=dtype), logits], 1).to(DEV)
    view = wide[:, 3:]
    calls = []
    real = ops.sampling._aligned_rows
    monkeypatch.setattr(ops.sampling, "_aligned_rows", lambda t: (calls.append(t.data_ptr()), real(t))[1])
    sl = ops.token_logprobs(view, idd).cpu()
    assert calls == [view.data_ptr()] and real(view).data_ptr() != view.data_ptr()
    assert torch.equal(sl[~nan], got[~nan])
    assert bool(torch.isnan(ops.token_logprobs(ld, torch.full((B,), V, dtype=torch.int32, device=DEV))).all())


# ------------------------------------------------------------------------------------------------
# contract: refused without a launch
# ------------------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments():
    lib = _native.load()
    c = R.case(17, 512)
    x, w, temps, seeds = _dev(c)
    ws = torch.empty(5 * 17 * 64, dtype=torch.float32, device=DEV)
    out = torch.full((17,), -7, dtype=torch.int32, device=DEV)
    lp = torch.full((17,), 7.0, dtype=torch.float32, device=DEV)
    p, st = _native.ptr, _native.stream()

    def tile(K=128, Vpad=512, vvalid=512, o=out, l=lp):
        return lib.penny_lm_head_sample_logprob(p(x), x.stride(0), p(w), K, 17, Vpad, vvalid, 0, p(temps), p(seeds),
                                                p(ws), p(o), p(l), st)

    def stream(K=128, Vpad=512, vvalid=512, o=out, l=lp, nf=4):
        return lib.penny_lm_head_stream_sample_logprob(p(x), x.stride(0), p(w), K, 17, Vpad, vvalid, 0, p(temps),
                                                       p(seeds), p(ws), p(o), p(l), nf, 1, 0, st)
    for f in (tile, stream):
        assert f(Vpad=500, vvalid=300) == INVALID      # Vpad % 256 (and % 64, % 128)
        assert f(K=96) == INVALID                      # K % 64
        assert f(vvalid=513) == INVALID                # vvalid > Vpad
        assert f(o=None) == INVALID and f(l=None) == INVALID
    assert tile(Vpad=384, vvalid=384) == INVALID       # a multiple of 128 that is no multiple of 256
    assert stream(nf=2) == INVALID
    lg = torch.zeros(2, 8, dtype=torch.float32, device=DEV)
    i2 = torch.zeros(2, dtype=torch.int32, device=DEV)
    assert lib.penny_token_logprob(None, 1, 8, p(i2), p(lp), 2, 8, st) == INVALID
    assert lib.penny_token_logprob(p(lg), 1, 8, None, p(lp), 2, 8, st) == INVALID
    assert lib.penny_token_logprob(p(lg), 1, 8, p(i2), None, 2, 8, st) == INVALID
    assert lib.penny_token_logprob(p(lg), 1, 8, p(i2), p(lp), 2, 0, st) == INVALID
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and bool((lp == 7.0).all())       # nothing ran


# ------------------------------------------------------------------------------------------------
# the engine (tiny Llama)
# ------------------------------------------------------------------------------------------------
# Drift between a token's log-probability reported at generation time and score() of the same
# tokens.  score() runs the prompt + output as prefill chunks (prefill attention, the tile LM head);
# generation ran decode attention and the streaming LM head (or the logits GEMM), which accumulate in
# other orders -- a bf16 hidden state landing on the neighbouring value moves a logit by one bf16 ulp,
# the cause of the 1.97e-3 chunking drift recorded in tests/test_logprob_gpu.py.  Measured on an
# MI355X over the scenario of gen_logprob_ref (max over its sampled positions, all step modes):
#   bf16 KV pool: 7.8230e-3 nats in both overlap modes (eager and hipGraph), 9.7752e-4 in both sync modes
#   fp8 KV pool:  7.8173e-3 nats (overlap, eager)
# -- one bf16 ulp of a logit in [1, 2) (2^-7 = 7.8125e-3), respectively in [0.125, 0.25) (2^-10), on
# top of f32 rounding: four times the chunking drift, the same cause.  The tests allow twice the
# larger value, the file convention of tests/test_logprob_gpu.py (2 x E2E_DRIFT).
GEN_DRIFT_BF16 = 7.822990e-3      # bf16 KV pool
GEN_DRIFT_FP8 = 7.817268e-3       # fp8 KV pool (its own value: the cache itself is quantised)

CFG = dict(model="llama-tiny", device="cuda", num_kv_blocks=128, max_model_len=1024, max_num_seqs=8,
           graph_batch_sizes=(1, 2, 3, 4, 5, 6, 7, 8), seed=0)
MODES = {"eager-overlap": (False, True), "graph-overlap": (True, True), "eager-sync": (False, False),
         "graph-sync": (True, False)}
_MODEL = {}


def _engine(graph, overlap, **kw):
    eng = LLMEngine(EngineConfig(use_cuda_graph=graph, async_scheduling=overlap, **{**CFG, **kw}),
                    model=_MODEL.get("m"))
    _MODEL["m"] = eng.model
    if graph:
        eng.warmup()
    return eng


@pytest.fixture(scope="module")
def automaton():
    from financial_chatbot_llm_amd.engine.tokenizer import SyntheticLlamaTokenizer
    return compile_tool_automaton([PROBE], SyntheticLlamaTokenizer())


def on_off(graph, overlap, automaton, **kw):
    """The scenario with logprobs off, then on, on two engines sharing one model: (off seqs, on seqs,
    on outputs, engine of the on run, pool states)."""
    e0 = _engine(graph, overlap, **kw)
    off, _ = R.run_scenario(e0, automaton, False, "g")
    s0 = R.pool_state(e0)
    assert e0.stats()["logprob_steps"] == 0 and not any(lp for _, _, lp in e0.runner.twins)
    e1 = _engine(graph, overlap, **kw)
    on, outs = R.run_scenario(e1, automaton, True, "g")
    return off, on, outs, e1, (s0, R.pool_state(e1))


@pytest.mark.parametrize("mode", list(MODES))
def test_engine_tokens_unchanged_aligned_and_drift(mode, automaton):
    graph, overlap = MODES[mode]
    off, on, outs, eng, (s0, s1) = on_off(graph, overlap, automaton)
    for n in R.NAMES:
        assert on[n].output_ids == off[n].output_ids, n
        assert on[n].finish_reason == off[n].finish_reason, n
    R.check_alignment(on, outs)
    assert s0 == s1                                     # block pool and prefix cache as without logprobs
    st = eng.runner.stats
    assert st["logprob_steps"] > 0
    if graph:    # the log-probability twins were captured lazily and replayed; the default graphs stand
        assert not eng.runner._twin_failed and st["graph_steps"] > 0
        assert {kind for _, kind, lp in eng.runner.twins if lp} >= {"fused", "fsm"}
    drift = R.score_drift(eng, on)
    print(f"{mode}: generation vs score() drift = {drift:.4e} nats, spec {eng.spec_stats}")
    assert drift <= 2 * GEN_DRIFT_BF16


def test_engine_fp8_kv_pool(automaton):
    off, on, outs, eng, (s0, s1) = on_off(False, True, automaton, kv_dtype="fp8")
    assert eng.stats()["kv_dtype"] == "fp8"
    for n in R.NAMES:
        assert on[n].output_ids == off[n].output_ids, n
    R.check_alignment(on, outs)
    assert s0 == s1
    drift = R.score_drift(eng, on)
    print(f"fp8 KV: generation vs score() drift = {drift:.4e} nats")
    assert drift <= 2 * GEN_DRIFT_FP8


def test_fused_steps_stay_fused(automaton):
    """A batch without filters or constraints keeps sampling inside the LM head when it asks for
    log-probabilities: no logits GEMM + sampler launch, only the log-probability entry points."""
    eng = _engine(False, True)
    calls = []
    real = _native.call
    _native.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        from financial_chatbot_llm_amd.engine import SamplingParams
        seqs = [eng.add_request(f"f{i}", list(range(200 + i, 240 + i)),
                                SamplingParams(temperature=0.7, max_tokens=6, seed=i, ignore_eos=True, logprobs=i == 0))
                for i in range(3)]
        while eng.has_work():
            eng.step()
    finally:
        _native.call = real
    assert len(seqs[0].output_logprobs) == 6 and seqs[1].output_logprobs == []
    lp_calls = [n for n in calls if n in ("penny_lm_head_sample_logprob", "penny_lm_head_stream_sample_logprob")]
    assert lp_calls and "penny_sample" not in calls and "penny_token_logprob" not in calls
    assert "penny_lm_head_sample" not in calls and "penny_lm_head_stream_sample" not in calls
