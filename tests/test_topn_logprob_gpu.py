"""Top-N alternatives on the GPU: ``penny_topn_logprob`` against the f64 reference of
``topn_logprob_ref`` (ids exactly, values bit-equal to ``ops.token_logprobs`` and within
``gen_logprob_ref.LOGPROB_TOL`` of f64 -- the bound tests/test_gen_logprob_gpu.py derives for this
reduction, whose code and order the kernel shares), and the engine end to end on the tiny Llama.
"""
import pytest
import torch

from financial_chatbot_llm_amd import ops
from financial_chatbot_llm_amd.agent.automaton import compile_tool_automaton
from financial_chatbot_llm_amd.config import EngineConfig
from financial_chatbot_llm_amd.engine import LLMEngine, SamplingParams
from financial_chatbot_llm_amd.engine.model_runner import TOPN_TWIN
from financial_chatbot_llm_amd.ops import _native
import gen_logprob_ref as G
import topn_logprob_ref as R
from test_constrain_cpu import PROBE
from test_gen_logprob_gpu import GEN_DRIFT_BF16

pytestmark = pytest.mark.gpu
DEV = "cuda"
INVALID = 1            # hipErrorInvalidValue
SENT_ID, SENT_LP = -7, 7.0
DTYPES = pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])


def _buffers(B):
    return (torch.full((B,), SENT_LP, dtype=torch.float32, device=DEV),
            torch.full((B, R.TOPN_MAX), SENT_ID, dtype=torch.int32, device=DEV),
            torch.full((B, R.TOPN_MAX), SENT_LP, dtype=torch.float32, device=DEV))


def _bits(t):
    return t.contiguous().view(torch.int32)


def _check_bit_equal_to_token_logprobs(c, ld, lp, top_ids, top_lp):
    """Column by column: top_lp[:, j] is what token_logprobs reports for the ids top_ids[:, j]; the
    chosen token's value likewise (rows that asked; -0 / NaN compared as bits, NaN rows as NaN)."""
    tn = c.topn.to(DEV)
    own = ops.token_logprobs(ld, c.ids.to(DEV))
    rows = tn > 0
    same = (_bits(own) == _bits(lp)) | (torch.isnan(own) & torch.isnan(lp))
    assert bool(same[rows].all()), c.name
    for j in range(int(tn.max())):
        rows = tn > j
        col = ops.token_logprobs(ld, top_ids[:, j].clamp(min=0).contiguous())
        same = (_bits(col) == _bits(top_lp[:, j])) | (torch.isnan(col) & torch.isnan(top_lp[:, j]))
        assert bool(same[rows].all()), (c.name, j)


# ------------------------------------------------------------------------------------------------
# the kernel
# ------------------------------------------------------------------------------------------------
@DTYPES
def test_kernel_matches_reference_on_every_case(dtype):
    """Shapes (n == V, ragged tails, one chunk either side of a full sweep, 128256), per-row n mixing
    0 / 1 / 5 / 20, the tie cases, -inf / NaN / +inf rows and ids outside the vocabulary, in
    sentinel-filled buffers."""
    for c in R.cases(dtype):
        ld = c.logits.to(DEV)
        bufs = _buffers(ld.shape[0])
        got = ops.topn_logprobs(ld, c.ids.to(DEV), c.topn.to(DEV), out=bufs)
        assert all(a is b for a, b in zip(got, bufs))
        R.check_case(c, *got, SENT_ID, SENT_LP, G.LOGPROB_TOL)
        _check_bit_equal_to_token_logprobs(c, ld, *got)
        # the same answer with the per-row n given on the host (validated there, exact max_n)
        again = ops.topn_logprobs(ld, c.ids.to(DEV), c.topn, out=_buffers(ld.shape[0]))
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, again)), c.name


@DTYPES
@pytest.mark.parametrize("B,V", [(1, 8), (5, 1000), (3, 128256)])
def test_values_against_f64_on_token_logprob_rows(B, V, dtype):
    """The inputs test_token_logprobs holds this reduction to 1e-4 nats on: every alternative's value
    within the same bound of the f64 log-softmax, the NaN row all NaN."""
    logits, ids, want = G.token_logprob_rows(B, V, dtype)
    n = min(R.TOPN_MAX, V)
    lp, top_ids, top_lp = (t.cpu() for t in ops.topn_logprobs(logits.to(DEV), ids.to(DEV), n))
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(lp), nan) and bool(nan[-1]) == (B >= 3)
    assert (lp[~nan].double() - want[~nan]).abs().max().item() <= G.LOGPROB_TOL
    worst = 0.0
    for b in range(B):
        if nan[b]:
            assert bool(torch.isnan(top_lp[b, :n]).all()) and bool(((top_ids[b, :n] >= 0) & (top_ids[b, :n] < V)).all())
            continue
        assert R.certificate(logits[b], top_ids[b, :n].tolist()) is None
        ref = torch.log_softmax(logits[b].double(), -1)[top_ids[b, :n].long()]
        worst = max(worst, (top_lp[b, :n].double() - ref).abs().max().item())
    print(f"topn values B={B} V={V} {dtype}: {worst:.3e}")
    assert worst <= G.LOGPROB_TOL


@DTYPES
def test_strided_view_takes_the_aligned_copy(dtype, monkeypatch):
    c = next(x for x in R.cases(dtype) if x.name == "rand V=1000 B=5")
    want = ops.topn_logprobs(c.logits.to(DEV), c.ids.to(DEV), c.topn.to(DEV), out=_buffers(5))
    wide = torch.cat([torch.zeros(5, 3, dtype=dtype), c.logits], 1).to(DEV)
    view = wide[:, 3:]                       # row stride V + 3, base off a 16-B boundary
    calls = []
    real = ops.sampling._aligned_rows
    monkeypatch.setattr(ops.sampling, "_aligned_rows", lambda t: (calls.append(t.data_ptr()), real(t))[1])
    got = ops.topn_logprobs(view, c.ids.to(DEV), c.topn.to(DEV), out=_buffers(5))
    assert calls == [view.data_ptr()] and real(view).data_ptr() != view.data_ptr()
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, want))


def test_entry_point_refuses_bad_arguments():
    lib = _native.load()
    p, st = _native.ptr, _native.stream()
    lg = torch.zeros(2, 64, dtype=torch.float32, device=DEV)
    ids = torch.zeros(2, dtype=torch.int32, device=DEV)
    tn = torch.full((2,), 3, dtype=torch.int32, device=DEV)
    lp, ti, tl = _buffers(2)

    def call(logits=lg, i=ids, n=tn, max_n=3, a=lp, b=ti, c=tl, V=64):
        return lib.penny_topn_logprob(p(logits), 1, 64, p(i), p(n), max_n, p(a), p(b), p(c), 2, V, st)
    for kw in (dict(logits=None), dict(i=None), dict(n=None), dict(a=None), dict(b=None), dict(c=None)):
        assert call(**kw) == INVALID, kw
    assert call(V=0) == INVALID and call(V=-5) == INVALID
    assert call(max_n=21) == INVALID                   # n > TOPN_MAX
    assert call(max_n=9, V=8) == INVALID               # n > V
    assert call(max_n=-1) == INVALID
    torch.cuda.synchronize()
    assert bool((lp == SENT_LP).all()) and bool((ti == SENT_ID).all()) and bool((tl == SENT_LP).all())   # nothing ran
    assert call() == 0                                 # and the same call within the contract runs
    torch.cuda.synchronize()
    assert ti[:, :3].tolist() == [[0, 1, 2], [0, 1, 2]] and bool((ti[:, 3:] == SENT_ID).all())
    # a device n above the host's bound is capped at it: no write past column max_n
    tn.fill_(20)
    lp, ti, tl = _buffers(2)
    assert call(a=lp, b=ti, c=tl) == 0
    torch.cuda.synchronize()
    assert bool((ti[:, 3:] == SENT_ID).all()) and bool((tl[:, 3:] == SENT_LP).all())
    with pytest.raises(ValueError):
        ops.topn_logprobs(lg, ids, torch.tensor([1, 21]))


@DTYPES
def test_graph_capture_and_replay(dtype):
    """Captured in a hipGraph and replayed twice on changed inputs (logits, ids and per-row n): equal
    to the eager launch bit for bit."""
    cs = [x for x in R.cases(dtype) if x.name in ("rand V=8200 B=5", "four values V=8200")]
    B, V = 5, 8200
    lg = torch.zeros(B, V, dtype=dtype, device=DEV)
    ids = torch.zeros(B, dtype=torch.int32, device=DEV)
    tn = torch.zeros(B, dtype=torch.int32, device=DEV)
    bufs = _buffers(B)
    ops.topn_logprobs(lg, ids, tn, out=bufs)            # warm up outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.topn_logprobs(lg, ids, tn, out=bufs)
    for c in cs + cs[:1]:
        b = c.logits.shape[0]
        lg.zero_()
        lg[:b].copy_(c.logits)
        ids.zero_()
        ids[:b].copy_(c.ids)
        tn.zero_()
        tn[:b].copy_(c.topn)
        for t, v in zip(bufs, (SENT_LP, SENT_ID, SENT_LP)):
            t.fill_(v)
        g.replay()
        eager = ops.topn_logprobs(lg, ids, tn, out=_buffers(B))
        torch.cuda.synchronize()
        assert all(torch.equal(_bits(a), _bits(e)) for a, e in zip(bufs, eager)), c.name
        R.check_case(c, bufs[0][:b], bufs[1][:b], bufs[2][:b], SENT_ID, SENT_LP, G.LOGPROB_TOL)


# ------------------------------------------------------------------------------------------------
# the engine (tiny Llama)
# ------------------------------------------------------------------------------------------------
CFG = dict(model="llama-tiny", device="cuda", num_kv_blocks=128, max_model_len=1024, max_num_seqs=8,
           graph_batch_sizes=(1, 2, 3, 4, 5, 6, 7, 8), seed=0)
MODES = {"eager-overlap": (False, True), "graph-overlap": (True, True), "eager-sync": (False, False),
         "graph-sync": (True, False)}
_MODEL = {}
TOP = 5


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


class _Spy:
    """Wraps ``ops.topn_logprobs`` as the runner calls it: certifies every top-N row of every eager call
    against the very logits it was given (the step's raw logits, or the LM-head logits GEMM's)."""

    def __init__(self):
        self.real = ops.topn_logprobs
        self.rows = 0

    def __call__(self, logits, ids, topn, out=None):
        res = self.real(logits, ids, topn, out=out)
        if torch.cuda.is_current_stream_capturing():
            return res
        lc, tn, ti, tl = logits.float().cpu(), topn.cpu().tolist(), res[1].cpu(), res[2].cpu()
        for b, n in enumerate(tn):
            if n > 0:
                sel = ti[b, :n].tolist()
                assert R.certificate(lc[b], sel) is None, (b, sel)
                assert R.values_ok(lc[b], sel, tl[b, :n].tolist(), G.LOGPROB_TOL) is None, b
                self.rows += 1
        return res


def _score_drift(eng, seqs) -> float:
    """max |listed value - score(prefix + listed token)| over every sampled position and every
    alternative: the same quantity from the decode path and from the prefill path."""
    worst = 0.0
    for s in seqs.values():
        for k, t in enumerate(s.output_top_logprobs):
            for tok, lp in t or ():
                ref = eng.score(s.prompt_ids + s.output_ids[:k] + [tok]).logprobs[-1]
                worst = max(worst, abs(ref - lp))
    return worst


@pytest.mark.parametrize("mode", list(MODES))
def test_engine_tokens_unchanged_and_lists_certified(mode, automaton, monkeypatch):
    graph, overlap = MODES[mode]
    e0 = _engine(graph, overlap)
    off, _ = R.run_scenario(e0, automaton, 0, "g")
    s0 = G.pool_state(e0)
    assert e0.stats()["top_logprob_steps"] == 0 and not any(k.endswith(TOPN_TWIN) for _, k, _ in e0.runner.twins)
    e1 = _engine(graph, overlap)
    spy = _Spy()
    monkeypatch.setattr(ops, "topn_logprobs", spy)
    on, outs = R.run_scenario(e1, automaton, TOP, "g")
    monkeypatch.setattr(ops, "topn_logprobs", spy.real)
    for n in R.NAMES:
        assert on[n].output_ids == off[n].output_ids, n
        assert on[n].finish_reason == off[n].finish_reason, n
    assert on["mate"].output_logprobs == [] and on["mate2"].output_top_logprobs == []
    R.check_alignment(on, outs, TOP, greedy_first=False)     # incl. chosen value == its list entry, bit for bit
    assert s0 == G.pool_state(e1)                            # block pool and prefix cache as without the feature
    st = e1.runner.stats
    assert st["top_logprob_steps"] > 0 and spy.rows > 0      # prefill-step rows are eager in every mode
    if graph:
        # the second group's requests and a batch mate once more, each alone: in the scenario the
        # constrained and the penalised one share their steps, and a constrained + penalised step runs
        # eagerly; alone, each decodes on its own twin (the mate on the default graph).  Rows sampled
        # inside a replayed graph leave no logits to certify against: the same checks of alignment and
        # of the chosen value against its list entry, and every listed value against score()
        replays = {"default": 0, "twin": 0}
        real_decode = e1.runner._graph_decode

        def counted(si, g):
            replays["default" if g is e1.runner.graphs.get(g.B) else "twin"] += 1
            return real_decode(si, g)
        monkeypatch.setattr(e1.runner, "_graph_decode", counted)
        before = st["graph_steps"]
        names = ("penalised", "filtered", "constrained", "mate")
        alone, alone_outs = {0: {}, TOP: {}}, []
        for eng, top in ((e0, 0), (e1, TOP)):
            by = R.scenario(eng.tokenizer, automaton, top)
            for name in names:
                alone[top][name] = eng.add_request(f"alone-{name}-{top}", *by[name])
                while eng.has_work():
                    got = eng.step()
                    if top:
                        alone_outs += got
        for name in names:
            assert alone[TOP][name].output_ids == alone[0][name].output_ids, name
            assert alone[TOP][name].finish_reason == alone[0][name].finish_reason, name
        R.check_alignment(alone[TOP], alone_outs, TOP, greedy_first=False)
        twins = {k for _, k, lp in e1.runner.twins if lp and k.endswith(TOPN_TWIN)}
        assert not e1.runner._twin_failed and not e0.runner._twin_failed
        assert twins == {k + TOPN_TWIN for k in ("fused", "fsm", "pen", "logits")}, e1.runner.twins
        assert not any(k.endswith(TOPN_TWIN) for _, k, _ in e0.runner.twins)
        # the mate's decode steps replayed the default graphs, the others' their twins
        assert replays["default"] > 0 and replays["twin"] > 0, replays
        assert replays["default"] + replays["twin"] == st["graph_steps"] - before
        asked = {n: on[n] for n in R.NAMES if not n.startswith("mate")}
        asked.update({"alone-" + n: s for n, s in alone[TOP].items()})
        drift = _score_drift(e1, asked)
        print(f"{mode}: listed values vs score() drift = {drift:.4e} nats")
        assert drift <= 2 * GEN_DRIFT_BF16
        drift = G.score_drift(e1, alone[TOP])
        print(f"{mode}: chosen values vs score() drift, requests alone = {drift:.4e} nats")
        assert drift <= 2 * GEN_DRIFT_BF16
    drift = G.score_drift(e1, on)
    print(f"{mode}: chosen values vs score() drift = {drift:.4e} nats, certified rows {spy.rows}")
    assert drift <= 2 * GEN_DRIFT_BF16


def test_fused_steps_stay_fused_and_add_gemm_and_topn():
    """A fused-kind step with a top-N row still samples through the fused LM head's entry point, then
    runs the logits GEMM and penny_topn_logprob; a step without such a row runs neither."""
    eng = _engine(False, True)
    calls, gemms = [], []
    real, real_logits = _native.call, eng.model.logits
    _native.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    eng.model.logits = lambda h: (gemms.append(h.shape[0]), real_logits(h))[1]

    def run(top):
        del calls[:], gemms[:]
        seqs = [eng.add_request(f"f{top}-{i}", list(range(200 + i, 240 + i)),
                                SamplingParams(temperature=0.7, max_tokens=6, seed=i, ignore_eos=True,
                                               top_logprobs=top if i == 0 else 0))
                for i in range(3)]
        while eng.has_work():
            eng.step()
        return seqs
    try:
        plain = run(0)
        assert "penny_topn_logprob" not in calls and not gemms
        assert any(n in ("penny_lm_head_sample", "penny_lm_head_stream_sample") for n in calls)
        seqs = run(4)
    finally:
        _native.call = real
        del eng.model.logits
    assert [s.output_ids for s in seqs] == [s.output_ids for s in plain]
    assert len(seqs[0].output_top_logprobs) == 6 and seqs[1].output_top_logprobs == [] and seqs[1].output_logprobs == []
    fused = [n for n in calls if n in ("penny_lm_head_sample_logprob", "penny_lm_head_stream_sample_logprob")]
    assert fused and calls.count("penny_topn_logprob") == len(fused) == len(gemms)
    assert "penny_sample" not in calls and "penny_token_logprob" not in calls
    assert eng.stats()["top_logprob_steps"] == len(fused)
