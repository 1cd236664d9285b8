"""Multi-LoRA on the GPU: ``penny_lora_shrink`` / ``penny_lora_expand`` bit for bit against the exact
reference of ``lora_ref`` and within its derived bound of fp64 on random inputs, then the model and the
engine on the tiny Llama."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

from financial_chatbot_llm_amd import ops
from financial_chatbot_llm_amd.agent.automaton import compile_tool_automaton
from financial_chatbot_llm_amd.config import EngineConfig
from financial_chatbot_llm_amd.engine import LLMEngine, SamplingParams
from financial_chatbot_llm_amd.engine.model_runner import LORA_TWIN
from financial_chatbot_llm_amd.models.configs import get_model_config
from financial_chatbot_llm_amd.models.llama import LlamaModel
from financial_chatbot_llm_amd.ops import _native
import gen_logprob_ref as G
import lora_ref as R
import topn_logprob_ref as T
from test_constrain_cpu import PROBE
from test_gen_logprob_gpu import GEN_DRIFT_BF16

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 777.0
_CASES = {}


def exact_case(i: int):
    """(case, its table on the device, x on the device), built once per shape."""
    if i not in _CASES:
        case = R.ExactCase(R.SHAPES[i])
        _CASES[i] = (case, case.table(DEV), case.x().to(DEV))
    return _CASES[i]


def _framed(base: torch.Tensor):
    """``base`` placed inside a sentinel-filled buffer with a row stride above N; returns (buffer, view)."""
    M, N = base.shape
    buf = torch.full((M + 2, N + 16), SENT, dtype=base.dtype, device=DEV)
    view = buf[1:M + 1, 8:8 + N]
    view.copy_(base)
    return buf, view


def _frame_intact(buf: torch.Tensor, M: int, N: int) -> bool:
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[1:M + 1, 8:8 + N] = False
    return bool((buf[mask] == SENT).all())


# ------------------------------------------------------------------------------------------------
# kernels, exact
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", ["bf16", "slabs"])
@pytest.mark.parametrize("i", range(len(R.SHAPES)))
def test_kernels_exact(i, target):
    case, table, x = exact_case(i)
    sh = case.sh
    for name, pat in R.slot_patterns(sh.M).items():
        rs = torch.from_numpy(pat).to(DEV)
        if target == "bf16":
            base = R.random_base(sh, torch.bfloat16)
            buf, out = _framed(base.to(DEV))
            ops.lora_delta(x, out, table, R.LAYER, sh.group, rs)
            torch.cuda.synchronize()
            assert _frame_intact(buf, sh.M, sh.N), name
        else:
            base = R.random_base(sh, torch.float32)
            slabs = R.slabs_target(base.to(DEV))
            assert ops.lora_delta(x, slabs, table, R.LAYER, sh.group, rs) is slabs
            out = slabs.P[0]
            assert all(bool((slabs.P[s] == 1000 + s).all()) for s in (1, 2)), name
        want = case.expected(base, pat)
        assert R.same_bits(out, want), (name, target, int((R.bits(out.cpu()) != R.bits(want)).sum()))
        keep = torch.from_numpy(~((pat >= 0) & (pat < case.slots)))
        assert R.same_bits(out.cpu()[keep], base[keep]), name           # a -0.0 included (random_base)


def test_rank_padding_and_absent_segment():
    case, table, x = exact_case(1)
    sh = case.sh
    pat = R.slot_patterns(sh.M)["alternating"]
    rs = torch.from_numpy(pat).to(DEV)
    base = R.random_base(sh, torch.bfloat16)
    out = base.to(DEV)
    ops.lora_delta(x, out, table, R.LAYER, sh.group, rs)
    wide = case.table(DEV, rank=64)                 # the rank-16 adapters zero-padded to 64: the R = 64 kernels
    out64 = base.to(DEV)
    ops.lora_delta(x, out64, wide, R.LAYER, sh.group, rs)
    assert table.R == 32 and wide.R == 64
    assert R.same_bits(out64, out) and R.same_bits(out, case.expected(base, pat))
    q, k = sh.segs[0], sh.segs[1]
    rows2 = torch.from_numpy(pat == 2)              # slot 2 does not target the k segment
    assert R.same_bits(out.cpu()[rows2][:, q:q + k], base[rows2][:, q:q + k])
    # layer 0 of the table is empty: nothing moves
    out0 = base.to(DEV)
    ops.lora_delta(x, out0, table, 0, sh.group, rs)
    assert R.same_bits(out0, base)


def test_batch_invariance():
    """A row's bits are the same alone, at another row index, and beside other slots."""
    case, table, x = exact_case(4)                  # 257 rows
    sh = case.sh
    rc = R.RandomCase(sh)                           # random data: sums whose bits depend on their order
    rtable, rx = rc.table(DEV), rc.x.to(DEV)
    base = R.random_base(sh, torch.bfloat16).to(DEV)
    pat = R.slot_patterns(sh.M)["alternating"]
    full = base.clone()
    ops.lora_delta(rx, full, rtable, R.LAYER, sh.group, torch.from_numpy(pat).to(DEV))
    again = base.clone()
    ops.lora_delta(rx, again, rtable, R.LAYER, sh.group, torch.from_numpy(pat).to(DEV))
    assert R.same_bits(full, again)                 # the run
    for m in (0, 1, 17, 100, 256):
        s = int(pat[m])
        for M2, pos in ((1, 0), (5, 3), (40, 33)):  # alone; other positions, its mates on one other slot or none
            xs = rx[:M2].clone()
            bs = base[:M2].clone()
            xs[pos], bs[pos] = rx[m], base[m]
            mates = np.full(M2, (s + 1) % 3 if M2 == 40 else -1, np.int32)
            mates[pos] = s
            ops.lora_delta(xs, bs, rtable, R.LAYER, sh.group, torch.from_numpy(mates).to(DEV))
            assert R.same_bits(bs[pos], full[m]), (m, M2)


def test_graph_replay_reads_row_slot():
    case, table, x = exact_case(1)
    sh = case.sh
    pats = R.slot_patterns(sh.M)
    base = R.random_base(sh, torch.bfloat16).to(DEV)
    xs = x.clone()
    rs = torch.from_numpy(pats["none"]).to(DEV)
    out = base.clone()
    for _ in range(2):
        ops.lora_delta(xs, out, table, R.LAYER, sh.group, rs)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.lora_delta(xs, out, table, R.LAYER, sh.group, rs)
    x2 = torch.flip(x, dims=(0,)).contiguous()
    for name, xin in (("alternating", x), ("runs", x2), ("none", x)):
        rs.copy_(torch.from_numpy(pats[name]).to(DEV))
        xs.copy_(xin)
        out.copy_(base)
        g.replay()
        eager = base.clone()
        ops.lora_delta(xin, eager, table, R.LAYER, sh.group, torch.from_numpy(pats[name]).to(DEV))
        torch.cuda.synchronize()
        assert R.same_bits(out, eager), name
        if xin is x:
            assert R.same_bits(out, case.expected(base.cpu(), pats[name])), name


def test_entry_points_refuse():
    """K or R off the kernels' granularity, misaligned pointers, a bad segment table: hipErrorInvalidValue,
    nothing launched, outputs untouched."""
    case, table, x = exact_case(1)
    sh = case.sh
    G_ = table.groups[sh.group]
    M, K, N, R_ = sh.M, sh.K, sh.N, table.R
    rs = torch.zeros(M, dtype=torch.int32, device=DEV)
    part = torch.full((1, M, G_.nseg * R_), SENT, dtype=torch.float32, device=DEV)
    out = torch.full((M, N), SENT, dtype=torch.bfloat16, device=DEV)
    st = _native.stream()
    A, B = G_.A[R.LAYER], G_.B[R.LAYER]
    pres, scale = G_.present[R.LAYER], G_.scale

    def shrink(x_=x, xs=K, rs_=rs, A_=None, slots=table.slots, nseg=G_.nseg, R2=R_, part_=None, M_=M, K_=K, off=0):
        _native.call("penny_lora_shrink", x_.data_ptr() + off, xs, rs_.data_ptr(), (A if A_ is None else A_).data_ptr(),
                     slots, nseg, R2, (part if part_ is None else part_).data_ptr(), M_, K_, st)

    def expand(segs=G_.seg_end, nseg=G_.nseg, R2=R_, S=1, os_=N, N_=N, off=0, slots=table.slots, f32=0):
        c = (ctypes.c_int * max(len(segs), 1))(*segs)
        _native.call("penny_lora_expand", part.data_ptr(), S, rs.data_ptr(), B.data_ptr(), pres.data_ptr(),
                     scale.data_ptr(), slots, c, nseg, R2, out.data_ptr() + off, f32, os_, M, N_, st)
    bad_shrink = [dict(K_=K - 8), dict(K_=K + 16, xs=K + 16), dict(R2=16), dict(R2=48), dict(nseg=0), dict(nseg=4),
                  dict(off=2), dict(xs=K + 4), dict(xs=K - 8), dict(slots=0), dict(M_=-1)]
    for kw in bad_shrink:
        with pytest.raises(RuntimeError, match="hipError 1"):
            shrink(**kw)
    q, k, v = G_.seg_end
    bad_expand = [dict(segs=(q, k, v - 16)), dict(segs=(q, q, v)), dict(segs=(k, q, v)), dict(segs=(q + 8, k, v)),
                  dict(segs=(q, k, v), nseg=4), dict(segs=(), nseg=0), dict(R2=16), dict(R2=40), dict(S=0), dict(off=2),
                  dict(os_=N + 4), dict(os_=N - 16), dict(N_=N - 8), dict(slots=0)]
    for kw in bad_expand:
        with pytest.raises(RuntimeError, match="hipError 1"):
            expand(**kw)
    torch.cuda.synchronize()
    assert bool((part == SENT).all()) and bool((out == SENT).all())
    shrink()                                         # the unmodified calls do run
    expand()
    torch.cuda.synchronize()
    assert not bool((out == SENT).all())


def test_lora_delta_runs_both_hip_kernels(monkeypatch):
    calls = []
    real = _native.call
    monkeypatch.setattr(_native, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    case, table, x = exact_case(0)
    out = R.random_base(case.sh, torch.bfloat16).to(DEV)
    ops.lora_delta(x, out, table, R.LAYER, case.sh.group, torch.zeros(case.sh.M, dtype=torch.int32, device=DEV))
    assert calls == ["penny_lora_shrink", "penny_lora_expand"]


# ------------------------------------------------------------------------------------------------
# kernels, random inputs
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(R.RANDOM_SHAPES)))
def test_kernels_random_within_bound(i):
    sh = R.RANDOM_SHAPES[i]
    case = R.RandomCase(sh)
    table = case.table(DEV)
    for pname in ("one", "alternating"):
        pat = R.slot_patterns(sh.M)[pname]
        for dtype in (torch.bfloat16, torch.float32):
            base = R.random_base(sh, dtype)
            out = base.to(DEV)
            ops.lora_delta(case.x.to(DEV), out, table, R.LAYER, sh.group, torch.from_numpy(pat).to(DEV))
            y, bound = case.f64_expected(base, pat, table.R)
            bad = R.violations(out, y, bound)
            worst = float(((out.double().cpu() - y).abs() / bound.clamp(min=1e-300)).max())
            print(f"{sh} {pname} {dtype}: violations {bad}, largest error / bound {worst:.3f}")
            assert bad == 0, (pname, dtype)


# ------------------------------------------------------------------------------------------------
# model and engine (tiny Llama)
# ------------------------------------------------------------------------------------------------
CFG = dict(model="llama-tiny", device="cuda", num_kv_blocks=128, max_model_len=1024, max_num_seqs=8,
           graph_batch_sizes=(1, 2, 3, 4, 5, 6, 7, 8), seed=0)
MODES = {"eager-sync": (False, False), "eager-overlap": (False, True), "graph-sync": (True, False),
         "graph-overlap": (True, True)}
_MODEL = {}
STD = 0.3            # adapter magnitude: moves llama-tiny's logits well past the bf16 noise (checked below)


def _adapters(cfg):
    return {"a": R.tiny_adapter(cfg, 1, r=8, std=STD), "b": R.tiny_adapter(cfg, 2, r=16, std=STD)}


def _engine(graph, overlap, load=True, **kw):
    eng = LLMEngine(EngineConfig(use_cuda_graph=graph, async_scheduling=overlap, **{**CFG, **kw}),
                    model=_MODEL.get("m"))
    _MODEL["m"] = eng.model
    if load:
        for name, sd in _adapters(eng.model.cfg).items():
            eng.load_adapter(name, sd, alpha=16.0)
    if graph:
        eng.warmup()
    return eng


@pytest.mark.parametrize("kv_dtype", ["bf16", "fp8"])
def test_gpu_logits_match_cpu_reference_under_adapter(kv_dtype):
    """The project's model-level bf16 bound (test_gpu_forward_matches_cpu_reference): mean |GPU - CPU| <=
    0.01 max|CPU| + 0.01 under an adapter on all five targets, the CPU torch path on the same weights,
    adapter and KV pool format; the adapter itself moves the CPU reference by at least 10 times that bound."""
    cfg = get_model_config("llama-tiny")
    gpu = LlamaModel(cfg, device="cuda", tp_rank=0, tp_size=1).init_random(seed=1)
    cpu = LlamaModel(cfg, device="cpu", tp_rank=0, tp_size=1)
    cpu.w = {k: v.cpu() for k, v in gpu.w.items()}
    sd = R.tiny_adapter(cfg, 1, r=8, std=0.4, dtype=torch.bfloat16)
    R.model_table(gpu, [(sd, 2.0)])
    R.model_table(cpu, [(sd, 2.0)])
    ids = list(range(3, 3 + 200))

    a, b = R.model_logits(gpu, ids, 0, kv_dtype), R.model_logits(cpu, ids, 0, kv_dtype)
    bound = 0.01 * b.abs().max().item() + 0.01
    err = (a - b).abs().mean().item()
    effect = (b - R.model_logits(cpu, ids, None, kv_dtype)).abs().mean().item()
    print(f"{kv_dtype}: mean |gpu - cpu| = {err:.4e}, bound {bound:.4e}, adapter effect on the cpu reference {effect:.4e}")
    assert effect >= 10 * bound
    assert err <= bound


@pytest.fixture(scope="module")
def automaton():
    from financial_chatbot_llm_amd.engine.tokenizer import SyntheticLlamaTokenizer
    return compile_tool_automaton([PROBE], SyntheticLlamaTokenizer())


ADAPTER_OF = {"plain": "a", "lookup": "b", "filtered": "a", "constrained": "b", "penalised": "a", "scripted": "b",
              "jump": "a", "mate": None, "mate2": None}


def _scenario(eng, automaton, tag):
    """The mixed requests of ``topn_logprob_ref`` (prompt-lookup, top-k / top-p, a constraint, penalties, a
    scripted output, jump-forward, two batch mates), on two adapters and the base model; the filtered one
    also asks for top-3 alternatives."""
    by = T.scenario(eng.tokenizer, automaton, 0)
    seqs = {}
    for group in T.GROUPS:
        for n in group:
            prompt, p = by[n]
            p = dataclasses.replace(p, adapter=ADAPTER_OF[n], top_logprobs=3 if n == "filtered" else 0)
            seqs[n] = eng.add_request(f"{n}-{tag}", prompt, p)
        while any(not seqs[n].finished for n in group) or eng.has_work():
            eng.step()
    return seqs


_RESULTS = {}


@pytest.mark.parametrize("mode", list(MODES))
def test_modes_agree(mode, automaton):
    graph, overlap = MODES[mode]
    eng = _engine(graph, overlap)
    default_graphs = dict(eng.runner.graphs)
    seqs = _scenario(eng, automaton, mode)
    got = {n: (s.output_ids, s.finish_reason) for n, s in seqs.items()}
    _RESULTS[mode] = (got, G.pool_state(eng))
    first = next(iter(_RESULTS.values()))
    assert got == first[0], mode
    assert G.pool_state(eng) == first[1], mode       # the block pool and the prefix cache end alike
    st = eng.stats()
    assert st["lora_steps"] > 0 and st["lora_rows"] > 0 and st["lora_slots_used"] == 2
    base = _engine(graph, overlap, load=False)
    plain = T.scenario(base.tokenizer, automaton, 0)
    mate = base.add_request("mate-alone", *plain["mate"])
    while base.has_work():
        base.step()
    assert got["mate"][0] == mate.output_ids          # base-model rows beside adapter rows: the base model's tokens
    if graph:
        # each kind of request once more, alone: its decode steps replay its own LoRA twin
        for n in ("plain", "filtered", "constrained", "penalised"):
            prompt, p = T.scenario(eng.tokenizer, automaton, 0)[n]
            s = eng.add_request(f"alone-{n}", prompt, dataclasses.replace(p, adapter=ADAPTER_OF[n]))
            while eng.has_work():
                eng.step()
        assert not eng.runner._twin_failed
        kinds = {k for _, k, _ in eng.runner.twins if k.endswith(LORA_TWIN)}
        assert {"fused" + LORA_TWIN, "logits" + LORA_TWIN, "fsm" + LORA_TWIN, "pen" + LORA_TWIN} <= kinds, eng.runner.twins
        assert all(eng.runner.graphs[b] is g for b, g in default_graphs.items())      # not recaptured
        assert not any(k.endswith(LORA_TWIN) for _, k, _ in base.runner.twins)


def test_default_path_untouched():
    """Adapters loaded, no adapter row in flight: the same native calls and tokens as an engine that never
    loaded one."""
    prompts = [list(range(100 + 7 * i, 140 + 9 * i)) for i in range(3)]
    sp = SamplingParams(temperature=0.7, max_tokens=6, seed=5, ignore_eos=True)
    runs = []
    for load in (False, True):
        eng = _engine(False, False, load=load)
        calls = []
        real = _native.call
        _native.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
        try:
            seqs = [eng.add_request(f"d{i}", p, sp) for i, p in enumerate(prompts)]
            while eng.has_work():
                eng.step()
        finally:
            _native.call = real
        runs.append((calls, [s.output_ids for s in seqs]))
        assert eng.stats()["lora_steps"] == 0
    assert runs[0] == runs[1] and not any("lora" in n for n in runs[1][0])


def test_prefix_isolation_and_score():
    eng = _engine(False, True)
    p = list(range(500, 700))                          # 3 full blocks
    sc = {a: eng.score(p, adapter=a).logprobs for a in (None, "a", "b")}
    assert sc[None] != sc["a"] and sc["a"] != sc["b"] and sc[None] != sc["b"]
    sp = dict(temperature=0.8, max_tokens=8, seed=3, ignore_eos=True, logprobs=True)
    hits, outs = [], {}
    for a in (None, "a", "b", "a", None):
        h0 = eng.bm.hits
        s = eng.add_request(f"iso-{a}-{len(hits)}", p, SamplingParams(adapter=a, **sp))
        while eng.has_work():
            eng.step()
        hits.append(eng.bm.hits - h0)
        if a in outs:
            assert outs[a].output_ids == s.output_ids  # a repeat on its own blocks reproduces its answer
        outs[a] = s
    assert hits == [0, 0, 0, 3, 3]                      # no cross hits; a repeat hits its own blocks
    assert len({tuple(s.output_ids) for s in outs.values()}) == 3
    # score(ids, adapter=) against the generation-time log-probabilities under the same adapter
    for a, s in outs.items():
        ref = eng.score(s.prompt_ids + s.output_ids, adapter=a).logprobs[len(s.prompt_ids) - 1:]
        drift = max(abs(x - y) for x, y in zip(s.output_logprobs, ref))
        print(f"adapter {a}: score() vs generation drift {drift:.4e} nats")
        assert drift <= 2 * GEN_DRIFT_BF16


def test_unload_and_slot_reuse():
    eng = _engine(True, True)
    p = list(range(40, 90))
    sp = SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True)
    ref = eng.generate([p], dataclasses.replace(sp, adapter="b"))[0]
    live = eng.add_request("live", p, dataclasses.replace(sp, adapter="a"))
    with pytest.raises(RuntimeError, match="live"):
        eng.unload_adapter("a")
    while eng.has_work():
        eng.step()
    eng.unload_adapter("a")
    assert eng.load_adapter("c", _adapters(eng.model.cfg)["b"], alpha=16.0) == 0
    assert eng.generate([p], dataclasses.replace(sp, adapter="c"))[0] == ref          # b's weights in a's old slot
    assert eng.generate([p], dataclasses.replace(sp, adapter="b"))[0] == ref
    assert live.output_ids != ref


@pytest.mark.timeout(240)
def test_process_engine_round_trip(tmp_path):
    """load -> generate -> unload across the process boundary, against the in-process engine."""
    import asyncio
    from financial_chatbot_llm_amd.engine.process_engine import ProcessAsyncEngine
    cfg = get_model_config("llama-tiny")
    path = R.write_peft_dir(str(tmp_path / "a"), _adapters(cfg)["a"], 8, 16.0)
    p = list(range(40, 90))
    sp = SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True)
    ref_eng = _engine(False, False)
    want = {a: ref_eng.generate([p], dataclasses.replace(sp, adapter=a))[0] for a in (None, "a")}
    assert want[None] != want["a"]
    eng = ProcessAsyncEngine(EngineConfig(use_cuda_graph=True, **{**CFG, "graph_batch_sizes": (1, 2)}))

    async def main():
        assert eng.load_adapter("a", path) == 0 and sorted(eng.adapters()) == ["a"]
        for a in (None, "a", None, "a"):
            out = await eng.generate_all(p, dataclasses.replace(sp, adapter=a))
            assert out.seq.output_ids == want[a], a
        with pytest.raises(Exception, match="nope"):
            await eng.generate_all(p, dataclasses.replace(sp, adapter="nope"))
        sc = (await eng.score(p, adapter="a")).logprobs
        assert sc != (await eng.score(p)).logprobs
        eng.unload_adapter("a")
        with pytest.raises(KeyError):
            eng.unload_adapter("a")
        assert eng.load_adapter("again", path) == 0          # the slot is free again
        assert (await eng.generate_all(p, dataclasses.replace(sp, adapter="again"))).seq.output_ids == want["a"]
        s = eng.stats()
        assert s["lora_slots_used"] == 1 and s["lora_steps"] > 0 and s["lora_table_mb"] > 0
    try:
        asyncio.run(main())
    finally:
        eng.shutdown()
    assert not eng._proc.is_alive()
