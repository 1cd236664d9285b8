"""Engine on the GPU: HIP forward vs CPU reference, hipGraph decode vs eager, MoE, encoder."""
import copy

import pytest
import torch

from financial_chatbot_llm_amd.config import EngineConfig
from financial_chatbot_llm_amd.engine import LLMEngine, SamplingParams
from financial_chatbot_llm_amd.models.common import AttentionMetadata, KVCache
from financial_chatbot_llm_amd.models.configs import get_model_config
from financial_chatbot_llm_amd.models.llama import LlamaModel
from financial_chatbot_llm_amd.models.mixtral import MixtralModel
from financial_chatbot_llm_amd.ops.attention import KV_BS

pytestmark = pytest.mark.gpu


def _logits(m, ids):
    T = len(ids)
    nb = (T + KV_BS - 1) // KV_BS
    dev = m.device
    kv = KVCache(m.cfg.num_layers, nb + 1, m.hkv, m.D, dtype=m.dtype, device=dev)
    bt = torch.arange(1, nb + 1, dtype=torch.int32)[None].to(dev)
    slots = torch.tensor([(1 + p // KV_BS) * KV_BS + p % KV_BS for p in range(T)], dtype=torch.int32).to(dev)
    meta = AttentionMetadata(slots=slots, num_prefill_tokens=T,
                             cu_q=torch.tensor([0, T], dtype=torch.int32).to(dev),
                             ctx_lens_p=torch.tensor([T], dtype=torch.int32).to(dev), block_tables_p=bt, max_q_len=T)
    h = m.forward(torch.tensor(ids, dtype=torch.int32).to(dev), torch.arange(T, dtype=torch.int32).to(dev), meta, kv)
    return m.logits(h).float().cpu()


@pytest.mark.parametrize("name", ["llama-tiny", "mixtral-tiny"])
def test_gpu_forward_matches_cpu_reference(name):
    cfg = get_model_config(name)
    cls = MixtralModel if cfg.arch == "mixtral" else LlamaModel
    gpu = cls(cfg, device="cuda", tp_rank=0, tp_size=1).init_random(seed=1)
    cpu = cls(cfg, device="cpu", tp_rank=0, tp_size=1)
    cpu.w = {k: v.cpu() for k, v in gpu.w.items()}
    ids = list(range(3, 3 + 200))
    a, b = _logits(gpu, ids), _logits(cpu, ids)
    # bf16 GPU vs fp32-math CPU reference; MoE routing can flip near-tied experts for a few
    # tokens, so bound the typical error and the argmax agreement rather than the worst token
    err = (a - b).abs().mean().item()
    assert err < 0.01 * b.abs().max().item() + 0.01, err
    assert (a.argmax(-1) == b.argmax(-1)).float().mean() > 0.85


def test_tiled_only_gate_up_weights(monkeypatch):
    """A gate|up shape kept only fragment-tiled (ops.gemm.TILED_ONLY, the 70B TP=1 setting) runs every
    path on the tiled copy: the prefill tile kernel's tiled form (300 tokens) matches the CPU reference
    on the row-major weight, and greedy decoding (eager + graphs) agrees with the two-copy model."""
    from financial_chatbot_llm_amd.ops import gemm
    cfg = get_model_config("llama-tiny")
    shape = (2 * cfg.intermediate_size, cfg.hidden_size)
    monkeypatch.setattr(gemm, "TILED_ONLY", {shape})
    gpu = LlamaModel(cfg, device="cuda", tp_rank=0, tp_size=1).init_random(seed=1)
    assert gpu.w["layers.0.gate_up"] is None and gpu.wt["layers.0.gate_up"] is not None
    cpu = LlamaModel(cfg, device="cpu", tp_rank=0, tp_size=1)
    cpu.w = {k: (v if v is not None else gemm.untile_weight(gpu.wt[k]).contiguous()).cpu() for k, v in gpu.w.items()}
    ids = list(range(3, 3 + 300))
    a, b = _logits(gpu, ids), _logits(cpu, ids)
    err = (a - b).abs().mean().item()
    assert err < 0.01 * b.abs().max().item() + 0.01, err
    base = dict(model="llama-tiny", device="cuda", num_kv_blocks=128, max_model_len=2048, max_num_seqs=16,
                graph_batch_sizes=(1, 2, 4, 8, 16))
    prompts = [list(range(100 + 7 * i, 100 + 7 * i + 30 + 17 * i)) for i in range(5)]
    sp = SamplingParams(temperature=0.0, max_tokens=10, ignore_eos=True)
    tiled = LLMEngine(EngineConfig(use_cuda_graph=True, **base), model=gpu)
    tiled.warmup()
    out_t = tiled.generate(prompts, sp)
    monkeypatch.setattr(gemm, "TILED_ONLY", set())
    ref_m = LlamaModel(cfg, device="cuda", tp_rank=0, tp_size=1)
    ref_m.w = {k: (v if v is not None else gemm.untile_weight(gpu.wt[k]).contiguous()) for k, v in gpu.w.items()}
    ref_m.prepare_decode_weights()
    out_r = LLMEngine(EngineConfig(use_cuda_graph=False, **base), model=ref_m).generate(prompts, sp)
    agree = sum(x == y for p, q in zip(out_t, out_r) for x, y in zip(p, q)) / 50
    assert agree >= 0.9, (out_t, out_r)


@pytest.mark.parametrize("model", ["llama-tiny", "mixtral-tiny"])
def test_graph_decode_matches_eager(model):
    """bf16 Mixtral included: its decode MoE must be capturable (no host sync)."""
    base = dict(model=model, device="cuda", num_kv_blocks=128, max_model_len=2048, max_num_seqs=16,
                graph_batch_sizes=(1, 2, 4, 8, 16))
    prompts = [list(range(100 + 7 * i, 100 + 7 * i + 30 + 17 * i)) for i in range(5)]
    sp = SamplingParams(temperature=0.0, max_tokens=10, ignore_eos=True)
    e1 = LLMEngine(EngineConfig(use_cuda_graph=False, **base))
    eager = e1.generate(prompts, sp)
    e2 = LLMEngine(EngineConfig(use_cuda_graph=True, **base), model=e1.model)
    e2.warmup()
    graph = e2.generate(prompts, sp)
    assert e2.runner.stats["graph_steps"] >= 9
    agree = sum(a == b for x, y in zip(eager, graph) for a, b in zip(x, y)) / 50
    assert agree >= 0.9, (eager, graph)


def test_sampling_seeded_reproducible_and_batch_invariant():
    cfg = EngineConfig(model="llama-tiny", device="cuda", num_kv_blocks=64, max_model_len=1024, max_num_seqs=8,
                       graph_batch_sizes=(1, 2, 4, 8))
    eng = LLMEngine(cfg)
    eng.warmup()
    sp = SamplingParams(temperature=0.7, max_tokens=6, ignore_eos=True, seed=1234)
    a = eng.generate([list(range(10, 50))], sp)[0]
    b = eng.generate([list(range(10, 50)), list(range(60, 90)), list(range(5, 9))], sp)[0]
    assert a == b


def test_top_k_top_p_decode_stays_on_graphs():
    """top-k/top-p requests no longer fall back to eager decode: the HIP threshold kernel is part
    of every captured graph; top_k=1 equals greedy at any temperature."""
    cfg = EngineConfig(model="llama-tiny", device="cuda", num_kv_blocks=64, max_model_len=1024, max_num_seqs=8,
                       graph_batch_sizes=(1, 2, 4, 8))
    eng = LLMEngine(cfg)
    eng.warmup()
    prompts = [list(range(10, 50)), list(range(60, 90))]
    greedy = eng.generate(prompts, SamplingParams(temperature=0.0, max_tokens=8, ignore_eos=True))
    g0 = eng.runner.stats["graph_steps"]
    k1 = eng.generate(prompts, SamplingParams(temperature=1.5, top_k=1, max_tokens=8, ignore_eos=True))
    assert k1 == greedy
    assert eng.runner.stats["graph_steps"] - g0 >= 7
    nuc = eng.generate(prompts, SamplingParams(temperature=0.8, top_k=40, top_p=0.9, max_tokens=8, ignore_eos=True,
                                               seed=7))
    assert all(len(o) == 8 for o in nuc)


def test_mixtral_fp8_experts_close_to_bf16():
    cfg = get_model_config("mixtral-tiny")
    m = MixtralModel(cfg, device="cuda", tp_rank=0, tp_size=1).init_random(seed=2)
    ids = list(range(50, 170))
    ref = _logits(m, ids)
    m.fp8 = True
    m.quantize_experts()
    got = _logits(m, ids)
    assert (got.argmax(-1) == ref.argmax(-1)).float().mean() > 0.8


def test_mixtral_fp8_prefill_scaled_mm_path():
    """Prefill-size MoE chunks (T*k > 1024) run fp8 x fp8 hipBLASLt GEMMs (torch._scaled_mm) on the
    untiled quantized experts: equal to the fp32 reference with per-row fp8 activations, and to
    the decode fp8 MFMA pipeline run over the same rows in decode-size chunks."""
    from financial_chatbot_llm_amd.ops import moe
    cfg = get_model_config("mixtral-tiny")
    m = MixtralModel(cfg, device="cuda", tp_rank=0, tp_size=1, fp8=True).init_random(seed=5, std=0.05)
    assert m.prefill_fp8 and "layers.0.w13_q" in m.w and "layers.0.w13_deq" not in m.w
    g = torch.Generator().manual_seed(1)
    h = torch.randn(601, cfg.hidden_size, generator=g).to(torch.bfloat16).cuda()
    got = m.mlp(0, h)                                             # 1202 pairs -> prefill path
    p = "layers.0."
    ref = moe.moe_fp8_reference(h.float(), m.w[p + "router"], m.w[p + "w13_q"], m.w[p + "w13_scale"],
                                m.w[p + "w2_q"], m.w[p + "w2_scale"], cfg.top_k_experts, quant_act=True)
    scale = ref.float().abs().max().item()
    assert (got.float() - ref.float()).abs().max().item() < 0.05 * scale
    dec = torch.cat([m.mlp(0, h[i:i + 200]) for i in range(0, 601, 200)])   # decode pipeline chunks
    assert (got.float() - dec.float()).abs().max().item() < 0.05 * scale


def test_mixtral_fp8_mlp_just_above_the_decode_limit_takes_the_tiles(monkeypatch):
    """One token more than the decode pipeline takes (T = fp8_limit // K + 1): ``MixtralModel.mlp``
    must run ``moe_prefill_fp8_tiles``, and every token must agree with the same layer on the
    per-expert hipBLASLt loop (PENNY_MOE_PREFILL_TILES=0).

    Limit per token, ||tiles_t - loop_t|| / ||loop_t|| <= 2^-3: the two paths compute the same
    sums and differ in how the SiLU intermediate is rounded to e4m3 (MX blocks of 32 against one
    scale per row), each within 2^-4 of every element, so their intermediates differ by at most
    2^-3 in norm, and the random W2 carries that ratio to the output row.  A row through a wrong
    expert or with a term missing is off by 0.5 and more.  Tokens whose bf16 logits tie exactly at
    the K-th place are left out: ``torch.topk`` (the loop's routing) leaves that choice open."""
    import numpy as np
    from financial_chatbot_llm_amd.ops import moe
    from moe_ref import check_per_token, route_ref
    cfg = get_model_config("mixtral-tiny")
    m = MixtralModel(cfg, device="cuda", tp_rank=0, tp_size=1, fp8=True).init_random(seed=5, std=0.05)
    assert m.prefill_fp8 and "layers.0.w13_q" in m.w
    K = cfg.top_k_experts
    T = 1024 // K + 1
    g = torch.Generator().manual_seed(2)
    h = torch.randn(T, cfg.hidden_size, generator=g).to(torch.bfloat16).cuda()
    seen = []
    real = moe.moe_prefill_fp8_tiles
    monkeypatch.setattr(moe, "moe_prefill_fp8_tiles", lambda *a, **k: (seen.append(a[0].shape[0]), real(*a, **k))[1])
    assert moe.PREFILL_TILES
    got = m.mlp(0, h)
    assert seen == [T]
    monkeypatch.setattr(moe, "PREFILL_TILES", False)
    loop = m.mlp(0, h)
    assert seen == [T]
    from financial_chatbot_llm_amd.ops.gemm import linear
    lg = linear(h, m.w["layers.0.router"]).to(torch.bfloat16).float().cpu().numpy()      # as mlp() forms them
    srt = -np.sort(-lg, axis=1)
    tie = srt[:, K - 1] == srt[:, K]
    assert not route_ref(lg, K).poisoned.any() and tie.mean() < 0.02, tie.sum()
    ratio = check_per_token(got.cpu()[~tie], loop.cpu()[~tie], 2.0 ** -3, "tiles vs expert loop")
    print("MOEFIG mixtral-mlp-tiles-vs-loop", f"per_token_max={ratio:.4g} ties={int(tie.sum())}", flush=True)


def test_bge_encoder_gpu_matches_cpu():
    from financial_chatbot_llm_amd.models.bert import BertEncoder
    cfg = get_model_config("bert-tiny")
    g = BertEncoder.build(cfg, device="cuda", seed=3)
    c = BertEncoder(cfg, device="cpu")
    c.w = {k: v.cpu() for k, v in g.w.items()}
    seqs = [[101, 2000, 3000, 102], [101] + list(range(1000, 1150)) + [102]]
    a, b = g.encode(seqs).cpu(), c.encode(seqs)
    assert torch.allclose(a, b, atol=3e-2), (a - b).abs().max()


def test_gemm_tuning_table_loads_and_matches_default():
    """The curated TunableOp table must pass the runtime's validators (else it is silently
    ignored) and its solutions must compute the same GEMM."""
    from financial_chatbot_llm_amd.ops.gemm import load_gemm_tuning
    x = torch.randn(128, 14336, device="cuda").to(torch.bfloat16)
    w = torch.randn(4096, 14336, device="cuda").to(torch.bfloat16)
    ref = torch.nn.functional.linear(x, w).float()
    assert load_gemm_tuning("llama3-8b") is not None
    assert len(torch.cuda.tunable.get_results()) > 0
    got = torch.nn.functional.linear(x, w).float()
    assert (got - ref).abs().max() <= 1e-2 * ref.abs().max()


def test_splitk_decode_path_matches(monkeypatch):
    """Forcing the split-K slab path on every decode-size projection (llama-tiny shapes are not in
    the tuned table) keeps the forward equal to the fp32 CPU reference and greedy decoding equal
    to the hipBLASLt path."""
    from financial_chatbot_llm_amd.ops import gemm
    cfg = get_model_config("llama-tiny")
    gpu = LlamaModel(cfg, device="cuda", tp_rank=0, tp_size=1).init_random(seed=4)
    cpu = LlamaModel(cfg, device="cpu", tp_rank=0, tp_size=1)
    cpu.w = {k: v.cpu() for k, v in gpu.w.items()}
    ids = list(range(7, 7 + 150))
    monkeypatch.setenv("PENNY_SPLITK", "force")
    gpu.prepare_decode_weights()      # tiny shapes get tiled copies only when the path is forced
    assert gpu.wt and gemm.splitk_config(150, 1536, 256) is not None
    a, b = _logits(gpu, ids), _logits(cpu, ids)
    assert (a - b).abs().mean().item() < 0.01 * b.abs().max().item() + 0.01
    assert (a.argmax(-1) == b.argmax(-1)).float().mean() > 0.85
    base = dict(model="llama-tiny", device="cuda", num_kv_blocks=128, max_model_len=2048, max_num_seqs=16,
                graph_batch_sizes=(1, 2, 4, 8, 16))
    prompts = [list(range(100 + 7 * i, 100 + 7 * i + 30 + 17 * i)) for i in range(5)]
    sp = SamplingParams(temperature=0.0, max_tokens=10, ignore_eos=True)
    forced = LLMEngine(EngineConfig(**base), model=gpu)
    forced.warmup()
    got = forced.generate(prompts, sp)
    monkeypatch.setenv("PENNY_SPLITK", "0")
    plain = LLMEngine(EngineConfig(use_cuda_graph=False, **base), model=gpu)
    want = plain.generate(prompts, sp)
    agree = sum(x == y for g_, w_ in zip(got, want) for x, y in zip(g_, w_)) / 50
    assert agree >= 0.9, (got, want)


@pytest.mark.timeout(240)
def test_llama3_8b_engine_end_to_end():
    """The real Llama-3-8B shapes through the whole engine on the GPU: chunked prefill with a
    prefix-cache hit, hipGraph decode on the tuned split-K / skinny kernels, a jump-forward
    decide call and a streamed respond -- the path the benchmark runs, at 8B scale."""
    from financial_chatbot_llm_amd.agent.grammar import ToolCallGrammar, jump_mask
    from financial_chatbot_llm_amd.agent.toolcall import format_tool_call
    from financial_chatbot_llm_amd.tools import ToolCall, make_retrieval_tool
    cfg = EngineConfig(model="llama3-8b", device="cuda", num_kv_blocks=512, max_model_len=8192, max_num_seqs=16,
                       max_num_batched_tokens=2048, graph_batch_sizes=(1, 2, 4, 8, 16))
    eng = LLMEngine(cfg)
    eng.warmup()
    tok = eng.tokenizer
    shared = list(range(1000, 1000 + 1500))
    prompts = [shared + list(range(5000 + 100 * i, 5000 + 100 * i + 300 + 50 * i)) for i in range(4)]
    outs = eng.generate(prompts, SamplingParams(temperature=0.5, max_tokens=12, ignore_eos=True, seed=3))
    assert all(len(o) == 12 for o in outs)
    assert eng.bm.hit_rate() > 0.3                                   # the shared 1.5k prefix was reused
    assert eng.runner.stats["graph_steps"] > 0
    eot = tok.special["<|eot_id|>"]
    call = format_tool_call(ToolCall("retrieve_transactions", {"search_query": "groceries", "num_transactions": 20}))
    forced = tok.encode(call, allow_special=False) + [eot]
    g = ToolCallGrammar([make_retrieval_tool(None)])
    steps0 = eng.runner.stats["steps"]
    out = eng.generate([shared + [7, 8, 9]], SamplingParams(temperature=0.5, max_tokens=96, forced_output=forced,
                                                           forced_jump=jump_mask(forced, tok.decode, g, eot), grammar=g))
    assert out[0] == forced
    assert eng.runner.stats["steps"] - steps0 < len(forced) - 10     # grammar-forced runs were chunked


def test_staged_step_inputs_match_arrays_and_plain_upload(monkeypatch):
    """Eager steps upload every StepInputs array with ONE pinned H2D copy (typed views of one
    device byte buffer); the views equal the host arrays, and an engine run with staging off
    produces the same greedy tokens."""
    import numpy as np
    from financial_chatbot_llm_amd.engine.model_runner import StepInputs
    base = dict(model="llama-tiny", device="cuda", num_kv_blocks=128, max_model_len=2048, max_num_seqs=8,
                use_cuda_graph=False)
    prompts = [list(range(50 + 5 * i, 50 + 5 * i + 40 + 13 * i)) for i in range(4)]
    sp = SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True)
    e1 = LLMEngine(EngineConfig(**base))
    staged = e1.generate(prompts, sp)
    runner = e1.runner
    i32 = lambda x: np.asarray(x, np.int32)  # noqa: E731
    si = StepInputs(i32([5, 6, 7]), i32([0, 1, 2]), i32([64, 65, 66]), i32([0, 3]), i32([3]),
                    i32([[1, 2, 3]]), 3, i32([]), np.zeros((0, 3), np.int32), np.asarray([2], np.int64),
                    np.asarray([0.5], np.float32), np.asarray([12345678901], np.int64), i32([0]),
                    np.asarray([1.0], np.float32), None)
    runner._stage_inputs(si)
    for name in ("ids", "positions", "slots", "cu_q", "ctx_p", "bt_p", "ctx_d", "bt_d", "logits_idx", "temps",
                 "seeds", "top_k", "top_p"):
        a = getattr(si, name)
        t = runner._to_dev(a)
        assert t.is_cuda and tuple(t.shape) == a.shape and t.dtype == torch.from_numpy(a).dtype, name
        assert np.array_equal(t.cpu().numpy(), a), name
    runner._staged = None
    monkeypatch.setenv("PENNY_STAGE_INPUTS", "0")
    e2 = LLMEngine(EngineConfig(**base), model=e1.model)
    assert not e2.runner._stage_enabled
    assert e2.generate(prompts, sp) == staged
