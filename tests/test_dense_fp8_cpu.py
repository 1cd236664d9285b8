"""fp8 dense Llama MLP on the CPU: the weight quantiser, the torch path of ``ops.mlp_fp8`` against the
self-quantising reference, the kernel config table against the kernel's contract, the configuration
switch, the exact test cases against a plain torch model of the kernel, and TP = 2 over gloo."""
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

import dense_fp8_ref as D
from mp_util import to_np, to_torch

from financial_chatbot_llm_amd import ops
from financial_chatbot_llm_amd.config import EngineConfig
from financial_chatbot_llm_amd.models import build_model
from financial_chatbot_llm_amd.models.configs import get_model_config
from financial_chatbot_llm_amd.ops import fp8_dense
from financial_chatbot_llm_amd.ops.gemm import interleave16


def _weights(H=256, F_=512, seed=0, std=0.05):
    g = torch.Generator().manual_seed(seed)
    gate, up = (torch.randn(F_, H, generator=g) * std).bfloat16(), (torch.randn(F_, H, generator=g) * std).bfloat16()
    down = (torch.randn(H, F_, generator=g) * std).bfloat16()
    return gate, up, down


# ------------------------------------------------------------------------------------------------
# quantiser
# ------------------------------------------------------------------------------------------------
def test_quantiser_round_trip_within_half_an_ulp_and_keeps_the_interleave():
    """codes * scale is within half an e4m3 ulp of every weight, in units of the row's scale: with
    t = w / scale (|t| <= 448) the e4m3 spacing at t is 2^(floor(log2 |t|) - 3), 2^-9 below 2^-6, and the
    code is the nearest value of the f32 quotient, itself within 2^-24 |t| of t.  The row with the
    largest magnitude maps to +-448 exactly.  Row-wise quantisation commutes with the 16-row gate|up
    interleave."""
    gate, up, down = _weights()
    gate[3] = 0.0                                     # an all-zero row: scale floor, codes 0
    gu = interleave16(gate, up).contiguous()
    w = ops.quantize_dense_mlp(gu, down)
    assert w.gate_up_q.dtype == torch.float8_e4m3fn and w.gate_up_s.dtype == torch.float32
    assert w.gate_up_q.shape == gu.shape and w.down_q.shape == down.shape
    assert w.gate_up_s.shape == (gu.shape[0],) and w.down_s.shape == (down.shape[0],)
    assert w.num_bytes() == gu.numel() + down.numel() + 4 * (gu.shape[0] + down.shape[0])
    for src, q, s in ((gu, w.gate_up_q, w.gate_up_s), (down, w.down_q, w.down_s)):
        t = src.double() / s.double()[:, None]
        ulp = torch.exp2(torch.floor(torch.log2(t.abs().clamp_min(2.0 ** -6))) - 3)
        err = (q.float().double() - t).abs()
        assert bool((err <= 0.5 * ulp + 2.0 ** -23 * t.abs()).all()), float((err / ulp).max())
        live = src.float().abs().amax(1) > 0
        assert bool((q.float().abs().amax(1)[live] == 448.0).all())
    gq, gs = ops.moe.quantize_fp8_rowwise(gate)
    uq, us = ops.moe.quantize_fp8_rowwise(up)
    assert torch.equal(w.gate_up_q.view(torch.uint8), interleave16(gq.view(torch.uint8), uq.view(torch.uint8)))
    assert torch.equal(w.gate_up_s, interleave16(gs[:, None], us[:, None])[:, 0])
    with pytest.raises(ValueError):
        ops.quantize_dense_mlp(gu, down.t().contiguous())


# ------------------------------------------------------------------------------------------------
# torch path
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 17, 300])
def test_torch_path_equals_the_reference(M):
    """The CPU path of ``mlp_fp8`` is the operation order of ``dense_fp8_reference(quant_act=True)``
    (``moe_fp8_reference`` with one expert and weight 1): equal bit for bit, the intermediate included;
    without the activation rounding the reference moves, by less than the e4m3 step allows."""
    gate, up, down = _weights(seed=1)
    w = ops.quantize_dense_mlp(interleave16(gate, up).contiguous(), down)
    h = torch.randn(M, 256, generator=torch.Generator().manual_seed(M)).bfloat16()
    assert fp8_dense.mlp_fp8_path(h, w) == "torch"
    y, a = ops.mlp_fp8(h, w, slabs=True)
    ref = ops.dense_fp8_reference(h, w, quant_act=True)
    assert y.dtype == torch.bfloat16 and y.shape == (M, 256) and a.shape == (M, 512) and a.dtype == torch.bfloat16
    assert torch.equal(y, ref)
    x = ops.moe._fake_quant_rows(h.float())
    w13 = w.gate_up_q.float() * w.gate_up_s[:, None]
    assert torch.equal(a, ops.silu_mul((x @ w13.t()).to(torch.bfloat16), interleave16=True))
    plain = ops.dense_fp8_reference(h, w, quant_act=False)
    rel = (plain.float() - ref.float()).norm(dim=1) / ref.float().norm(dim=1)
    assert 0 < float(rel.max()) < 0.25, float(rel.max())


# ------------------------------------------------------------------------------------------------
# config table
# ------------------------------------------------------------------------------------------------
PRODUCTION = [(28672, 4096), (4096, 14336), (57344, 8192), (8192, 28672), (7168, 8192), (8192, 3584)]


def test_every_table_entry_satisfies_the_kernel_contract():
    """DENSE_FP8 covers the 8B, 70B and 70B TP=8 MLP shapes; every entry, at every M it is chosen for and
    for every epilogue, is inside ``penny_dense_fp8_gemm``'s checked contract: ntf in {2, 4}, N a multiple
    of 16 ntf, K a multiple of 128 S, 1 <= S <= 16, S = 1 unless the output is slabs; rows are ordered by
    max M and end at 256."""
    for shape in PRODUCTION:
        assert shape in fp8_dense.DENSE_FP8, shape
    for (N, K), rows in fp8_dense.DENSE_FP8.items():
        assert [r[0] for r in rows] == sorted(r[0] for r in rows) and rows[-1][0] == fp8_dense.MAX_M, (N, K)
        for M in range(1, 257):
            want = next((S, ntf) for max_m, S, ntf in rows if M <= max_m)
            for epi in ("silu", "bf16", "slabs"):
                S, ntf = fp8_dense.dense_fp8_config(M, N, K, epi)
                assert ntf == want[1] and S == (want[0] if epi == "slabs" else 1), (M, N, K, epi)
                assert ntf in (2, 4) and N % (16 * ntf) == 0 and K % (128 * S) == 0 and 1 <= S <= fp8_dense.MAX_S
    # outside the contract: no config (mlp_fp8 then takes the tile kernel or the torch path)
    assert fp8_dense.dense_fp8_config(257, 4096, 14336, "slabs") is None
    assert fp8_dense.dense_fp8_config(0, 4096, 14336, "slabs") is None
    assert fp8_dense.dense_fp8_config(16, 4096, 14336 + 64, "slabs") is None
    assert fp8_dense.dense_fp8_config(16, 4096 + 16, 14336, "slabs") is None
    # unmeasured shapes (llama-tiny's): the default fills the CUs with K slices the kernel accepts
    for N, K in ((1024, 256), (256, 512), (32, 128)):
        S, ntf = fp8_dense.dense_fp8_config(64, N, K, "slabs")
        assert ntf == 2 and K % (128 * S) == 0 and fp8_dense.dense_fp8_config(64, N, K, "silu") == (1, 2)


def test_table_entries_name_a_profile_that_has_their_shape():
    """Every table shape was measured: profiles/dense_fp8_mlp.jsonl holds rows for it."""
    import json
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dense_fp8_mlp.jsonl")
    seen = set()
    with open(path) as fh:
        for line in fh:
            row = json.loads(line)
            for key in ("gate_up", "down"):
                if key in row:
                    seen.add(tuple(row[key]["shape"]))
    for shape in fp8_dense.DENSE_FP8:
        assert shape in seen, f"{shape} has a table entry and no row in {path}"


# ------------------------------------------------------------------------------------------------
# configuration
# ------------------------------------------------------------------------------------------------
def test_config_env_flag_and_bad_values(monkeypatch):
    monkeypatch.delenv("PENNY_MLP_DTYPE", raising=False)
    assert EngineConfig().mlp_dtype == "bf16" and EngineConfig.from_env().mlp_dtype == "bf16"
    monkeypatch.setenv("PENNY_MLP_DTYPE", "fp8")
    assert EngineConfig().mlp_dtype == "fp8" and EngineConfig.from_env().mlp_dtype == "fp8"
    assert EngineConfig.from_env(mlp_dtype="bf16").mlp_dtype == "bf16"
    monkeypatch.setenv("PENNY_MLP_DTYPE", "int4")
    with pytest.raises(ValueError, match="mlp_dtype"):
        EngineConfig()
    monkeypatch.delenv("PENNY_MLP_DTYPE")
    with pytest.raises(ValueError, match="mlp_dtype"):
        EngineConfig(mlp_dtype="fp4")
    from financial_chatbot_llm_amd.serving import launch
    assert launch.parse([]).mlp_dtype == "bf16"
    assert launch.parse(["--mlp-dtype", "fp8"]).mlp_dtype == "fp8"
    monkeypatch.setenv("PENNY_MLP_DTYPE", "fp8")
    assert launch.parse([]).mlp_dtype == "fp8"


def test_build_model_quantises_llama_and_refuses_mixtral():
    m = build_model(EngineConfig(model="llama-tiny", device="cpu", mlp_dtype="fp8"), torch.device("cpu"))
    ref = build_model(EngineConfig(model="llama-tiny", device="cpu"), torch.device("cpu"))
    c = m.cfg
    assert m.mlp_dtype == "fp8" and ref.mlp_dtype == "bf16" and not ref.mlp_q
    assert not any(k.endswith((".gate_up", ".down")) for k in m.w) and not any(k.endswith((".gate_up", ".down")) for k in m.wt)
    per_layer = 3 * c.hidden_size * c.intermediate_size
    saved = c.num_layers * (per_layer * 2 - per_layer - 4 * (2 * c.intermediate_size + c.hidden_size))
    assert ref.num_bytes() - m.num_bytes() == saved
    w0 = ops.quantize_dense_mlp(ref.w["layers.0.gate_up"], ref.w["layers.0.down"])
    assert torch.equal(m.mlp_q[0].gate_up_q.view(torch.uint8), w0.gate_up_q.view(torch.uint8))
    assert m.w["layers.0.down_q"] is m.mlp_q[0].down_q
    with pytest.raises(ValueError, match="dtype='fp8'"):
        build_model(EngineConfig(model="mixtral-tiny", device="cpu", mlp_dtype="fp8"), torch.device("cpu"))
    from financial_chatbot_llm_amd.models.mixtral import MixtralModel
    with pytest.raises(ValueError, match="dtype='fp8'"):
        MixtralModel(get_model_config("mixtral-tiny"), device="cpu", tp_rank=0, tp_size=1).init_random(seed=0).quantize_mlp()


def test_engine_reports_mlp_dtype_and_switch_off_is_the_old_path():
    from financial_chatbot_llm_amd.engine import LLMEngine, SamplingParams
    base = dict(model="llama-tiny", device="cpu", num_kv_blocks=32, max_model_len=512, use_cuda_graph=False)
    sp = SamplingParams(temperature=0.0, max_tokens=4, ignore_eos=True)
    off = LLMEngine(EngineConfig(**base))
    assert off.stats()["mlp_dtype"] == "bf16" and "layers.0.gate_up" in off.model.w and not off.model.mlp_q
    called = []
    real = ops.mlp_fp8
    try:
        ops.mlp_fp8 = lambda *a, **k: (called.append(1), real(*a, **k))[1]
        out_off = off.generate([list(range(5, 40))], sp)
        assert not called
        on = LLMEngine(EngineConfig(mlp_dtype="fp8", **base))
        assert on.stats()["mlp_dtype"] == "fp8"
        out_on = on.generate([list(range(5, 40))], sp)
        assert called and len(out_on[0]) == len(out_off[0]) == 4
    finally:
        ops.mlp_fp8 = real


# ------------------------------------------------------------------------------------------------
# the exact cases against a plain model of the kernel
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,S", [(32, 128, 1), (64, 256, 2), (64, 512, 4)])
def test_exact_cases_agree_with_a_plain_torch_model(N, K, S):
    """The expectations the GPU tests compare bits with (computed from the non-zero columns alone) equal
    an f64 matmul model of the contract, for both kinds of exact case and all three epilogues; the
    one-hot calls cover every required column."""
    M = 17
    cols = D.required_columns(K, S)
    assert set(range(128)) <= set(cols) and set(range(K - 128, K)) <= set(cols)
    for s in range(1, S):
        assert {s * K // S - 1, s * K // S} <= set(cols)
    ncalls = -(-len(cols) // M)
    padded = torch.tensor((cols * 2)[:ncalls * M]).view(ncalls, M)
    cases = [D.onehot_case(M, N, K, padded[c], seed=c) for c in range(0, ncalls, 5)]
    cases += [D.few_term_case(M, N, K, S, seed=3), D.few_term_case(M, N, K, S, seed=4, silu=True)]
    for case in cases:
        nnz = (D.values_of(case.xq[:M, :K].contiguous()) != 0).sum(1)
        assert int(nnz.max()) <= 4 and int(nnz.min()) >= 1
        assert bool((case.xq[M:] == D.NAN_CODE).all()) and bool(torch.isnan(case.xs[M:]).all())
        for epi in ("silu", "bf16", "slabs"):
            s_ = S if epi == "slabs" else 1
            want, model = D.expected(case, epi, s_, ops.silu_mul), D.emulate(case, epi, s_, ops.silu_mul)
            assert torch.equal(D.bits(want), D.bits(model)), (epi, N, K)
            ref = D.reference_f64(case, epi, s_)
            assert bool(((want.double() - ref.ref).abs() <= ref.bound).all()), (epi, N, K)
    few = cases[-2]
    slabs = D.expected(few, "slabs", S, ops.silu_mul)
    assert int((slabs != 0).any(-1).any(-1).sum()) == S          # every K slice holds terms


def test_sentinel_buffers_detect_a_stray_write():
    for epi, S in (("silu", 1), ("bf16", 1), ("slabs", 2)):
        buf = D.out_buffer(5, 64, epi, S, "cpu")
        assert D.untouched(buf) and D.result(buf).shape[-1] == buf.width
        D.result(buf).fill_(1.0)
        assert D.untouched(buf)
        buf.view[..., buf.width] = 1.0
        assert not D.untouched(buf)
        buf = D.out_buffer(5, 64, epi, S, "cpu")
        buf.flat[-1] = 0.0
        assert not D.untouched(buf)


# ------------------------------------------------------------------------------------------------
# TP over gloo
# ------------------------------------------------------------------------------------------------
def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


IDS = list(range(3, 140))


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    try:
        from financial_chatbot_llm_amd.models.llama import LlamaModel
        from financial_chatbot_llm_amd.parallel.dist import init_distributed, shutdown
        from test_model_parity import _prefill_logits
        init_distributed(tp_size=world, backend="gloo", device_type="cpu")
        cfg = get_model_config("llama-tiny-tp")
        tp = LlamaModel(cfg, device="cpu", dtype=torch.float32).init_random(seed=7).quantize_mlp()
        assert tp.mlp_q[0].down_q.shape == (cfg.hidden_size, cfg.intermediate_size // world)
        q.put((rank, to_np(_prefill_logits(tp, IDS)), None))
        shutdown()
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, "ERR", traceback.format_exc()))


@pytest.mark.timeout(300)
def test_tp2_fp8_logits_close_to_tp1():
    """Each rank quantises its own shard, and down's activation scale is per shard: TP = 2 is close to
    TP = 1, not bit-equal.  The model is build_model's random init (default std).  Criterion: the fp8 Mixtral layer's, max error < 0.05 x max |reference|
    (tests/test_engine_gpu.py, test_mixtral_fp8_prefill_scaled_mm_path)."""
    from financial_chatbot_llm_amd.models.llama import LlamaModel
    from test_model_parity import _prefill_logits
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    for _ in range(world):
        r, a, b = q.get(timeout=240)
        assert not (isinstance(a, str) and a == "ERR"), b
        res[r] = to_torch(a)
    for p in procs:
        p.join(timeout=60)
    cfg = get_model_config("llama-tiny-tp")
    one = LlamaModel(cfg, device="cpu", tp_rank=0, tp_size=1, dtype=torch.float32).init_random(seed=7)
    bf16 = _prefill_logits(one, IDS)
    ref = _prefill_logits(one.quantize_mlp(), IDS)
    scale = ref.abs().max().item()
    for r in range(world):
        err = (res[r] - ref).abs().max().item()
        print(f"rank {r}: max |tp2 - tp1| = {err:.4e}, 0.05 x max |ref| = {0.05 * scale:.4e}")
        assert err < 0.05 * scale
    assert torch.equal(res[0], res[1])
    # the quantisation itself is visible in the logits (the two runs above did take the fp8 path)
    q_err = (ref - bf16).abs().max().item()
    print(f"max |fp8 - bf16| = {q_err:.4e} of max |bf16| = {bf16.abs().max().item():.4e}")
    assert q_err > 0
