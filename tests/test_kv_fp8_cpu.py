"""fp8 (e4m3) paged KV cache, CPU side: the layout mirror, the reference quantiser, the reference ops
on an fp8 cache, the engine on ``kv_dtype="fp8"`` and the scale calibration."""
import dataclasses

import pytest
import torch

import kv_fp8_ref as R
from financial_chatbot_llm_amd import ops
from financial_chatbot_llm_amd.config import EngineConfig
from financial_chatbot_llm_amd.engine import LLMEngine, SamplingParams, calibrate_kv_scales, save_kv_scales
from financial_chatbot_llm_amd.engine.llm_engine import plan_kv_blocks
from financial_chatbot_llm_amd.models.common import KVCache
from financial_chatbot_llm_amd.models.configs import get_model_config
from financial_chatbot_llm_amd.models.llama import LlamaModel
from financial_chatbot_llm_amd.ops import attention as A

D, HKV, KV_BS = R.D, R.HKV, R.KV_BS


# ---------------------------------------------------------------------------------------------
# layout
# ---------------------------------------------------------------------------------------------
def test_layout_bijection_and_formula():
    for index8, index16 in ((A.k_index8, A.k_index), (A.v_index8, A.v_index)):
        seen = set()
        for key in range(KV_BS):
            for d in range(D):
                e = index16(key, d, D)                      # bf16 layout: ((f * 64 + lane) << 3) + j
                f, lane, j = e >> 9, (e >> 3) & 63, e & 7
                want = ((f >> 1) * 64 + lane) * 16 + (f & 1) * 8 + j
                assert index8(key, d, D) == want
                seen.add(want)
        assert seen == set(range(KV_BS * D))
    ki, vi = A.kv_index_tables8(D)
    assert ki[17, 40] == A.k_index8(17, 40, D) and vi[63, 127] == A.v_index8(63, 127, D)


# ---------------------------------------------------------------------------------------------
# quantiser
# ---------------------------------------------------------------------------------------------
def _q(vals, inv=None):
    x = torch.tensor(vals, dtype=torch.float32).view(-1, 1, 1)
    return A.quantize_kv_ref(x, None if inv is None else torch.tensor([inv])).view(-1)


def test_quantiser_pins():
    # ties to even: e4m3 has steps of 2 in [16, 32) and of 4 in [32, 64)... 17 is halfway 16 | 18, 19 halfway 18 | 20
    assert _q([17.0, 19.0, -17.0, -19.0]).float().tolist() == [16.0, 20.0, -16.0, -20.0]
    assert _q([34.0, 38.0]).float().tolist() == [32.0, 40.0]
    # subnormals: multiples of 2^-9 below 2^-6, ties to even there too
    s = 2.0 ** -9
    got = _q([s, 3 * s, 7 * s, 0.5 * s, 1.5 * s, 2.5 * s, 0.49 * s, -2.5 * s]).float().tolist()
    assert got == [s, 3 * s, 7 * s, 0.0, 2 * s, 2 * s, 0.0, -2 * s]
    # saturation, not NaN
    c = _q([448.0, 449.0, 1000.0, float("inf"), -1000.0, float("-inf"), 464.0, 480.0])
    assert c.float().tolist() == [448.0, 448.0, 448.0, 448.0, -448.0, -448.0, 448.0, 448.0]
    assert c.view(torch.uint8).tolist() == [0x7E, 0x7E, 0x7E, 0x7E, 0xFE, 0xFE, 0x7E, 0x7E]
    # NaN stays a NaN code
    n = _q([float("nan")]).view(torch.uint8)
    assert bool(R.is_nan_code(n).all())
    # per-head scale: x * inv, in f32
    x = torch.tensor([[[17.0], [17.0]], [[1000.0], [1000.0]]])             # [T=2, Hkv=2, D=1]
    sc = A.make_kv_scales([0.5, 3.0], [1.0, 1.0])
    q = A.quantize_kv_ref(x, sc.inv[0]).float()
    assert q[:, 0, 0].tolist() == [32.0, 448.0]                            # 34 -> 32 (tie to even), 2000 -> 448
    assert q[0, 1, 0].item() == (17.0 * (1.0 / torch.tensor(3.0))).to(A.FP8).float().item()
    assert q[1, 1, 0].item() == 320.0                                      # 333.3 -> 320 (steps of 32)
    assert torch.equal(sc.inv, 1.0 / sc.scale)
    with pytest.raises(ValueError):
        A.make_kv_scales([0.0, 1.0], [1.0, 1.0])


def test_write_gather_round_trip():
    g = torch.Generator().manual_seed(1)
    sc = R.scales(R.SCALED)
    T = 11
    k, v = torch.randn(T, HKV, D, generator=g) * 4, torch.randn(T, HKV, D, generator=g)
    slots = torch.arange(60, 60 + T, dtype=torch.int32)                    # crosses the block boundary at 64
    slots[4] = -1
    kc, vc = R.empty_cache(3), R.empty_cache(3)
    kc.view(torch.uint8)[2].fill_(0x38)                                    # 1.0 everywhere in an untouched block
    A.write_kv_ref(k, v, slots, kc, vc, sc)
    K, V = A.gather_kv_ref(kc, vc, torch.tensor([0, 1, 2]), 3 * KV_BS, sc)
    keep = slots >= 0
    kq = A.quantize_kv_ref(k, sc.inv[0]).float() * sc.scale[0][None, :, None]
    vq = A.quantize_kv_ref(v, sc.inv[1]).float() * sc.scale[1][None, :, None]
    assert torch.equal(K[slots[keep].long()], kq[keep]) and torch.equal(V[slots[keep].long()], vq[keep])
    untouched = torch.ones(3 * KV_BS, dtype=torch.bool)
    untouched[slots[keep].long()] = False
    assert bool((V[untouched] == 0).all()) and bool((K[:128][untouched[:128]] == 0).all())
    assert torch.equal(K[128:], torch.ones(KV_BS, HKV, D) * sc.scale[0][None, :, None])
    # block order follows the table
    K2, _ = A.gather_kv_ref(kc, vc, torch.tensor([1, 0]), 2 * KV_BS, sc)
    assert torch.equal(K2[:KV_BS], K[KV_BS:2 * KV_BS]) and torch.equal(K2[KV_BS:], K[:KV_BS])


def test_rope_kv_write_cpu_fp8():
    """K is rotated in f32 and quantised without a bf16 rounding in between; q is as for a bf16 cache."""
    g = torch.Generator().manual_seed(2)
    Hq, T = 8, 9
    qkv = torch.randn(T, (Hq + 2 * HKV) * D, generator=g).to(torch.bfloat16)
    pos = torch.arange(100, 100 + T, dtype=torch.int32)
    cs = ops.rope_cos_sin(D, 256, 500000.0)
    slots = torch.arange(60, 60 + T, dtype=torch.int32)
    sc = R.scales(R.SCALED)
    kc, vc = R.empty_cache(2), R.empty_cache(2)
    q = ops.rope_kv_write(qkv, pos, cs, slots, kc, vc, Hq, HKV, D, kv_scales=sc)
    kb, vb = torch.zeros(2, HKV, KV_BS * D, dtype=torch.bfloat16), torch.zeros(2, HKV, KV_BS * D, dtype=torch.bfloat16)
    q16 = ops.rope_kv_write(qkv, pos, cs, slots, kb, vb, Hq, HKV, D)
    assert torch.equal(q, q16)
    x = qkv.view(T, Hq + 2 * HKV, D)
    kf = A._rope_f32(x[:, Hq:Hq + HKV], pos, cs)
    K, V = A.gather_kv_ref(kc, vc, torch.tensor([0, 1]), 60 + T, sc)
    assert torch.equal(K[60:], A.quantize_kv_ref(kf, sc.inv[0]).float() * sc.scale[0][None, :, None])
    assert torch.equal(V[60:], A.quantize_kv_ref(x[:, Hq + HKV:], sc.inv[1]).float() * sc.scale[1][None, :, None])
    with pytest.raises(ValueError, match="head dim"):
        ops.rope_kv_write(torch.zeros(1, 3 * 64, dtype=torch.bfloat16), pos[:1], None, slots[:1],
                          torch.zeros(1, 1, 64 * 64, dtype=torch.uint8).view(A.FP8),
                          torch.zeros(1, 1, 64 * 64, dtype=torch.uint8).view(A.FP8), 1, 1, 64, False)


# ---------------------------------------------------------------------------------------------
# reference consistency
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", [R.UNIT, R.SCALED], ids=["unit", "scaled"])
def test_reference_ops_match_dequantised_bf16_cache(setting):
    g = torch.Generator().manual_seed(3)
    sc = R.scales(setting)
    ctxs = [1, 65, 200]
    tables, nb = R.tables_for(ctxs, g)
    kc, vc = R.random_cache(nb, sc, g)
    kb = ops.kv_dequant(kc, sc.scale[0] if sc else None)
    vb = ops.kv_dequant(vc, sc.scale[1] if sc else None)
    K8, V8 = A.gather_kv_ref(kc, vc, tables[2], 200, sc)
    K16, V16 = A.gather_kv_ref(kb, vb, tables[2], 200)
    assert torch.equal(K8, K16.float()) and torch.equal(V8, V16.float())      # these scales keep bf16 exact
    Hq = 8
    q = torch.randn(3, Hq, D, generator=g).to(torch.bfloat16)
    ctx = torch.tensor(ctxs, dtype=torch.int32)
    marked = tables.clone()
    marked[1, 0] = -marked[1, 0] - 1
    a = ops.decode(q, ctx, marked, kc, vc, 0.088, kv_scales=sc)
    b = ops.decode(q, ctx, tables, kb, vb, 0.088)
    assert (a.float() - b.float()).abs().max().item() <= 1e-6
    qlens = [1, 30, 70]
    T = sum(qlens)
    qp = torch.randn(T, Hq, D, generator=g).to(torch.bfloat16)
    cu = torch.tensor([0, 1, 31, 101], dtype=torch.int32)
    l8, l16 = torch.empty(T, Hq), torch.empty(T, Hq)
    a = ops.prefill(qp, cu, ctx, tables, kc, vc, 0.088, True, lse=l8, kv_scales=sc)
    b = ops.prefill(qp, cu, ctx, tables, kb, vb, 0.088, True, lse=l16)
    assert (a.float() - b.float()).abs().max().item() <= 1e-6
    assert (l8 - l16).abs().max().item() <= 1e-6
    with pytest.raises(ValueError, match="causal"):
        ops.prefill(qp, cu, ctx, tables, kc, vc, 0.088, causal=False, kv_scales=sc)


# ---------------------------------------------------------------------------------------------
# engine
# ---------------------------------------------------------------------------------------------
BASE = dict(model="llama-tiny", device="cpu", num_kv_blocks=32, max_model_len=512, max_num_seqs=4)


@pytest.fixture(scope="module")
def tiny_model():
    return LlamaModel(get_model_config("llama-tiny"), device="cpu", tp_rank=0, tp_size=1).init_random(seed=0)


def test_engine_fp8_kv_cpu(tiny_model, monkeypatch):
    monkeypatch.delenv("PENNY_KV_DTYPE", raising=False)
    sp = SamplingParams(temperature=0.0, max_tokens=4, ignore_eos=True)
    eng = LLMEngine(EngineConfig(kv_dtype="fp8", **BASE), model=tiny_model)
    assert eng.kv.buf.dtype == torch.float8_e4m3fn and eng.kv.elt == 1 and eng.stats()["kv_dtype"] == "fp8"
    shared = list(range(5, 5 + 130))
    first = eng.generate([shared + [7, 8, 9]], sp)[0]
    assert len(first) == 4
    h0 = eng.bm.hit_rate()
    hit = eng.generate([shared + [11, 12]], sp)[0]
    assert eng.bm.hit_rate() > h0                                             # two shared blocks reused
    cold = LLMEngine(EngineConfig(kv_dtype="fp8", enable_prefix_caching=False, **BASE), model=tiny_model)
    assert hit == cold.generate([shared + [11, 12]], sp)[0]
    # a default config still builds a bf16 pool
    dflt = LLMEngine(EngineConfig(**BASE), model=tiny_model)
    assert EngineConfig().kv_dtype == "bf16" and dflt.kv.buf.dtype == torch.bfloat16 and dflt.kv.scales(0) is None
    assert dflt.stats()["kv_dtype"] == "bf16"
    monkeypatch.setenv("PENNY_KV_DTYPE", "fp8")
    assert EngineConfig().kv_dtype == "fp8"                                   # read when constructed


def test_plan_kv_blocks_and_refusals(tiny_model, monkeypatch):
    monkeypatch.delenv("PENNY_KV_DTYPE", raising=False)
    base = {k: v for k, v in BASE.items() if k != "num_kv_blocks"}
    dev = torch.device("cpu")
    c16, c8 = EngineConfig(**base), EngineConfig(kv_dtype="fp8", **base)
    assert plan_kv_blocks(c16, tiny_model, dev) == plan_kv_blocks(c8, tiny_model, dev)      # CPU: a token count

    # the GPU branch sizes the pool from free memory: same bytes, twice the blocks
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda d: (40 << 30, 64 << 30))
    cuda = torch.device("cuda", 0)
    n16, n8 = plan_kv_blocks(c16, tiny_model, cuda), plan_kv_blocks(c8, tiny_model, cuda)
    assert n16 > 1000 and n8 in (2 * n16, 2 * n16 + 1)
    L, H = tiny_model.cfg.num_layers, tiny_model.hkv
    assert KVCache.bytes_per_block(L, H, D, elt=1) * 2 == KVCache.bytes_per_block(L, H, D)
    for bad in (dict(tp_size=2), dict(cp_size=2), dict(shard_of_tp=8)):
        with pytest.raises(NotImplementedError, match="fp8 KV"):
            LLMEngine(EngineConfig(kv_dtype="fp8", **{**BASE, **bad}), model=tiny_model)
    with pytest.raises(ValueError, match="kv_dtype"):
        LLMEngine(EngineConfig(kv_dtype="int4", **BASE), model=tiny_model)
    with pytest.raises(ValueError, match="head dim"):
        KVCache(1, 2, 1, 64, device="cpu", kv_dtype="fp8")
    d64 = dataclasses.replace(tiny_model.cfg)
    fake = type("M", (), {"cfg": d64, "hkv": 2, "D": 64, "tp_size": 1})()
    from financial_chatbot_llm_amd.engine.llm_engine import check_kv_dtype
    with pytest.raises(ValueError, match="head dim"):
        check_kv_dtype(EngineConfig(kv_dtype="fp8", **BASE), fake)


# ---------------------------------------------------------------------------------------------
# calibration
# ---------------------------------------------------------------------------------------------
def test_calibration(tiny_model, tmp_path):
    prompts = [list(range(10, 90)), list(range(200, 270))]
    margin = 2.0
    ks, vs = calibrate_kv_scales(tiny_model, prompts, margin=margin)
    L, H = tiny_model.cfg.num_layers, tiny_model.hkv
    assert ks.shape == (L, H) and vs.shape == (L, H) and ks.dtype == torch.float32
    assert bool((ks > 0).all()) and bool((vs > 0).all())
    # the same absmax, measured independently through an fp8-free prefill of the first prompt
    kv = KVCache(L, 3, H, D, dtype=tiny_model.dtype, device="cpu")
    ids = prompts[0]
    R.logits_into(tiny_model, ids, kv)
    for layer in range(L):
        k, v = A.gather_kv_ref(kv.k(layer), kv.v(layer), torch.tensor([1, 2]), len(ids))
        assert bool((k.float().abs().amax(dim=(0, 2)) / ks[layer] <= 448 / margin * (1 + 1e-6)).all())
        assert bool((v.float().abs().amax(dim=(0, 2)) / vs[layer] <= 448 / margin * (1 + 1e-6)).all())
    path = str(tmp_path / "kv_scales.safetensors")
    save_kv_scales(path, ks, vs)
    eng = LLMEngine(EngineConfig(kv_dtype="fp8", kv_scales=path, **BASE), model=tiny_model)
    assert torch.equal(eng.kv.scale[:, 0], ks) and torch.equal(eng.kv.scale[:, 1], vs)
    assert torch.equal(eng.kv.scales(1).inv, 1.0 / eng.kv.scale[1])
    out = eng.generate([prompts[0]], SamplingParams(temperature=0.0, max_tokens=3, ignore_eos=True))[0]
    ref = LLMEngine(EngineConfig(**BASE), model=tiny_model).generate(
        [prompts[0]], SamplingParams(temperature=0.0, max_tokens=3, ignore_eos=True))[0]
    assert len(out) == 3
    print(f"calibrated fp8 KV vs bf16 KV greedy tokens: {out} vs {ref}")
    zero = torch.zeros_like(ks)
    zs, _ = calibrate_kv_scales(tiny_model, [], margin=margin)
    assert bool((zs > 0).all()) and zero.shape == zs.shape                   # tiny floor: no zero scale
