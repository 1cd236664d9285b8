"""fp8 dense Llama MLP on the GPU: ``penny_dense_fp8_gemm`` bit for bit on exact inputs (layout, K
splits, row edges, sentinels, contract), its arithmetic against the f64 certificate of ``moe_ref``, the
``mlp_fp8`` pipeline on both kernels, and the model / engine with ``mlp_dtype="fp8"``."""
import functools

import pytest
import torch

import dense_fp8_ref as D
import lora_ref as R
import moe_ref

from financial_chatbot_llm_amd import ops
from financial_chatbot_llm_amd.config import EngineConfig
from financial_chatbot_llm_amd.engine import LLMEngine, SamplingParams
from financial_chatbot_llm_amd.models import build_model
from financial_chatbot_llm_amd.models.common import AttentionMetadata, KVCache
from financial_chatbot_llm_amd.models.configs import get_model_config
from financial_chatbot_llm_amd.models.llama import LlamaModel
from financial_chatbot_llm_amd.ops import _native, fp8_dense
from financial_chatbot_llm_amd.ops.attention import KV_BS
from financial_chatbot_llm_amd.ops.gemm import Slabs, interleave16

pytestmark = pytest.mark.gpu
DEV = "cuda"

MS = [1, 15, 16, 17, 64, 65, 255, 256]
SMALL = [(32, 128), (1024, 256), (256, 512)]            # (32, 128): the smallest N and K the contract allows
PRODUCTION = {"silu": (28672, 4096), "slabs": (4096, 14336)}   # one pair per epilogue, at M = 128


def _configs(N, K, epi):
    """Every (S, ntf) the small shapes can run: both row groups N allows, every power-of-two K split."""
    ntfs = [2, 4] if N % 64 == 0 else [2]
    Ss = [s for s in (1, 2, 4) if K % (128 * s) == 0] if epi == "slabs" else [1]
    return [(S, ntf) for ntf in ntfs for S in Ss]


def _run(case, epi, S, ntf):
    buf = D.out_buffer(case.M, case.N, epi, S, case.xq.device)
    ops.dense_fp8_gemm(case.x_view(), case.xs, case.wq, case.ws, epi, S, ntf, out=buf.view, M=case.M)
    return buf


def _check_exact(case, epi, S, ntf, what):
    buf = _run(case, epi, S, ntf)
    want = D.expected(case, epi, S, ops.silu_mul)
    got = D.result(buf)
    same = D.bits(got) == D.bits(want)
    if not bool(same.all()):
        i = tuple(int(v) for v in (~same).nonzero()[0])
        raise AssertionError(f"{what} {epi} S={S} ntf={ntf} M={case.M} N={case.N} K={case.K}: {int((~same).sum())} elements "
                             f"differ; {i}: got {float(got[i])!r}, expected {float(want[i])!r}")
    assert D.untouched(buf), f"{what} {epi} S={S} ntf={ntf}: wrote outside [M, width]"


# ------------------------------------------------------------------------------------------------
# exact layout
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", SMALL)
@pytest.mark.parametrize("M", MS)
def test_one_hot_rows_bit_exact(M, N, K):
    """Y[m, n] = W[n, k(m)] * x * xs[m] * ws[n] bit for bit (f32 slabs, bf16, and silu_mul of the bf16
    gate|up), k(m) over the calls covering every required column; rows >= M of Xq / xs are NaN codes and
    the outputs sit in sentinel buffers with padded strides."""
    for epi in ("slabs", "bf16", "silu"):
        for S, ntf in _configs(N, K, epi):
            for case in D.onehot_cases(M, N, K, S, seed=M + N, dev=DEV):
                _check_exact(case, epi, S, ntf, "one-hot")


@pytest.mark.parametrize("N,K", SMALL)
@pytest.mark.parametrize("M", MS)
def test_few_term_sums_bit_exact(M, N, K):
    """At most 4 integer terms per row, one per K split: exact under any accumulation width."""
    for epi in ("slabs", "bf16", "silu"):
        for S, ntf in _configs(N, K, epi):
            case = D.few_term_case(M, N, K, S, seed=7 * M + K, silu=epi == "silu").to(DEV)
            _check_exact(case, epi, S, ntf, "few-term")


@functools.lru_cache(maxsize=None)
def _production_w(N, K, kind):
    g = torch.Generator(device=DEV).manual_seed(N + K)
    if kind == "int":
        return D.codes_of(torch.randint(-8, 9, (N, K), device=DEV, generator=g).float())
    c = torch.randint(0, 256, (N, K), device=DEV, generator=g, dtype=torch.int32).to(torch.uint8)
    c[(c & 0x7F) == D.NAN_CODE] = 0
    return c


@pytest.mark.parametrize("epi", ["silu", "slabs"])
def test_production_shapes_bit_exact(epi):
    """(28672, 4096) with the SiLU epilogue and (4096, 14336) as slabs at M = 128: every table config
    for the shape plus S = 1, one-hot (all required columns) and few-term cases."""
    N, K = PRODUCTION[epi]
    M = 128
    cfgs = D.table_splits(N, K)
    assert cfgs, (N, K)
    for S, ntf in cfgs:
        S = S if epi == "slabs" else 1
        for case in D.onehot_cases(M, N, K, S, seed=1, dev=DEV, wq=_production_w(N, K, "codes")):
            _check_exact(case, epi, S, ntf, "production one-hot")
        case = D.few_term_case(M, N, K, S, seed=2, wq=_production_w(N, K, "int"), silu=epi == "silu").to(DEV)
        _check_exact(case, epi, S, ntf, "production few-term")


def test_contract_violations_return_invalid_value_and_write_nothing():
    """Each clause of the checked contract violated once: hipErrorInvalidValue (1), output untouched."""
    M, N, K = 17, 64, 256
    case = D.few_term_case(M, N, K, 1, seed=3).to(DEV)
    good = dict(xq=case.x_view(), ldx=case.xq.stride(0), xs=case.xs, wq=case.wq, ws=case.ws, M=M, N=N, K=K, S=1, ntf=2)

    def call(epi, buf, **kw):
        a = {**good, **kw}
        ldy = a.pop("ldy", buf.view.stride(-2))
        y = a.pop("y", buf.view)
        _native.call("penny_dense_fp8_gemm", _native.ptr(a["xq"]), a["ldx"], _native.ptr(a["xs"]), _native.ptr(a["wq"]),
                     _native.ptr(a["ws"]), _native.ptr(y), ldy, a["M"], a["N"], a["K"], fp8_dense.EPI.get(epi, epi),
                     a["S"], a["ntf"], _native.stream())

    bad = {
        "K not a multiple of 128": ("bf16", dict(K=192)),
        "N not a multiple of the row group": ("bf16", dict(N=48)),
        "N not a multiple of the 64-row group": ("bf16", dict(N=96, ntf=4)),
        "row group other than 2 or 4": ("bf16", dict(ntf=3)),
        "ldx not 16-byte aligned": ("bf16", dict(ldx=K + 8)),
        "ldx below K": ("bf16", dict(ldx=K - 16)),
        "ldy not 16-byte aligned (bf16)": ("bf16", dict(ldy=N + 4)),
        "ldy not 16-byte aligned (f32)": ("slabs", dict(ldy=N + 2)),
        "ldy below the width": ("silu", dict(ldy=N // 2 - 8)),
        "xs null": ("bf16", dict(xs=None)),
        "ws null": ("bf16", dict(ws=None)),
        "M = 0": ("bf16", dict(M=0)),
        "M = 257": ("bf16", dict(M=257)),
        "S = 2 with a bf16 output": ("bf16", dict(S=2)),
        "S = 2 with the SiLU output": ("silu", dict(S=2)),
        "S = 17": ("slabs", dict(S=17)),
        "S = 0": ("slabs", dict(S=0)),
        "K not a multiple of 128 S": ("slabs", dict(S=4)),
        "Xq misaligned": ("bf16", dict(xq=case.xq.view(-1)[8:])),
        "unknown epilogue": (9, dict()),
    }
    for why, (epi, kw) in bad.items():
        buf = D.out_buffer(M, N, epi if isinstance(epi, str) else "bf16", 1, DEV)
        with pytest.raises(RuntimeError, match="hipError 1"):
            call(epi, buf, **kw)
        assert D.untouched(buf) and bool((buf.flat == D.SENTINEL).all()), why
    for epi in ("silu", "bf16", "slabs"):                # and the unviolated call goes through
        buf = D.out_buffer(M, N, epi, 1, DEV)
        call(epi, buf)
        assert torch.equal(D.bits(D.result(buf)), D.bits(D.expected(case, epi, 1, ops.silu_mul)))


# ------------------------------------------------------------------------------------------------
# arithmetic
# ------------------------------------------------------------------------------------------------
def _check_arith(case, epi, S, ntf):
    ref = D.reference_f64(case, epi, S)
    buf = _run(case, epi, S, ntf)
    got = D.result(buf).clone()
    what = f"{epi} S={S} ntf={ntf} M={case.M} N={case.N} K={case.K}"
    ratio = moe_ref.check_within(got, ref.ref, ref.bound, what)
    units = moe_ref.acc_units(got, ref.ref, ref.ssc) if ref.ssc is not None else float("nan")
    print(f"{what}: largest error / bound {ratio:.3f}, proven accumulation error {units:.1f} x 2^-24 S")
    assert D.untouched(buf)
    again = _run(case, epi, S, ntf)
    assert torch.equal(D.bits(D.result(again)), D.bits(got)), f"{what}: two calls differ"
    return got


@pytest.mark.parametrize("N,K", SMALL)
@pytest.mark.parametrize("M", [17, 128, 256])
def test_random_inputs_within_the_f64_certificate(M, N, K):
    """Random e4m3 inputs and scales: every element within acc_bound(K) * S + the output roundings of the
    f64 reference of the kernel's own Xq and xs; two calls bit-equal; a row's bits do not depend on the
    other rows' contents."""
    case = D.random_case(M, N, K, seed=M + K).to(DEV)
    other = D.random_case(M, N, K, seed=M + K + 1)
    keep = [0, M // 2, M - 1]
    xq2, xs2 = other.xq.clone(), other.xs.clone()
    xq2[keep], xs2[keep] = case.xq[keep].cpu(), case.xs[keep].cpu()
    mixed = D.Case(M, N, K, xq2.to(DEV), xs2.to(DEV), case.wq, case.ws)
    for epi in ("slabs", "bf16", "silu"):
        for S, ntf in _configs(N, K, epi):
            got = _check_arith(case, epi, S, ntf)
            alt = D.result(_run(mixed, epi, S, ntf))
            assert torch.equal(D.bits(alt[..., keep, :]), D.bits(got[..., keep, :])), (epi, S, ntf)


@pytest.mark.parametrize("epi", ["silu", "slabs"])
def test_production_shapes_within_the_f64_certificate(epi):
    N, K = PRODUCTION[epi]
    case = D.random_case(128, 64, K, seed=5)             # X and scales from the small builder, W on the device
    g = torch.Generator(device=DEV).manual_seed(9)
    wq = torch.randn((N, K), device=DEV, generator=g).to(D.FP8).view(torch.uint8)
    ws = torch.rand((N,), device=DEV, generator=g) * 0.02 + 0.001
    case = D.Case(128, N, K, case.xq.to(DEV), case.xs.to(DEV), wq, ws)
    for S, ntf in D.table_splits(N, K):
        _check_arith(case, epi, S if epi == "slabs" else 1, ntf)


# ------------------------------------------------------------------------------------------------
# pipeline (llama-tiny's shapes: H = 256, F = 512)
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tiny_mlp():
    g = torch.Generator().manual_seed(11)
    H, F_ = 256, 512
    gate, up = (torch.randn(F_, H, generator=g) * 0.05).bfloat16(), (torch.randn(F_, H, generator=g) * 0.05).bfloat16()
    down = (torch.randn(H, F_, generator=g) * 0.05).bfloat16()
    cpu = ops.quantize_dense_mlp(interleave16(gate, up).contiguous(), down)
    gpu = ops.DenseFp8MLP(*(t.to(DEV) for t in cpu.tensors()))
    h = torch.randn(600, H, generator=g).bfloat16()
    return cpu, gpu, h, ops.dense_fp8_reference(h, cpu, quant_act=True)


def _dense(out):
    return out.materialize() if isinstance(out, Slabs) else out


@pytest.mark.parametrize("M", [1, 128, 256, 257, 600])
def test_mlp_fp8_against_the_self_quantising_reference(M):
    """Per token ||got - ref|| / ||ref|| <= moe_ref.PER_TOKEN_LIMIT against dense_fp8_reference(quant_act=True)
    -- the Mixtral pipeline's arithmetic with one expert, and its limit -- on the streaming kernel (M <= 256)
    and the tile kernel (M > 256), slabs and bf16 outputs alike; the intermediate is the bf16 SiLU product."""
    cpu, gpu, h, ref = _tiny_mlp()
    hd = h[:M].to(DEV)
    assert fp8_dense.mlp_fp8_path(hd, gpu) == ("stream" if M <= 256 else "tiles")
    for slabs in (True, False):
        out, a = ops.mlp_fp8(hd, gpu, slabs=slabs)
        assert isinstance(out, Slabs) == (slabs and M <= 256)
        assert a.shape == (M, 512) and a.dtype == torch.bfloat16
        worst = moe_ref.check_per_token(_dense(out).float().cpu(), ref[:M].float(), moe_ref.PER_TOKEN_LIMIT,
                                        f"mlp_fp8 M={M} slabs={slabs}")
        print(f"mlp_fp8 M={M} slabs={slabs}: largest per-token error {worst:.4f} (limit {moe_ref.PER_TOKEN_LIMIT})")


def test_mlp_fp8_paths_agree_on_the_same_rows():
    cpu, gpu, h, ref = _tiny_mlp()
    hd = h.to(DEV)
    tiles, _ = ops.mlp_fp8(hd, gpu)                      # 600 rows: tile kernel
    stream, _ = ops.mlp_fp8(hd[:256], gpu)               # the first 256 of them: streaming kernel
    worst = moe_ref.check_per_token(stream.float().cpu(), tiles[:256].float().cpu(), moe_ref.PER_TOKEN_LIMIT, "stream vs tiles")
    print(f"stream vs tiles: largest per-token difference {worst:.4f}")


def test_mlp_fp8_graph_replay_is_bit_equal_to_eager():
    cpu, gpu, h, ref = _tiny_mlp()
    hd = h[:64].to(DEV).clone()
    eager, a_e = ops.mlp_fp8(hd, gpu, slabs=True)
    eager, a_e = eager.P.clone(), a_e.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.mlp_fp8(hd, gpu, slabs=True)                 # warm the allocator on the capture stream
        with torch.cuda.graph(g, stream=s):
            out, a = ops.mlp_fp8(hd, gpu, slabs=True)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        out.P.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(D.bits(out.P), D.bits(eager)) and torch.equal(D.bits(a), D.bits(a_e))


# ------------------------------------------------------------------------------------------------
# model and engine (llama-tiny)
# ------------------------------------------------------------------------------------------------
def _cpu_twin(gpu):
    """The CPU model on the same quantised weights (the torch path of every op)."""
    cpu = LlamaModel(gpu.cfg, device="cpu", tp_rank=0, tp_size=1)
    cpu.w = {k: v.cpu() for k, v in gpu.w.items()}
    cpu.mlp_dtype = gpu.mlp_dtype
    cpu.mlp_q = {i: ops.DenseFp8MLP(*(t.cpu() for t in q.tensors())) for i, q in gpu.mlp_q.items()}
    return cpu


def _prefill_then_decode(m, ids, steps):
    """Logits [len(ids) + len(steps), V] (f32, CPU): one prefill of ``ids``, then one decode step per forced
    token of ``steps`` on the same KV pool."""
    dev = m.device
    T = len(ids)
    total = T + len(steps)
    nb = (total + KV_BS - 1) // KV_BS
    kv = KVCache(m.cfg.num_layers, nb + 1, m.hkv, m.D, dtype=m.dtype, device=dev)
    bt = torch.arange(1, nb + 1, dtype=torch.int32)[None].to(dev)

    def slot(p):
        return (1 + p // KV_BS) * KV_BS + p % KV_BS
    meta = AttentionMetadata(slots=torch.tensor([slot(p) for p in range(T)], dtype=torch.int32).to(dev),
                             num_prefill_tokens=T, cu_q=torch.tensor([0, T], dtype=torch.int32).to(dev),
                             ctx_lens_p=torch.tensor([T], dtype=torch.int32).to(dev), block_tables_p=bt, max_q_len=T)
    out = [m.logits(m.forward(torch.tensor(ids, dtype=torch.int32).to(dev), torch.arange(T, dtype=torch.int32).to(dev),
                              meta, kv)).float().cpu()]
    for j, tok in enumerate(steps):
        p = T + j
        meta = AttentionMetadata(slots=torch.tensor([slot(p)], dtype=torch.int32).to(dev), num_decode=1,
                                 ctx_lens_d=torch.tensor([p + 1], dtype=torch.int32).to(dev), block_tables_d=bt)
        h = m.forward(torch.tensor([tok], dtype=torch.int32).to(dev), torch.tensor([p], dtype=torch.int32).to(dev), meta, kv)
        out.append(m.logits(h).float().cpu())
    return torch.cat(out)


def test_fp8_model_logits_match_the_cpu_path_of_the_same_quantised_model():
    """A 300-token prefill (tile kernel) and the following decode steps (streaming kernel) against the CPU
    torch path on the same codes and scales: max error < 0.05 x max |ref|, the tolerance
    tests/test_engine_gpu.py applies to the fp8 Mixtral layer (line 152)."""
    cfg = get_model_config("llama-tiny")
    gpu = LlamaModel(cfg, device="cuda", tp_rank=0, tp_size=1).init_random(seed=1).quantize_mlp()
    cpu = _cpu_twin(gpu)
    ids, steps = list(range(3, 303)), [11, 200, 4096]
    calls = []
    real = _native.call
    _native.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        a = _prefill_then_decode(gpu, ids, steps)
    finally:
        _native.call = real
    assert "penny_dense_fp8_gemm" in calls and "penny_moe_gemm_prefill_fp8" in calls
    b = _prefill_then_decode(cpu, ids, steps)
    scale = b.abs().max().item()
    err_p, err_d = (a[:300] - b[:300]).abs().max().item(), (a[300:] - b[300:]).abs().max().item()
    print(f"fp8 llama-tiny: max |gpu - cpu| prefill {err_p:.4e}, decode {err_d:.4e}; 0.05 x max |ref| = {0.05 * scale:.4e}")
    assert err_p < 0.05 * scale and err_d < 0.05 * scale


def test_fp8_model_frees_the_bf16_mlp_weights():
    cfg = get_model_config("llama-tiny")
    bf16 = LlamaModel(cfg, device="cuda", tp_rank=0, tp_size=1).init_random(seed=1)
    before = bf16.num_bytes()
    mlp_bf16 = sum(bf16.w[f"layers.{i}.{n}"].numel() * 2 for i in range(cfg.num_layers) for n in ("gate_up", "down"))
    fp8 = bf16.quantize_mlp()
    mlp_fp8 = sum(q.num_bytes() for q in fp8.mlp_q.values())
    assert mlp_fp8 < 0.51 * mlp_bf16 + 4 * 3 * 1024 * cfg.num_layers
    assert before - fp8.num_bytes() >= mlp_bf16 - mlp_fp8
    names = [k for k in list(fp8.w) + list(fp8.wt) if k.endswith((".gate_up", ".down"))]
    assert not names, names
    for i in range(cfg.num_layers):
        for t in fp8.mlp_q[i].tensors():
            assert t.dtype in (torch.float8_e4m3fn, torch.float32) and t.is_cuda


CFG = dict(model="llama-tiny", device="cuda", num_kv_blocks=128, max_model_len=1024, max_num_seqs=8,
           graph_batch_sizes=(1, 2, 3, 4, 5, 6, 7, 8), seed=0)
MODES = {"eager-sync": (False, False), "eager-overlap": (False, True), "graph-sync": (True, False),
         "graph-overlap": (True, True)}
_MODEL = {}
_RESULTS = {}
PROMPTS = [list(range(100 + 7 * i, 140 + 9 * i)) for i in range(3)]


def _engine(graph, overlap, mlp_dtype="fp8"):
    eng = LLMEngine(EngineConfig(use_cuda_graph=graph, async_scheduling=overlap, mlp_dtype=mlp_dtype, **CFG),
                    model=_MODEL.get(mlp_dtype))
    _MODEL[mlp_dtype] = eng.model
    if graph:
        eng.warmup()
    return eng


@pytest.mark.parametrize("mode", list(MODES))
def test_fp8_engine_modes_agree(mode):
    """Seeded generation on the fp8 model: the same tokens eager and under hipGraph, with synchronous and
    overlapped stepping (a row's MLP result does not depend on the batch around it)."""
    graph, overlap = MODES[mode]
    eng = _engine(graph, overlap)
    assert eng.model.mlp_dtype == "fp8" and eng.stats()["mlp_dtype"] == "fp8"
    sp = SamplingParams(temperature=0.7, max_tokens=8, seed=5, ignore_eos=True)
    got = eng.generate(PROMPTS, sp)
    assert all(len(o) == 8 for o in got)
    if graph:
        assert eng.runner.stats["graph_steps"] > 0
    _RESULTS[mode] = got
    assert got == next(iter(_RESULTS.values())), mode


def test_lora_request_on_the_fp8_model():
    """The down delta is ops.lora_delta on the intermediate mlp_fp8 returns (bit for bit), and an adapter
    request runs through the engine on the fp8 model."""
    cfg = get_model_config("llama-tiny")
    m = LlamaModel(cfg, device="cuda", tp_rank=0, tp_size=1).init_random(seed=1).quantize_mlp()
    sd = R.tiny_adapter(cfg, 1, r=8, std=0.3, dtype=torch.bfloat16)
    table = R.model_table(m, [(sd, 2.0)])
    g = torch.Generator().manual_seed(3)
    for M in (5, 300):
        h = torch.randn(M, cfg.hidden_size, generator=g).bfloat16().to(DEV)
        rs = torch.tensor([0 if i % 2 else -1 for i in range(M)], dtype=torch.int32, device=DEV)
        got = _dense(m.mlp(1, h, row_slot=rs))
        base, a = ops.mlp_fp8(h, m.mlp_q[1], slabs=True)
        plain = _dense(base).clone()
        want = _dense(ops.lora_delta(a, base, table, 1, "down", rs))
        assert torch.equal(D.bits(got), D.bits(want))
        assert torch.equal(D.bits(got[rs < 0]), D.bits(plain[rs < 0])) and not torch.equal(got[rs >= 0], plain[rs >= 0])
    m.lora = None                                        # the engine brings its own table
    eng = LLMEngine(EngineConfig(use_cuda_graph=False, mlp_dtype="fp8", **CFG), model=m)
    eng.load_adapter("a", R.tiny_adapter(cfg, 1, r=8, std=0.3), alpha=16.0)
    sp = SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True)
    import dataclasses
    out = eng.generate(PROMPTS[:2], dataclasses.replace(sp, adapter="a"))
    assert all(len(o) == 6 for o in out) and eng.stats()["lora_rows"] > 0


def test_switch_off_is_the_bf16_model_and_path():
    """mlp_dtype left at its default: build_model returns the bf16 weights (the keys and tensors init_random
    makes), mlp() never reaches the fp8 ops, and a seeded generation equals the directly constructed
    model's."""
    cfg = EngineConfig(use_cuda_graph=False, **CFG)
    assert cfg.mlp_dtype == "bf16"
    built = build_model(cfg, torch.device("cuda", torch.cuda.current_device()))
    direct = LlamaModel(get_model_config("llama-tiny"), device="cuda").init_random(seed=0)
    assert built.mlp_dtype == "bf16" and not built.mlp_q
    assert list(built.w) == list(direct.w) and list(built.wt) == list(direct.wt)
    assert all(torch.equal(built.w[k], direct.w[k]) for k in direct.w if direct.w[k] is not None)
    sp = SamplingParams(temperature=0.7, max_tokens=6, seed=5, ignore_eos=True)
    calls = []
    real = _native.call
    _native.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        a = LLMEngine(cfg, model=built).generate(PROMPTS, sp)
    finally:
        _native.call = real
    assert "penny_dense_fp8_gemm" not in calls and "penny_quant_rows_fp8" not in calls
    b = LLMEngine(cfg, model=direct).generate(PROMPTS, sp)
    assert a == b
