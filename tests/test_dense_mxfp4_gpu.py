"""MXFP4 dense Llama MLP on the GPU: ``penny_dense_mxfp4_gemm`` bit for bit on exact inputs (nibble order,
k-block / lane map, scale byte, K splits, row edges, sentinels, contract), ``penny_mxfp4_expand`` against the
CPU expansion, the arithmetic against the f64 certificate of ``moe_ref``, the ``mlp_mxfp4`` pipeline on both
paths, and the model / engine with ``mlp_dtype="mxfp4"``."""
import functools

import pytest
import torch

import dense_mxfp4_ref as D4
import lora_ref as R
import moe_ref

from financial_chatbot_llm_amd import ops
from financial_chatbot_llm_amd.config import EngineConfig
from financial_chatbot_llm_amd.engine import LLMEngine, SamplingParams
from financial_chatbot_llm_amd.models import build_model
from financial_chatbot_llm_amd.models.common import AttentionMetadata, KVCache
from financial_chatbot_llm_amd.models.configs import get_model_config
from financial_chatbot_llm_amd.models.llama import LlamaModel
from financial_chatbot_llm_amd.ops import _native, mxfp4_dense
from financial_chatbot_llm_amd.ops.attention import KV_BS
from financial_chatbot_llm_amd.ops.gemm import Slabs, interleave16

pytestmark = pytest.mark.gpu
DEV = "cuda"

MS = [1, 15, 16, 17, 64, 65, 255, 256]
SMALL = [(32, 256), (1024, 256), (256, 512)]            # (32, 256): the smallest N and K the contract allows
PRODUCTION = {"silu": (28672, 4096), "slabs": (4096, 14336)}   # one pair per epilogue, at M = 128


def _configs(N, K, epi):
    """Every (S, ntf) the small shapes can run: what the default yields and S = 1, both row groups N allows,
    every power-of-two K split up to 4."""
    ntfs = [2, 4] if N % 64 == 0 else [2]
    Ss = [s for s in (1, 2, 4) if K % (256 * s) == 0] if epi == "slabs" else [1]
    cfgs = [(S, ntf) for ntf in ntfs for S in Ss]
    for c in D4.table_splits(N, K):
        c = c if epi == "slabs" else (1, c[1])
        if c not in cfgs:
            cfgs.append(c)
    return cfgs


def _run(case, epi, S, ntf):
    buf = D4.out_buffer(case.M, case.N, epi, S, case.xq.device)
    ops.dense_mxfp4_gemm(case.x_view(), case.xs, case.wc, case.we, case.ws, epi, S, ntf, out=buf.view, M=case.M)
    return buf


def _check_exact(case, epi, S, ntf, what):
    buf = _run(case, epi, S, ntf)
    want = D4.expected(case, epi, S, ops.silu_mul)
    got = D4.result(buf)
    same = D4.bits(got) == D4.bits(want)
    if not bool(same.all()):
        i = tuple(int(v) for v in (~same).nonzero()[0])
        raise AssertionError(f"{what} {epi} S={S} ntf={ntf} M={case.M} N={case.N} K={case.K}: {int((~same).sum())} elements "
                             f"differ; {i}: got {float(got[i])!r}, expected {float(want[i])!r}")
    assert D4.untouched(buf), f"{what} {epi} S={S} ntf={ntf}: wrote outside [M, width]"


# ------------------------------------------------------------------------------------------------
# exact layout
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K", SMALL)
@pytest.mark.parametrize("M", MS)
def test_one_hot_rows_bit_exact(M, N, K):
    """Y[m, n] = W[n, k(m)] * x * xs[m] * ws[n] bit for bit (f32 slabs, bf16, and silu_mul of the bf16
    gate|up), k(m) over the calls covering every required column, W every code (-0 included) at random block
    exponents -8 .. 0: this pins the nibble order (even k low), the k-block / lane map and the scale byte.
    Rows >= M of Xq / xs are NaN codes and the outputs sit in sentinel buffers with padded strides."""
    for epi in ("slabs", "bf16", "silu"):
        for S, ntf in _configs(N, K, epi):
            for case in D4.onehot_cases(M, N, K, S, seed=M + N, dev=DEV):
                _check_exact(case, epi, S, ntf, "one-hot")


@pytest.mark.parametrize("N,K", SMALL)
@pytest.mark.parametrize("M", MS)
def test_few_term_sums_bit_exact(M, N, K):
    """At most 4 integer terms per row, one per K split: exact under any accumulation width."""
    for epi in ("slabs", "bf16", "silu"):
        for S, ntf in _configs(N, K, epi):
            case = D4.few_term_case(M, N, K, S, seed=7 * M + K, silu=epi == "silu").to(DEV)
            _check_exact(case, epi, S, ntf, "few-term")


@functools.lru_cache(maxsize=None)
def _production_w(N, K, kind):
    g = torch.Generator(device=DEV).manual_seed(N + K)
    return D4.int_w(N, K, g, dev=DEV) if kind == "int" else D4.random_w(N, K, g, dev=DEV)


@pytest.mark.parametrize("epi", ["silu", "slabs"])
def test_production_shapes_bit_exact(epi):
    """(28672, 4096) with the SiLU epilogue and (4096, 14336) as slabs at M = 128: every table config
    for the shape plus S = 1, one-hot (all required columns) and few-term cases."""
    N, K = PRODUCTION[epi]
    M = 128
    cfgs = D4.table_splits(N, K)
    assert cfgs, (N, K)
    for S, ntf in cfgs:
        S = S if epi == "slabs" else 1
        for case in D4.onehot_cases(M, N, K, S, seed=1, dev=DEV, w=_production_w(N, K, "codes")):
            _check_exact(case, epi, S, ntf, "production one-hot")
        case = D4.few_term_case(M, N, K, S, seed=2, w=_production_w(N, K, "int"), silu=epi == "silu")
        _check_exact(case, epi, S, ntf, "production few-term")


def test_exact_case_agrees_with_the_fp8_kernel_on_the_expansion():
    """The expansion argument on the hardware: penny_mxfp4_expand + penny_dense_fp8_gemm and the 4-bit kernel
    give the same bits on a few-term exact case, for every epilogue."""
    M, N, K = 65, 256, 512
    for epi, S in (("slabs", 2), ("bf16", 1), ("silu", 1)):
        case = D4.few_term_case(M, N, K, S, seed=11, silu=epi == "silu").to(DEV)
        wq = ops.expand_mxfp4(case.wc, case.we)
        assert torch.equal(wq.view(torch.uint8), case.wq)
        buf8 = D4.out_buffer(M, N, epi, S, DEV)
        ops.dense_fp8_gemm(case.x_view(), case.xs, wq, case.ws, epi, S, 2, out=buf8.view, M=M)
        buf4 = _run(case, epi, S, 2)
        assert torch.equal(D4.bits(D4.result(buf4)), D4.bits(D4.result(buf8))), epi
        assert torch.equal(D4.bits(D4.result(buf4)), D4.bits(D4.expected(case, epi, S, ops.silu_mul))), epi


# ------------------------------------------------------------------------------------------------
# expansion
# ------------------------------------------------------------------------------------------------
GUARD = 64


def _expand_guarded(wc, we):
    Nr, K = wc.shape[0], wc.shape[1] * 2
    flat = torch.full((GUARD + Nr * K + GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    out = flat[GUARD:GUARD + Nr * K].view(Nr, K)
    assert ops.expand_mxfp4(wc.to(DEV), we.to(DEV), out=out) is out
    torch.cuda.synchronize()
    assert bool((flat[:GUARD] == 0x5A).all()) and bool((flat[GUARD + Nr * K:] == 0x5A).all()), "wrote outside [N, K]"
    return out.cpu()


def test_expand_every_code_and_exponent_equals_the_cpu_expansion():
    wc, we = D4.all_codes_and_exponents()
    got = _expand_guarded(wc, we)
    assert torch.equal(got, ops.expand_mxfp4(wc, we).view(torch.uint8))
    assert torch.equal(got, D4.w_fp8(wc, we))
    assert not bool(((got & 0x7F) == 0x7F).any())
    assert bool((got[D4.unpack(wc) == 8] == 0x80).all())             # -0 -> e4m3 -0


@pytest.mark.parametrize("N,K", [(16, 32), (33, 288), (1024, 256)])
def test_expand_shapes_equal_the_cpu_expansion(N, K):
    g = torch.Generator().manual_seed(N + K)
    wc, we = D4.random_w(N, K, g)
    got = _expand_guarded(wc, we)
    assert torch.equal(got, ops.expand_mxfp4(wc, we).view(torch.uint8))
    assert torch.equal(got, D4.w_fp8(wc, we))


def test_expand_contract_violations_return_invalid_value_and_write_nothing():
    g = torch.Generator().manual_seed(1)
    wc, we = (t.to(DEV) for t in D4.random_w(16, 64, g))
    out = torch.full((16 * 64 + 32,), 0x5A, dtype=torch.uint8, device=DEV)
    p = _native.ptr
    bad = {
        "K not a multiple of 32": (p(wc), p(we), p(out), 16, 48),
        "K = 0": (p(wc), p(we), p(out), 16, 0),
        "N = 0": (p(wc), p(we), p(out), 0, 64),
        "codes null": (None, p(we), p(out), 16, 64),
        "exponents null": (p(wc), None, p(out), 16, 64),
        "out null": (p(wc), p(we), None, 16, 64),
        "codes misaligned": (p(wc.view(-1)[8:]), p(we), p(out), 8, 64),
        "out misaligned": (p(wc), p(we), p(out[8:]), 16, 64),
    }
    for why, args in bad.items():
        with pytest.raises(RuntimeError, match="hipError 1"):
            _native.call("penny_mxfp4_expand", *args, _native.stream())
        assert bool((out == 0x5A).all()), why
    _native.call("penny_mxfp4_expand", p(wc), p(we), p(out), 16, 64, _native.stream())
    assert torch.equal(out[:16 * 64].view(16, 64).cpu(), D4.w_fp8(wc.cpu(), we.cpu())) and bool((out[16 * 64:] == 0x5A).all())


def test_contract_violations_return_invalid_value_and_write_nothing():
    """Each clause of the checked contract violated once: hipErrorInvalidValue (1), output untouched."""
    M, N, K = 17, 64, 512
    case = D4.few_term_case(M, N, K, 1, seed=3).to(DEV)
    good = dict(xq=case.x_view(), ldx=case.xq.stride(0), xs=case.xs, wc=case.wc, we=case.we, ws=case.ws, M=M, N=N, K=K,
                S=1, ntf=2)

    def call(epi, buf, **kw):
        a = {**good, **kw}
        ldy = a.pop("ldy", buf.view.stride(-2))
        y = a.pop("y", buf.view)
        _native.call("penny_dense_mxfp4_gemm", _native.ptr(a["xq"]), a["ldx"], _native.ptr(a["xs"]), _native.ptr(a["wc"]),
                     _native.ptr(a["we"]), _native.ptr(a["ws"]), _native.ptr(y), ldy, a["M"], a["N"], a["K"],
                     mxfp4_dense.EPI.get(epi, epi), a["S"], a["ntf"], _native.stream())

    bad = {
        "K not a multiple of 256": ("bf16", dict(K=384)),
        "N not a multiple of the row group": ("bf16", dict(N=48)),
        "N not a multiple of the 64-row group": ("bf16", dict(N=96, ntf=4)),
        "row group other than 2 or 4": ("bf16", dict(ntf=3)),
        "ldx not 16-byte aligned": ("bf16", dict(ldx=K + 8)),
        "ldx below K": ("bf16", dict(ldx=K - 16)),
        "ldx beyond the 32-bit lane offsets": ("bf16", dict(ldx=1 << 23)),
        "ldy not 16-byte aligned (bf16)": ("bf16", dict(ldy=N + 4)),
        "ldy not 16-byte aligned (f32)": ("slabs", dict(ldy=N + 2)),
        "ldy below the width": ("silu", dict(ldy=N // 2 - 8)),
        "xs null": ("bf16", dict(xs=None)),
        "ws null": ("bf16", dict(ws=None)),
        "codes null": ("bf16", dict(wc=None)),
        "exponents null": ("bf16", dict(we=None)),
        "M = 0": ("bf16", dict(M=0)),
        "M = 257": ("bf16", dict(M=257)),
        "S = 2 with a bf16 output": ("bf16", dict(S=2)),
        "S = 2 with the SiLU output": ("silu", dict(S=2)),
        "S = 17": ("slabs", dict(S=17)),
        "S = 0": ("slabs", dict(S=0)),
        "K not a multiple of 256 S": ("slabs", dict(S=4)),
        "Xq misaligned": ("bf16", dict(xq=case.xq.view(-1)[8:])),
        "codes misaligned": ("bf16", dict(wc=case.wc.view(-1)[8:])),
        "exponents misaligned": ("bf16", dict(we=case.we.view(-1)[8:])),
        "xs misaligned": ("bf16", dict(xs=case.xs[1:])),
        "ws misaligned": ("bf16", dict(ws=case.ws[1:])),
        "unknown epilogue": (9, dict()),
    }
    for why, (epi, kw) in bad.items():
        buf = D4.out_buffer(M, N, epi if isinstance(epi, str) else "bf16", 1, DEV)
        with pytest.raises(RuntimeError, match="hipError 1"):
            call(epi, buf, **kw)
        assert D4.untouched(buf) and bool((buf.flat == D4.SENTINEL).all()), why
    for epi in ("silu", "bf16", "slabs"):                # and the unviolated call goes through
        buf = D4.out_buffer(M, N, epi, 1, DEV)
        call(epi, buf)
        assert torch.equal(D4.bits(D4.result(buf)), D4.bits(D4.expected(case, epi, 1, ops.silu_mul)))


# ------------------------------------------------------------------------------------------------
# arithmetic
# ------------------------------------------------------------------------------------------------
def _check_arith(case, epi, S, ntf):
    ref = D4.reference_f64(case, epi, S)
    buf = _run(case, epi, S, ntf)
    got = D4.result(buf).clone()
    what = f"{epi} S={S} ntf={ntf} M={case.M} N={case.N} K={case.K}"
    units = moe_ref.acc_units(got, ref.ref, ref.ssc) if ref.ssc is not None else float("nan")
    worst = float(((got.double().cpu() - ref.ref).abs() / ref.bound.clamp_min(1e-300)).max())
    print(f"{what}: largest error / bound {worst:.3f}, proven accumulation error {units:.1f} x 2^-24 S")
    moe_ref.check_within(got, ref.ref, ref.bound, what)
    assert D4.untouched(buf)
    again = _run(case, epi, S, ntf)
    assert torch.equal(D4.bits(D4.result(again)), D4.bits(got)), f"{what}: two calls differ"
    return got


@pytest.mark.parametrize("N,K", SMALL)
@pytest.mark.parametrize("M", [17, 128, 256])
def test_random_inputs_within_the_f64_certificate(M, N, K):
    """Random e4m3 activations, random 4-bit weights (every code, exponents -8 .. 0) and scales: every element
    within acc_bound(K) * S_abs + the output roundings of the f64 reference of the kernel's own Xq and xs; two
    calls bit-equal; a row's bits do not depend on the other rows' contents."""
    case = D4.random_case(M, N, K, seed=M + K).to(DEV)
    other = D4.random_case(M, N, K, seed=M + K + 1)
    keep = [0, M // 2, M - 1]
    xq2, xs2 = other.xq.clone(), other.xs.clone()
    xq2[keep], xs2[keep] = case.xq[keep].cpu(), case.xs[keep].cpu()
    mixed = case._replace(xq=xq2.to(DEV), xs=xs2.to(DEV))
    for epi in ("slabs", "bf16", "silu"):
        for S, ntf in _configs(N, K, epi):
            got = _check_arith(case, epi, S, ntf)
            alt = D4.result(_run(mixed, epi, S, ntf))
            assert torch.equal(D4.bits(alt[..., keep, :]), D4.bits(got[..., keep, :])), (epi, S, ntf)


@pytest.mark.parametrize("epi", ["silu", "slabs"])
def test_production_shapes_within_the_f64_certificate(epi):
    N, K = PRODUCTION[epi]
    small = D4.random_case(128, 64, K, seed=5)           # X and scales from the small builder, W on the device
    g = torch.Generator(device=DEV).manual_seed(9)
    wc, we = D4.random_w(N, K, g, dev=DEV)
    ws = torch.rand((N,), device=DEV, generator=g) * 0.02 + 0.001
    case = D4.Case(128, N, K, small.xq.to(DEV), small.xs.to(DEV), wc, we, ws, D4.w_fp8(wc, we))
    for S, ntf in D4.table_splits(N, K):
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
    cpu = ops.quantize_dense_mlp_mxfp4(interleave16(gate, up).contiguous(), down)
    gpu = ops.DenseMxfp4MLP(*(t.to(DEV) for t in cpu.tensors()))
    h = torch.randn(600, H, generator=g).bfloat16()
    return cpu, gpu, h, ops.dense_mxfp4_reference(h, cpu, quant_act=True)


def _dense(out):
    return out.materialize() if isinstance(out, Slabs) else out


def test_quantiser_on_the_device_equals_the_cpu():
    cpu, gpu, h, ref = _tiny_mlp()
    g = torch.Generator().manual_seed(11)
    gate = (torch.randn(512, 256, generator=g) * 0.05).bfloat16()
    c, e, s = ops.quantize_mxfp4_rowwise(gate)
    cd, ed, sd = ops.quantize_mxfp4_rowwise(gate.to(DEV))
    assert cd.is_cuda and torch.equal(cd.cpu(), c) and torch.equal(ed.cpu(), e) and torch.equal(sd.cpu(), s)


@pytest.mark.parametrize("M", [1, 128, 256, 257, 600])
def test_mlp_mxfp4_against_the_self_quantising_reference(M):
    """Per token ||got - ref|| / ||ref|| <= moe_ref.PER_TOKEN_LIMIT against dense_mxfp4_reference(quant_act=True)
    on the streaming kernel (M <= 256) and the expand path (M > 256), slabs and bf16 outputs alike; the
    intermediate is the bf16 SiLU product."""
    cpu, gpu, h, ref = _tiny_mlp()
    hd = h[:M].to(DEV)
    assert mxfp4_dense.mlp_mxfp4_path(hd, gpu) == ("stream" if M <= 256 else "expand")
    for slabs in (True, False):
        out, a = ops.mlp_mxfp4(hd, gpu, slabs=slabs)
        assert isinstance(out, Slabs) == (slabs and M <= 256)
        assert a.shape == (M, 512) and a.dtype == torch.bfloat16
        got, want = _dense(out).float().cpu(), ref[:M].float()
        worst = float(((got - want).norm(dim=1) / want.norm(dim=1)).max())
        print(f"mlp_mxfp4 M={M} slabs={slabs}: largest per-token error {worst:.4f} (limit {moe_ref.PER_TOKEN_LIMIT})")
        moe_ref.check_per_token(got, want, moe_ref.PER_TOKEN_LIMIT, f"mlp_mxfp4 M={M} slabs={slabs}")


def test_mlp_mxfp4_paths_agree_on_the_same_rows():
    cpu, gpu, h, ref = _tiny_mlp()
    hd = h.to(DEV)
    expand, _ = ops.mlp_mxfp4(hd, gpu)                   # 600 rows: expansion + the fp8 tile kernel
    stream, _ = ops.mlp_mxfp4(hd[:256], gpu)             # the first 256 of them: the 4-bit streaming kernel
    a, b = stream.float().cpu(), expand[:256].float().cpu()
    print(f"stream vs expand: largest per-token difference {float(((a - b).norm(dim=1) / b.norm(dim=1)).max()):.4f}")
    moe_ref.check_per_token(a, b, moe_ref.PER_TOKEN_LIMIT, "stream vs expand")


def test_mlp_mxfp4_graph_replay_is_bit_equal_to_eager():
    cpu, gpu, h, ref = _tiny_mlp()
    hd = h[:64].to(DEV).clone()
    eager, a_e = ops.mlp_mxfp4(hd, gpu, slabs=True)
    eager, a_e = eager.P.clone(), a_e.clone()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.mlp_mxfp4(hd, gpu, slabs=True)               # warm the allocator on the capture stream
        with torch.cuda.graph(g, stream=s):
            out, a = ops.mlp_mxfp4(hd, gpu, slabs=True)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        out.P.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(D4.bits(out.P), D4.bits(eager)) and torch.equal(D4.bits(a), D4.bits(a_e))


# ------------------------------------------------------------------------------------------------
# model and engine (llama-tiny)
# ------------------------------------------------------------------------------------------------
def _cpu_twin(gpu):
    """The CPU model on the same codes, exponents and scales (the torch path of every op)."""
    cpu = LlamaModel(gpu.cfg, device="cpu", tp_rank=0, tp_size=1)
    cpu.w = {k: v.cpu() for k, v in gpu.w.items() if not k.startswith("mlp_expand.")}
    cpu.mlp_dtype = gpu.mlp_dtype
    cpu.mlp_q = {i: ops.DenseMxfp4MLP(*(t.cpu() for t in q.tensors())) for i, q in gpu.mlp_q.items()}
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


def test_mxfp4_model_logits_match_the_cpu_path_of_the_same_quantised_model():
    """A 300-token prefill (expansion + the fp8 tile kernel) and the following decode steps (the 4-bit streaming
    kernel) against the CPU torch path on the same codes, exponents and scales: max error < 0.05 x max |ref|,
    the fp8 model test's tolerance."""
    cfg = get_model_config("llama-tiny")
    gpu = LlamaModel(cfg, device="cuda", tp_rank=0, tp_size=1).init_random(seed=1).quantize_mlp("mxfp4")
    cpu = _cpu_twin(gpu)
    ids, steps = list(range(3, 303)), [11, 200, 4096]
    calls = []
    real = _native.call
    _native.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        a = _prefill_then_decode(gpu, ids, steps)
    finally:
        _native.call = real
    assert "penny_dense_mxfp4_gemm" in calls and "penny_mxfp4_expand" in calls
    b = _prefill_then_decode(cpu, ids, steps)
    scale = b.abs().max().item()
    err_p, err_d = (a[:300] - b[:300]).abs().max().item(), (a[300:] - b[300:]).abs().max().item()
    print(f"mxfp4 llama-tiny: max |gpu - cpu| prefill {err_p:.4e}, decode {err_d:.4e}; 0.05 x max |ref| = {0.05 * scale:.4e}")
    assert err_p < 0.05 * scale and err_d < 0.05 * scale


def test_mxfp4_model_frees_the_bf16_mlp_weights():
    """The bf16 MLP weights and their tiled copies are gone; the 4-bit MLP is below 0.27 x the bf16 bytes plus the
    row scales, and num_bytes() counts it and the one expansion scratch (one layer's e4m3 MLP) all layers share."""
    cfg = get_model_config("llama-tiny")
    bf16 = LlamaModel(cfg, device="cuda", tp_rank=0, tp_size=1).init_random(seed=1)
    before = bf16.num_bytes()
    mlp_bf16 = sum(bf16.w[f"layers.{i}.{n}"].numel() * 2 for i in range(cfg.num_layers) for n in ("gate_up", "down"))
    m = bf16.quantize_mlp("mxfp4")
    mlp_4 = sum(q.num_bytes() for q in m.mlp_q.values())
    scales = 4 * (2 * cfg.intermediate_size + cfg.hidden_size) * cfg.num_layers
    scratch = 3 * cfg.intermediate_size * cfg.hidden_size
    assert mlp_4 < 0.27 * mlp_bf16 + scales
    assert m.mlp_q[0].scratch is m.mlp_q[cfg.num_layers - 1].scratch and m.mlp_q[0].scratch.num_bytes() == scratch
    assert before - m.num_bytes() == mlp_bf16 - mlp_4 - scratch
    assert m.num_bytes() - (before - mlp_bf16) < 0.27 * mlp_bf16 + scales + scratch
    names = [k for k in list(m.w) + list(m.wt) if k.endswith((".gate_up", ".down"))]
    assert not names, names
    for i in range(cfg.num_layers):
        for t in m.mlp_q[i].tensors():
            assert t.dtype in (torch.uint8, torch.float32) and t.is_cuda


CFG = dict(model="llama-tiny", device="cuda", num_kv_blocks=128, max_model_len=1024, max_num_seqs=8,
           graph_batch_sizes=(1, 2, 3, 4, 5, 6, 7, 8), seed=0)
MODES = {"eager-sync": (False, False), "eager-overlap": (False, True), "graph-sync": (True, False),
         "graph-overlap": (True, True)}
_MODEL = {}
_RESULTS = {}
PROMPTS = [list(range(100 + 7 * i, 140 + 9 * i)) for i in range(3)]


def _engine(graph, overlap, mlp_dtype="mxfp4"):
    eng = LLMEngine(EngineConfig(use_cuda_graph=graph, async_scheduling=overlap, mlp_dtype=mlp_dtype, **CFG),
                    model=_MODEL.get(mlp_dtype))
    _MODEL[mlp_dtype] = eng.model
    if graph:
        eng.warmup()
    return eng


@pytest.mark.parametrize("mode", list(MODES))
def test_mxfp4_engine_modes_agree(mode):
    """Seeded generation on the mxfp4 model: the same tokens eager and under hipGraph, with synchronous and
    overlapped stepping (a row's MLP result does not depend on the batch around it)."""
    graph, overlap = MODES[mode]
    eng = _engine(graph, overlap)
    assert eng.model.mlp_dtype == "mxfp4" and eng.stats()["mlp_dtype"] == "mxfp4"
    sp = SamplingParams(temperature=0.7, max_tokens=8, seed=5, ignore_eos=True)
    got = eng.generate(PROMPTS, sp)
    assert all(len(o) == 8 for o in got)
    if graph:
        assert eng.runner.stats["graph_steps"] > 0
    _RESULTS[mode] = got
    assert got == next(iter(_RESULTS.values())), mode


def test_lora_request_on_the_mxfp4_model():
    """The down delta is ops.lora_delta on the intermediate mlp_mxfp4 returns (bit for bit), on both paths, and
    an adapter request runs through the engine on the mxfp4 model."""
    cfg = get_model_config("llama-tiny")
    m = LlamaModel(cfg, device="cuda", tp_rank=0, tp_size=1).init_random(seed=1).quantize_mlp("mxfp4")
    sd = R.tiny_adapter(cfg, 1, r=8, std=0.3, dtype=torch.bfloat16)
    table = R.model_table(m, [(sd, 2.0)])
    g = torch.Generator().manual_seed(3)
    for M in (5, 300):
        h = torch.randn(M, cfg.hidden_size, generator=g).bfloat16().to(DEV)
        rs = torch.tensor([0 if i % 2 else -1 for i in range(M)], dtype=torch.int32, device=DEV)
        got = _dense(m.mlp(1, h, row_slot=rs))
        base, a = ops.mlp_mxfp4(h, m.mlp_q[1], slabs=True)
        plain = _dense(base).clone()
        want = _dense(ops.lora_delta(a, base, table, 1, "down", rs))
        assert torch.equal(D4.bits(got), D4.bits(want))
        assert torch.equal(D4.bits(got[rs < 0]), D4.bits(plain[rs < 0])) and not torch.equal(got[rs >= 0], plain[rs >= 0])
    m.lora = None                                        # the engine brings its own table
    eng = LLMEngine(EngineConfig(use_cuda_graph=False, mlp_dtype="mxfp4", **CFG), model=m)
    eng.load_adapter("a", R.tiny_adapter(cfg, 1, r=8, std=0.3), alpha=16.0)
    sp = SamplingParams(temperature=0.0, max_tokens=6, ignore_eos=True)
    import dataclasses
    out = eng.generate(PROMPTS[:2], dataclasses.replace(sp, adapter="a"))
    assert all(len(o) == 6 for o in out) and eng.stats()["lora_rows"] > 0


def test_switch_off_is_the_bf16_model_and_path():
    """mlp_dtype left at its default: build_model returns the bf16 weights (the keys and tensors init_random
    makes), mlp() never reaches the fp8 or mxfp4 ops, and a seeded generation equals the directly constructed
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
    assert not {"penny_dense_mxfp4_gemm", "penny_mxfp4_expand", "penny_dense_fp8_gemm", "penny_quant_rows_fp8"} & set(calls)
    b = LLMEngine(cfg, model=direct).generate(PROMPTS, sp)
    assert a == b
