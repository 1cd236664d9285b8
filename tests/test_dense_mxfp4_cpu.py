"""MXFP4 dense Llama MLP on the CPU: the quantiser, pack / unpack, the exact e4m3 expansion, the torch path
of ``ops.mlp_mxfp4`` against the self-quantising reference, the kernel config table against the kernel's
contract, the configuration switch, the exact test cases against a plain torch model of the kernel, and
TP = 2 over gloo."""
import json
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

import dense_mxfp4_ref as D4
from mp_util import to_np, to_torch

from financial_chatbot_llm_amd import ops
from financial_chatbot_llm_amd.config import EngineConfig
from financial_chatbot_llm_amd.models import build_model
from financial_chatbot_llm_amd.models.configs import get_model_config
from financial_chatbot_llm_amd.ops import mxfp4_dense
from financial_chatbot_llm_amd.ops.gemm import interleave16

FP8 = torch.float8_e4m3fn
GRID = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


def _weights(H=256, F_=512, seed=0, std=0.05):
    g = torch.Generator().manual_seed(seed)
    gate, up = (torch.randn(F_, H, generator=g) * std).bfloat16(), (torch.randn(F_, H, generator=g) * std).bfloat16()
    down = (torch.randn(H, F_, generator=g) * std).bfloat16()
    return gate, up, down


def _dequant(c, e, s):
    return D4.w_values(c, e) * s[:, None]


# ------------------------------------------------------------------------------------------------
# quantiser
# ------------------------------------------------------------------------------------------------
def test_values_on_the_grid_round_trip_bit_for_bit():
    """Rows whose values are e2m1 x 2^e x (a bf16 row scale) with the row maximum on 6: the quantiser gives
    back exactly those codes and exponents, for every code and every exponent -8 .. 0; -0 is not produced."""
    g = torch.Generator().manual_seed(0)
    N, K = 24, 32 * 9
    mag = torch.randint(0, 8, (N, K), generator=g)
    sign = torch.randint(0, 2, (N, K), generator=g)
    e = torch.arange(0, -9, -1).repeat(N, 1)                       # block b of every row: exponent -b
    mag[:, 0] = 7                                                  # row amax: 6 at exponent 0
    mag.view(N, 9, 32)[:, :, 1] = 7                                # every block holds a 6: its exponent is forced
    scale = torch.exp2(torch.randint(-6, 3, (N,), generator=g).float()) * 1.5
    vals = torch.tensor(GRID)[mag] * (1.0 - 2.0 * sign) * torch.exp2(e.float()).repeat_interleave(32, dim=1)
    w = (vals * scale[:, None]).bfloat16()
    assert torch.equal(w.float(), vals * scale[:, None])           # representable: 2 bits x 2 bits of significand
    c, ex, ws = ops.quantize_mxfp4_rowwise(w)
    assert c.dtype == torch.uint8 and c.shape == (N, K // 2) and ex.dtype == torch.uint8 and ex.shape == (N, 9)
    assert ws.dtype == torch.float32 and torch.equal(ws, scale)
    assert torch.equal(ex.long() - 127, e)
    want = (mag | ((sign == 1) & (mag > 0)).long() << 3).to(torch.uint8)
    assert torch.equal(D4.unpack(c), want)
    assert torch.equal(_dequant(c, ex, ws), w.float())


def test_the_exponent_is_the_smallest_admissible_one():
    """For every block: amax_block <= 6 ws 2^e, and (unless e = -8) not with e - 1; boundary blocks whose
    amax is exactly 6 ws 2^e for e = 0 .. -8, and one just above each boundary."""
    g = torch.Generator().manual_seed(1)
    w = (torch.randn(64, 512, generator=g) * 0.05).bfloat16()
    w[0, :32 * 9] = 0
    for b in range(9):                                             # row 0: amax 6 (block 15), blocks on the boundaries
        w[0, 32 * b] = 6.0 * 2.0 ** -b
    w[0, 32 * 15] = 6.0
    w[1] = w[0]
    for b in range(1, 9):                                          # row 1: one bf16 ulp above each boundary
        w[1, 32 * b] = 6.0 * 2.0 ** -b * (1 + 2.0 ** -7)
    w[0, 32 * 9:32 * 15] = 0
    w[1, 32 * 9:32 * 15] = 0
    w[0, 32 * 15 + 1:], w[1, 32 * 15 + 1:] = 0, 0
    c, ex, ws = ops.quantize_mxfp4_rowwise(w)
    e = ex.double() - 127
    assert int(e.min()) >= -8 and int(e.max()) <= 0
    bmax = w.double().abs().view(64, 16, 32).amax(2)
    top = 6.0 * ws.double()[:, None]
    # ws = fl(amax / 6), so 6 ws can fall one f32 rounding short of the row's amax: that block sits at the clamp e = 0
    assert bool(((bmax <= top * torch.exp2(e)) | ((e == 0) & (bmax <= top * (1 + 2.0 ** -23)))).all())
    tight = (e > -8) & (bmax > 0)
    assert bool((bmax > top * torch.exp2(e - 1))[tight].all())
    assert bool((e[bmax == 0] == -8).all())
    assert (ex[0, :9].long() - 127).tolist() == [0, -1, -2, -3, -4, -5, -6, -7, -8]
    assert (ex[1, :9].long() - 127).tolist() == [0, 0, -1, -2, -3, -4, -5, -6, -7]


def test_ties_round_to_the_even_code_and_nothing_saturates():
    """The midpoints of neighbouring e2m1 values go to the even code (0.25 -> 0, 0.75 -> 1, 1.25 -> 1,
    1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4), either sign; no |w / (ws 2^e)| exceeds 6 on Gaussian weights."""
    ties = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
    w = torch.zeros(2, 32)
    w[0, :7], w[1, :7] = ties, -ties
    w[:, 31] = 6.0                                                  # row scale 1, exponent 0
    c, ex, ws = ops.quantize_mxfp4_rowwise(w.bfloat16())
    assert torch.equal(ws, torch.ones(2)) and bool((ex == 127).all())
    got = D4.unpack(c)
    assert got[0, :7].tolist() == [0, 2, 2, 4, 4, 6, 6]
    assert got[1, :7].tolist() == [0, 10, 10, 12, 12, 14, 14]       # -0.25 -> code 0, not -0
    gate, up, down = _weights()
    for src in (gate, down):
        c, ex, ws = ops.quantize_mxfp4_rowwise(src)
        t = src.double().abs() / (ws.double()[:, None] * torch.exp2(ex.double() - 127).repeat_interleave(32, dim=1))
        assert float(t.max()) <= 6.0 * (1 + 2.0 ** -23)
        # round to nearest: within half the local grid spacing (0.25 below 2, 0.5 below 4, 1 above)
        err = (D4.w_values(c, ex).double().abs() * torch.exp2(127 - ex.double()).repeat_interleave(32, dim=1) - t).abs()
        half = torch.where(t < 2, 0.25, torch.where(t < 4, 0.5, 1.0))
        assert bool((err <= half + 1e-9).all())


def test_zero_rows_zero_blocks_and_gaussian_weights_hit_no_clamp():
    gate, up, down = _weights()
    gate[3] = 0.0                                                   # an all-zero row
    gate[5, 64:96] = 0.0                                            # an all-zero block
    gu = interleave16(gate, up).contiguous()
    w = ops.quantize_dense_mlp_mxfp4(gu, down)
    assert w.H == 256 and w.F == 512 and len(w.tensors()) == 6
    assert w.num_bytes() == (gu.numel() + down.numel()) // 2 + (gu.numel() + down.numel()) // 32 + 4 * (1024 + 256)
    gc, ge, gs = ops.quantize_mxfp4_rowwise(gate)
    assert gs[3] == 1.0 and bool((gc[3] == 0).all()) and bool((ge[3] == 119).all())
    assert ge[5, 2] == 119 and bool((gc[5, 32:48] == 0).all())
    for src in _weights(seed=2):                                    # llama-tiny's shapes, untouched Gaussians
        c, ex, ws = ops.quantize_mxfp4_rowwise(src)
        assert int(ex.min()) > 119, "a Gaussian block hit the -8 clamp"
        rel = ((_dequant(c, ex, ws) - src.float()).norm() / src.float().norm()).item()
        print(f"weight-only relative RMS error {rel:.4f} on {tuple(src.shape)}")
        assert 0.08 < rel < 0.14
    # row-wise: commutes with the 16-row gate|up interleave
    uc, ue, us = ops.quantize_mxfp4_rowwise(up)
    assert torch.equal(w.gate_up_c, interleave16(gc, uc)) and torch.equal(w.gate_up_e, interleave16(ge, ue))
    assert torch.equal(w.gate_up_s, interleave16(gs[:, None], us[:, None])[:, 0])
    with pytest.raises(ValueError):
        ops.quantize_dense_mlp_mxfp4(gu, down.t().contiguous())
    with pytest.raises(ValueError):
        ops.quantize_mxfp4_rowwise(torch.zeros(4, 48))


def test_a_column_shard_with_the_whole_rows_amax_gets_the_unsharded_codes():
    """``row_amax``: a K shard quantised with the whole row's amax holds the codes, exponents and scale the
    whole weight has in those columns; without it the shard's own amax gives other codes wherever the row's
    maximum lies outside the shard; an amax below the shard's own is refused."""
    _, _, down = _weights(seed=4)
    c, e, s = ops.quantize_mxfp4_rowwise(down)
    amax = down.float().abs().amax(dim=1)
    differs = False
    for lo, hi in ((0, 256), (256, 512)):
        part = down[:, lo:hi].contiguous()
        pc, pe, ps = ops.quantize_mxfp4_rowwise(part, row_amax=amax)
        assert torch.equal(pc, c[:, lo // 2:hi // 2]) and torch.equal(pe, e[:, lo // 32:hi // 32]) and torch.equal(ps, s)
        oc, oe, os_ = ops.quantize_mxfp4_rowwise(part)
        own = part.float().abs().amax(dim=1) == amax
        assert torch.equal(oc[own], pc[own]) and torch.equal(os_[own], ps[own])
        differs |= not torch.equal(oc, pc)
    assert differs
    with pytest.raises(ValueError, match="row_amax"):
        ops.quantize_mxfp4_rowwise(down[:, :256].contiguous(), row_amax=amax * 0.5)
    with pytest.raises(ValueError, match="row_amax"):
        ops.quantize_mxfp4_rowwise(down, row_amax=amax[:-1])


def test_pack_unpack_round_trip():
    g = torch.Generator().manual_seed(3)
    codes = torch.randint(0, 16, (7, 64), generator=g).to(torch.uint8)
    packed = mxfp4_dense.pack_codes(codes)
    assert packed.shape == (7, 32) and torch.equal(packed, D4.pack(codes))
    assert int(packed[0, 0]) == int(codes[0, 0]) | int(codes[0, 1]) << 4          # even k: the low nibble
    assert torch.equal(mxfp4_dense.unpack_codes(packed), codes)
    exps = torch.randint(119, 128, (7, 2), generator=g).to(torch.uint8)
    assert torch.equal(ops.unpack_mxfp4(packed, exps), D4.w_values(packed, exps))


# ------------------------------------------------------------------------------------------------
# expansion
# ------------------------------------------------------------------------------------------------
def test_expansion_is_exact_for_every_code_and_exponent():
    wc, we = D4.all_codes_and_exponents()
    q = ops.expand_mxfp4(wc, we)
    assert q.dtype == FP8 and q.shape == (144, 32)
    v = ops.unpack_mxfp4(wc, we)
    assert torch.equal(q.float(), v), "an e2m1 x 2^e value is not an e4m3 value"
    assert torch.equal(q.view(torch.uint8), v.to(FP8).view(torch.uint8))
    assert torch.equal(q.view(torch.uint8), D4.w_fp8(wc, we))
    u = q.view(torch.uint8)
    assert not bool(((u & 0x7F) == 0x7F).any())                     # never a NaN code
    neg0 = D4.unpack(wc) == 8
    assert bool((u[neg0] == 0x80).all()) and bool((u[D4.unpack(wc) == 0] == 0).all())
    assert float(v.abs().max()) == 6.0 and float(v.abs()[v != 0].min()) == 2.0 ** -9
    ws = torch.rand(144) + 0.5
    assert torch.equal(q.float() * ws[:, None], v * ws[:, None])    # times ws: the unpacked weight
    # e = -9 would not be exact: 1.5 * 2^-9 is no e4m3 value
    assert (torch.tensor(1.5 * 2.0 ** -9).to(FP8).float() != 1.5 * 2.0 ** -9)
    out = torch.full((144, 32), 0x55, dtype=torch.uint8)
    assert ops.expand_mxfp4(wc, we, out=out) is out and torch.equal(out, u)
    with pytest.raises(ValueError):
        ops.expand_mxfp4(wc, we, out=torch.empty((144, 16), dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------
# torch path
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 17, 300])
def test_torch_path_equals_the_reference(M):
    """The CPU path of ``mlp_mxfp4`` is the operation order of ``dense_mxfp4_reference(quant_act=True)``:
    equal bit for bit, the intermediate included; the reference is ``dense_fp8_reference`` on the unpacked
    weights; without the activation rounding it moves, by less than the e4m3 step allows."""
    gate, up, down = _weights(seed=1)
    w = ops.quantize_dense_mlp_mxfp4(interleave16(gate, up).contiguous(), down)
    h = torch.randn(M, 256, generator=torch.Generator().manual_seed(M)).bfloat16()
    assert mxfp4_dense.mlp_mxfp4_path(h, w) == "torch"
    y, a = ops.mlp_mxfp4(h, w, slabs=True)
    ref = ops.dense_mxfp4_reference(h, w, quant_act=True)
    assert y.dtype == torch.bfloat16 and y.shape == (M, 256) and a.shape == (M, 512) and a.dtype == torch.bfloat16
    assert torch.equal(y, ref)
    as_fp8 = ops.DenseFp8MLP(D4.w_fp8(w.gate_up_c, w.gate_up_e).view(FP8), w.gate_up_s,
                             D4.w_fp8(w.down_c, w.down_e).view(FP8), w.down_s)
    assert torch.equal(ref, ops.dense_fp8_reference(h, as_fp8, quant_act=True))
    x = ops.moe._fake_quant_rows(h.float())
    w13 = _dequant(w.gate_up_c, w.gate_up_e, w.gate_up_s)
    assert torch.equal(a, ops.silu_mul((x @ w13.t()).to(torch.bfloat16), interleave16=True))
    plain = ops.dense_mxfp4_reference(h, w, quant_act=False)
    rel = (plain.float() - ref.float()).norm(dim=1) / ref.float().norm(dim=1)
    assert 0 < float(rel.max()) < 0.25, float(rel.max())


# ------------------------------------------------------------------------------------------------
# config table
# ------------------------------------------------------------------------------------------------
PRODUCTION = [(28672, 4096), (4096, 14336), (57344, 8192), (8192, 28672), (7168, 8192), (8192, 3584)]


def test_every_table_entry_satisfies_the_kernel_contract():
    """DENSE_MXFP4 covers the 8B, 70B and 70B TP=8 MLP shapes; every entry, at every M it is chosen for and
    for every epilogue, is inside ``penny_dense_mxfp4_gemm``'s checked contract: ntf in {2, 4}, N a multiple
    of 16 ntf, K a multiple of 256 S, 1 <= S <= 16, S = 1 unless the output is slabs; rows are ordered by
    max M and end at 256."""
    for shape in PRODUCTION:
        assert shape in mxfp4_dense.DENSE_MXFP4, shape
    for (N, K), rows in mxfp4_dense.DENSE_MXFP4.items():
        assert [r[0] for r in rows] == sorted(r[0] for r in rows) and rows[-1][0] == mxfp4_dense.MAX_M, (N, K)
        for M in range(1, 257):
            want = next((S, ntf) for max_m, S, ntf in rows if M <= max_m)
            for epi in ("silu", "bf16", "slabs"):
                S, ntf = mxfp4_dense.dense_mxfp4_config(M, N, K, epi)
                assert ntf == want[1] and S == (want[0] if epi == "slabs" else 1), (M, N, K, epi)
                assert ntf in (2, 4) and N % (16 * ntf) == 0 and K % (256 * S) == 0 and 1 <= S <= mxfp4_dense.MAX_S
    assert mxfp4_dense.dense_mxfp4_config(257, 4096, 14336, "slabs") is None
    assert mxfp4_dense.dense_mxfp4_config(0, 4096, 14336, "slabs") is None
    assert mxfp4_dense.dense_mxfp4_config(16, 4096, 14336 + 128, "slabs") is None       # K % 256
    assert mxfp4_dense.dense_mxfp4_config(16, 4096 + 16, 14336, "slabs") is None
    for N, K in ((1024, 256), (256, 512), (32, 256)):               # unmeasured shapes: the default
        S, ntf = mxfp4_dense.dense_mxfp4_config(64, N, K, "slabs")
        assert ntf == 2 and K % (256 * S) == 0 and mxfp4_dense.dense_mxfp4_config(64, N, K, "silu") == (1, 2)
    assert mxfp4_dense.dense_mxfp4_config(64, 256, 384, "bf16") is None                 # a multiple of 128 only


def test_table_entries_name_a_profile_that_has_their_shape():
    """Every table shape was measured: profiles/dense_mxfp4_mlp.jsonl holds rows for it."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dense_mxfp4_mlp.jsonl")
    seen = set()
    with open(path) as fh:
        for line in fh:
            row = json.loads(line)
            for key in ("gate_up", "down"):
                if key in row:
                    seen.add(tuple(row[key]["shape"]))
    for shape in mxfp4_dense.DENSE_MXFP4:
        assert shape in seen, f"{shape} has a table entry and no row in {path}"


# ------------------------------------------------------------------------------------------------
# configuration
# ------------------------------------------------------------------------------------------------
def test_config_env_flag_and_bad_values(monkeypatch):
    monkeypatch.delenv("PENNY_MLP_DTYPE", raising=False)
    assert EngineConfig().mlp_dtype == "bf16"
    assert EngineConfig(mlp_dtype="mxfp4").mlp_dtype == "mxfp4"
    monkeypatch.setenv("PENNY_MLP_DTYPE", "mxfp4")
    assert EngineConfig().mlp_dtype == "mxfp4" and EngineConfig.from_env().mlp_dtype == "mxfp4"
    assert EngineConfig.from_env(mlp_dtype="fp8").mlp_dtype == "fp8"
    from financial_chatbot_llm_amd.serving import launch
    assert launch.parse([]).mlp_dtype == "mxfp4"
    assert launch.parse(["--mlp-dtype", "bf16"]).mlp_dtype == "bf16"
    monkeypatch.delenv("PENNY_MLP_DTYPE")
    assert launch.parse(["--mlp-dtype", "mxfp4"]).mlp_dtype == "mxfp4"
    for bad in ("fp4", "int4", "nf4"):
        with pytest.raises(ValueError, match="mlp_dtype"):
            EngineConfig(mlp_dtype=bad)
        monkeypatch.setenv("PENNY_MLP_DTYPE", bad)
        with pytest.raises(ValueError, match="mlp_dtype"):
            EngineConfig()
        monkeypatch.delenv("PENNY_MLP_DTYPE")


def test_build_model_quantises_llama_and_refuses_mixtral():
    m = build_model(EngineConfig(model="llama-tiny", device="cpu", mlp_dtype="mxfp4"), torch.device("cpu"))
    ref = build_model(EngineConfig(model="llama-tiny", device="cpu"), torch.device("cpu"))
    c = m.cfg
    assert m.mlp_dtype == "mxfp4" and ref.mlp_dtype == "bf16" and not ref.mlp_q
    assert not any(k.endswith((".gate_up", ".down")) for k in m.w) and not any(k.endswith((".gate_up", ".down")) for k in m.wt)
    per_layer = 3 * c.hidden_size * c.intermediate_size
    resident = per_layer // 2 + per_layer // 32 + 4 * (2 * c.intermediate_size + c.hidden_size)
    assert ref.num_bytes() - m.num_bytes() == c.num_layers * (per_layer * 2 - resident)      # no scratch on the CPU
    w0 = ops.quantize_dense_mlp_mxfp4(ref.w["layers.0.gate_up"], ref.w["layers.0.down"])
    assert torch.equal(m.mlp_q[0].gate_up_c, w0.gate_up_c) and torch.equal(m.mlp_q[0].down_e, w0.down_e)
    assert m.w["layers.0.down_c"] is m.mlp_q[0].down_c and m.w["layers.0.gate_up_scale"] is m.mlp_q[0].gate_up_s
    for key in ("gate_up_c", "gate_up_e", "gate_up_scale", "down_c", "down_e", "down_scale"):
        assert f"layers.1.{key}" in m.w
    assert m.quantize_mlp("mxfp4") is m                             # already there: no-op
    with pytest.raises(ValueError, match="already quantised"):
        m.quantize_mlp("fp8")
    with pytest.raises(ValueError, match="already quantised"):
        build_model(EngineConfig(model="llama-tiny", device="cpu", mlp_dtype="fp8"), torch.device("cpu")).quantize_mlp("mxfp4")
    with pytest.raises(ValueError, match="mlp_dtype"):
        ref.quantize_mlp("int4")
    with pytest.raises(ValueError, match="dtype='fp8'"):
        build_model(EngineConfig(model="mixtral-tiny", device="cpu", mlp_dtype="mxfp4"), torch.device("cpu"))
    from financial_chatbot_llm_amd.models.mixtral import MixtralModel
    with pytest.raises(ValueError, match="dtype='fp8'"):
        MixtralModel(get_model_config("mixtral-tiny"), device="cpu", tp_rank=0, tp_size=1).init_random(seed=0).quantize_mlp("mxfp4")


def test_engine_reports_mlp_dtype_and_switch_off_is_the_old_path():
    from financial_chatbot_llm_amd.engine import LLMEngine, SamplingParams
    base = dict(model="llama-tiny", device="cpu", num_kv_blocks=32, max_model_len=512, use_cuda_graph=False)
    sp = SamplingParams(temperature=0.0, max_tokens=4, ignore_eos=True)
    off = LLMEngine(EngineConfig(**base))
    assert off.stats()["mlp_dtype"] == "bf16" and "layers.0.gate_up" in off.model.w and not off.model.mlp_q
    called = []
    real = ops.mlp_mxfp4
    try:
        ops.mlp_mxfp4 = lambda *a, **k: (called.append(1), real(*a, **k))[1]
        out_off = off.generate([list(range(5, 40))], sp)
        assert not called
        on = LLMEngine(EngineConfig(mlp_dtype="mxfp4", **base))
        assert on.stats()["mlp_dtype"] == "mxfp4"
        out_on = on.generate([list(range(5, 40))], sp)
        assert called and len(out_on[0]) == len(out_off[0]) == 4
    finally:
        ops.mlp_mxfp4 = real


# ------------------------------------------------------------------------------------------------
# the exact cases against a plain model of the kernel
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,S", [(32, 256, 1), (64, 512, 2), (64, 1024, 4)])
def test_exact_cases_agree_with_a_plain_torch_model(N, K, S):
    """The expectations the GPU tests compare bits with equal an f64 matmul model of the contract on the
    unpacked weights, for both kinds of exact case and all three epilogues; the one-hot calls cover every
    required column, with non-zero block exponents and every code (-0 included) in W."""
    M = 17
    cols = D4.required_columns(K, S)
    assert set(range(256)) <= set(cols) and set(range(K - 256, K)) <= set(cols)
    for b in list(range(256, K, 256)) + [s * K // S for s in range(1, S)]:
        assert {b - 1, b} <= set(cols)
    cases = D4.onehot_cases(M, N, K, S, seed=5)
    hit = set()
    for case in cases:
        x = D4.values_of(case.xq[:M, :K].contiguous())
        assert bool(((x != 0).sum(1) == 1).all())
        hit |= set((x != 0).nonzero()[:, 1].tolist())
    assert hit == set(cols)
    w = cases[0]
    assert set(D4.unpack(w.wc).flatten().tolist()) == set(range(16))
    assert set(w.we.flatten().tolist()) == set(range(119, 128))
    assert torch.equal(D4.values_of(w.wq), D4.w_values(w.wc, w.we))
    cases = cases[::5] + [D4.few_term_case(M, N, K, S, seed=3), D4.few_term_case(M, N, K, S, seed=4, silu=True)]
    for case in cases:
        nnz = (D4.values_of(case.xq[:M, :K].contiguous()) != 0).sum(1)
        assert int(nnz.max()) <= 4 and int(nnz.min()) >= 1
        assert bool((case.xq[M:] == D4.NAN_CODE).all()) and bool(torch.isnan(case.xs[M:]).all())
        assert case.xs.data_ptr() % 16 == 0
        for epi in ("silu", "bf16", "slabs"):
            s_ = S if epi == "slabs" else 1
            want, model = D4.expected(case, epi, s_, ops.silu_mul), D4.emulate(case, epi, s_, ops.silu_mul)
            assert torch.equal(D4.bits(want), D4.bits(model)), (epi, N, K)
            ref = D4.reference_f64(case, epi, s_)
            assert bool(((want.double() - ref.ref).abs() <= ref.bound).all()), (epi, N, K)
    few = cases[-2]
    wv = D4.w_values(few.wc, few.we)
    assert torch.equal(wv, wv.round()) and float(wv.abs().max()) == 6.0            # integer W
    slabs = D4.expected(few, "slabs", S, ops.silu_mul)
    assert int((slabs != 0).any(-1).any(-1).sum()) == S            # every K slice holds terms


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
        tp = LlamaModel(cfg, device="cpu", dtype=torch.float32).init_random(seed=7).quantize_mlp("mxfp4")
        assert tp.mlp_q[0].down_c.shape == (cfg.hidden_size, cfg.intermediate_size // world // 2)
        one = LlamaModel(cfg, device="cpu", tp_rank=0, tp_size=1, dtype=torch.float32).init_random(seed=7).quantize_mlp("mxfp4")
        Fs = cfg.intermediate_size // world
        for i in (0, cfg.num_layers - 1):
            full, mine = one.mlp_q[i], tp.mlp_q[i]
            assert torch.equal(mine.down_c, full.down_c[:, rank * Fs // 2:(rank + 1) * Fs // 2])
            assert torch.equal(mine.down_e, full.down_e[:, rank * Fs // 32:(rank + 1) * Fs // 32])
            assert torch.equal(mine.down_s, full.down_s)
        q.put((rank, to_np(_prefill_logits(tp, IDS)), None))
        shutdown()
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, "ERR", traceback.format_exc()))


@pytest.mark.timeout(300)
def test_tp2_mxfp4_logits_close_to_tp1():
    """Each rank quantises its own shard (down's blocks and activation scale are per shard): TP = 2 is close
    to TP = 1, not bit-equal.  Criterion: the fp8 gloo test's, max error < 0.05 x max |reference|.

    down is sharded along K, and its row scale is the whole row's (the maximum of the ranks' shard amax), so
    every rank holds exactly the codes, exponents and scales TP = 1 has in its columns (checked in the worker);
    what is left is the per-shard activation scale of the down GEMM, as for fp8.  With per-shard row scales the
    two quantisations of down differ and the same comparison gives 8.27e-2 against the bound 7.89e-2."""
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
    ref = _prefill_logits(one.quantize_mlp("mxfp4"), IDS)
    scale = ref.abs().max().item()
    for r in range(world):
        err = (res[r] - ref).abs().max().item()
        print(f"rank {r}: max |tp2 - tp1| = {err:.4e}, 0.05 x max |ref| = {0.05 * scale:.4e}")
        assert err < 0.05 * scale
    assert torch.equal(res[0], res[1])
    q_err = (ref - bf16).abs().max().item()
    print(f"max |mxfp4 - bf16| = {q_err:.4e} of max |bf16| = {bf16.abs().max().item():.4e}")
    assert q_err > 0
