"""Prompt scoring on the GPU: the fused LM-head log-likelihood kernel (gemm_prefill.hip EPI_LOGPROB +
its merge kernel), the cross-shard merge, and ``LLMEngine.score`` end to end.

The kernel accumulates exactly like the bf16 tile GEMM, so against ``gemm.prefill_gemm`` logits the
row maximum, the target logit and the argmax are exact, and only log(sum exp) carries f32 rounding.
LOGPROB_TOL is derived, not tuned: both maxima are exact; the sum passes through at most ~56 f32
additions (32 per lane, 2 shuffles, <= 16 + 6 in the merge) and __expf's argument rounding
(<= 4e-6 relative), so log S is good to about 2e-5 and 1e-4 nats leaves a 5x margin.
"""
import dataclasses

import pytest
import torch

from financial_chatbot_llm_amd import ops
from financial_chatbot_llm_amd.ops import gemm

pytestmark = pytest.mark.gpu
DEV = "cuda"
LOGPROB_TOL = 1e-4
F32_EVAL_TOL = 1e-5      # two f32 evaluations of the same tl - Mx - log S (see the first test)
NEG_INF = float("-inf")


def rnd(*shape, scale=1.0, dtype=torch.bfloat16, gen=None):
    return (torch.randn(*shape, generator=gen) * scale).to(dtype)


def _targets(M, V, gen):
    """Target vectors for M rows: column 0, column V-1, the lane-map seams 127 / 128 / 255 / 256 and
    'no target' (-1) all occur; the other rows are random.  Fewer than 7 rows: one vector per
    rotation, so every special value is still scored."""
    special = [0, V - 1, 127, 128, 255, 256, -1]
    out = []
    for rot in range(1 if M >= len(special) else len(special)):
        t = torch.randint(0, V, (M,), generator=gen, dtype=torch.int32)
        for i in range(min(M, len(special))):
            t[i] = special[(i + rot) % len(special)]
        if M > 40:
            t[-1], t[-2] = V - 1, -1          # the last token tile's rows too
        out.append(t)
    return out


def _unpack(stats):
    return stats[:, 0], stats[:, 1], stats[:, 2], stats.contiguous().view(torch.int32)[:, 3]


def _gathered(logits, tg, col0=0):
    """(target logit f32 with -inf where absent, log-softmax at the target in f64) from logits of
    the global columns col0 .. col0 + width - 1."""
    V = logits.shape[1]
    loc = tg.long() - col0
    inside = (tg >= 0) & (loc >= 0) & (loc < V)
    idx = loc.clamp(0, V - 1)[:, None]
    tl = torch.where(inside, logits.float().gather(1, idx)[:, 0], torch.full((len(tg),), NEG_INF, device=logits.device))
    lp = torch.log_softmax(logits.double(), -1).gather(1, idx)[:, 0]
    return tl, torch.where(inside, lp, torch.full_like(lp, NEG_INF))


def _greedy(logits):
    M = logits.shape[0]
    return ops.sample(logits, torch.zeros(M, device=DEV), torch.zeros(M, dtype=torch.int64, device=DEV))


@pytest.mark.parametrize("M,V,K", [(1, 2048, 512), (37, 4096, 1024), (256, 2048, 512), (300, 1024, 256),
                                   (128, 128256, 4096)])
def test_fused_logprob_matches_logits_then_log_softmax(M, V, K):
    g = torch.Generator().manual_seed(M + V)
    x, w = rnd(M, K, gen=g).to(DEV), rnd(V, K, scale=0.05, gen=g).to(DEV)
    assert ops.fused_logprob_ok(x, w)
    logits = gemm.prefill_gemm(x, w)
    want_top1 = _greedy(logits)
    for tg in _targets(M, V, g):
        tg = tg.to(DEV)
        stats = ops.lm_head_logprobs(x, w, tg, return_stats=True)
        lp = ops.lm_head_logprobs(x, w, tg)
        mx, s, tl, top1 = _unpack(stats)
        want_tl, want_lp = _gathered(logits, tg)
        assert torch.equal(mx, logits.float().max(-1).values)
        assert torch.equal(tl, want_tl)
        assert torch.equal(top1, want_top1)
        has = tg >= 0
        err = (lp[has].double() - want_lp[has]).abs().max().item() if bool(has.any()) else 0.0
        print(f"M={M} V={V} K={K}: max |logprob - f64 log_softmax| = {err:.3e}")
        assert err <= LOGPROB_TOL
        assert bool((lp[~has] == NEG_INF).all())
        # the kernel's own logprob and the stats formula agree: two f32 evaluations of tl - Mx - log S
        # with |values| < 32 (half an ulp, 1.9e-6, per subtraction, logf vs torch.log within 2 ulp of 12)
        assert torch.allclose(lp[has], (tl - mx - torch.log(s))[has], atol=F32_EVAL_TOL, rtol=0)
        if M > 1:   # batch invariance: row 1 alone is bit-equal to row 1 in the batch
            one = ops.lm_head_logprobs(x[1:2].contiguous(), w, tg[1:2].contiguous(), return_stats=True)
            assert torch.equal(one.view(torch.int32), stats[1:2].contiguous().view(torch.int32))


def test_fused_logprob_vocab_shard():
    """Vpad = 1024, vvalid = 800, voff = 12345: the wave half of columns 768..895 holds 32 valid
    columns, the half 896..1023 none.  Stats equal the full computation over w[:800]; targets
    outside the shard (below voff, in the padding, past it) give tl = -inf."""
    M, Vpad, vvalid, voff, K = 70, 1024, 800, 12345, 256
    g = torch.Generator().manual_seed(5)
    x, w = rnd(M, K, gen=g).to(DEV), rnd(Vpad, K, scale=0.05, gen=g).to(DEV)
    tg = torch.randint(voff, voff + vvalid, (M,), generator=g, dtype=torch.int32)
    tg[:9] = torch.tensor([voff, voff + vvalid - 1, voff + 767, voff + 768, voff + vvalid, voff + Vpad - 1,
                           voff - 1, 0, -1], dtype=torch.int32)
    tg = tg.to(DEV)
    stats = ops.lm_head_logprobs(x, w, tg, vvalid=vvalid, voff=voff, return_stats=True)
    mx, s, tl, top1 = _unpack(stats)
    logits = gemm.prefill_gemm(x, w)[:, :vvalid].contiguous()
    want_tl, want_lp = _gathered(logits, tg, col0=voff)
    assert torch.equal(mx, logits.float().max(-1).values)
    assert torch.equal(tl, want_tl)
    assert bool((tl[4:9] == NEG_INF).all()) and bool(torch.isfinite(tl[:4]).all())
    assert torch.equal(top1, _greedy(logits) + voff)
    has = torch.isfinite(want_tl)
    got_lp = (tl - mx - torch.log(s)).double()
    assert (got_lp[has] - want_lp[has]).abs().max().item() <= LOGPROB_TOL


def test_two_shards_merge_to_single_shard():
    """V = 2048 split into 1000 + 1048 rows, each padded to a multiple of 256."""
    M, V, K = 70, 2048, 512
    g = torch.Generator().manual_seed(11)
    x, w = rnd(M, K, gen=g).to(DEV), rnd(V, K, scale=0.05, gen=g).to(DEV)
    tg = _targets(M, V, g)[0]
    tg[7:11] = torch.tensor([999, 1000, 1001, 2047], dtype=torch.int32)      # the shard seam
    tg = tg.to(DEV)
    single_lp, single_top1 = ops.merge_logprob_stats(ops.lm_head_logprobs(x, w, tg, return_stats=True)[None])
    parts = []
    for lo, hi in ((0, 1000), (1000, 2048)):
        pad = torch.zeros((-(-(hi - lo) // 256) * 256, K), dtype=w.dtype, device=DEV)
        pad[:hi - lo] = w[lo:hi]
        parts.append(ops.lm_head_logprobs(x, pad, tg, vvalid=hi - lo, voff=lo, return_stats=True))
    lp, top1 = ops.merge_logprob_stats(torch.stack(parts))
    assert torch.equal(top1, single_top1)
    has = tg >= 0
    assert (lp[has] - single_lp[has]).abs().max().item() <= LOGPROB_TOL
    assert bool((lp[~has] == NEG_INF).all())
    assert torch.allclose(single_lp[has], ops.lm_head_logprobs(x, w, tg)[has], atol=F32_EVAL_TOL, rtol=0)


def test_reference_path_on_device_matches_fused(monkeypatch):
    """PENNY_FUSED_LOGPROB=0 takes linear -> log-softmax on the device and yields the same stats layout."""
    M, V, K = 37, 4096, 1024
    g = torch.Generator().manual_seed(3)
    x, w = rnd(M, K, gen=g).to(DEV), rnd(V, K, scale=0.05, gen=g).to(DEV)
    tg = _targets(M, V, g)[0].to(DEV)
    fused = ops.lm_head_logprobs(x, w, tg)
    monkeypatch.setenv("PENNY_FUSED_LOGPROB", "0")
    assert not ops.fused_logprob_ok(x, w)
    ref = ops.lm_head_logprobs(x, w, tg)
    st = ops.lm_head_logprobs(x, w, tg, return_stats=True)
    assert st.shape == (M, 4) and st.dtype == torch.float32
    has = tg >= 0
    # two GEMM kernels with their own accumulation orders: a logit can land on the neighbouring bf16
    # value.  |l| < 8 here (one bf16 ulp in [4, 8) is 2^-5); the target logit and the log-sum-exp
    # each move by at most one ulp
    assert float(_unpack(st)[0].abs().max()) < 8
    assert (fused[has] - ref[has]).abs().max().item() <= 2 * 2 ** -5
    assert bool((ref[~has] == NEG_INF).all())


# ------------------------------------------------------------------------------------------------
# end to end: LLMEngine.score on the tiny Llama
# ------------------------------------------------------------------------------------------------
# Drift already present on this engine between runner.forward_logits -> f32 log_softmax run in one
# chunk and run in 64-token chunks on the prompts below (same attention and GEMM paths, none of the
# scoring code), measured on an MI355X: max |delta logprob| = 1.9712e-3 nats (a bf16 hidden state
# landing on the neighbouring value moves a logit by one bf16 ulp).  The tests below allow twice that.
# Measured with the scoring code: fused vs reference 9.5e-7, 64-token chunks vs one chunk 1.9712e-3.
E2E_DRIFT = 1.9712448e-3


def _prompts():
    g = torch.Generator().manual_seed(2024)
    return [torch.randint(0, 128256, (n,), generator=g).tolist() for n in (200, 333)]


@pytest.fixture(scope="module")
def tiny_engine():
    from financial_chatbot_llm_amd.config import EngineConfig
    from financial_chatbot_llm_amd.engine import LLMEngine
    cfg = EngineConfig(model="llama-tiny", device="cuda", num_kv_blocks=64, max_model_len=1024, max_num_seqs=4,
                       max_num_batched_tokens=1024, use_cuda_graph=False)
    return LLMEngine(cfg)


def _score_all(eng, chunk):
    eng.cfg = dataclasses.replace(eng.cfg, max_num_batched_tokens=chunk)
    return torch.cat([torch.tensor(eng.score(p).logprobs) for p in _prompts()])


def test_engine_score_fused_matches_reference_and_chunked(tiny_engine, monkeypatch):
    """LLMEngine.score with the fused kernel vs PENNY_FUSED_LOGPROB=0, and 64-token chunks (4 and 6
    chunks) vs one chunk, each within 2 x E2E_DRIFT = 3.94e-3 nats, E2E_DRIFT = 1.9712e-3 being the
    drift of forward_logits -> f32 log_softmax between the same two chunkings without any scoring
    code (measured: fused vs reference 9.5e-7, chunked vs one chunk 1.9712e-3)."""
    from financial_chatbot_llm_amd.ops import _native
    eng = tiny_engine
    calls = []
    real = _native.call
    monkeypatch.setattr(_native, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    free = eng.bm.num_free()
    fused = _score_all(eng, 1024)
    assert calls.count("penny_lm_head_logprob") == 2          # one chunk per prompt, on the tile kernel
    monkeypatch.setenv("PENNY_FUSED_LOGPROB", "0")
    ref = _score_all(eng, 1024)
    assert calls.count("penny_lm_head_logprob") == 2
    monkeypatch.delenv("PENNY_FUSED_LOGPROB")
    chunked = _score_all(eng, 64)
    assert calls.count("penny_lm_head_logprob") == 2 + 4 + 6
    assert eng.bm.num_free() == free and len(fused) == 199 + 332
    assert bool(torch.isfinite(fused).all())
    d_ref, d_chunk = (fused - ref).abs().max().item(), (fused - chunked).abs().max().item()
    print(f"fused vs reference {d_ref:.3e}, chunked vs one chunk {d_chunk:.3e}, bound {2 * E2E_DRIFT:.3e}")
    assert d_ref <= 2 * E2E_DRIFT
    assert d_chunk <= 2 * E2E_DRIFT
