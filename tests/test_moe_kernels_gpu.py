"""Per-row tests of the fp8 sparse-MoE pipelines (``moe.hip``, the grouped fp8 tile GEMMs of
``gemm_prefill.hip``) against the float64 certificates of ``moe_ref`` (run on MI355X).

Routing is FORCED: the logits put chosen numbers of (token, expert) pairs into each bucket, so the
bucket bounds sit on the kernels' own edges (64-pair chunks of ``moe_gemm_kernel``, 256-row tiles
of the tile kernel).  Every pipeline is run stage by stage through ``_native.call`` on the test's
own buffers, each stage is checked against a reference of THAT stage computed from the kernel's own
inputs, the wrapper in ``ops/moe.py`` must give the same bits (twice: repeatability), and every
token's output row is compared with ``moe_fp8_reference``.

Each test prints its figures (``MOEFIG ...``: largest error / bound per certificate, largest
per-token ratio) before it asserts.
"""
import functools
from collections import namedtuple

import numpy as np
import pytest
import torch

from financial_chatbot_llm_amd.ops import _native as N
from financial_chatbot_llm_amd.ops import gemm, moe
from moe_ref import (PER_TOKEN_LIMIT, acc_units, check_buckets, check_mx_intermediate, check_per_token, check_within,
                     combine_ref, expert_of_pos, fp8_f64, gemm1_silu_ref, gemm2_ref, mx_decode, mx_scale_exponents, pipeline_ref,
                     route_ref)

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
I32 = dict(dtype=torch.int32, device=DEV)
F32 = dict(dtype=torch.float32, device=DEV)

Bank = namedtuple("Bank", "q13 s13 q2 s2 q13d s13d q2d s2d w13t w2t")


@functools.lru_cache(maxsize=None)
def bank(E, H, F_):
    """Quantised experts (CPU copies for the references; row-major and fragment-tiled on the GPU)."""
    g = torch.Generator().manual_seed(1000 * E + H + F_)
    w13 = (torch.randn(E, 2 * F_, H, generator=g) * 0.05).to(BF)
    w2 = (torch.randn(E, H, F_, generator=g) * 0.05).to(BF)
    w13i = torch.stack([gemm.interleave16(w13[e, :F_], w13[e, F_:]) for e in range(E)])
    q13, s13 = moe.quantize_fp8_rowwise(w13i)
    q2, s2 = moe.quantize_fp8_rowwise(w2)
    s13, s2 = s13.float().contiguous(), s2.float().contiguous()
    q13d, q2d = q13.to(DEV).contiguous(), q2.to(DEV).contiguous()
    return Bank(q13, s13, q2, s2, q13d, s13.to(DEV), q2d, s2.to(DEV), moe.tile_fp8_weight(q13d), moe.tile_fp8_weight(q2d))


# bucket sizes (pairs per expert), K = 2.  The eight edge sizes sum to 961, which no K = 2 routing can
# give (T*K is even): a ninth expert takes 31 pairs, so all eight sizes sit in one case
CASES = {
    "edges": (0, 1, 63, 64, 65, 255, 256, 257, 31),
    "two_experts": (0, 0, 700, 0, 0, 700, 0, 0),
    "one_empty": (40, 40, 40, 0, 40, 40, 40, 40),
}
K = 2
DECODE_SHAPE = (512, 384)      # H, F of the decode-shaped kernels' tests
TILE_SHAPE = (1024, 1536)      # ... of the tile kernel's


@functools.lru_cache(maxsize=None)
def forced(case, H):
    """-> (h [T, H] bf16, logits [T, E] bf16), CPU: every token's two largest logits sit on the
    experts that give the case's bucket sizes (greedy pairing of the two fullest buckets)."""
    counts = CASES[case]
    E, T = len(counts), sum(counts) // K
    rem, pairs = list(counts), []
    for _ in range(T):
        a, b = sorted(range(E), key=lambda e: -rem[e])[:2]
        assert rem[b] > 0
        pairs.append((a, b))
        rem[a] -= 1
        rem[b] -= 1
    g = torch.Generator().manual_seed(len(case) + H)
    lg = torch.randn(T, E, generator=g) * 0.5
    top = torch.rand(T, 2, generator=g) * 0.5
    for t, (a, b) in zip(torch.randperm(T, generator=g).tolist(), pairs):
        lg[t, a], lg[t, b] = 8.0 + top[t, 0], 7.0 + top[t, 1]
    lg = lg.to(BF)
    assert np.bincount(route_ref(lg, K).ids.reshape(-1), minlength=E).tolist() == list(counts)
    return torch.randn(T, H, generator=g).to(BF), lg


def fig(name, **kv):
    print("MOEFIG", name, " ".join(f"{k}={v:.4g}" for k, v in kv.items()), flush=True)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


# ---------------------------------------------------------------------------------------------
# the pipelines, stage by stage on the test's own buffers
# ---------------------------------------------------------------------------------------------
def run_stages(h, b, route, gemm_kind, logits=None, ids=None, mx=False, sched=0, top_k=K):
    """route: "decode" (penny_moe_route + quant_rows), "prefill" (penny_moe_route_quant) or
    "grouped" (rows tagged with an expert id, -1 = padding; sorted as moe_grouped_fp8 does);
    gemm_kind: "decode" (moe_gemm_kernel) or "tiles" (gemm_prefill.hip; ``mx``: the MX hand-off,
    ``sched``: 16 = the plain fragment-read schedule).  -> every stage's tensors."""
    T, H = h.shape
    E, F2 = b.s13.shape
    F_ = F2 // 2
    st = N.stream()
    r = dict(T=T, E=E, K=top_k, F=F_, mx=mx, route=route)
    xq = torch.zeros((T, H), dtype=torch.uint8, device=DEV)
    xs = torch.zeros(T, **F32)
    if route == "grouped":
        P = T
        idl = ids.long()
        key = torch.where(idl >= 0, idl, torch.full_like(idl, E))
        order = torch.argsort(key, stable=True)
        counts = torch.zeros(E + 1, **I32)
        counts.scatter_add_(0, key, torch.ones_like(key, dtype=torch.int32))
        offsets = torch.zeros(E + 1, **I32)
        offsets[1:] = counts[:E].cumsum(0)
        rows, w, inv = order.to(torch.int32), torch.ones(P, **F32), None
        r["order"] = order
        N.call("penny_quant_rows_fp8", N.ptr(h), h.stride(0), T, H, N.ptr(xq), N.ptr(xs), st)
    else:
        P = T * top_k
        rows, w, inv, offsets = torch.zeros(P, **I32), torch.zeros(P, **F32), torch.zeros(P, **I32), torch.zeros(E + 1, **I32)
        if route == "decode":
            N.call("penny_moe_route", N.ptr(logits), T, E, top_k, N.ptr(rows), N.ptr(w), N.ptr(offsets), N.ptr(inv), st)
            N.call("penny_quant_rows_fp8", N.ptr(h), h.stride(0), T, H, N.ptr(xq), N.ptr(xs), st)
        else:
            pe, pw = torch.zeros(P, **I32), torch.zeros(P, **F32)
            N.call("penny_moe_route_quant", N.ptr(h), h.stride(0), N.ptr(logits), T, H, E, top_k, N.ptr(xq), N.ptr(xs),
                   N.ptr(pe), N.ptr(pw), N.ptr(rows), N.ptr(w), N.ptr(offsets), N.ptr(inv), st)
            r.update(pe=pe, pw=pw)
    a = torch.zeros((P, F_), dtype=BF, device=DEV)
    aq = torch.zeros((P, F_), dtype=torch.uint8, device=DEV)
    as_ = torch.zeros(P, **F32)
    y2 = torch.zeros((P, H), dtype=BF, device=DEV)
    if gemm_kind == "decode":
        ntf13, ntf2 = moe.MOE_NTF
        N.call("penny_moe_gemm_fp8", N.ptr(xq), N.ptr(xs), N.ptr(rows), N.ptr(offsets), N.ptr(b.w13t), N.ptr(b.s13d),
               None, N.ptr(a), E, F2, H, 1, ntf13, st)
        N.call("penny_quant_rows_fp8", N.ptr(a), F_, P, F_, N.ptr(aq), N.ptr(as_), st)
        N.call("penny_moe_gemm_fp8", N.ptr(aq), N.ptr(as_), None, N.ptr(offsets), N.ptr(b.w2t), N.ptr(b.s2d), N.ptr(w),
               N.ptr(y2), E, H, F_, 2, ntf2, st)
    elif mx:
        nkt = F_ // 128
        mxs = torch.zeros((((P + 255) // 256 + E) * nkt * 256,), **I32)
        N.call("penny_moe_gemm_prefill_fp8_mx", N.ptr(xq), H, N.ptr(rows), N.ptr(xs), N.ptr(offsets), N.ptr(b.q13d),
               N.ptr(b.s13d), None, N.ptr(aq), F_, P, E, F2, H, 10, N.ptr(mxs), nkt, st)
        N.call("penny_moe_gemm_prefill_fp8_mx", N.ptr(aq), F_, None, None, N.ptr(offsets), N.ptr(b.q2d), N.ptr(b.s2d),
               N.ptr(w), N.ptr(y2), H, P, E, H, F_, 11, N.ptr(mxs), nkt, st)
        r["mxs"] = mxs
    else:
        N.call("penny_moe_gemm_prefill_fp8", N.ptr(xq), H, N.ptr(rows), N.ptr(xs), N.ptr(offsets), N.ptr(b.q13d),
               N.ptr(b.s13d), None, N.ptr(a), F_, P, E, F2, H, 7 + sched, st)
        N.call("penny_quant_rows_fp8", N.ptr(a), F_, P, F_, N.ptr(aq), N.ptr(as_), st)
        N.call("penny_moe_gemm_prefill_fp8", N.ptr(aq), F_, None, N.ptr(as_), N.ptr(offsets), N.ptr(b.q2d), N.ptr(b.s2d),
               N.ptr(w), N.ptr(y2), H, P, E, H, F_, 8 + sched, st)
    if inv is not None:
        out = torch.zeros((T, H), dtype=BF, device=DEV)
        N.call("penny_moe_combine", N.ptr(y2), N.ptr(inv), T, top_k, H, N.ptr(out), st)
    else:
        out = torch.empty_like(y2)
        out.index_copy_(0, order, y2)
    torch.cuda.synchronize()
    r.update(P=P, xq=xq, xs=xs, rows=rows, w=w, inv=inv, offsets=offsets, a=a, aq=aq, as_=as_, y2=y2, out=out)
    return r


def certify(name, r, b, logits=None):
    """Every stage certificate on the tensors of :func:`run_stages`."""
    T, E, P, F_, top_k = r["T"], r["E"], r["P"], r["F"], r["K"]
    figs = {}
    if r["route"] != "grouped":
        figs["weights"] = check_buckets(r["offsets"], r["rows"], r["w"], r["inv"], route_ref(logits, top_k), T, E, top_k)
    inb = expert_of_pos(r["offsets"], P) < E                     # rows inside a bucket (padding sorts last)
    ref, bound = gemm1_silu_ref(r["xq"], r["xs"], r["rows"], r["offsets"], b.q13, b.s13)
    if r["mx"]:
        X = mx_scale_exponents(r["mxs"], r["offsets"], P, E, F_)
        figs["gemm1"] = check_mx_intermediate(r["aq"], X, ref, bound, rows=inb)
        a64, a_scale = mx_decode(r["aq"], X), None
    else:
        figs["gemm1"] = check_within(r["a"], ref, bound, "GEMM1 + SiLU")
        a64, a_scale = fp8_f64(r["aq"]), r["as_"]
    a64[torch.as_tensor(~inb)] = 0.0
    ref, bound, ssc = gemm2_ref(a64, a_scale, r["offsets"], b.q2, b.s2, r["w"])
    figs["gemm2_acc_units"] = acc_units(r["y2"], ref, ssc)
    figs["gemm2"] = check_within(r["y2"], ref, bound, "GEMM2")
    if r["inv"] is not None:
        assert same_bits(r["out"].cpu(), combine_ref(r["y2"], r["inv"], top_k)), "combine is not bit-exact"
    fig(name, **figs)
    return figs


def per_token(name, out, h, logits, b, quant_act=True, top_k=K):
    ref = pipeline_ref(h, logits, b.q13, b.s13, b.q2, b.s2, top_k, quant_act=quant_act)
    ratio = np.linalg.norm(out.float().cpu().double().numpy() - ref.double().numpy(), axis=1) / \
        np.linalg.norm(ref.double().numpy(), axis=1)
    fig(name, per_token_max=float(ratio.max()), per_token_median=float(np.median(ratio)))
    return check_per_token(out, ref, PER_TOKEN_LIMIT, name)


# ---------------------------------------------------------------------------------------------
# forced routing
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pipeline", ["decode", "prefill"])
@pytest.mark.parametrize("case", list(CASES))
def test_forced_routing_decode_shaped(case, pipeline):
    """``moe_decode_fp8`` and ``moe_prefill_fp8`` (the 64-pair-chunk grouped GEMM) with the bucket
    bounds on the chunk edges: bucket certificate, GEMM1 + SiLU and GEMM2 elementwise within the
    derived bounds, bit-exact combine, the wrapper bit-equal to the staged run on both of two calls,
    and every token within PER_TOKEN_LIMIT of ``moe_fp8_reference(quant_act=True)``.

    PER_TOKEN_LIMIT = 0.195: the largest per-token ratio measured on MI355X with the kernels as
    they were before the non-finite routing fix, over all forced-routing cases and pipelines
    (decode, prefill, tiles with the MX hand-off, per-row and plain schedule, grouped), was 0.0487
    (grouped decode-shaped kernel, two-experts case; the median token is at 0.0025), and the limit
    is 4 x that floor.  The floor is that high because the reference quantises for itself: a row
    whose largest intermediate lands one bf16 step away gets another e4m3 scale, and all its
    elements re-round -- discrete and input-dependent, hence the margin.  Stage certificates, largest
    error / bound over the same runs: routing weights 0.18, GEMM1 + SiLU 0.83, GEMM2 0.96 (the
    bf16 rounding of the output, saturated); largest proven accumulation error 406 x 2^-24 S."""
    H, F_ = DECODE_SHAPE
    h, lg = forced(case, H)
    b = bank(lg.shape[1], H, F_)
    hd, lgd = h.to(DEV), lg.to(DEV)
    r = run_stages(hd, b, pipeline, "decode", logits=lgd)
    name = f"{pipeline}/{case}"
    certify(name, r, b, lg)
    for _ in range(2):
        if pipeline == "decode":
            ws = moe.MoEWorkspace(h.shape[0], K, b.s13.shape[0], H, F_, DEV)
            out = moe.moe_decode_fp8(hd, lgd, b.w13t, b.s13d, b.w2t, b.s2d, K, ws)
        else:
            out = moe.moe_prefill_fp8(hd, lgd, b.w13t, b.s13d, b.w2t, b.s2d, K)
        assert same_bits(out, r["out"]), "the wrapper and the staged run differ"
    per_token(name, r["out"], h, lg, b)


TILE_VARIANTS = {"mx": (True, 0), "rowq": (False, 0), "plain": (False, 16)}


@pytest.mark.parametrize("variant", list(TILE_VARIANTS))
@pytest.mark.parametrize("case", list(CASES))
def test_forced_routing_tiles(case, variant, monkeypatch):
    """``moe_prefill_fp8_tiles`` with the bucket bounds on the 256-row tile edges: with the MX
    hand-off (GEMM1's e4m3 bytes and E8M0 block scales certified against stage (a), GEMM2 against
    the decoded MX intermediate), with the per-row hand-off, and with the plain fragment-read
    schedule (PENNY_MOE_TILE_SCHED=plain).  Same checks as the decode-shaped test."""
    mx, sched = TILE_VARIANTS[variant]
    H, F_ = TILE_SHAPE
    h, lg = forced(case, H)
    b = bank(lg.shape[1], H, F_)
    hd, lgd = h.to(DEV), lg.to(DEV)
    r = run_stages(hd, b, "prefill", "tiles", logits=lgd, mx=mx, sched=sched)
    name = f"tiles-{variant}/{case}"
    certify(name, r, b, lg)
    monkeypatch.setattr(moe, "MX_HANDOFF", mx)
    monkeypatch.setattr(moe, "TILE_SCHED", sched)
    for _ in range(2):
        out = moe.moe_prefill_fp8_tiles(hd, lgd, b.q13d, b.s13d, b.q2d, b.s2d, K)
        assert same_bits(out, r["out"]), "the wrapper and the staged run differ"
    per_token(name, r["out"], h, lg, b, quant_act="mx" if mx else True)


@pytest.mark.parametrize("kind", ["decode", "tiles"])
@pytest.mark.parametrize("case", list(CASES))
def test_forced_buckets_grouped(case, kind):
    """``moe_grouped_fp8`` / ``moe_grouped_fp8_tiles`` (expert-parallel receive side): rows tagged
    with their expert so the buckets have the case's sizes, plus 37 padding rows (-1) scattered
    among them.  Stage certificates, padding rows exactly zero, wrapper bit-equal twice, and every
    valid row within PER_TOKEN_LIMIT of the reference with that row's expert at weight 1."""
    counts = CASES[case]
    E = len(counts)
    H, F_ = DECODE_SHAPE if kind == "decode" else TILE_SHAPE
    b = bank(E, H, F_)
    g = torch.Generator().manual_seed(7 + len(case))
    ids = torch.cat([torch.full((c,), e, dtype=torch.int32) for e, c in enumerate(counts)] +
                    [torch.full((37,), -1, dtype=torch.int32)])
    ids = ids[torch.randperm(ids.numel(), generator=g)]
    M = ids.numel()
    x = torch.randn(M, H, generator=g).to(BF)
    xd, idd = x.to(DEV), ids.to(DEV)
    r = run_stages(xd, b, "grouped", kind, ids=idd)
    name = f"grouped-{kind}/{case}"
    assert np.array_equal(np.diff(r["offsets"].cpu().numpy()), np.array(counts))
    assert np.array_equal(ids[r["rows"].cpu().long()][:sum(counts)].numpy(), expert_of_pos(r["offsets"], sum(counts)))
    certify(name, r, b)
    valid = ids >= 0
    assert float(r["out"][idd < 0].float().abs().max()) == 0.0
    for _ in range(2):
        if kind == "decode":
            out = moe.moe_grouped_fp8(xd, idd, b.w13t, b.s13d, b.w2t, b.s2d)
        else:
            out = moe.moe_grouped_fp8_tiles(xd, idd, b.q13d, b.s13d, b.q2d, b.s2d)
        assert same_bits(out, r["out"]), "the wrapper and the staged run differ"
    routing = (torch.ones(int(valid.sum()), 1), ids[valid][:, None].long())
    ref = moe.moe_fp8_reference(x[valid].float(), None, b.q13, b.s13, b.q2, b.s2, 1, quant_act=True, routing=routing)
    got = r["out"].cpu()[valid]
    fig(name, per_token_max=check_per_token(got, ref, PER_TOKEN_LIMIT, name))


# ---------------------------------------------------------------------------------------------
# routing exactness
# ---------------------------------------------------------------------------------------------
def route_only(kernel, lg, top_k, H=64, seed=0):
    """penny_moe_route / penny_moe_route_quant on zero-filled buffers -> dict of CPU tensors."""
    T, E = lg.shape
    P = T * top_k
    lgd = lg.to(DEV).contiguous()
    rows, w, inv, offsets = torch.zeros(P, **I32), torch.zeros(P, **F32), torch.zeros(P, **I32), torch.zeros(E + 1, **I32)
    r = {}
    if kernel == "route":
        N.call("penny_moe_route", N.ptr(lgd), T, E, top_k, N.ptr(rows), N.ptr(w), N.ptr(offsets), N.ptr(inv), N.stream())
    else:
        h = torch.randn(T, H, generator=torch.Generator().manual_seed(seed)).to(BF).to(DEV)
        xq, xs = torch.zeros((T, H), dtype=torch.uint8, device=DEV), torch.zeros(T, **F32)
        pe, pw = torch.zeros(P, **I32), torch.zeros(P, **F32)
        N.call("penny_moe_route_quant", N.ptr(h), h.stride(0), N.ptr(lgd), T, H, E, top_k, N.ptr(xq), N.ptr(xs),
               N.ptr(pe), N.ptr(pw), N.ptr(rows), N.ptr(w), N.ptr(offsets), N.ptr(inv), N.stream())
        r.update(xq=xq.cpu(), xs=xs.cpu(), pe=pe.cpu(), pw=pw.cpu())
    torch.cuda.synchronize()
    r.update(rows=rows.cpu(), w=w.cpu(), inv=inv.cpu(), offsets=offsets.cpu())
    return r


def exactness_logits(E, top_k, T=192, seed=0):
    """Rows where a top-k goes wrong: all-equal rows, a tie exactly at the K-th place, many bf16
    ties (half-integer logits), spreads whose exp underflows to 0 for all but one expert (the others
    distinct, 200 and more below), and a single -inf among finite logits."""
    g = torch.Generator().manual_seed(seed + 100 * E + top_k)
    lg = torch.randn(T, E, generator=g) * 2
    lg[0:16] = torch.randn(16, 1, generator=g)                                   # all equal
    for t in range(16, 48):                                                      # tie at the K-th place
        p = torch.randperm(E, generator=g)
        lg[t] = -torch.arange(E).float()[torch.argsort(p)]                       # distinct ranks
        if top_k < E:
            lg[t, p[top_k]] = lg[t, p[top_k - 1]]                                # K-th and (K+1)-th equal
        if top_k >= 2:
            lg[t, p[top_k - 2]] = lg[t, p[top_k - 1]]
    lg[48:96] = torch.round(lg[48:96] * 2) / 2                                   # coarse: many ties
    for t in range(96, 128):                                                     # underflow spreads
        lg[t] = -200.0 - 8.0 * torch.randperm(E, generator=g).float()
        lg[t, int(torch.randint(0, E, (1,), generator=g))] = 3.0
    for t in range(128, 160):                                                    # one -inf
        lg[t, int(torch.randint(0, E, (1,), generator=g))] = -float("inf")
    return lg.to(BF)


@pytest.mark.parametrize("kernel", ["route", "route_quant"])
@pytest.mark.parametrize("E,top_k", [(4, 1), (4, 2), (8, 1), (8, 2), (8, 6), (8, 8), (64, 1), (64, 2), (64, 6), (64, 8)])
def test_routing_exactness(kernel, E, top_k):
    """Both routing kernels pick exactly the reference's experts (ties to the smaller id) with
    weights within a few f32 ulps of float64, on rows built to break a top-k."""
    lg = exactness_logits(E, top_k)
    T = lg.shape[0]
    ref = route_ref(lg, top_k)
    assert not ref.poisoned.any()
    r = route_only(kernel, lg, top_k)
    fig(f"{kernel}/E{E}K{top_k}", weights=check_buckets(r["offsets"], r["rows"], r["w"], r["inv"], ref, T, E, top_k))


# ---------------------------------------------------------------------------------------------
# non-finite rows
# ---------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")
PLANTED = {17: "all_nan", 101: "all_ninf", 200: "one_nan", 299: "one_inf"}


def plant(lg):
    lg = lg.clone()
    E = lg.shape[1]
    lg[17], lg[101], lg[200, E // 2], lg[299, E - 1] = NAN, -INF, NAN, INF
    return lg


@pytest.mark.parametrize("kernel", ["route", "route_quant"])
@pytest.mark.parametrize("E,top_k", [(8, 2), (64, 6)])
def test_nonfinite_router_rows(kernel, E, top_k):
    """The routing kernels are total: among 300 clean rows, an all-NaN row, an all -inf row, a row
    with one NaN and a row with one +inf each get K ids in [0, E), every slot stored once (the
    zero-filled weight scratch holds NaN in all their slots), NaN weights, and valid buckets
    (``check_buckets``); the clean rows' experts, weights and quantised hidden rows are bit-equal
    to the same call with the planted rows zeroed."""
    T = 300
    g = torch.Generator().manual_seed(E)
    base = (torch.randn(T, E, generator=g) * 2).to(BF)
    lg = plant(base)
    zeroed = base.clone()
    zeroed[list(PLANTED)] = 0
    ref = route_ref(lg, top_k)
    assert np.nonzero(ref.poisoned)[0].tolist() == sorted(PLANTED)
    r = route_only(kernel, lg, top_k)
    check_buckets(r["offsets"], r["rows"], r["w"], r["inv"], ref, T, E, top_k)
    if kernel == "route_quant":
        pe, pw = r["pe"].view(T, top_k), r["pw"].view(T, top_k)
        assert bool(((pe >= 0) & (pe < E)).all())
        assert bool(torch.isnan(pw[list(PLANTED)]).all()) and bool(torch.isfinite(pw[~torch.as_tensor(ref.poisoned)]).all())
    z = route_only(kernel, zeroed, top_k)
    check_buckets(z["offsets"], z["rows"], z["w"], z["inv"], route_ref(zeroed, top_k), T, E, top_k)
    clean = torch.as_tensor(~ref.poisoned)

    def pairs(q):       # per token: (expert, weight bits) of its K slots, in slot order
        e = torch.as_tensor(expert_of_pos(q["offsets"], T * top_k))[q["inv"].long()].view(T, top_k)
        return e, q["w"][q["inv"].long()].view(T, top_k).view(torch.int32)
    (e1, w1), (e0, w0) = pairs(r), pairs(z)
    assert torch.equal(e1[clean], e0[clean]) and torch.equal(w1[clean], w0[clean])
    if kernel == "route_quant":
        assert torch.equal(r["xq"], z["xq"]) and torch.equal(r["xs"], z["xs"])


PIPELINES = ["decode", "prefill", "tiles-mx", "tiles-rowq", "tiles-plain"]


def run_pipeline(pipeline, hd, lgd, monkeypatch):
    if pipeline in ("decode", "prefill"):
        H, F_ = DECODE_SHAPE
        b = bank(8, H, F_)
        if pipeline == "decode":
            ws = moe.MoEWorkspace(hd.shape[0], K, 8, H, F_, DEV)
            return moe.moe_decode_fp8(hd, lgd, b.w13t, b.s13d, b.w2t, b.s2d, K, ws)
        return moe.moe_prefill_fp8(hd, lgd, b.w13t, b.s13d, b.w2t, b.s2d, K)
    mx, sched = TILE_VARIANTS[pipeline.split("-")[1]]
    monkeypatch.setattr(moe, "MX_HANDOFF", mx)
    monkeypatch.setattr(moe, "TILE_SCHED", sched)
    b = bank(8, *TILE_SHAPE)
    return moe.moe_prefill_fp8_tiles(hd, lgd, b.q13d, b.s13d, b.q2d, b.s2d, K)


@pytest.mark.parametrize("pipeline", PIPELINES)
def test_nan_hidden_row_gives_a_nan_output_row_only(pipeline, monkeypatch):
    """A NaN activation row (logits = h @ router, so its logits are NaN too) comes out as a NaN row;
    every other token is bit-equal to the run with that row zeroed, and the device is healthy."""
    H = DECODE_SHAPE[0] if pipeline in ("decode", "prefill") else TILE_SHAPE[0]
    T, t0 = 300, 137
    g = torch.Generator().manual_seed(H)
    h = torch.randn(T, H, generator=g).to(BF)
    router = (torch.randn(8, H, generator=g) * 0.2).to(BF).to(DEV)
    outs = []
    for fill in (NAN, 0.0):
        hd = h.clone()
        hd[t0] = fill
        hd = hd.to(DEV)
        lgd = (hd @ router.t()).contiguous()
        outs.append(run_pipeline(pipeline, hd, lgd, monkeypatch))
        torch.cuda.synchronize()
    got, zero = (o.cpu() for o in outs)
    assert bool(torch.isnan(got[t0]).all()), "the NaN token's output row is not all NaN"
    others = torch.arange(T) != t0
    assert bool(torch.isfinite(got[others].float()).all())
    assert same_bits(got[others], zero[others]), "a NaN row changed another token's output"


# ---------------------------------------------------------------------------------------------
# decode cap, combine
# ---------------------------------------------------------------------------------------------
def test_decode_pipeline_at_the_route_cap():
    """``moe_decode_fp8`` at T*K == 4096, the cap of the single-workgroup route kernel (Mixtral
    sends up to that): bucket certificate and the per-token check on every one of the 2048 tokens;
    one pair more is refused with hipErrorInvalidValue before anything is launched."""
    H, F_ = DECODE_SHAPE
    T = 4096 // K
    b = bank(8, H, F_)
    g = torch.Generator().manual_seed(4096)
    h = torch.randn(T, H, generator=g).to(BF)
    lg = (torch.randn(T, 8, generator=g) * 2).to(BF)
    ws = moe.MoEWorkspace(T, K, 8, H, F_, DEV)
    out = moe.moe_decode_fp8(h.to(DEV), lg.to(DEV), b.w13t, b.s13d, b.w2t, b.s2d, K, ws)
    torch.cuda.synchronize()
    check_buckets(ws.offsets, ws.sorted_tok, ws.sorted_w, ws.inv, route_ref(lg, K), T, 8, K)
    per_token("decode/cap4096", out, h, lg, b)
    lg1 = torch.zeros(4097, 8, dtype=BF, device=DEV)
    buf = [torch.zeros(4097, **I32), torch.zeros(4097, **F32), torch.zeros(9, **I32), torch.zeros(4097, **I32)]
    rc = N.load().penny_moe_route(N.ptr(lg1), 4097, 8, 1, *(N.ptr(t) for t in buf), N.stream())
    assert rc == 1                                               # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert all(int(t.abs().sum()) == 0 for t in buf)


@pytest.mark.parametrize("H", [8, 520, 4096])
@pytest.mark.parametrize("top_k", [1, 2, 6])
def test_combine_is_bit_exact(top_k, H):
    """``penny_moe_combine`` and ``penny_moe_combine_weighted`` == the f32 chain in j order, one
    rounding per term, rounded to bf16 (``combine_ref``), bit for bit."""
    T = 37
    g = torch.Generator().manual_seed(top_k * 10000 + H)
    y2 = (torch.randn(T * top_k, H, generator=g) * 3).to(BF)
    inv = torch.randperm(T * top_k, generator=g).to(torch.int32)
    w = torch.rand(T * top_k, generator=g)
    y2d, invd, wd = y2.to(DEV), inv.to(DEV), w.to(DEV)
    out = torch.zeros((T, H), dtype=BF, device=DEV)
    N.call("penny_moe_combine", N.ptr(y2d), N.ptr(invd), T, top_k, H, N.ptr(out), N.stream())
    assert same_bits(out.cpu(), combine_ref(y2, inv, top_k))
    outw = torch.zeros((T, H), dtype=BF, device=DEV)
    N.call("penny_moe_combine_weighted", N.ptr(y2d), N.ptr(invd), N.ptr(wd), T, top_k, H, N.ptr(outw), N.stream())
    assert same_bits(outw.cpu(), combine_ref(y2, inv, top_k, w))
