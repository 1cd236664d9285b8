"""The certificates of ``moe_ref`` catch a subtly wrong MoE pipeline (CPU only).

The result under test is a pure-torch emulation of the fp8 pipeline built from the pieces of
``ops/moe.py`` (routing, per-row e4m3 quantisation, per-bucket GEMMs with the kernels' epilogue
roundings, combine).  Unmutated it must pass every checker; each test then applies one mutation of
the kind a kernel bug produces and shows which checker rejects it.  The last tests show that the
aggregate criteria of the older pipeline tests accept one wrong row in 2500, and that the lane-level
emulation of the routing wave gives every slot one writer for non-finite rows.
"""
from fractions import Fraction

import numpy as np
import pytest
import torch

from financial_chatbot_llm_amd.ops import gemm, moe
from financial_chatbot_llm_amd.ops.activation import silu_mul
from moe_ref import (PER_TOKEN_LIMIT, check_buckets, check_mx_intermediate, check_per_token, check_within, combine_ref,
                     fp8_f64, gemm1_silu_ref, gemm2_ref, per_token_ratio, pipeline_ref, route_quant_lanes, route_ref)

BF = torch.bfloat16


def _bank(g, E, H, F_):
    w13 = (torch.randn(E, 2 * F_, H, generator=g) * 0.05).to(BF)
    w2 = (torch.randn(E, H, F_, generator=g) * 0.05).to(BF)
    w13i = torch.stack([gemm.interleave16(w13[e, :F_], w13[e, F_:]) for e in range(E)])
    q13, s13 = moe.quantize_fp8_rowwise(w13i)
    q2, s2 = moe.quantize_fp8_rowwise(w2)
    return q13, s13.float(), q2, s2.float()


def _case(T=96, E=8, H=128, F_=64, seed=0, ties=True):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(T, H, generator=g).to(BF)
    logits = (torch.randn(T, E, generator=g) * 2).to(BF)
    if ties:
        logits[5] = 0.25                        # an all-equal row
        logits[6, 3] = logits[6, 1]             # a bf16 tie
        logits[7] = torch.tensor([1.0, 3.0, 2.0, 2.0, -1.0, 2.0, 0.0, -2.0][:E]).to(BF)   # tie at the K-th place
    return h, logits, _bank(g, E, H, F_)


def emulate(h, logits, bank, K, mutate=None):
    """The fp8 MoE pipeline in plain torch on the CPU, every stage's tensors returned."""
    q13, s13, q2, s2 = bank
    E, F2 = s13.shape
    F_ = F2 // 2
    T, H = h.shape
    l32 = logits.to(BF).float()
    p = torch.exp(l32 - l32.max(1, keepdim=True).values)
    if mutate == "tie_larger":
        ids = (E - 1 - torch.sort(-p.flip(1), dim=1, stable=True).indices)[:, :K]
    else:
        ids = torch.sort(-p, dim=1, stable=True).indices[:, :K]
    topw = p.gather(1, ids)
    topw = topw / (p.sum(1, keepdim=True) if mutate == "no_renorm" else topw.sum(1, keepdim=True))
    order, offsets, tok_idx, tok_w = moe.route(ids.to(torch.int32), topw, E)
    inv = torch.empty_like(order)
    inv[order] = torch.arange(order.numel())
    tok_w = tok_w.clone()
    off = offsets.tolist()
    big = max(range(E), key=lambda e: off[e + 1] - off[e])      # a bucket that is surely not empty
    if mutate == "swap_w":
        t0 = int(tok_idx[off[big]])
        a, b = int(inv[t0 * K]), int(inv[t0 * K + 1])
        tok_w[a], tok_w[b] = tok_w[b].clone(), tok_w[a].clone()
    if mutate == "offsets_short":
        offsets = offsets.clone()
        offsets[E] -= 1
    if mutate == "inv_dup":
        inv = inv.clone()
        inv[1] = inv[0]
    xq, xs = moe.quantize_fp8_rowwise(h)
    xs = xs.float()
    a = torch.zeros((T * K, F_), dtype=BF)
    for e in range(E):
        lo, hi = off[e], off[e + 1]
        if hi <= lo:
            continue
        tok = tok_idx[lo:hi]
        acc = xq[tok].float() @ q13[e].float().t()
        sc = s13[e].expand(hi - lo, F2).clone()
        if mutate == "wrong_expert" and e == big:                # the bucket's first row: the next expert's weights
            e1 = (e + 1) % E
            acc[0] = xq[tok[0]].float() @ q13[e1].float().t()
            sc[0] = s13[e1]
        gu = (acc * xs[tok, None] * sc).to(BF)
        if mutate == "swap_group" and e == big:                  # one 16-column gate|up group swapped
            v = gu.view(hi - lo, F_ // 16, 2, 16)
            v[0, 1] = v[0, 1].flip(0)
        a[lo:hi] = silu_mul(gu, interleave16=True)
    aq, as_ = moe.quantize_fp8_rowwise(a)
    as_ = as_.float()
    y2 = torch.zeros((T * K, H), dtype=BF)
    for e in range(E):
        lo, hi = off[e], off[e + 1]
        if hi > lo:
            y2[lo:hi] = (aq[lo:hi].float() @ q2[e].float().t() * as_[lo:hi, None] * s2[e][None, :]
                         * tok_w[lo:hi, None]).to(BF)
    if mutate == "drop_last_row":
        y2[off[big + 1] - 1] = 0
    acc = torch.zeros((T, H))
    for j in range(K - 1 if mutate == "combine_short" else K):
        acc += y2[inv.view(T, K)[:, j]].float()
    return dict(logits=logits, K=K, E=E, T=T, offsets=offsets, tok=tok_idx, w=tok_w, inv=inv, xq=xq, xs=xs, a=a, aq=aq,
                as_=as_, y2=y2, out=acc.to(BF), bank=bank, h=h)


def run_checks(r, only=None):
    """Every certificate on an emulation result; ``only`` names one of them."""
    q13, s13, q2, s2 = r["bank"]
    T, E, K = r["T"], r["E"], r["K"]

    def buckets():
        check_buckets(r["offsets"], r["tok"], r["w"], r["inv"], route_ref(r["logits"], K), T, E, K)

    def gemm1():
        ref, bound = gemm1_silu_ref(r["xq"], r["xs"], r["tok"], r["offsets"], q13, s13)
        check_within(r["a"], ref, bound, "GEMM1 + SiLU")

    def gemm2():
        ref, bound, _ = gemm2_ref(fp8_f64(r["aq"]), r["as_"], r["offsets"], q2, s2, r["w"])
        check_within(r["y2"], ref, bound, "GEMM2")

    def combine():
        want = combine_ref(r["y2"], r["inv"], K)
        assert torch.equal(r["out"].view(torch.int16), want.view(torch.int16)), "combine is not bit-exact"

    def per_token():
        ref = pipeline_ref(r["h"], r["logits"], q13, s13, q2, s2, K)
        check_per_token(r["out"], ref, PER_TOKEN_LIMIT)
    for name, fn in (("buckets", buckets), ("gemm1", gemm1), ("gemm2", gemm2), ("combine", combine),
                     ("per_token", per_token)):
        if only is None or only == name:
            fn()


def test_clean_emulation_passes_every_checker():
    h, logits, bank = _case()
    run_checks(emulate(h, logits, bank, 2))
    h, logits, bank = _case(T=40, E=8, seed=3)
    run_checks(emulate(h, logits, bank, 3), only="buckets")


# mutation -> the certificate that must reject it (and a fragment of its message)
MUTATIONS = [
    ("drop_last_row", "gemm2", "GEMM2"),
    ("wrong_expert", "gemm1", r"GEMM1 \+ SiLU"),
    ("swap_w", "buckets", "wrong weights"),
    ("tie_larger", "buckets", "wrong buckets"),
    ("offsets_short", "buckets", r"offsets\[E\]"),
    ("inv_dup", "buckets", "no permutation"),
    ("no_renorm", "buckets", "wrong weights"),
    ("combine_short", "combine", "bit-exact"),
    ("swap_group", "gemm1", r"GEMM1 \+ SiLU"),
]


@pytest.mark.parametrize("mutation,checker,message", MUTATIONS)
def test_mutation_is_rejected(mutation, checker, message):
    h, logits, bank = _case()
    r = emulate(h, logits, bank, 2, mutate=mutation)
    with pytest.raises(AssertionError, match=message):
        run_checks(r, only=checker)


@pytest.mark.parametrize("mutation", ["drop_last_row", "wrong_expert", "combine_short"])
def test_per_token_check_rejects_a_wrong_row(mutation):
    """The end-to-end check alone sees every mutation that replaces or drops a row's term."""
    h, logits, bank = _case(ties=False)
    r = emulate(h, logits, bank, 2, mutate=mutation)
    with pytest.raises(AssertionError, match="tokens off"):
        run_checks(r, only="per_token")


@pytest.mark.parametrize("mutation", ["swap_w", "swap_group"])
def test_per_token_check_alone_misses_small_mutations(mutation):
    """Why the stage certificates exist: two routing weights swapped, or one 16-column group of 64
    swapped, move a row by less than the end-to-end limit (the reference quantises for itself, so
    that limit cannot be tight); ``test_mutation_is_rejected`` shows the certificate that sees each."""
    h, logits, bank = _case(ties=False)
    run_checks(emulate(h, logits, bank, 2, mutate=mutation), only="per_token")


def test_aggregate_criteria_accept_one_wrong_row_in_2500():
    """The reason for the per-row certificates.  The criteria of the older pipeline tests -- mean
    error below 1 % of the mean magnitude; max error below 3 % of the global max -- accept a token
    row computed with the neighbouring expert: the mean one for any token, the max one for a quiet
    token (hidden row 1/8 of the usual norm: its whole output is below 3 % of the loudest element).
    The per-token check rejects both."""
    h, logits, bank = _case(T=2500, E=8, H=128, F_=64, seed=7, ties=False)
    q13, s13, q2, s2 = bank
    for quiet in (False, True):
        hh = h.clone()
        clean = emulate(hh, logits, bank, 2)
        off = clean["offsets"].tolist()
        big = max(range(8), key=lambda e: off[e + 1] - off[e])
        t0 = int(clean["tok"][off[big]])                        # the token the mutation hits
        if quiet:
            hh[t0] = (hh[t0].float() / 8).to(BF)
        ref = pipeline_ref(hh, logits, q13, s13, q2, s2, 2).float()
        got = emulate(hh, logits, bank, 2, mutate="wrong_expert")["out"].float()
        err = (got - ref).abs()
        rows = (per_token_ratio(got, ref) > PER_TOKEN_LIMIT).nonzero()[0]
        assert rows.tolist() == [t0]                            # exactly one wrong row
        assert err.mean() < 0.01 * ref.abs().mean() + 1e-4      # test_moe_fp8_pipeline's criterion: accepts
        if quiet:
            assert float(err.max() / ref.abs().max()) < 0.03    # ..._tiles_matches_expert_loop's: accepts
        with pytest.raises(AssertionError, match="1 of 2500 tokens off"):
            check_per_token(got, ref, PER_TOKEN_LIMIT)


def test_mx_intermediate_check():
    """The MX hand-off certificate accepts ``_fake_quant_mx``'s own blocks and rejects a scale
    exponent one too large, one too small, and a wrong value."""
    g = torch.Generator().manual_seed(2)
    ref = (torch.randn(24, 256, generator=g) * 0.3).to(BF).double()
    bound = ref.abs() * 2.0 ** -8 + 1e-6
    b = moe.mx_blocks(ref.float())
    amax = b.abs().amax(-1)
    X = torch.ceil(torch.log2(amax / 448.0)).to(torch.int32)
    aq = moe.mx_unblocks((b / torch.exp2(X.float())[..., None]).to(moe.FP8).float()).to(moe.FP8).view(torch.uint8)
    check_mx_intermediate(aq, X, ref, bound)
    for d in (2, -2):
        Xm = X.clone()
        Xm[3, 1, 2] += d
        with pytest.raises(AssertionError, match="MX scale blocks off"):
            check_mx_intermediate(aq, Xm, ref, bound)
    bad = aq.clone()
    bad[7, 100] ^= 0x10
    with pytest.raises(AssertionError, match="MX intermediate"):
        check_mx_intermediate(bad, X, ref, bound)


def test_combine_ref_is_the_exactly_rounded_fma_chain():
    """``combine_ref`` against exact rational arithmetic, one rounding per term, on values spread
    over 40 binades (where the float64 sum is no longer exact and the residual path runs)."""
    g = torch.Generator().manual_seed(4)
    K, T, H = 3, 6, 8
    y2 = (torch.randn(T * K, H, generator=g) * torch.exp2(torch.randint(-20, 20, (T * K, 1), generator=g).float())).to(BF)
    w = torch.rand(T * K, generator=g)
    inv = torch.randperm(T * K, generator=g)
    for wv in (None, w):
        got = combine_ref(y2, inv, K, wv)
        for t in range(T):
            for c in range(H):
                acc = np.float32(0)
                for j in range(K):
                    pos = int(inv[t * K + j])
                    exact = Fraction(float(acc)) + Fraction(float(y2[pos, c])) * (1 if wv is None else Fraction(float(wv[pos])))
                    lo = np.float32(float(exact))               # float(Fraction) rounds correctly to f64; then
                    cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
                    acc = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(v.view(np.uint32)) & 1))
                assert float(torch.tensor(float(acc)).to(BF)) == float(got[t, c]), (t, c)


# ---------------------------------------------------------------------------------------------
# the routing wave, lane by lane
# ---------------------------------------------------------------------------------------------
NAN, INF = float("nan"), float("inf")


def _rows(E):
    base = np.linspace(-1.0, 1.0, E).astype(np.float32)
    one_nan, one_inf, one_ninf = base.copy(), base.copy(), base.copy()
    one_nan[E // 2], one_inf[E // 3], one_ninf[1] = NAN, INF, -INF
    return {"all_nan": np.full(E, NAN, np.float32), "all_ninf": np.full(E, -INF, np.float32), "one_nan": one_nan,
            "one_inf": one_inf, "one_ninf": one_ninf, "finite": base, "all_equal": np.zeros(E, np.float32)}


@pytest.mark.parametrize("E,K", [(8, 2), (8, 3), (64, 6), (4, 1), (8, 8), (64, 8)])
def test_fixed_routing_wave_gives_every_slot_one_writer(E, K):
    """Lane-exact emulation of the fixed arg-max loop: whatever the row, slots 0..K-1 are each
    stored by exactly one lane, the stored id is below E, the ids are distinct, and the weights are
    NaN exactly on the rows whose float64 softmax is not finite."""
    for name, row in _rows(E).items():
        stores = route_quant_lanes(row, E, K, fixed=True)
        assert sorted(s[0] for s in stores) == list(range(K)), (name, stores)
        assert all(0 <= s[1] < E for s in stores) and len({s[1] for s in stores}) == K, (name, stores)
        poisoned = bool(route_ref(torch.tensor(row[None]).to(BF), K).poisoned[0])
        assert poisoned == (name in ("all_nan", "all_ninf", "one_nan", "one_inf")), name
        assert all(np.isnan(s[2]) == poisoned for s in stores), (name, stores)
        if not poisoned:
            ref = route_ref(torch.tensor(row[None]).to(BF), K)
            assert [s[1] for s in sorted(stores)] == ref.ids[0].tolist(), (name, stores)


def test_former_routing_wave_stored_expert_id_E_for_an_all_nan_row():
    """The loop before the fix, on the CPU only: with NaN in the compares the lanes disagree on the
    winner -- slot 0 of an all-NaN row (E = 8, K = 2) is stored by lanes 1..8, lane 8 writing the
    out-of-range expert id 8, and with K = 3 slot 1 is stored by nobody.  Finite rows were fine."""
    stores = route_quant_lanes(_rows(8)["all_nan"], 8, 2, fixed=False)
    assert sorted(s[1] for s in stores if s[0] == 0) == list(range(1, 9))
    stores = route_quant_lanes(_rows(8)["all_nan"], 8, 3, fixed=False)
    assert 1 not in {s[0] for s in stores}
    stores = route_quant_lanes(_rows(8)["all_ninf"], 8, 2, fixed=False)
    assert max(s[1] for s in stores) == 8
    for name in ("finite", "all_equal", "one_ninf"):
        assert route_quant_lanes(_rows(8)[name], 8, 2, fixed=False) == route_quant_lanes(_rows(8)[name], 8, 2)
