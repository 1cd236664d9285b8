"""Exact-answer tests of the sampler (``sampler.hip``) and the filtered top-k search
(``retrieval.hip``) on the GPU.

Both kernels give discrete answers, so they are checked exactly: a sampled token must be the
argmax of the fp64 score ``logit / T + noise(seed, token id)`` computed by the numpy replica of
the kernel's counter-based noise (``selection_ref.sample_ref``), and a top-k list must pass the
validity certificate of ``selection_ref.check_topk_certificate``.  Inputs are built on the CPU
with seeded generators; ``tests/test_selection_checks.py`` shows on the CPU that both checkers
reject subtly wrong answers.
"""
import numpy as np
import pytest
import torch

from financial_chatbot_llm_amd import ops
from financial_chatbot_llm_amd.ops import retrieval as retrieval_ops
from financial_chatbot_llm_amd.ops.sampling import topk_topp_threshold
from selection_ref import check_sampled, check_topk_certificate, noise_bits, sample_ref, to_np

pytestmark = pytest.mark.gpu
DEV = "cuda"

# Score tolerance of the sampler tests.  The float32 floor -- the largest difference between the
# score formula evaluated in numpy float32 with correctly rounded logs and in float64
# (selection_ref.score_floor_f32) over every sampler input of this file -- is 1.453e-6 (the
# V = 128256 float32 rows; scores reach 16 .. 32 there, where one float32 ulp is 1.9e-6).
# eps = 16 x floor = 2.34e-5: the factor covers the two nested fast logs and the 1/T multiply.
# A wrong token trails the best score by order 1.  (On record, not an input to eps: the largest
# deviation of the MI355X kernel's returned scores from fp64 over these tests is 1.72e-6.)
SCORE_FLOOR_F32 = 1.46e-6
EPS = 16 * SCORE_FLOOR_F32

_seen = {"dev": 0.0}


def _score_dev(pairs, ref_scores, temps, voff=0):
    """Returned score bits vs the fp64 score of the returned id: exact on greedy rows, within EPS on
    sampled rows.  Prints the largest deviation seen so far (on record in the test log)."""
    pairs = pairs.cpu()
    sc = to_np(pairs[:, 0].contiguous().view(torch.float32), np.float64)
    loc = to_np(pairs[:, 1], np.int64) - voff
    assert np.isfinite(sc).all(), "non-finite score bits"
    dev = np.abs(sc - ref_scores[np.arange(len(loc)), loc])
    samp = to_np(temps) > 0
    assert (dev[~samp] == 0).all(), "greedy score is not the logit"
    worst = float(dev[samp].max()) if samp.any() else 0.0
    _seen["dev"] = max(_seen["dev"], worst)
    print(f"sampler score deviation: this case {worst:.3e}, largest so far {_seen['dev']:.3e} (eps {EPS:.3e})")
    assert worst <= EPS, f"GPU score off the fp64 score by {worst:.3e} > eps {EPS:.3e}"


# =============================================================================================
# sampler
# =============================================================================================
VOCABS = [7, 8, 9, 120, 1001, 4096, 128256]
TEMPS = [0.5, 1.0, 2.0, 0.0, 2.0, 0.0, 1.0, 0.5]


def sampler_case(V, dtype):
    B = 64 if V == 128256 else 32
    g = torch.Generator().manual_seed(100 + V)
    logits = (torch.randn(B, V, generator=g) * 3.0).to(dtype)
    temps = torch.tensor((TEMPS * 8)[:B])
    seeds = torch.arange(B, dtype=torch.int64) * 7919 + 3 + 1000003 * V
    return logits, temps, seeds


def _dev(*ts):
    return [t.to(DEV) for t in ts]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", VOCABS)
def test_sample_exact_tokens(V, dtype):
    """V = 7: tail only; 9: one chunk + tail; 120: fewer chunks than slices; 1001: aligned copy."""
    logits, temps, seeds = sampler_case(V, dtype)
    scores, _, _ = sample_ref(logits, temps, seeds)
    d_logits, d_temps, d_seeds = _dev(logits, temps, seeds)
    tok = ops.sample(d_logits, d_temps, d_seeds).cpu()
    check_sampled(tok, scores, EPS, greedy=temps <= 0)
    pairs = ops.sample_shard(d_logits, d_temps, d_seeds, 0, V)
    assert torch.equal(pairs[:, 1].cpu(), tok)
    _score_dev(pairs, scores, temps)


def strided_case():
    V, B = 4096, 16
    g = torch.Generator().manual_seed(77)
    buf = torch.full((B, V + 24), 100.0)             # anything read past V would win the row
    buf[:, :V] = torch.randn(B, V, generator=g) * 3.0
    temps = torch.tensor((TEMPS * 2)[:B])
    seeds = torch.arange(B, dtype=torch.int64) * 104729 + 13
    return buf, V, temps, seeds


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_sample_strided_view(dtype):
    buf, V, temps, seeds = strided_case()
    buf = buf.to(dtype)
    view = buf.to(DEV)[:, :V]
    assert view.stride(0) == V + 24 and view.stride(0) % 8 == 0 and not view.is_contiguous()
    scores, _, _ = sample_ref(buf[:, :V], temps, seeds)
    tok = ops.sample(view, *_dev(temps, seeds)).cpu()
    check_sampled(tok, scores, EPS, greedy=temps <= 0)


def shard_case(Vs):
    B, R = 9, 8
    g = torch.Generator().manual_seed(Vs)
    full = (torch.randn(B, R * Vs, generator=g) * 3.0).to(torch.bfloat16)
    temps = torch.tensor((TEMPS * 2)[:B])
    seeds = torch.arange(B, dtype=torch.int64) * 7919 + 11
    return full, R, temps, seeds


@pytest.mark.parametrize("Vs", [1001, 16033])
def test_sample_shards(Vs):
    """Each shard's (score, global id) against the reference with voff; the 8 shards merged by
    pick_pairs equal the single-kernel sample of the concatenated row exactly.  The shards are
    column slices of the full logits, so most start off a 16-B boundary."""
    full, R, temps, seeds = shard_case(Vs)
    V = R * Vs
    d_full, d_temps, d_seeds = _dev(full, temps, seeds)
    allp = []
    for r in range(R):
        voff = r * Vs
        pairs = ops.sample_shard(d_full[:, voff:voff + Vs], d_temps, d_seeds, voff, V)
        scores, _, _ = sample_ref(full[:, voff:voff + Vs], temps, seeds, voff=voff)
        check_sampled(pairs[:, 1].cpu(), scores, EPS, voff=voff, greedy=temps <= 0)
        _score_dev(pairs, scores, temps, voff=voff)
        allp.append(pairs)
    whole = ops.sample(d_full, d_temps, d_seeds).cpu()
    assert torch.equal(ops.pick_pairs(torch.stack(allp)).cpu(), whole)
    check_sampled(whole, sample_ref(full, temps, seeds)[0], EPS, greedy=temps <= 0)


# (seed, token id) pairs of the Llama-3 vocabulary whose noise bits are 0xFFFFFF in the top 24:
# six of the 16 that a scan of the seeds row * 7919 + 3, row < 2048, finds with the numpy replica
TOP_MANTISSA = [(411791, 47583), (704794, 98048), (2130214, 110843), (2644949, 99507), (3579391, 89154),
                (4141640, 4663)]


def top_mantissa_case():
    V = 128256
    n = len(TOP_MANTISSA)
    g = torch.Generator().manual_seed(1234)
    logits = torch.randn(2 * n, V, generator=g) * 3.0
    seeds = torch.tensor([s for s, _ in TOP_MANTISSA] * 2, dtype=torch.int64)
    for r, (_, idx) in enumerate(TOP_MANTISSA):
        logits[n + r, idx] = -30.0            # second half: that token cannot win with finite noise
    return logits, torch.ones(2 * n), seeds


def test_top_mantissa_noise_is_finite():
    """u01_from_bits used 24 bits + 0.5f, which rounds to u == 1.0f at the top mantissa: noise
    +inf, so that token won whatever the logits.  These rows draw that mantissa."""
    for seed, idx in TOP_MANTISSA:
        assert int(noise_bits(seed, idx)) >> 8 == (1 << 24) - 1
    logits, temps, seeds = top_mantissa_case()
    V = logits.shape[1]
    scores, _, ids = sample_ref(logits, temps, seeds)
    n = len(TOP_MANTISSA)
    assert all(int(ids[n + r]) != TOP_MANTISSA[r][1] for r in range(n))
    pairs = ops.sample_shard(*_dev(logits, temps, seeds), 0, V).cpu()
    sc = pairs[:, 0].contiguous().view(torch.float32)
    assert bool(torch.isfinite(sc).all()), f"infinite sampled scores: {sc.tolist()}"
    check_sampled(pairs[:, 1], scores, EPS)
    _score_dev(pairs, scores, temps)
    check_sampled(ops.sample(*_dev(logits, temps, seeds)).cpu(), scores, EPS)


def _greedy(logits):
    B = logits.shape[0]
    return ops.sample(logits.to(DEV), torch.zeros(B, device=DEV), torch.arange(B, dtype=torch.int64, device=DEV)).cpu()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_greedy_ties_pick_the_smallest_index(dtype):
    g = torch.Generator().manual_seed(3)
    # all-equal rows
    for V in (7, 8, 1001, 4096):
        assert _greedy(torch.full((2, V), 1.5, dtype=dtype)).tolist() == [0, 0]
    # V = 128256: 16032 chunks of 8, 1002 chunks (8016 tokens) per slice; a lane strides 256 chunks
    per = 8016
    big = [[(5 + 256) * 8 + 3, 5 * 8 + 3],            # one lane, two strides
           [300 * 8 + 1, 10 * 8 + 1],                 # two lanes of one slice
           [9 * per + 5, 3 * per + 17],               # two slices
           [15 * per + 100, 128255, 7 * per],         # last slice, last token, a middle slice
           [per, per - 1]]                            # either side of a slice boundary
    small = {1001: [[1000, 500], [1000, 992]],        # V % 8 tail against a chunk
             1003: [[1002, 1001], [1002, 1000]],      # inside the tail
             9: [[8, 2]], 7: [[6, 1]], 8: [[7, 3]]}
    for V, dups in [(128256, big)] + list(small.items()):
        lg = torch.randn(len(dups), V, generator=g).clamp_(max=3.0)
        for r, pos in enumerate(dups):
            lg[r, pos] = 50.0
        assert _greedy(lg.to(dtype)).tolist() == [min(p) for p in dups], V


def test_greedy_tie_across_shards():
    Vs, R = 1001, 4
    g = torch.Generator().manual_seed(4)
    full = torch.randn(3, R * Vs, generator=g).clamp_(max=3.0)
    dups = [[3 * Vs + 2, Vs + 7], [2 * Vs, Vs - 1], [3 * Vs + 1000, 3 * Vs + 999, 5]]
    for r, pos in enumerate(dups):
        full[r, pos] = 50.0
    d_full = full.to(torch.bfloat16).to(DEV)
    temps, seeds = torch.zeros(3, device=DEV), torch.arange(3, dtype=torch.int64, device=DEV)
    allp = torch.stack([ops.sample_shard(d_full[:, r * Vs:(r + 1) * Vs], temps, seeds, r * Vs, R * Vs)
                        for r in range(R)])
    assert ops.pick_pairs(allp).cpu().tolist() == [min(p) for p in dups]
    assert ops.sample(d_full, temps, seeds).cpu().tolist() == [min(p) for p in dups]


def masked_case():
    V, B = 1001, 512
    logits = torch.full((B, V), float("-inf"))
    live = {5: 0.0, 640: 0.5, 1000: -0.3}
    for i, v in live.items():
        logits[:, i] = v
    return logits, torch.ones(B), torch.arange(B, dtype=torch.int64) * 104729 + 13, live


def test_masked_rows_draw_only_live_tokens():
    """All but 3 logits at -inf, as grammar masking leaves them: 512 seeds, every draw exact."""
    logits, temps, seeds, live = masked_case()
    tok = ops.sample(*_dev(logits, temps, seeds)).cpu()
    assert set(tok.tolist()) == set(live)
    check_sampled(tok, sample_ref(logits, temps, seeds)[0], EPS)


# ---- top-k / top-p threshold ----------------------------------------------------------------
def _check_threshold(lg_row, th, kk, pp, tt, tag):
    """The rules of test_kernels_gpu.py::test_topk_topp_threshold_matches_reference for one row."""
    row = lg_row.float()
    V = row.numel()
    th = float(th)
    k_on = 0 < kk < V
    if not k_on and pp >= 1:
        assert th == float("-inf"), f"{tag}: filters off but threshold {th}"
        return
    kept = row >= th
    m = ops.apply_top_k_top_p(lg_row[None].float(), torch.tensor([kk]), torch.tensor([pp]), torch.tensor([tt]))[0]
    ref = torch.isfinite(m)
    assert bool((kept | ~ref).all()), f"{tag}: kernel dropped a reference token"
    extra = kept & ~ref
    assert bool((row[extra] == th).all()), f"{tag}: extra tokens not ties of the threshold"
    if k_on:
        assert int((row > th).sum()) < kk, f"{tag}: k or more tokens above the threshold"
        if pp >= 1:
            assert int(kept.sum()) >= kk, f"{tag}: fewer than k tokens kept"
    if pp < 1:
        surv = row >= (torch.sort(row, descending=True).values[kk - 1] if k_on else -float("inf"))
        probs = torch.softmax(torch.where(surv, row / tt, torch.tensor(-float("inf"))), -1)
        assert float(probs[kept].sum()) >= pp - 1e-3, tag
        assert float(probs[row > th].sum()) < pp + 1e-3, tag


def _threshold_rows(rows, V, dtype):
    """rows: list of (logit row, k, p, T) -> checks each against the kernel's threshold."""
    lg = torch.stack([r[0] for r in rows]).to(dtype)
    k = torch.tensor([r[1] for r in rows], dtype=torch.int32)
    p = torch.tensor([r[2] for r in rows], dtype=torch.float32)
    t = torch.tensor([r[3] for r in rows], dtype=torch.float32)
    th = topk_topp_threshold(*_dev(lg, t, k, p)).cpu()
    for i, (_, kk, pp, tt) in enumerate(rows):
        _check_threshold(lg[i], th[i], kk, pp, tt, f"V={V} row {i} k={kk} p={pp} T={tt}")
    return th


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("V", [1, 5, 300, 1024, 1025])
def test_threshold_edges(V, dtype):
    g = torch.Generator().manual_seed(500 + V)
    rows = []
    for kk in (1, V - 1, V, V + 5):
        for pp, tt in ((1.0, 1.0), (0.6, 0.7), (0.95, 1.3)):
            rows.append((torch.randn(V, generator=g) * 3.0, kk, pp, tt))
    th = _threshold_rows(rows, V, dtype)
    for i, (_, kk, pp, _) in enumerate(rows):
        if kk >= V and pp >= 1:
            assert float(th[i]) == float("-inf")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_threshold_ties_zeros_and_infinities(dtype):
    g = torch.Generator().manual_seed(41)
    V = 1024
    combos = [(3, 1.0, 1.0), (100, 1.0, 1.0), (0, 0.5, 1.0), (100, 0.6, 0.7), (V - 1, 0.9, 1.3)]
    # all-equal row: the threshold is the value, everything is kept
    flat = torch.full((V,), 2.5)
    th = _threshold_rows([(flat, *c) for c in combos], V, dtype)
    assert th.tolist() == [2.5] * len(combos)
    # heavy duplicates at the k-th value: all ties kept, #(> th) < k <= #(>= th)
    coarse = torch.randint(-3, 4, (V,), generator=g).float() * 0.5
    th = _threshold_rows([(coarse, *c) for c in combos], V, dtype)
    for (kk, pp, _), t in zip(combos, th.tolist()):
        if pp >= 1:
            assert int((coarse > t).sum()) < kk <= int((coarse >= t).sum())
    # +0.0 and -0.0 compare equal: a cut at zero keeps both signs
    zeros = torch.randn(V, generator=g)
    zeros[100:140] = 0.0
    zeros[300:340] = -0.0
    above = int((zeros > 0).sum())
    for kk in (above + 1, above + 40, above + 41, above + 80):
        th = _threshold_rows([(zeros, kk, 1.0, 1.0)], V, dtype)
        assert float(th[0]) == 0.0 and int((zeros.to(dtype).float() >= th[0]).sum()) == above + 80
    # -inf entries (masked tokens): never above a finite threshold; k beyond the finite ones keeps all
    holes = torch.randn(V, generator=g) * 3.0
    holes[::3] = float("-inf")
    finite = int(torch.isfinite(holes).sum())
    th = _threshold_rows([(holes, 50, 1.0, 1.0), (holes, 0, 0.8, 1.0), (holes, finite, 0.9, 0.7),
                          (holes, finite + 10, 1.0, 1.0)], V, dtype)
    assert float(th[3]) == float("-inf") and all(np.isfinite(th[:3].tolist()))


def boundary_is_clear(row, kk, pp, tt):
    """(ok, why): the k-th and (k+1)-th values differ, and the nucleus mass on either side of the
    cut is at least 1e-3 away from p (fp64)."""
    s = np.sort(to_np(row, np.float64))[::-1]
    if 0 < kk < s.size:
        if s[kk - 1] == s[kk]:
            return False, "tie at the top-k boundary"
        s = s[:kk]
    if pp < 1:
        pr = np.exp((s - s[0]) / tt)
        pr /= pr.sum()
        above = np.cumsum(pr) - pr                        # mass strictly above each token
        cut = int((above < pp).sum())                     # tokens kept
        if pp - above[cut - 1] < 1e-3:
            return False, "nucleus mass within 1e-3 below p"
        if cut < s.size and above[cut] - pp < 1e-3:
            return False, "nucleus mass within 1e-3 above p"
    return True, ""


def filtered_sampled_case():
    """fp32 logits chosen so that the top-k / nucleus boundary is clear of ties and roundings:
    each row is the first of a seeded sequence of N(0, 4T) rows that passes boundary_is_clear
    (peaked enough that single tokens near the cut hold more than 2e-3 of the mass)."""
    V = 1024
    combos = [(20, 1.0), (0, 0.8), (50, 0.9), (1, 1.0), (5, 0.5), (0, 0.3), (V + 5, 0.6), (300, 1.0)]
    rows, ks, ps, ts = [], [], [], []
    for ci, (kk, pp) in enumerate(combos):
        for ti, tt in enumerate((0.5, 1.0, 2.0)):
            for attempt in range(200):
                g = torch.Generator().manual_seed(900 + 1000 * attempt + 10 * ci + ti)
                row = torch.randn(V, generator=g) * 4.0 * tt
                if boundary_is_clear(row, kk, pp, tt)[0]:
                    break
            rows.append(row), ks.append(kk), ps.append(pp), ts.append(tt)
    B = len(rows)
    seeds = torch.arange(B, dtype=torch.int64) * 7919 + 29
    return (torch.stack(rows), torch.tensor(ks, dtype=torch.int32), torch.tensor(ps, dtype=torch.float32),
            torch.tensor(ts, dtype=torch.float32), seeds)


def assert_boundary_is_clear(logits, k, p, temps):
    for b in range(logits.shape[0]):
        ok, why = boundary_is_clear(logits[b], int(k[b]), float(p[b]), float(temps[b]))
        assert ok, f"row {b}: {why}"


def test_filtered_rows_sample_exactly():
    logits, k, p, temps, seeds = filtered_sampled_case()
    assert_boundary_is_clear(logits, k, p, temps)
    keep = torch.isfinite(ops.apply_top_k_top_p(logits, k, p, temps))
    scores, _, ids = sample_ref(logits, temps, seeds, keep=keep)
    assert bool(keep[torch.arange(len(ids)), torch.from_numpy(ids)].all())
    tok = ops.sample(*_dev(logits, temps, seeds), top_k=k.to(DEV), top_p=p.to(DEV)).cpu()
    check_sampled(tok, scores, EPS)
    unfiltered = sample_ref(logits, temps, seeds)[2]
    assert (unfiltered != ids).any()                  # the filter decides some of these rows


# =============================================================================================
# filtered top-k
# =============================================================================================
SENTINEL = -(1 << 62)


def _search(corpus, users, dates, queries, q_user, q_floor, ks, kmax, cap=65536):
    """Run the kernel on CPU-built inputs and pass the result through the certificate."""
    out = ops.filtered_topk(*_dev(corpus, users, dates, queries, q_user, q_floor, ks), kmax, cap)
    ids, sc, cnt = (x.cpu() for x in out)
    assert ids.dtype == torch.int32 and sc.dtype == torch.float32 and cnt.dtype == torch.int32
    check_topk_certificate(ids, sc, cnt, corpus, users, dates, queries, q_user, q_floor, ks, kmax)
    return ids, sc, cnt


def _i32(x):
    return torch.tensor(x, dtype=torch.int32)


def _i64(x):
    return torch.tensor(x, dtype=torch.int64)


def _vectors(n, D, g):
    return torch.randn(n, D, generator=g).to(torch.bfloat16)


@pytest.mark.parametrize("N", [1, 255, 256, 257, 5000])
def test_topk_row_counts(N):
    g = torch.Generator().manual_seed(N)
    corpus = _vectors(N, 8, g)
    users = torch.randint(0, 3, (N,), generator=g, dtype=torch.int32)
    users[N - 1] = 1                                 # the last row matches a query
    dates = torch.randint(-100, 100, (N,), generator=g, dtype=torch.int64)
    ids, _, cnt = _search(corpus, users, dates, _vectors(4, 8, g), _i32([0, 1, 2, 1]), _i64([0, SENTINEL, -50, 0]),
                          _i32([5, N, 3, 2]), 8)
    assert int(cnt[1]) == min(8, int((users == 1).sum()))


def test_topk_second_grid_stride_pass():
    """N > 4096 x 256: rows from 2^20 on are reached by the second pass of filter_compact."""
    N = 4096 * 256 + 300
    g = torch.Generator().manual_seed(17)
    corpus = _vectors(N, 8, g)
    users = torch.full((N,), 9, dtype=torch.int32)
    low = torch.randperm(1 << 20, generator=g)[:20]
    high = torch.cat([torch.tensor([1 << 20, N - 1]), (1 << 20) + 1 + torch.randperm(298, generator=g)[:28]])
    users[low] = 0
    users[high] = 0
    dates = torch.zeros(N, dtype=torch.int64)
    dates[high[:5]] = -1                              # five of the far rows fail query 2's floor
    ids, _, cnt = _search(corpus, users, dates, _vectors(3, 8, g), _i32([0, 0, 0]), _i64([SENTINEL, SENTINEL, 0]),
                          _i32([64, 5, 64]), 64)
    assert cnt.tolist() == [50, 5, 45]
    assert int((ids[0, :50] >= (1 << 20)).sum()) == 30 and int((ids[2, :45] >= (1 << 20)).sum()) == 25


@pytest.mark.parametrize("D", [8, 64, 384, 520, 768, 1024])
def test_topk_vector_widths(D):
    """D = 520 is 65 chunks of 8: one lane takes a second chunk; 1024 fills both."""
    g = torch.Generator().manual_seed(D)
    N = 300
    users = torch.randint(0, 3, (N,), generator=g, dtype=torch.int32)
    dates = torch.randint(0, 100, (N,), generator=g, dtype=torch.int64)
    _search(_vectors(N, D, g), users, dates, _vectors(3, D, g), _i32([0, 1, 2]), _i64([0, 50, SENTINEL]),
            _i32([10, 200, 1]), 16)


@pytest.mark.parametrize("D", [1032, 12])
def test_topk_bad_width_raises_and_writes_nothing(D):
    g = torch.Generator().manual_seed(D)
    N = 64
    users, dates = torch.zeros(N, dtype=torch.int32), torch.zeros(N, dtype=torch.int64)
    args = (_i32([0, 0]), _i64([0, 0]), _i32([4, 4]), 4)
    _search(_vectors(N, 8, g), users, dates, _vectors(2, 8, g), *args)       # sizes the workspace for (2, N)
    ws = retrieval_ops._WS
    ws.counts.fill_(7), ws.cand.fill_(7), ws.scores.fill_(7.0)
    with pytest.raises(RuntimeError):
        ops.filtered_topk(*_dev(_vectors(N, D, g), users, dates, _vectors(2, D, g), *args[:3]), 4)
    torch.cuda.synchronize()
    assert bool((ws.counts == 7).all()) and bool((ws.cand == 7).all()) and bool((ws.scores == 7.0).all())


def test_topk_query_counts():
    """1, 64, 65 (split 64 + 1) and 130 queries, one after another in this process: the workspace
    is reallocated between the launches."""
    g = torch.Generator().manual_seed(23)
    N = 2000
    corpus = _vectors(N, 8, g)
    users = torch.randint(0, 40, (N,), generator=g, dtype=torch.int32)
    dates = torch.randint(0, 1000, (N,), generator=g, dtype=torch.int64)
    for nq in (1, 64, 65, 130):
        q_user = (torch.arange(nq, dtype=torch.int32) * 7) % 43 - 1           # -1 and 40, 41: nobody
        q_floor = torch.where(torch.arange(nq) % 3 == 0, SENTINEL, torch.randint(0, 1000, (nq,), generator=g))
        ks = torch.randint(0, 13, (nq,), generator=g, dtype=torch.int32)
        _, _, cnt = _search(corpus, users, dates, _vectors(nq, 8, g), q_user, q_floor.to(torch.int64), ks, 8)
        assert cnt.shape == (nq,)


def _users_with_counts(N, counts, g):
    """user code u gets exactly counts[u] rows at random positions, the rest code 99"""
    users = torch.full((N,), 99, dtype=torch.int32)
    perm = torch.randperm(N, generator=g)
    at = 0
    for u, c in counts.items():
        users[perm[at:at + c]] = u
        at += c
    return users


def test_topk_candidate_counts():
    """0 .. 8192 candidates are selected in the kernel; 8193 is finished on the host from the
    candidate list."""
    counts = {1: 1, 2: 2, 3: 3, 4: 4097, 5: 8191, 6: 8192, 7: 8193}
    g = torch.Generator().manual_seed(29)
    N = 40000
    corpus = _vectors(N, 8, g)
    users = _users_with_counts(N, counts, g)
    dates = torch.zeros(N, dtype=torch.int64)
    q_user = _i32(list(range(8)))
    _, _, cnt = _search(corpus, users, dates, _vectors(8, 8, g), q_user, _i64([0] * 8), _i32([10] * 8), 16)
    assert cnt.tolist() == [0, 1, 2, 3, 10, 10, 10, 10]
    # every candidate returned: the whole sort network's output, and the host finish, in full
    _, _, cnt = _search(corpus, users, dates, _vectors(3, 8, g), _i32([5, 6, 7]), _i64([0] * 3), _i32([9000] * 3), 9000)
    assert cnt.tolist() == [8191, 8192, 8193]


def test_topk_cap_overflow():
    """More matches than the 65536-entry candidate list: the full-matrix fallback."""
    g = torch.Generator().manual_seed(31)
    N = 70000
    corpus = _vectors(N, 8, g)
    users = _users_with_counts(N, {1: 66000, 2: 3000}, g)
    dates = torch.randint(0, 10, (N,), generator=g, dtype=torch.int64)
    _, _, cnt = _search(corpus, users, dates, _vectors(3, 8, g), _i32([1, 2, 1]), _i64([SENTINEL, 0, 0]),
                        _i32([10, 10, 300]), 300)
    assert cnt.tolist() == [10, 10, 300]


def test_topk_filter_semantics():
    """64-bit dates (values that differ only above bit 32, negatives), date == floor included,
    floor - 1 excluded, the no-floor sentinel, user code -1."""
    H = 1 << 32
    dates0 = [2 * H + 5, 2 * H + 4, H + 9, 3 * H + 1, 3 * H + 5, -5, -(1 << 40), 0, (1 << 62) + 1, 5]
    g = torch.Generator().manual_seed(37)
    n0 = len(dates0)
    N = n0 + 20
    corpus = _vectors(N, 8, g)
    users = torch.cat([torch.zeros(n0, dtype=torch.int32), torch.full((20,), 1, dtype=torch.int32)])
    dates = torch.cat([_i64(dates0), torch.full((20,), 3 * H, dtype=torch.int64)])
    floors = [2 * H + 5, -10, SENTINEL, SENTINEL, -(1 << 40), -(1 << 40) + 1, 6]
    q_user = _i32([0, 0, 0, -1, 0, 0, 0])
    ids, _, cnt = _search(corpus, users, dates, _vectors(7, 8, g), q_user, _i64(floors), _i32([16] * 7), 16)
    got = [sorted(ids[i, :int(cnt[i])].tolist()) for i in range(7)]
    assert got[0] == [0, 3, 4, 8]                      # == floor in, floor - 1 out, low words irrelevant
    assert got[1] == [0, 1, 2, 3, 4, 5, 7, 8, 9]       # negative floor: -5 in, -2^40 out
    assert got[2] == list(range(n0))                   # sentinel: no date filter
    assert got[3] == []                                # user code -1 matches nothing
    assert got[4] == list(range(n0)) and got[5] == [0, 1, 2, 3, 4, 5, 7, 8, 9]
    assert got[6] == [0, 1, 2, 3, 4, 8]


def test_topk_limits():
    g = torch.Generator().manual_seed(43)
    N = 300
    corpus = _vectors(N, 8, g)
    users = _users_with_counts(N, {0: 100}, g)
    dates = torch.zeros(N, dtype=torch.int64)
    for kmax, want in ((20, [0, 20, 20, 1]), (200, [0, 100, 50, 1])):
        _, _, cnt = _search(corpus, users, dates, _vectors(4, 8, g), _i32([0] * 4), _i64([0] * 4),
                            _i32([0, 500, 50, 1]), kmax)
        assert cnt.tolist() == want


# (N, rows of the heavy user): select in the kernel; host finish from the candidate list
# (> 8192 candidates); host finish from the full score matrix (> 65536 candidates)
TIE_PATHS = {"kernel": (5000, 3000), "host_list": (20000, 9000), "host_full": (70000, 66000)}


def tie_case(path):
    """40 rows of the heavy user share one vector (the query itself, the best score by far), at
    random row ids: bit-equal scores at the top of the list and across the k = 25 cut."""
    N, heavy = TIE_PATHS[path]
    g = torch.Generator().manual_seed(N)
    corpus = _vectors(N, 8, g)
    users = _users_with_counts(N, {0: heavy}, g)
    mine = (users == 0).nonzero().flatten()
    dup = mine[torch.randperm(heavy, generator=g)[:40]].sort().values
    v = torch.full((8,), 4.0, dtype=torch.bfloat16)
    corpus[dup] = v
    queries = torch.stack([v, v, _vectors(1, 8, g)[0]])
    return (corpus, users, torch.zeros(N, dtype=torch.int64), queries, _i32([0, 0, 0]), _i64([0, 0, 0]),
            _i32([25, 60, 60]), 64), dup


@pytest.mark.parametrize("path", list(TIE_PATHS))
def test_topk_ties_come_back_by_ascending_row_id(path):
    args, dup = tie_case(path)
    ids, sc, cnt = _search(*args)
    assert cnt.tolist() == [25, 60, 60]
    assert ids[0, :25].tolist() == dup[:25].tolist()
    assert ids[1, :40].tolist() == dup.tolist() and not bool(torch.isin(ids[1, 40:60], dup).any())
    assert float(sc[1, 0]) == float(sc[1, 39]) == 128.0
    # the third query ranks the duplicates wherever they fall: still one run of ascending ids
    where = torch.isin(ids[2, :60], dup).nonzero().flatten()
    if where.numel():
        assert ids[2, where].tolist() == dup[:where.numel()].tolist()
        assert where.tolist() == list(range(int(where[0]), int(where[0]) + where.numel()))


@pytest.mark.parametrize("path", ["kernel", "host_list"])
def test_topk_is_bitwise_repeatable(path):
    args, _ = tie_case(path)
    dev_args = _dev(*args[:7])
    a = ops.filtered_topk(*dev_args, args[7])
    b = ops.filtered_topk(*dev_args, args[7])
    for x, y in zip(a, b):
        assert torch.equal(x.cpu(), y.cpu())
