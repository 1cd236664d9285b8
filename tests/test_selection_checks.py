"""The checkers of ``selection_ref`` catch a subtly wrong sampler or top-k kernel (CPU only).

Each test builds a correct answer with the host reference, shows that the checker accepts it, then
applies one mutation of the kind a kernel bug produces and shows that the checker rejects it.  The
noise replica is checked for the properties the GPU sampler relies on (finite, strictly inside
(0, 1), Gumbel moments), and the float32 arithmetic of the former 24-bit formula is pinned.
"""
import math

import numpy as np
import pytest
import torch

from financial_chatbot_llm_amd.ops.retrieval import filtered_topk_ref
from selection_ref import (check_sampled, check_topk_certificate, gumbel_noise_ref, noise_bits, sample_ref, to_np,
                           topk_tol_row, u01_from_bits, u01_from_bits_24bit)

EPS = 1e-4     # far below the ~1 gap a wrong token shows; the GPU tests derive their own


# ---------------------------------------------------------------------------------------------
# noise replica
# ---------------------------------------------------------------------------------------------
def test_u01_is_strictly_inside_unit_interval_for_every_mantissa():
    b = np.arange(1 << 23, dtype=np.uint32) << np.uint32(9)
    u = u01_from_bits(b)
    assert u.dtype == np.float32
    assert float(u.min()) > 0.0 and float(u.max()) < 1.0
    # exact in float32: the float64 evaluation of the same formula gives the same values
    exact = ((b >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    assert np.array_equal(u.astype(np.float64), exact)
    assert np.unique(u).size == 1 << 23          # no two mantissas collapse
    # the low 9 bits are ignored, including all-ones
    assert np.array_equal(u01_from_bits(b | np.uint32(0x1FF)), u)
    n = -np.log(-np.log(u.astype(np.float64)))
    assert np.isfinite(n).all()
    assert float(n.max()) < 16.7 and float(n.min()) > -2.9


def test_noise_is_finite_for_all_24_bit_inputs():
    """Every value of the 24 bits the former formula consumed (hence every 32-bit input: the rest
    are shifted out) gives finite noise now."""
    b = np.arange(1 << 24, dtype=np.uint32) << np.uint32(8)
    u = u01_from_bits(b)
    assert float(u.min()) > 0.0 and float(u.max()) < 1.0
    assert np.isfinite(-np.log(-np.log(u.astype(np.float64)))).all()
    assert 0.0 < float(u01_from_bits(np.uint32(0xFFFFFFFF))) < 1.0
    assert 0.0 < float(u01_from_bits(np.uint32(0))) < 1.0


def test_former_24_bit_formula_rounds_to_one():
    """x + 0.5f is not representable from 2^23 upwards: at x = 2^24 - 1 it rounds to 2^24, u is
    exactly 1.0f and -log(-log(u)) is +inf.  Pure float32 arithmetic; documents the bug."""
    top = np.uint32(0xFFFFFF00)
    assert float(u01_from_bits_24bit(top)) == 1.0
    x = np.float32(2 ** 24 - 1)
    assert x + np.float32(0.5) == np.float32(2 ** 24)
    # the fused form x * 2^-24 + 2^-25 rounds to 1.0 as well
    assert np.float32(float(x) * 2.0 ** -24 + 2.0 ** -25) == np.float32(1.0)
    with np.errstate(divide="ignore"):
        assert np.isposinf(-np.log(-np.log(np.float64(u01_from_bits_24bit(top)))))
    # neighbouring mantissas collapse in pairs above 2^23
    hi = (np.arange(1 << 23, 1 << 24, dtype=np.uint32)) << np.uint32(8)
    assert np.unique(u01_from_bits_24bit(hi)).size < hi.size
    # two (seed, token id) pairs within the Llama-3 vocabulary that draw that mantissa
    for seed, idx in ((411791, 47583), (704794, 98048)):
        assert int(noise_bits(seed, idx)) >> 8 == (1 << 24) - 1
        assert np.isfinite(gumbel_noise_ref(seed, idx))


def test_noise_moments_match_gumbel():
    seeds = (np.arange(16, dtype=np.int64) * 7919 + 3)[:, None]
    n = gumbel_noise_ref(seeds, np.arange(1 << 16, dtype=np.int64)[None, :]).ravel()
    assert n.size >= 10 ** 6
    assert abs(float(n.mean()) - 0.5772156649) < 0.01
    assert abs(float(n.var()) - math.pi ** 2 / 6) < 0.02
    # the token index and the seed both enter: shifting either changes every draw
    a = gumbel_noise_ref(5, np.arange(64))
    assert not np.isclose(a, gumbel_noise_ref(5, np.arange(64) + 1)).any()
    assert not np.isclose(a, gumbel_noise_ref(6, np.arange(64))).any()
    # negative seeds wrap like the kernel's unsigned read
    assert np.array_equal(noise_bits(-1, np.arange(8)), noise_bits(np.uint64(2 ** 64 - 1), np.arange(8)))


def test_mix64_known_answer():
    """splitmix64's first outputs for state 0 (public test vector of the generator)."""
    from selection_ref import mix64
    assert int(mix64(np.uint64(0))) == 0xE220A8397B1DCDAF
    assert int(mix64(np.uint64(0x9E3779B97F4A7C15))) == 0x6E789E6AA1B965F4


# ---------------------------------------------------------------------------------------------
# check_sampled
# ---------------------------------------------------------------------------------------------
def _sampler_case(B=48, V=1001, voff=3000):
    g = torch.Generator().manual_seed(21)
    logits = torch.randn(B, V, generator=g) * 3.0
    for b in range(0, B, 3):                       # some winners in the last slice and in the V % 8 tail
        logits[b, V - 1 - b % 30] += 12.0
    temps = torch.tensor([0.5, 1.0, 2.0, 0.0] * (B // 4))
    seeds = torch.arange(B, dtype=torch.int64) * 7919 + 3
    return logits, temps, seeds, voff


def _argmax_with_noise(logits, temps, noise):
    """A sampler 'kernel' on the host: argmax of logit/T + the given noise (greedy rows: logits)."""
    lg, t = to_np(logits, np.float64), to_np(temps, np.float64)
    s = np.where((t > 0)[:, None], lg / np.where(t > 0, t, 1.0)[:, None] + noise, lg)
    return s.argmax(1)


def test_check_sampled_accepts_the_reference_and_rejects_mutations():
    logits, temps, seeds, voff = _sampler_case()
    B, V = logits.shape
    scores, best, ids = sample_ref(logits, temps, seeds, voff=voff)
    greedy = temps <= 0
    short = check_sampled(ids, scores, EPS, voff=voff, greedy=greedy)
    assert float(short.max()) == 0.0
    assert np.array_equal(ids[to_np(greedy)] - voff, to_np(logits)[to_np(greedy)].argmax(1))
    sd = to_np(seeds)[:, None]
    cols = np.arange(V, dtype=np.int64)[None, :]

    # noise indexed idx instead of idx + 1
    wrong = _argmax_with_noise(logits, temps, gumbel_noise_ref(sd, cols + voff - 1)) + voff
    with pytest.raises(AssertionError):
        check_sampled(wrong, scores, EPS, voff=voff, greedy=greedy)
    # voff ignored in the noise index
    wrong = _argmax_with_noise(logits, temps, gumbel_noise_ref(sd, cols)) + voff
    with pytest.raises(AssertionError):
        check_sampled(wrong, scores, EPS, voff=voff, greedy=greedy)
    # voff ignored in the returned id
    with pytest.raises(AssertionError):
        check_sampled(ids - voff, scores, EPS, voff=voff, greedy=greedy)
    # the last of 16 slices never scanned (chunks of 8 tokens, ceil(chunks / 16) per slice)
    per = -(-(V // 8) // 16) * 8
    cut = scores.copy()
    cut[:, 15 * per:] = -np.inf
    wrong = cut.argmax(1) + voff
    assert (wrong != ids).any()
    with pytest.raises(AssertionError):
        check_sampled(wrong, scores, EPS, voff=voff, greedy=greedy)
    # an infinite noise value injected at one token of every sampled row
    noise = gumbel_noise_ref(sd, cols + voff)
    noise[:, 123] = np.inf
    wrong = _argmax_with_noise(logits, temps, noise) + voff
    with pytest.raises(AssertionError):
        check_sampled(wrong, scores, EPS, voff=voff, greedy=greedy)
    # a greedy tie resolved to the larger index
    tied = logits.clone()
    tied[3, 10] = tied[3, 700] = 99.0
    s2, _, i2 = sample_ref(tied, temps, seeds, voff=voff)
    assert int(i2[3]) == voff + 10
    check_sampled(i2, s2, EPS, voff=voff, greedy=greedy)
    i2[3] = voff + 700
    with pytest.raises(AssertionError):
        check_sampled(i2, s2, EPS, voff=voff, greedy=greedy)


def test_check_sampled_never_skips_a_row():
    logits, temps, seeds, voff = _sampler_case()
    scores, _, ids = sample_ref(logits, temps, seeds, voff=voff)
    for row in (0, 17, len(ids) - 1):
        bad = ids.copy()
        bad[row] = voff + (int(ids[row]) - voff + 1) % logits.shape[1]
        with pytest.raises(AssertionError):
            check_sampled(bad, scores, EPS, voff=voff)
    with pytest.raises(AssertionError):        # an id outside the shard
        bad = ids.copy()
        bad[5] = voff + logits.shape[1]
        check_sampled(bad, scores, EPS, voff=voff)


def test_sample_ref_keep_mask_and_wrong_token_gap():
    logits, temps, seeds, _ = _sampler_case()
    keep = torch.zeros_like(logits, dtype=torch.bool)
    keep[:, ::7] = True
    scores, best, ids = sample_ref(logits, temps, seeds, keep=keep)
    samp = to_np(temps) > 0
    assert (ids[samp] % 7 == 0).all()                              # sampled rows stay inside keep
    assert np.array_equal(ids[~samp], to_np(logits)[~samp].argmax(1))   # greedy rows ignore it
    # the runner-up of a Gumbel-max row trails the winner by order 1: eps has room by 4 decimal orders
    full, _, _ = sample_ref(logits, temps, seeds)
    top2 = np.sort(full[samp], axis=1)[:, -2:]
    assert float(np.median(top2[:, 1] - top2[:, 0])) > 0.2


def test_reference_filter_is_off_at_p_one():
    """apply_top_k_top_p with p >= 1 keeps all k survivors: the fp32 cumulative mass above the tail
    tokens rounds up to 1.0, which used to drop them."""
    from financial_chatbot_llm_amd.ops import apply_top_k_top_p
    g = torch.Generator().manual_seed(1525)
    lg = torch.randn(4, 1025, generator=g) * 3.0
    k = torch.tensor([1024, 300, 0, 1024], dtype=torch.int32)
    kept = torch.isfinite(apply_top_k_top_p(lg, k, torch.ones(4), torch.ones(4))).sum(1)
    assert kept.tolist() == [1024, 300, 1025, 1024]


# ---------------------------------------------------------------------------------------------
# check_topk_certificate
# ---------------------------------------------------------------------------------------------
def _topk_case():
    g = torch.Generator().manual_seed(31)
    N, D, kmax = 600, 64, 12
    corpus = torch.randn(N, D, generator=g).to(torch.bfloat16)
    users = torch.randint(0, 3, (N,), generator=g, dtype=torch.int32)
    dates = torch.randint(-50, 50, (N,), generator=g, dtype=torch.int64)
    dup = (users == 1).nonzero().flatten()[5:45:4]       # bit-equal vectors -> bit-equal scores
    corpus[dup] = corpus[dup[0]].clone()
    queries = torch.randn(4, D, generator=g).to(torch.bfloat16)
    queries[1] = corpus[dup[0]].clone()                          # the duplicates lead query 1
    q_user = torch.tensor([0, 1, 2, 7], dtype=torch.int32)
    q_floor = torch.tensor([0, -(1 << 62), 10, 0], dtype=torch.int64)
    ks = torch.tensor([12, 8, 5, 3], dtype=torch.int32)
    return dict(corpus=corpus, users=users, dates=dates, queries=queries, q_user=q_user, q_floor=q_floor, ks=ks,
                kmax=kmax), dup


def _ref(case):
    ids, sc, cnt = filtered_topk_ref(case["corpus"], case["users"], case["dates"], case["queries"],
                                     case["q_user"].tolist(), case["q_floor"].tolist(), case["ks"].tolist(),
                                     case["kmax"])
    return ids.clone(), sc.clone(), cnt.clone()


def _true_score(case, row, qi):
    return float(case["corpus"][row].double() @ case["queries"][qi].double())


def test_certificate_accepts_the_reference():
    case, dup = _topk_case()
    ids, sc, cnt = _ref(case)
    check_topk_certificate(ids, sc, cnt, **case)
    assert cnt.tolist() == [12, 8, 5, 0]
    assert ids[1, :8].tolist() == dup[:8].tolist()       # ties by ascending row id
    assert float(sc[1, 0]) == float(sc[1, 7])


MUTATIONS = ["swap_adjacent", "drop_best", "other_user", "below_floor", "count_minus_one", "count_plus_one",
             "ties_descending", "score_4tol", "duplicate_id", "dirty_tail"]


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_certificate_rejects(mutation):
    case, dup = _topk_case()
    ids, sc, cnt = _ref(case)
    users, dates = case["users"], case["dates"]
    if mutation == "swap_adjacent":
        ids[0, [3, 4]] = ids[0, [4, 3]]
        sc[0, [3, 4]] = sc[0, [4, 3]]
    elif mutation == "drop_best":                        # rest shifted up, the 13th-best fills the end
        rows = ((users == 0) & (dates >= 0)).nonzero().flatten()
        s = case["corpus"][rows].float() @ case["queries"][0].float()
        order = torch.sort(-s, stable=True).indices
        ids[0] = rows[order[1:13]].to(torch.int32)
        sc[0] = s[order[1:13]]
    elif mutation == "other_user":
        row = int((users == 2).nonzero()[0])
        ids[0, 6], sc[0, 6] = row, _true_score(case, row, 0)
    elif mutation == "below_floor":
        row = int(((users == 2) & (dates == 9)).nonzero()[0])      # floor of query 2 is 10
        ids[2, 4], sc[2, 4] = row, _true_score(case, row, 2)
    elif mutation == "count_minus_one":
        cnt[0] -= 1
        ids[0, 11], sc[0, 11] = -1, 0.0
    elif mutation == "count_plus_one":
        row = int(((users == 2) & (dates >= 10)).nonzero()[-1])
        cnt[2] += 1
        ids[2, 5], sc[2, 5] = row, _true_score(case, row, 2)
    elif mutation == "ties_descending":
        ids[1, [2, 3]] = ids[1, [3, 2]]
    elif mutation == "score_4tol":
        row = int(ids[0, 5])
        tol = float(topk_tol_row(to_np(case["corpus"][row:row + 1], np.float64), to_np(case["queries"][0], np.float64))[0])
        sc[0, 5] = float(sc[0, 5]) - 4 * tol
        assert float(sc[0, 6]) < float(sc[0, 5]) < float(sc[0, 4])      # still in order: only the value is off
    elif mutation == "duplicate_id":
        ids[0, 7], sc[0, 7] = ids[0, 6], sc[0, 6]
    elif mutation == "dirty_tail":
        ids[2, 9] = 4
    with pytest.raises(AssertionError):
        check_topk_certificate(ids, sc, cnt, **case)


def test_certificate_tolerance_is_tight_but_sufficient():
    """A float32 dot product summed in another order than the reference's stays inside tol_row."""
    case, _ = _topk_case()
    ids, sc, cnt = _ref(case)
    rows = to_np(case["corpus"], np.float32)[to_np(ids[0, :12], np.int64)]
    q = to_np(case["queries"][0], np.float32)
    acc = np.zeros(12, dtype=np.float32)
    for j in reversed(range(q.size)):                    # sequential float32, reversed order
        acc = (acc + rows[:, j] * q[j]).astype(np.float32)
    sc[0, :12] = torch.from_numpy(acc)
    order = np.lexsort((to_np(ids[0, :12]), -acc))
    ids[0, :12], sc[0, :12] = ids[0, :12][order], sc[0, :12][order]
    check_topk_certificate(ids, sc, cnt, **case)
    # relative to the magnitude sum it is 32 float32 half-ulps, whatever the vectors' scale
    tol = topk_tol_row(rows.astype(np.float64), q.astype(np.float64))
    assert np.allclose(tol / (np.abs(rows.astype(np.float64)) @ np.abs(q.astype(np.float64))), 32 * 2.0 ** -24)
