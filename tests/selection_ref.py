"""Host references and checkers for the two kernels with discrete answers: the Gumbel-max sampler
(``sampler.hip``) and the filtered top-k search (``retrieval.hip``).

Everything here is numpy in float64 (the noise bits in uint64 wrap-around arithmetic), takes torch
or numpy inputs, and never touches a device.  The checkers raise ``AssertionError`` naming the
first offending row; they test a result for VALIDITY against the fp64 scores (a token whose score
is the row's best, a top-k list that is a correct answer), not for equality with another
implementation's output, so they hold for any summation order a kernel may use.
"""
from __future__ import annotations

import numpy as np
import torch

_U64 = np.uint64
_GOLD = _U64(0x9E3779B97F4A7C15)
_M1 = _U64(0xBF58476D1CE4E5B9)
_M2 = _U64(0x94D049BB133111EB)
_IDX = _U64(0xD1B54A32D192ED03)


def to_np(x, dtype=None):
    """torch (any dtype, bf16 included) or array-like -> numpy, exact."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu()
        if x.dtype == torch.bfloat16:
            x = x.float()
        x = x.numpy()
    x = np.asarray(x)
    return x if dtype is None else x.astype(dtype)


def _as_u64(x):
    """int64 (negative values wrap, as the kernel reads seeds as unsigned long long) -> uint64"""
    x = np.asarray(to_np(x))
    if x.dtype == np.uint64:
        return x
    return x.astype(np.int64).astype(np.uint64)


def mix64(z):
    """``common.h`` mix64 (splitmix64 finaliser) on uint64 arrays."""
    with np.errstate(over="ignore"):
        z = _as_u64(z) + _GOLD
        z = (z ^ (z >> _U64(30))) * _M1
        z = (z ^ (z >> _U64(27))) * _M2
        return z ^ (z >> _U64(31))


def noise_bits(seed, idx):
    """The 32 random bits ``gumbel_noise(seed, idx)`` feeds to ``u01_from_bits``."""
    with np.errstate(over="ignore"):
        r = mix64(_as_u64(seed) ^ (_IDX * (_as_u64(idx) + _U64(1))))
    return (r & _U64(0xFFFFFFFF)).astype(np.uint32)


def u01_from_bits(b):
    """``common.h`` u01_from_bits, formed as the kernel forms it: every step is exact in float32
    (23 bits + 0.5 needs 24 significant bits; the scale is a power of two)."""
    x = (np.asarray(b, dtype=np.uint32) >> np.uint32(9)).astype(np.float32)
    return (x + np.float32(0.5)) * np.float32(2.0 ** -23)


def u01_from_bits_24bit(b):
    """The formula ``u01_from_bits`` used before: 24 bits + 0.5 does not fit a float32 significand
    from 2^23 upwards, and rounds to exactly 1.0 at the top.  Kept to document that bug."""
    x = (np.asarray(b, dtype=np.uint32) >> np.uint32(8)).astype(np.float32)
    return (x + np.float32(0.5)) * np.float32(2.0 ** -24)


def gumbel_noise_ref(seed, idx):
    """float64 Gumbel noise of (seed, idx): the kernel's exact u, then -log(-log(u)) in fp64."""
    u = u01_from_bits(noise_bits(seed, idx)).astype(np.float64)
    return -np.log(-np.log(u))


def sample_ref(logits, temps, seeds, voff=0, keep=None):
    """-> (scores [B, V] f64, best [B] f64, ids [B] int64 GLOBAL token ids).

    Sampled rows (T > 0): score_i = logit_i / T + noise(seed, voff + i), -inf where ``keep`` (the
    boolean mask of top-k / top-p survivors) is False.  Greedy rows (T <= 0): score_i = logit_i,
    ``keep`` ignored, as in the kernel.  ids: the first index of the best score, plus voff."""
    lg = to_np(logits, np.float64)
    B, V = lg.shape
    t = to_np(temps, np.float64).reshape(B)
    sd = _as_u64(seeds).reshape(B)
    sampled = t > 0
    idx = (np.arange(V, dtype=np.int64) + int(voff))[None, :]
    scores = lg.copy()
    if sampled.any():
        rows = np.nonzero(sampled)[0]
        noise = gumbel_noise_ref(sd[rows][:, None], idx)
        with np.errstate(invalid="ignore"):
            scores[rows] = lg[rows] / t[rows][:, None] + noise
        if keep is not None:
            kp = to_np(keep).astype(bool)
            sub = scores[rows]
            sub[~kp[rows]] = -np.inf
            scores[rows] = sub
    ids = scores.argmax(1)
    best = scores[np.arange(B), ids]
    return scores, best, ids.astype(np.int64) + int(voff)


def check_sampled(tokens, ref_scores, eps, voff=0, greedy=None):
    """Every row's token must score within ``eps`` of the row's best fp64 score:
    ``ref_scores[row, token - voff] >= best - eps``.  No row is skipped.  Rows flagged in
    ``greedy`` have exact scores, so there the token must be the FIRST index of the maximum.
    Returns each row's shortfall (best - score of the chosen token)."""
    tok = to_np(tokens, np.int64).reshape(-1)
    B, V = ref_scores.shape
    assert tok.shape[0] == B, f"{tok.shape[0]} tokens for {B} rows"
    loc = tok - int(voff)
    bad = np.nonzero((loc < 0) | (loc >= V))[0]
    assert bad.size == 0, f"row {bad[0]}: token {tok[bad[0]]} outside [{voff}, {voff + V})"
    best = ref_scores.max(1)
    assert np.isfinite(best).all(), "reference best score is not finite"
    got = ref_scores[np.arange(B), loc]
    short = best - got
    ok = got >= best - eps
    if greedy is not None:
        g = to_np(greedy).astype(bool).reshape(B)
        ok &= ~g | (loc == ref_scores.argmax(1))
    bad = np.nonzero(~ok)[0]
    assert bad.size == 0, (f"{bad.size} of {B} rows wrong; row {bad[0]}: token {tok[bad[0]]} scores {got[bad[0]]!r}, "
                           f"best {best[bad[0]]!r} at {ref_scores[bad[0]].argmax() + voff}")
    return short


def score_floor_f32(logits, temps, seeds, voff=0):
    """Largest |float32 score - float64 score| over sampled rows, the float32 score formed as the
    kernel forms it (1/T rounded, logit * (1/T) rounded, noise from two correctly rounded float32
    logs, the sum rounded): the error no float32 implementation of the formula can avoid."""
    lg = to_np(logits, np.float32)
    B, V = lg.shape
    t = to_np(temps, np.float32).reshape(B)
    rows = np.nonzero(t > 0)[0]
    if rows.size == 0:
        return 0.0
    sd = _as_u64(seeds).reshape(B)[rows][:, None]
    idx = (np.arange(V, dtype=np.int64) + int(voff))[None, :]
    u = u01_from_bits(noise_bits(sd, idx))
    inner = (-np.log(u.astype(np.float64))).astype(np.float32)          # correctly rounded -log(u)
    noise = (-np.log(inner.astype(np.float64))).astype(np.float32)      # correctly rounded outer log
    inv_t = (np.float32(1.0) / t[rows])[:, None]
    s32 = (lg[rows] * inv_t).astype(np.float32) + noise
    s64 = lg[rows].astype(np.float64) / t[rows].astype(np.float64)[:, None] + (-np.log(-np.log(u.astype(np.float64))))
    d = np.abs(s32.astype(np.float64) - s64)
    d = d[np.isfinite(s64)]
    return float(d.max()) if d.size else 0.0


TOL_ROW_FACTOR = 32.0 * 2.0 ** -24


def topk_tol_row(rows64, q64):
    """32 * 2^-24 * sum_i |a_i| |b_i| per row: products of two bf16 values are exact in float32, a
    lane adds at most 16 of them and six wave-reduction adds follow -- 22 roundings, bounded by 32."""
    return TOL_ROW_FACTOR * (np.abs(rows64) @ np.abs(q64))


def check_topk_certificate(ids, scores, counts, corpus, users, dates, queries, q_user, q_floor, ks, kmax):
    """Is (ids, scores, counts) a VALID filtered top-k answer?  Per query:
      * count == min(k, matches, kmax);
      * the ids are distinct rows that pass the filter;
      * each returned score is that row's fp64 dot product within tol_row;
      * the list is strictly ordered by (returned score descending, row id ascending);
      * no row left out scores (fp64) above the last returned row by more than the two rows'
        tolerances together (tol_row of the row left out + tol_row of the last one, i.e. at most
        2 * tol_row: the kernel ranked its own float32 scores, each within tol_row of fp64);
      * slots past count hold id -1 and score 0."""
    ids, scores, counts = to_np(ids, np.int64), to_np(scores, np.float64), to_np(counts, np.int64)
    users, dates = to_np(users, np.int64), to_np(dates, np.int64)
    q_user, q_floor, ks = to_np(q_user, np.int64), to_np(q_floor, np.int64), to_np(ks, np.int64)
    corpus_np = to_np(corpus)            # float32 holds bf16 exactly; rows go to fp64 as needed
    q64 = to_np(queries, np.float64)
    nq = q64.shape[0]
    N = corpus_np.shape[0]
    assert ids.shape == (nq, kmax) and scores.shape == (nq, kmax) and counts.shape == (nq,), "output shapes"
    for qi in range(nq):
        mask = (users == q_user[qi]) & (dates >= q_floor[qi])
        match = np.nonzero(mask)[0]
        want = int(min(max(int(ks[qi]), 0), match.size, kmax))
        c = int(counts[qi])
        assert c == want, f"query {qi}: count {c}, expected min(k={ks[qi]}, matches={match.size}, kmax={kmax})"
        assert (ids[qi, c:] == -1).all() and (scores[qi, c:] == 0).all(), f"query {qi}: slots past count not (-1, 0)"
        if c == 0:
            continue
        got, sc = ids[qi, :c], scores[qi, :c]
        assert ((got >= 0) & (got < N)).all(), f"query {qi}: row id out of range"
        assert np.unique(got).size == c, f"query {qi}: duplicate ids"
        assert mask[got].all(), f"query {qi}: row {got[~mask[got]][0]} fails the filter"
        rows64 = corpus_np[match].astype(np.float64)
        s64 = rows64 @ q64[qi]
        tol = topk_tol_row(rows64, q64[qi])
        pos = np.searchsorted(match, got)                 # match is ascending
        err = np.abs(sc - s64[pos])
        bad = np.nonzero(err > tol[pos])[0]
        assert bad.size == 0, (f"query {qi} slot {bad[0]}: score {sc[bad[0]]!r} vs fp64 {s64[pos[bad[0]]]!r} "
                               f"(tol_row {tol[pos[bad[0]]]:.3g})")
        a_s, b_s, a_i, b_i = sc[:-1], sc[1:], got[:-1], got[1:]
        ordered = (a_s > b_s) | ((a_s == b_s) & (a_i < b_i))
        bad = np.nonzero(~ordered)[0]
        assert bad.size == 0, f"query {qi}: slots {bad[0]},{bad[0] + 1} out of (score desc, id asc) order"
        out = np.ones(match.size, dtype=bool)
        out[pos] = False
        over = out & (s64 > s64[pos[-1]] + tol + tol[pos[-1]])
        assert not over.any(), (f"query {qi}: row {match[np.nonzero(over)[0][0]]} left out, fp64 score "
                                f"{s64[np.nonzero(over)[0][0]]!r} above the last returned {s64[pos[-1]]!r}")
