"""Validity certificate of the hybrid (dense + BM25) filtered top-k search, modelled on
``selection_ref.check_topk_certificate``: numpy in float64, never touches a device, and tests an
answer for VALIDITY against the fp64 value of

    score(q, d) = dw * <q, v_d> + r[n_d] * sum_{j : t_j in terms(d)} u_j

evaluated on the same float32 ``u``, ``dw`` and ``r`` the kernel was given.

Tolerance (derived, not measured).  The dense part is the dense kernel's sum (``topk_tol_row``: 22
roundings, bounded by 32 * 2^-24 * sum |a_i||b_i|) followed by one multiply by ``dw``: 23 roundings of
values no larger than |dw| * sum |a_i||b_i|.  The lexical part: a lane holds 4 slots and visits
4 * 16 (slot, query term) pairs in fixed order, one sum per slot; with distinct query terms a slot
matches at most one of them, so the slot sums are exact and the 3 adds that join them are the lane's
only roundings; then the 6 adds of the wave reduction, one multiply by ``r[n_d]`` and the final add
of the two parts: 3 + 6 + 1 + 1 = 11 roundings of values no larger than r[n_d] * sum_matched |u_j| (the
final add rounds the whole score, whose dense share falls under the dense bound's spare roundings:
23 + 1 <= 32).
Both counts stay below 32, so per row

    tol = |dw| * topk_tol_row(row, q) + 32 * 2^-24 * r[n_d] * sum_matched |u_j|.

A row that matches nothing under dw = 0 has tol = 0: its score is exactly 0.

Preconditions (asserted): the non-zero terms of a row are distinct, and so are those of a query --
what ``retrieval.lexical.terms`` produces.  A duplicated slot would be added twice by the kernel.
"""
from __future__ import annotations

import numpy as np
import torch

from financial_chatbot_llm_amd.ops.retrieval import hybrid_query_weights
from financial_chatbot_llm_amd.retrieval.lexical import QUERY_TERMS, term_rows
from selection_ref import TOL_ROW_FACTOR, to_np, topk_tol_row


def _distinct_nonzero(rows, what):
    for i, row in enumerate(rows):
        nz = row[row != 0]
        assert np.unique(nz).size == nz.size, f"{what} {i}: duplicate terms"


def hybrid_scores64(vec_rows, term_rows, q, qt, qu, dw, r):
    """-> (fp64 scores, tol) of the rows for one query.  vec_rows [m, D], term_rows [m, 32] int32,
    q [D], qt [16] int32, qu [16] float32, dw float32 scalar, r [33] float32."""
    rows64 = to_np(vec_rows).astype(np.float64)
    q64 = to_np(q, np.float64)
    T = to_np(term_rows, np.int64)
    qt, qu = to_np(qt, np.int64), to_np(qu, np.float64)
    dw, r = float(to_np(dw, np.float64)), to_np(r, np.float64)
    lex = np.zeros(T.shape[0])
    lex_abs = np.zeros(T.shape[0])
    for j in range(qt.shape[0]):
        if qt[j] != 0:
            hit = (T == qt[j]).any(1)
            lex += qu[j] * hit
            lex_abs += abs(qu[j]) * hit
    rn = r[(T != 0).sum(1)]
    dense = rows64 @ q64 if dw != 0.0 else np.zeros(T.shape[0])
    s64 = dw * dense + rn * lex
    tol = abs(dw) * topk_tol_row(rows64, q64) + TOL_ROW_FACTOR * np.abs(rn) * lex_abs
    return s64, tol


def check_hybrid_certificate(ids, scores, counts, corpus, users, dates, terms, queries, q_user, q_floor, ks, kmax,
                             q_terms, q_u, q_dw, r):
    """Is (ids, scores, counts) a VALID hybrid filtered top-k answer?  Per query, as the dense
    certificate: count == min(k, matches, kmax); distinct ids that pass the filter; each returned score
    within tol of the row's fp64 score; strict (score descending, row id ascending) order; no row
    left out above the last returned row by more than the two rows' tolerances together; slots past
    count hold (-1, 0)."""
    ids, scores, counts = to_np(ids, np.int64), to_np(scores, np.float64), to_np(counts, np.int64)
    users, dates = to_np(users, np.int64), to_np(dates, np.int64)
    q_user, q_floor, ks = to_np(q_user, np.int64), to_np(q_floor, np.int64), to_np(ks, np.int64)
    corpus_np, terms_np, qt_np = to_np(corpus), to_np(terms), to_np(q_terms)
    nq = qt_np.shape[0]
    N = corpus_np.shape[0]
    assert terms_np.shape == (N, 32) and qt_np.shape == (nq, 16), "term table shapes"
    _distinct_nonzero(terms_np, "row")
    _distinct_nonzero(qt_np, "query")
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
        s64, tol = hybrid_scores64(corpus_np[match], terms_np[match], to_np(queries)[qi], qt_np[qi], to_np(q_u)[qi],
                                   to_np(q_dw)[qi], r)
        pos = np.searchsorted(match, got)                 # match is ascending
        err = np.abs(sc - s64[pos])
        bad = np.nonzero(err > tol[pos])[0]
        assert bad.size == 0, (f"query {qi} slot {bad[0]}: score {sc[bad[0]]!r} vs fp64 {s64[pos[bad[0]]]!r} "
                               f"(tol {tol[pos[bad[0]]]:.3g})")
        a_s, b_s, a_i, b_i = sc[:-1], sc[1:], got[:-1], got[1:]
        ordered = (a_s > b_s) | ((a_s == b_s) & (a_i < b_i))
        bad = np.nonzero(~ordered)[0]
        assert bad.size == 0, f"query {qi}: slots {bad[0]},{bad[0] + 1} out of (score desc, id asc) order"
        out = np.ones(match.size, dtype=bool)
        out[pos] = False
        over = out & (s64 > s64[pos[-1]] + tol + tol[pos[-1]])
        assert not over.any(), (f"query {qi}: row {match[np.nonzero(over)[0][0]]} left out, fp64 score "
                                f"{s64[np.nonzero(over)[0][0]]!r} above the last returned {s64[pos[-1]]!r}")


# ---- a store-level case shared by the CPU and the GPU store tests ---------------------------------
DAY = 86400


def doc(text, user, date):
    return {"page_content": text, "metadata": {"user_id": user, "date": date}}


def exact_unit_vectors(n, D, g):
    """Rows of a entries +-4, b entries +-2 and c entries +-1 with 16 a + 4 b + c = 64: every norm is 8, so
    the normalised rows are exact in bf16 and float32 and the numpy store (float32 rows) and the device
    store (bf16 rows) hold the same numbers."""
    out = np.zeros((n, D), np.float32)
    for i in range(n):
        a = int(g.integers(0, 3))
        b = int(g.integers(0, 7))
        c = 64 - 16 * a - 4 * b
        mags = np.array([4.0] * a + [2.0] * b + [1.0] * c, np.float32)
        assert mags.size <= D
        out[i, g.permutation(D)[: mags.size]] = mags * (g.integers(0, 2, size=mags.size) * 2 - 1)
    return out


def store_case(seed=5, n=60, D=64):
    """Documents of three users with varied merchants and lengths, exactly normalisable vectors, five queries."""
    g = np.random.default_rng(seed)
    merchants = ["Starbucks", "Chevron", "Whole Foods", "Netflix", "Uber", "Costco", "Delta Air Lines", "Equinox"]
    notes = ["", " | Note: team lunch", " | Note: refund pending review by the card issuer", " | Note: gift"]
    docs = []
    for i in range(n):
        m = merchants[int(g.integers(len(merchants)))]
        text = (f"Date: 2024-03-{1 + i % 28:02d} | Merchant: {m} | Amount: ${1 + i}.{i % 100:02d} | "
                f"Category: c{int(g.integers(5))}{notes[int(g.integers(len(notes)))]}")
        docs.append(doc(text, f"u{i % 3}", int(g.integers(0, 30)) * DAY))
    vecs = exact_unit_vectors(n, D, g)
    qtexts = ["starbucks", "whole foods groceries", "uber refund", "delta air lines gift", "lunch at costco"]
    qvecs = exact_unit_vectors(len(qtexts), D, g)
    users = ["u0", "u1", "u2", "u0", "u1"]
    floors = [None, 5 * DAY, None, None, 2 * DAY]
    limits = [3, 4, 5, 2, 3]
    return docs, vecs, qtexts, qvecs, users, floors, limits


def fill_case(store, docs, vecs, batches=2):
    step = (len(docs) + batches - 1) // batches
    for s in range(0, len(docs), step):
        part = docs[s:s + step]
        store.add(vecs[s:s + step], [d["metadata"]["user_id"] for d in part], [d["metadata"]["date"] for d in part], part)


def assert_topk_boundary_is_clear(store, qvecs, qtexts, users, floors, limits, alpha):
    """Every gap between neighbouring fp64 scores among a query's best k + 1 rows exceeds the two rows'
    tolerances together, so the ranked ids are the same for any summation order within tol."""
    qt = torch.from_numpy(term_rows(qtexts, QUERY_TERMS))
    u, dw, r = hybrid_query_weights(qt, alpha, torch.from_numpy(store.df), len(store.corpus), store.total_terms)
    q = qvecs / np.linalg.norm(qvecs, axis=1, keepdims=True)
    for i in range(len(qtexts)):
        mask = store.corpus.user_codes == store.corpus.code(users[i])
        if floors[i] is not None:
            mask &= store.corpus.dates >= floors[i]
        rows = np.nonzero(mask)[0]
        assert rows.size > limits[i], f"query {i}: fewer than k + 1 candidates"
        s64, tol = hybrid_scores64(store.vectors[rows], store.terms[rows], q[i], qt[i], u[i], dw[i], r)
        order = np.argsort(-s64, kind="stable")[: limits[i] + 1]
        gaps = s64[order][:-1] - s64[order][1:]
        need = tol[order][:-1] + tol[order][1:]
        assert (gaps > need).all(), f"query {i}: gap {gaps.min():.3g} within tolerance {need.max():.3g}"
