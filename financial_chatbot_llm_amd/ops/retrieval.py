"""K15: filtered exact top-k over an HBM-resident corpus (user_id == u AND date >= t)."""
from __future__ import annotations

from typing import Tuple

import torch

from . import _native as N

SORT_CAP = 8192


def filtered_topk_ref(corpus, user_codes, dates, queries, q_user, q_floor, ks, kmax):
    nq = queries.shape[0]
    ids = torch.full((nq, kmax), -1, dtype=torch.int32, device=corpus.device)
    scores = torch.zeros((nq, kmax), dtype=torch.float32, device=corpus.device)
    counts = torch.zeros((nq,), dtype=torch.int32, device=corpus.device)
    for i in range(nq):
        mask = (user_codes == q_user[i]) & (dates >= q_floor[i])
        rows = torch.nonzero(mask).flatten()
        if rows.numel() == 0:
            continue
        s = corpus[rows].float() @ queries[i].float()
        # descending score, ties by smaller row id (rows are ascending -> stable sort)
        order = torch.sort(-s, stable=True).indices
        k = min(int(ks[i]), rows.numel(), kmax)
        ids[i, :k] = rows[order[:k]].to(torch.int32)
        scores[i, :k] = s[order[:k]]
        counts[i] = k
    return ids, scores, counts


def _best_first(scores: torch.Tensor, ids: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The k best of (score descending, row id ascending), the select kernel's order.  torch.topk
    leaves the order of tied scores open (and the candidate list's order comes from atomics), so
    only its k-th score is used: every candidate at or above it is ordered by the pair."""
    if k <= 0:
        return ids[:0], scores[:0]
    kth = torch.topk(scores, k).values[-1]
    sel = (scores >= kth).nonzero().flatten()
    sel = sel[torch.argsort(ids[sel], stable=True)]
    sel = sel[torch.sort(scores[sel], descending=True, stable=True).indices][:k]
    return ids[sel], scores[sel]


class _Workspace:
    def __init__(self):
        self.key = None

    def get(self, nq: int, cap: int, device):
        key = (nq, cap, str(device))
        if self.key != key:
            self.counts = torch.empty((nq,), dtype=torch.int32, device=device)
            self.cand = torch.empty((nq, cap), dtype=torch.int32, device=device)
            self.scores = torch.empty((nq, cap), dtype=torch.float32, device=device)
            self.key = key
        return self.counts, self.cand, self.scores


_WS = _Workspace()


def filtered_topk(corpus: torch.Tensor, user_codes: torch.Tensor, dates: torch.Tensor, queries: torch.Tensor,
                  q_user: torch.Tensor, q_floor: torch.Tensor, ks: torch.Tensor, kmax: int,
                  cap: int = 65536) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> (row ids [nq,kmax] int32, scores [nq,kmax] f32, counts [nq] int32), best first."""
    nq, D = queries.shape
    if not N.use_native(corpus):
        return filtered_topk_ref(corpus, user_codes, dates, queries, q_user.tolist(), q_floor.tolist(),
                                 ks.tolist(), kmax)
    if nq > 64:  # kernel handles 64 queries per launch
        parts = [filtered_topk(corpus, user_codes, dates, queries[i:i + 64], q_user[i:i + 64], q_floor[i:i + 64],
                               ks[i:i + 64], kmax, cap) for i in range(0, nq, 64)]
        return tuple(torch.cat(x) for x in zip(*parts))
    cap = max(SORT_CAP, min(cap, corpus.shape[0]))
    counts, cand, scores = _WS.get(nq, cap, corpus.device)
    out_ids = torch.full((nq, kmax), -1, dtype=torch.int32, device=corpus.device)
    out_scores = torch.zeros((nq, kmax), dtype=torch.float32, device=corpus.device)
    out_count = torch.empty((nq,), dtype=torch.int32, device=corpus.device)
    queries = queries.to(torch.bfloat16).contiguous()
    # converted inputs bound to names: as N.ptr(x.to(...)) temporaries they would be freed before
    # the launch and the next conversion could reuse (overwrite) their memory on the stream
    qu, qf, kk = q_user.to(torch.int32).contiguous(), q_floor.to(torch.int64).contiguous(), ks.to(torch.int32).contiguous()
    N.call("penny_filtered_topk", N.ptr(corpus), N.ptr(user_codes), N.ptr(dates), corpus.shape[0], D,
           N.ptr(queries), N.ptr(qu), N.ptr(qf), N.ptr(kk), nq, kmax, N.ptr(counts), N.ptr(cand), N.ptr(scores), cap,
           N.ptr(out_ids), N.ptr(out_scores), N.ptr(out_count), N.stream())
    oc = out_count.cpu()
    big = (oc < 0).nonzero().flatten().tolist()
    for i in big:  # > SORT_CAP candidates: finish on device, in the select kernel's order
        total = -int(oc[i])
        k = min(int(ks[i]), total, kmax)
        if total <= cap:
            out_ids[i, :k], out_scores[i, :k] = _best_first(scores[i, :total], cand[i, :total], k)
        else:
            mask = (user_codes == q_user[i]) & (dates >= q_floor[i])
            full = (corpus.float() @ queries[i].float()).masked_fill(~mask, float("-inf"))
            rows = torch.arange(full.numel(), dtype=torch.int32, device=full.device)
            out_ids[i, :k], out_scores[i, :k] = _best_first(full, rows, k)
        oc[i] = k
    return out_ids, out_scores, oc.to(corpus.device)


# ---- hybrid retrieval: dense cosine + BM25 term score ---------------------------------------------
# score(q, d) = dw * <q, v_d> + r[n_d] * sum_{j : t_j in terms(d)} u_j  (retrieval/lexical.py makes the
# term rows; rows hold distinct non-zero hashes, zero-padded, and n_d counts the non-zero slots).
DOC_TERMS = 32
QUERY_TERMS = 16
DF_BUCKETS = 1 << 20
BM25_K1 = 1.2
BM25_B = 0.75


def hybrid_query_weights(q_terms: torch.Tensor, alpha, df: torch.Tensor, n_rows: int, total_terms: int,
                         k1: float = BM25_K1, b: float = BM25_B):
    """-> (q_u [nq,16] f32, q_dw [nq] f32, r [33] f32) on ``df``'s device: what both the kernel and the
    reference score with.  idf_j = log1p((N - df_j + 0.5) / (df_j + 0.5)) with df_j clipped to N,
    u_j = alpha * idf_j / sum_j idf_j (0 for empty slots and for a zero sum), dw = 1 - alpha, and
    r[n] = (1 + k1) / (1 + k1 * (1 - b + b * n / avgdl)): BM25 at term frequency 1 over the score of
    an average-length row that matches every query term."""
    dev = df.device
    qt = q_terms.to(dev)
    nq = qt.shape[0]
    a = torch.as_tensor(alpha, dtype=torch.float32, device=dev).reshape(-1)
    a = a.expand(nq) if a.numel() == 1 else a.reshape(nq)       # one alpha for all, or one per query
    if nq and (bool((a < 0).any()) or bool((a > 1).any())):
        raise ValueError("hybrid alpha outside [0, 1]")
    n = float(max(int(n_rows), 0))
    dfj = df[(qt.to(torch.int64) & (DF_BUCKETS - 1))].to(torch.float32).clamp(max=n)
    idf = torch.log1p((n - dfj + 0.5) / (dfj + 0.5))
    idf = torch.where(qt != 0, idf, torch.zeros_like(idf))
    w = idf.sum(1, keepdim=True)
    u = torch.where(w > 0, a[:, None] * idf / torch.where(w > 0, w, torch.ones_like(w)), torch.zeros_like(idf))
    avgdl = float(total_terms) / n if n > 0 and total_terms > 0 else 1.0
    nn = torch.arange(DOC_TERMS + 1, dtype=torch.float32, device=dev)
    r = (1.0 + k1) / (1.0 + k1 * (1.0 - b + b * nn / avgdl))
    return u.contiguous(), (1.0 - a).contiguous(), r.to(torch.float32).contiguous()


def _lexical_scores(term_rows: torch.Tensor, qt: torch.Tensor, qu: torch.Tensor, r: torch.Tensor) -> torch.Tensor:
    """r[n_d] * sum of u_j over the query terms present in each row, float32, query slots in order."""
    lex = torch.zeros((term_rows.shape[0],), dtype=torch.float32, device=term_rows.device)
    for j in range(qt.numel()):
        if int(qt[j]) != 0:
            lex = lex + qu[j] * (term_rows == qt[j]).any(1).to(torch.float32)
    n_d = (term_rows != 0).sum(1)
    return r[n_d] * lex


def _hybrid_scores(vec_rows, term_rows, q, qt, qu, dw, r) -> torch.Tensor:
    lex = _lexical_scores(term_rows, qt, qu, r)
    if float(dw) == 0.0:        # purely lexical: the vectors are not read
        return lex
    return dw * (vec_rows.float() @ q.float()) + lex


def filtered_topk_hybrid_ref(corpus, user_codes, dates, terms, queries, q_user, q_floor, ks, kmax, q_terms, q_u,
                             q_dw, r):
    """The torch path of ``filtered_topk_hybrid`` (CPU tensors) and the oracle of its tests."""
    nq = queries.shape[0]
    ids = torch.full((nq, kmax), -1, dtype=torch.int32, device=corpus.device)
    scores = torch.zeros((nq, kmax), dtype=torch.float32, device=corpus.device)
    counts = torch.zeros((nq,), dtype=torch.int32, device=corpus.device)
    for i in range(nq):
        mask = (user_codes == int(q_user[i])) & (dates >= int(q_floor[i]))
        rows = torch.nonzero(mask).flatten()
        if rows.numel() == 0:
            continue
        s = _hybrid_scores(corpus[rows], terms[rows], queries[i], q_terms[i], q_u[i], q_dw[i], r)
        order = torch.sort(-s, stable=True).indices
        k = min(int(ks[i]), rows.numel(), kmax)
        ids[i, :k] = rows[order[:k]].to(torch.int32)
        scores[i, :k] = s[order[:k]]
        counts[i] = k
    return ids, scores, counts


def filtered_topk_hybrid(corpus: torch.Tensor, user_codes: torch.Tensor, dates: torch.Tensor, terms: torch.Tensor,
                         queries: torch.Tensor, q_user: torch.Tensor, q_floor: torch.Tensor, ks: torch.Tensor,
                         kmax: int, q_terms: torch.Tensor, q_u: torch.Tensor, q_dw: torch.Tensor, r: torch.Tensor,
                         cap: int = 65536) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``filtered_topk`` with the hybrid score: terms [N,32] int32, q_terms [nq,16] int32, q_u [nq,16]
    f32, q_dw [nq] f32, r [33] f32 (``hybrid_query_weights``).  Same filter, order, counts and padding."""
    nq, D = queries.shape
    if terms.shape != (corpus.shape[0], DOC_TERMS) or terms.dtype != torch.int32:
        raise ValueError(f"terms must be int32 [{corpus.shape[0]}, {DOC_TERMS}]")
    if q_terms.shape != (nq, QUERY_TERMS) or q_u.shape != (nq, QUERY_TERMS) or q_dw.shape != (nq,) or \
            r.shape != (DOC_TERMS + 1,):
        raise ValueError("q_terms / q_u must be [nq, 16], q_dw [nq], r [33]")
    if not N.use_native(corpus):
        return filtered_topk_hybrid_ref(corpus, user_codes, dates, terms, queries, q_user.tolist(), q_floor.tolist(),
                                        ks.tolist(), kmax, q_terms, q_u, q_dw, r)
    if nq > 64:  # kernel handles 64 queries per launch
        parts = [filtered_topk_hybrid(corpus, user_codes, dates, terms, queries[i:i + 64], q_user[i:i + 64],
                                      q_floor[i:i + 64], ks[i:i + 64], kmax, q_terms[i:i + 64], q_u[i:i + 64],
                                      q_dw[i:i + 64], r, cap) for i in range(0, nq, 64)]
        return tuple(torch.cat(x) for x in zip(*parts))
    cap = max(SORT_CAP, min(cap, corpus.shape[0]))
    counts, cand, scores = _WS.get(nq, cap, corpus.device)
    out_ids = torch.full((nq, kmax), -1, dtype=torch.int32, device=corpus.device)
    out_scores = torch.zeros((nq, kmax), dtype=torch.float32, device=corpus.device)
    out_count = torch.empty((nq,), dtype=torch.int32, device=corpus.device)
    queries = queries.to(torch.bfloat16).contiguous()
    # converted inputs bound to names, as in filtered_topk
    qu, qf, kk = q_user.to(torch.int32).contiguous(), q_floor.to(torch.int64).contiguous(), ks.to(torch.int32).contiguous()
    terms, qt = terms.contiguous(), q_terms.to(torch.int32).contiguous()
    wu, wd, rt = q_u.to(torch.float32).contiguous(), q_dw.to(torch.float32).contiguous(), r.to(torch.float32).contiguous()
    N.call("penny_filtered_topk_hybrid", N.ptr(corpus), N.ptr(user_codes), N.ptr(dates), corpus.shape[0], D,
           N.ptr(terms), N.ptr(queries), N.ptr(qu), N.ptr(qf), N.ptr(kk), N.ptr(qt), N.ptr(wu), N.ptr(wd), N.ptr(rt),
           nq, kmax, N.ptr(counts), N.ptr(cand), N.ptr(scores), cap, N.ptr(out_ids), N.ptr(out_scores),
           N.ptr(out_count), N.stream())
    oc = out_count.cpu()
    big = (oc < 0).nonzero().flatten().tolist()
    for i in big:  # > SORT_CAP candidates: finish on device, in the select kernel's order
        total = -int(oc[i])
        k = min(int(ks[i]), total, kmax)
        if total <= cap:
            out_ids[i, :k], out_scores[i, :k] = _best_first(scores[i, :total], cand[i, :total], k)
        else:
            mask = (user_codes == q_user[i]) & (dates >= q_floor[i])
            full = _hybrid_scores(corpus, terms, queries[i], qt[i], wu[i], wd[i], rt).masked_fill(~mask, float("-inf"))
            rows = torch.arange(full.numel(), dtype=torch.int32, device=full.device)
            out_ids[i, :k], out_scores[i, :k] = _best_first(full, rows, k)
        oc[i] = k
    return out_ids, out_scores, oc.to(corpus.device)


def lex_df_add(terms: torch.Tensor, df: torch.Tensor) -> None:
    """df[hash & (2^20 - 1)] += 1 for every non-zero slot of the new rows ``terms`` [n,32] int32, in place."""
    if terms.dim() != 2 or terms.shape[1] != DOC_TERMS or terms.dtype != torch.int32:
        raise ValueError(f"terms must be int32 [n, {DOC_TERMS}]")
    if df.shape != (DF_BUCKETS,) or df.dtype != torch.int32 or not df.is_contiguous():
        raise ValueError(f"df must be a contiguous int32 [{DF_BUCKETS}]")
    if terms.shape[0] == 0:
        return
    if N.use_native(df):
        terms = terms.to(df.device).contiguous()
        N.call("penny_lex_df_add", N.ptr(terms), terms.shape[0], N.ptr(df), N.stream())
        return
    t = terms.to(df.device).reshape(-1)
    idx = t[t != 0].to(torch.int64) & (DF_BUCKETS - 1)
    df += torch.bincount(idx, minlength=DF_BUCKETS).to(torch.int32)
