"""Hybrid (dense + BM25) retrieval on the CPU: term extraction, the query weights, the stores'
torch/numpy paths, snapshots, the service and config switches, and a demonstration that the
certificate of ``hybrid_ref`` rejects wrong answers.  The kernels are tested in
``test_hybrid_retrieval_gpu.py``.
"""
import logging
import math

import numpy as np
import pytest
import torch

from financial_chatbot_llm_amd import config, ops
from financial_chatbot_llm_amd.ops import retrieval as retrieval_ops
from financial_chatbot_llm_amd.retrieval import DeviceVectorStore, HashEmbedder, NumpyVectorStore, RetrievalService
from financial_chatbot_llm_amd.retrieval import lexical
from financial_chatbot_llm_amd.retrieval.ingest import CorpusIngestor, ensure_lexical
from financial_chatbot_llm_amd.utils.metrics import METRICS
from hybrid_ref import (assert_topk_boundary_is_clear, check_hybrid_certificate, fill_case, hybrid_scores64,
                        store_case)

DAY = 86400


# ---- terms ------------------------------------------------------------------------------------
def test_terms_known_answers_and_constants():
    assert lexical.terms("a") == [0xE40C292C]
    assert lexical.terms("foobar") == [0xBF9CF968]
    assert lexical.fnv1a("") == 0x811C9DC5
    assert (retrieval_ops.DOC_TERMS, retrieval_ops.QUERY_TERMS, retrieval_ops.DF_BUCKETS) == \
        (lexical.DOC_TERMS, lexical.QUERY_TERMS, lexical.DF_BUCKETS) == (32, 16, 1 << 20)


def test_terms_order_case_dedup_and_limits():
    a, foobar, b2 = lexical.fnv1a("a"), lexical.fnv1a("foobar"), lexical.fnv1a("b2")
    assert lexical.terms("FooBar, a | foobar: B2 -- A!") == [foobar, a, b2]
    words = [f"w{i}" for i in range(40)]
    want = [lexical.fnv1a(w) for w in words]
    assert lexical.terms(" ".join(words)) == want[:32]
    assert lexical.terms(" ".join(words), lexical.QUERY_TERMS) == want[:16]
    assert lexical.terms(" ".join(words[:17]), lexical.QUERY_TERMS) == want[:16]      # the 17th word is dropped
    assert lexical.terms("") == [] and lexical.terms(" |$ ") == []
    rows = lexical.term_rows(["a foobar", None, "", " ".join(words)])
    assert rows.dtype == np.int32 and rows.shape == (4, 32)
    assert rows[0].view(np.uint32).tolist() == [a, foobar] + [0] * 30                  # top bit set: negative int32
    assert rows[0, 0] < 0 and not rows[1].any() and not rows[2].any()
    assert rows[3].view(np.uint32).tolist() == want[:32]


def test_terms_zero_hash_becomes_one(monkeypatch):
    monkeypatch.setattr(lexical, "_FNV_PRIME", 0)            # every word now hashes to 0 ...
    monkeypatch.setattr(lexical, "_MEMO", {})
    assert lexical.fnv1a("anything") == 1                    # ... which marks an empty slot, so it becomes 1
    assert lexical.terms("two words") == [1]


def test_buckets_take_the_unsigned_low_bits():
    rows = np.array([[0x80000001, 0, 0x00100005, 5]], np.uint32).view(np.int32)
    assert lexical.buckets(rows).tolist() == [1, 5, 5]


# ---- query weights -----------------------------------------------------------------------------
def test_hybrid_query_weights_formula():
    df = torch.zeros(1 << 20, dtype=torch.int32)
    df[7], df[9] = 3, 500                                    # 500 > N: clipped to N
    top = np.array([0x80000007], np.uint32).view(np.int32)[0]                          # shares bucket 7
    qt = torch.zeros((3, 16), dtype=torch.int32)
    qt[0, :4] = torch.tensor([7, int(top), 9, (1 << 20) + 7])
    qt[1, 0] = 9
    u, dw, r = ops.hybrid_query_weights(qt, torch.tensor([0.5, 1.0, 0.25]), df, 100, 1200)
    assert u.dtype == dw.dtype == r.dtype == torch.float32 and u.shape == (3, 16) and r.shape == (33,)
    idf3 = math.log1p((100 - 3 + 0.5) / 3.5)
    idfN = math.log1p(0.5 / 100.5)
    W = 3 * idf3 + idfN
    np.testing.assert_allclose(u[0, :4].numpy(), [0.5 * idf3 / W] * 2 + [0.5 * idfN / W, 0.5 * idf3 / W], rtol=1e-6)
    assert float(u[0, 0]) == float(u[0, 1]) == float(u[0, 3])                          # one bucket, one df
    assert not u[0, 4:].any() and not u[2].any()                                       # empty slots, W = 0
    np.testing.assert_allclose(float(u[1, 0]), 1.0, rtol=1e-6)
    assert dw.tolist() == [0.5, 0.0, 0.75]
    n = np.arange(33)
    np.testing.assert_allclose(r.numpy(), 2.2 / (1 + 1.2 * (0.25 + 0.75 * n / 12.0)), rtol=1e-6)
    _, _, r1 = ops.hybrid_query_weights(qt, 0.5, df, 0, 0)                             # empty store: avgdl = 1
    np.testing.assert_allclose(r1.numpy(), 2.2 / (1 + 1.2 * (0.25 + 0.75 * n)), rtol=1e-6)
    with pytest.raises(ValueError):
        ops.hybrid_query_weights(qt, 1.5, df, 100, 1200)


def test_lex_df_add_torch_path_is_bincount():
    g = np.random.default_rng(3)
    rows = g.integers(0, 1 << 32, size=(300, 32), dtype=np.uint64).astype(np.uint32)
    rows[g.random((300, 32)) < 0.4] = 0
    rows[:, 0] = 0x80000007
    df = torch.zeros(1 << 20, dtype=torch.int32)
    t = torch.from_numpy(rows.view(np.int32))
    ops.lex_df_add(t, df)
    ops.lex_df_add(t[:10], df)
    want = np.bincount(lexical.buckets(rows.view(np.int32)), minlength=1 << 20) + \
        np.bincount(lexical.buckets(rows[:10].view(np.int32)), minlength=1 << 20)
    assert np.array_equal(df.numpy(), want) and int(df[7]) >= 310


# ---- stores ------------------------------------------------------------------------------------
def _doc(text, user, date):
    return {"page_content": text, "metadata": {"user_id": user, "date": date}}


HAND = [
    _doc("Date: 2024-03-01 | Merchant: Starbucks | Amount: $4.50 | Category: Dining", "u1", 10 * DAY),
    _doc("Date: 2024-03-02 | Merchant: Starbucks Reserve Roastery Seattle | Amount: $14.25 | Category: Dining | "
         "Note: birthday coffee with the whole team downtown", "u1", 11 * DAY),
    _doc("Date: 2024-03-03 | Merchant: Chevron | Amount: $40.00 | Category: Gas", "u1", 12 * DAY),
    _doc("Date: 2024-03-04 | Merchant: Starbucks | Amount: $5.00 | Category: Dining", "u2", 12 * DAY),
    _doc("Date: 2024-03-05 | Merchant: Whole Foods | Amount: $61.20 | Category: Groceries", "u1", 13 * DAY),
]


def _fill(store, docs=HAND, seed=0, batches=1):
    emb = HashEmbedder(store.corpus.dim)
    step = (len(docs) + batches - 1) // batches
    for s in range(0, len(docs), step):
        part = docs[s:s + step]
        store.add(emb.embed([d["page_content"] for d in part]), [d["metadata"]["user_id"] for d in part],
                  [d["metadata"]["date"] for d in part], part)
    return emb


def test_numpy_store_bm25_prefers_the_shorter_matching_row():
    st = NumpyVectorStore(64, lexical=True)
    emb = _fill(st)
    assert st.terms.shape == (5, 32) and st.total_terms == int(np.count_nonzero(st.terms))
    assert int(st.df[lexical.fnv1a("starbucks") & 0xFFFFF]) == 3 and int(st.df[lexical.fnv1a("date") & 0xFFFFF]) == 5
    hits = st.search_batch(emb.embed(["starbucks"]), ["u1"], [None], [10], texts=["starbucks"], alpha=1.0)[0]
    assert [h.id for h in hits] == [0, 1, 2, 4]              # short match, long match, then ties by row id
    assert hits[0].score > hits[1].score > 0.0
    assert hits[2].score == 0.0 and hits[3].score == 0.0     # no matching term, no dense share: exactly 0
    assert hits[0].payload is HAND[0]
    # the date floor and the limit apply as before
    hits = st.search_batch(emb.embed(["starbucks"]), ["u1"], [11 * DAY], [1], texts=["starbucks"], alpha=1.0)[0]
    assert [h.id for h in hits] == [1]
    assert st.search_batch(emb.embed(["x"]), ["nobody"], [None], [3], texts=["x"], alpha=0.5) == [[]]


@pytest.mark.parametrize("make", [lambda lex: NumpyVectorStore(64, lexical=lex),
                                  lambda lex: DeviceVectorStore(64, device="cpu", lexical=lex)], ids=["numpy", "torch"])
def test_alpha_zero_is_todays_answer(make):
    plain, lex = make(False), make(True)
    emb = _fill(plain)
    _fill(lex)
    qs = ["starbucks coffee", "gas", "groceries at whole foods"]
    q = emb.embed(qs)
    args = (q, ["u1", "u1", "u2"], [None, 11 * DAY, None], [3, 2, 5])
    want = plain.search_batch(*args)
    for got in (lex.search_batch(*args), lex.search_batch(*args, texts=qs, alpha=0.0),
                lex.search_batch(*args, texts=qs, alpha=[0.0] * 3), plain.search_batch(*args, texts=qs, alpha=0.7)):
        assert [[(h.id, h.score) for h in hs] for hs in got] == [[(h.id, h.score) for h in hs] for hs in want]
    with pytest.raises(ValueError):
        lex.search_batch(*args, texts=qs, alpha=1.5)
    with pytest.raises(ValueError):
        lex.search_batch(*args, texts=qs[:2], alpha=0.5)


def test_device_store_torch_path_agrees_with_numpy_store():
    docs, vecs, qtexts, qvecs, users, floors, limits = store_case()
    ref = NumpyVectorStore(64, lexical=True)
    dev = DeviceVectorStore(64, device="cpu", lexical=True)
    fill_case(ref, docs, vecs, batches=1)
    fill_case(dev, docs, vecs, batches=2)
    assert np.array_equal(dev.terms[: dev.size].numpy(), ref.terms) and np.array_equal(dev.df.numpy(), ref.df)
    assert dev.total_terms == ref.total_terms
    for alpha in (0.5, 1.0, [0.0, 0.25, 0.5, 0.75, 1.0]):
        if alpha == 0.5:
            assert_topk_boundary_is_clear(ref, qvecs, qtexts, users, floors, limits, alpha)
        want = ref.search_batch(qvecs, users, floors, limits, texts=qtexts, alpha=alpha)
        got = dev.search_batch(qvecs, users, floors, limits, texts=qtexts, alpha=alpha)
        assert [[h.id for h in hs] for hs in got] == [[h.id for h in hs] for hs in want]
        np.testing.assert_allclose([h.score for hs in got for h in hs], [h.score for hs in want for h in hs],
                                   rtol=1e-5, atol=1e-6)
    dense = ref.search_batch(qvecs, users, floors, limits)
    hybrid = ref.search_batch(qvecs, users, floors, limits, texts=qtexts, alpha=0.5)
    assert [[h.id for h in hs] for hs in dense] != [[h.id for h in hs] for hs in hybrid]       # the terms matter


def test_build_lexical_matches_incremental_tables():
    docs, vecs, *_ = store_case()
    a = DeviceVectorStore(64, device="cpu", lexical=True)
    b = DeviceVectorStore(64, device="cpu")
    fill_case(a, docs, vecs, batches=3)
    fill_case(b, docs, vecs, batches=1)
    assert not b.lexical and b.df is None
    b.build_lexical()
    assert b.lexical and torch.equal(a.terms[: a.size], b.terms[: b.size]) and torch.equal(a.df, b.df)
    assert a.total_terms == b.total_terms > 0


def test_load_synthetic_lexical_terms_come_from_the_payload_text():
    st = DeviceVectorStore(16, device="cpu")
    st.load_synthetic(200, 5, seed=2, now=1_700_000_000, lexical=True)
    assert st.lexical and st.terms.shape[0] >= 200
    for r in (0, 57, 199):
        want = lexical.term_rows([st.corpus.payload(r)["page_content"]])[0]
        assert np.array_equal(st.terms[r].numpy(), want)
    assert int(st.df[lexical.fnv1a("merchant") & 0xFFFFF]) == 200


def test_snapshot_round_trip_with_lexical_tables(tmp_path):
    import os
    docs, vecs, qtexts, qvecs, users, floors, limits = store_case()
    st = DeviceVectorStore(64, device="cpu", lexical=True)
    fill_case(st, docs, vecs)
    st.save(str(tmp_path / "snap"))
    assert sorted(os.listdir(tmp_path / "snap")) == ["corpus.json", "lexical.safetensors", "payloads.jsonl",
                                                     "vectors.safetensors"]
    back = DeviceVectorStore.load(str(tmp_path / "snap"), device="cpu")
    assert back.lexical and back.total_terms == st.total_terms
    assert torch.equal(back.terms[: back.size], st.terms[: st.size]) and torch.equal(back.df, st.df)
    want = st.search_batch(qvecs, users, floors, limits, texts=qtexts, alpha=0.5)
    got = back.search_batch(qvecs, users, floors, limits, texts=qtexts, alpha=0.5)
    assert [[(h.id, h.score) for h in hs] for hs in got] == [[(h.id, h.score) for h in hs] for hs in want]
    back.add(vecs[:2], ["u0", "u0"], [0, 0], docs[:2])                                   # the tables keep growing
    assert back.total_terms > st.total_terms


def test_old_layout_snapshot_loads_and_serves_dense(tmp_path, caplog):
    import os
    docs, vecs, qtexts, qvecs, users, floors, limits = store_case()
    st = DeviceVectorStore(64, device="cpu")
    fill_case(st, docs, vecs)
    st.save(str(tmp_path / "old"))
    assert not os.path.exists(tmp_path / "old" / "lexical.safetensors")
    back = DeviceVectorStore.load(str(tmp_path / "old"), device="cpu")
    assert not back.lexical
    want = st.search_batch(qvecs, users, floors, limits)
    got = back.search_batch(qvecs, users, floors, limits, texts=qtexts, alpha=0.5)       # no tables: dense
    assert [[(h.id, h.score) for h in hs] for hs in got] == [[(h.id, h.score) for h in hs] for hs in want]
    assert ensure_lexical(back) and back.lexical                                         # payloads: rebuilt
    # vectors alone (no payloads): one warning, dense
    os.remove(tmp_path / "old" / "payloads.jsonl")
    bare = DeviceVectorStore.load(str(tmp_path / "old"), device="cpu")
    with caplog.at_level(logging.WARNING):
        assert not ensure_lexical(bare)
    assert not bare.lexical


def test_ingestor_turns_lexical_on():
    st = NumpyVectorStore(32)
    ing = CorpusIngestor(HashEmbedder(32), st, batch_size=2, lexical=True)
    assert st.lexical
    ing.ingest(HAND)
    assert st.terms.shape == (5, 32) and st.total_terms > 0


# ---- service and config ----------------------------------------------------------------------------
class FourArgStore:
    """A store with the signature from before hybrid retrieval."""

    def __init__(self):
        self.calls = []

    def search_batch(self, qvecs, user_ids, date_gte, limits):
        self.calls.append((len(qvecs), user_ids, date_gte, limits))
        return [[] for _ in user_ids]


def test_service_alpha_zero_keeps_the_four_argument_call():
    store = FourArgStore()
    svc = RetrievalService(HashEmbedder(16), store)
    before = METRICS.snapshot().get("retrieval_hybrid_queries_total") or 0
    assert svc.run_batch(["coffee", "gas"], ["u1", "u2"], [None, 5], [3, 4]) == [[], []]
    assert store.calls == [(2, ["u1", "u2"], [None, 5], [3, 4])]
    assert (METRICS.snapshot().get("retrieval_hybrid_queries_total") or 0) == before


def test_service_passes_texts_and_alpha_and_counts():
    st = NumpyVectorStore(64, lexical=True)
    emb = _fill(st)
    seen = {}
    inner = st.search_batch

    def spy(*a, **kw):
        seen.update(kw)
        return inner(*a, **kw)
    st.search_batch = spy
    before = METRICS.snapshot().get("retrieval_hybrid_queries_total") or 0
    hits = RetrievalService(emb, st, hybrid_alpha=1.0).search_sync("Starbucks", "u1", None, 2)
    assert seen == {"texts": ["Starbucks"], "alpha": 1.0} and [h.id for h in hits] == [0, 1]
    assert METRICS.snapshot().get("retrieval_hybrid_queries_total") == before + 1
    with pytest.raises(ValueError):
        RetrievalService(emb, st, hybrid_alpha=1.01)


def test_retrieval_config_hybrid_alpha(monkeypatch):
    monkeypatch.delenv("PENNY_HYBRID_ALPHA", raising=False)
    assert config.RetrievalConfig.from_env().hybrid_alpha == 0.0
    monkeypatch.setenv("PENNY_HYBRID_ALPHA", "0.3")
    assert config.RetrievalConfig.from_env().hybrid_alpha == pytest.approx(0.3)
    assert config.RetrievalConfig.from_env(hybrid_alpha=1.0).hybrid_alpha == 1.0
    for bad in ("1.5", "-0.1"):
        monkeypatch.setenv("PENNY_HYBRID_ALPHA", bad)
        with pytest.raises(ValueError):
            config.RetrievalConfig.from_env()
    with pytest.raises(ValueError):
        config.RetrievalConfig(hybrid_alpha=2.0)


def test_launcher_has_the_switch():
    from financial_chatbot_llm_amd.serving.launch import parse as parse_args
    assert parse_args(["--hybrid-alpha", "0.4"]).hybrid_alpha == pytest.approx(0.4)
    assert parse_args([]).hybrid_alpha is None


# ---- the certificate rejects wrong answers ---------------------------------------------------------
def certificate_case():
    g = torch.Generator().manual_seed(11)
    N, D = 40, 8
    corpus = torch.randn(N, D, generator=g).to(torch.bfloat16)
    users = torch.zeros(N, dtype=torch.int32)
    dates = torch.zeros(N, dtype=torch.int64)
    texts = [f"merchant m{i % 7} category c{i % 3} " + " ".join(f"x{i}n{k}" for k in range(i % 5)) for i in range(N)]
    terms = torch.from_numpy(lexical.term_rows(texts))
    df = torch.zeros(1 << 20, dtype=torch.int32)
    ops.lex_df_add(terms, df)
    queries = torch.randn(2, D, generator=g).to(torch.bfloat16)
    qt = torch.from_numpy(lexical.term_rows(["m3 c1", "merchant m5"], 16))
    u, dw, r = ops.hybrid_query_weights(qt, torch.tensor([0.5, 1.0]), df, N, int((terms != 0).sum()))
    args = (corpus, users, dates, terms, queries, torch.tensor([0, 0], dtype=torch.int32),
            torch.tensor([0, 0], dtype=torch.int64), torch.tensor([6, 6], dtype=torch.int32), 8, qt, u, dw, r)
    return args


def test_certificate_accepts_the_reference_and_rejects_wrong_answers():
    args = certificate_case()
    corpus, users, dates, terms, queries, q_user, q_floor, ks, kmax, qt, u, dw, r = args
    ids, sc, cnt = ops.filtered_topk_hybrid_ref(*args[:5], q_user.tolist(), q_floor.tolist(), ks.tolist(), kmax,
                                                qt, u, dw, r)
    rest = (corpus, users, dates, terms, queries, q_user, q_floor, ks, kmax, qt, u, dw, r)
    check_hybrid_certificate(ids, sc, cnt, *rest)
    assert cnt.tolist() == [6, 6]
    # a mis-ranked answer: the best row replaced by one from far down the list, with its true score
    s64, tol = hybrid_scores64(corpus, terms, queries[0], qt[0], u[0], dw[0], r)
    worst = int(np.argmin(s64))
    assert s64[int(ids[0, 5])] - s64[worst] > 100 * tol.max()
    bad_ids, bad_sc = ids.clone(), sc.clone()
    bad_ids[0, 5], bad_sc[0, 5] = worst, float(s64[worst])
    with pytest.raises(AssertionError, match="left out"):
        check_hybrid_certificate(bad_ids, bad_sc, cnt, *rest)
    # two neighbours swapped: order
    bad_ids, bad_sc = ids.clone(), sc.clone()
    bad_ids[1, [0, 1]], bad_sc[1, [0, 1]] = ids[1, [1, 0]], sc[1, [1, 0]]
    with pytest.raises(AssertionError, match="order"):
        check_hybrid_certificate(bad_ids, bad_sc, cnt, *rest)
    # a score off by 2 * tol is rejected, one off by tol / 2 passes
    row = int(ids[0, 2])
    t = float(tol[row])
    assert t > 0
    for off, ok in ((2 * t, False), (-2 * t, False), (0.5 * t, True)):
        bad_sc = sc.clone().double()
        bad_sc[0, 2] = s64[row] + off
        if ok:
            check_hybrid_certificate(ids, bad_sc, cnt, *rest)
        else:
            with pytest.raises(AssertionError, match="vs fp64"):
                check_hybrid_certificate(ids, bad_sc, cnt, *rest)
    # a duplicated term in a row is outside the kernel's contract
    dup = terms.clone()
    dup[3, 1] = dup[3, 0]
    with pytest.raises(AssertionError, match="duplicate terms"):
        check_hybrid_certificate(ids, sc, cnt, corpus, users, dates, dup, *rest[4:])
