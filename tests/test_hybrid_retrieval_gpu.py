"""The hybrid (dense + BM25) filtered top-k kernel and the document-frequency kernel of
``retrieval.hip`` on the GPU.  Every answer goes through ``hybrid_ref.check_hybrid_certificate`` (fp64
scores, derived tolerance); ``tests/test_hybrid_retrieval.py`` shows on the CPU that the certificate
rejects wrong answers.  Inputs are built on the CPU with seeded generators.
"""
import numpy as np
import pytest
import torch

from financial_chatbot_llm_amd import ops
from financial_chatbot_llm_amd.ops import retrieval as retrieval_ops
from financial_chatbot_llm_amd.retrieval import DeviceVectorStore, NumpyVectorStore, lexical
from hybrid_ref import assert_topk_boundary_is_clear, check_hybrid_certificate, fill_case, store_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -(1 << 62)


def _bits(x):
    """unsigned 32-bit hash -> the int32 that holds its bit pattern"""
    return int(np.array([x], np.uint32).view(np.int32)[0])


TOP = _bits(0x80000005)                      # a hash with the top bit set: a negative int32
ONE = 1                                      # what a hash of 0 is stored as
BKT, BKT2 = 0x00012345, 0x00112345           # two terms that share a df bucket
SPECIAL = [TOP, ONE, BKT, BKT2]
POOL = 0x40000000                            # POOL + i: ordinary terms


def _dev(*ts):
    return [t.to(DEV) for t in ts]


def _i32(x):
    return torch.tensor(x, dtype=torch.int32)


def _i64(x):
    return torch.tensor(x, dtype=torch.int64)


def _vectors(n, D, g):
    return torch.randn(n, D, generator=g).to(torch.bfloat16)


def _qterms(lists):
    qt = torch.zeros((len(lists), 16), dtype=torch.int32)
    for i, ts in enumerate(lists):
        qt[i, :len(ts)] = _i32(ts)
    return qt


def _weights(terms, qt, alpha):
    """df of the rows (torch path), then the weights both the kernel and the certificate use."""
    df = torch.zeros(1 << 20, dtype=torch.int32)
    ops.lex_df_add(terms, df)
    return ops.hybrid_query_weights(qt, alpha, df, terms.shape[0], int((terms != 0).sum()))


def _search(corpus, users, dates, terms, queries, q_user, q_floor, ks, kmax, qt, u, dw, r, cap=65536):
    """Run the kernel on CPU-built inputs and pass the result through the certificate."""
    out = ops.filtered_topk_hybrid(*_dev(corpus, users, dates, terms, queries, q_user, q_floor, ks), kmax,
                                   *_dev(qt, u, dw, r), cap)
    ids, sc, cnt = (x.cpu() for x in out)
    assert ids.dtype == torch.int32 and sc.dtype == torch.float32 and cnt.dtype == torch.int32
    check_hybrid_certificate(ids, sc, cnt, corpus, users, dates, terms, queries, q_user, q_floor, ks, kmax, qt, u, dw, r)
    return ids, sc, cnt


def edge_terms(N, g):
    """Rows of 32, 0, 1 and 31 terms in turn; full and 31-term rows carry one special term (top bit set,
    remapped zero, the two bucket sharers) in slot 0, 3, 4 or the last one -- the 16-byte boundaries of
    the eight lanes' loads and the end of the row."""
    rows = np.zeros((N, 32), np.int64)
    for i in range(N):
        n = (32, 0, 1, 31)[i % 4]
        rows[i, :n] = POOL + g.permutation(200)[:n]
        special = SPECIAL[(i // 4) % 4]
        if n >= 31:
            rows[i, (0, 3, 4, n - 1)[(i // 16) % 4]] = special
        elif n == 1 and (i // 4) % 2:
            rows[i, 0] = special
    return torch.from_numpy(rows.astype(np.int32))


EDGE_QUERIES = [[], [TOP], SPECIAL + [POOL + i for i in range(12)], SPECIAL + [POOL + i for i in range(12)],
                [BKT2, ONE], [BKT]]
EDGE_ALPHA = [0.5, 1.0, 0.5, 0.0, 0.25, 1.0]


@pytest.mark.parametrize("D", [8, 768])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_hybrid_rows_widths_slots_and_alphas(N, D):
    """Row counts around one wave's worth of candidates and past one block's, both widths, every row
    occupancy and match slot, 0 / 1 / 16 query terms, and a different alpha per query in one launch."""
    g = torch.Generator().manual_seed(1000 * D + N)
    terms = edge_terms(N, np.random.default_rng(N))
    users = torch.randint(0, 2, (N,), generator=g, dtype=torch.int32)
    users[0] = 1                                              # the full row with TOP in slot 0 matches
    dates = torch.randint(-100, 100, (N,), generator=g, dtype=torch.int64)
    qt = _qterms(EDGE_QUERIES)
    u, dw, r = _weights(terms, qt, torch.tensor(EDGE_ALPHA))
    assert float(u[2, 2]) == float(u[2, 3]) > 0 and dw.tolist() == [0.5, 0.0, 0.5, 1.0, 0.75, 0.0]
    ids, sc, cnt = _search(_vectors(N, D, g), users, dates, terms, _vectors(6, D, g), _i32([1, 1, 1, 0, 1, 1]),
                           _i64([SENTINEL, SENTINEL, -50, SENTINEL, 0, SENTINEL]), _i32([5, N, 3, 4, 300, 7]), 8, qt,
                           u, dw, r)
    mine = users == 1
    assert int(cnt[1]) == min(8, int(mine.sum()))
    has_top = ((terms == TOP).any(1) & mine).nonzero().flatten()
    k = int(cnt[1])
    # alpha = 1, one term: exactly the rows that hold it score above 0, the rest exactly 0
    assert int((sc[1, :k] > 0).sum()) == min(k, has_top.numel()) and has_top.numel() >= 1
    assert set(ids[1, :min(k, has_top.numel())].tolist()) <= set(has_top.tolist())


def test_hybrid_text_cases():
    """Through ``lexical``: a 17-word query drops its last word; a word repeated in a row and in a query
    counts once."""
    words = [f"w{i}" for i in range(17)]
    docs = ["w16 shop", "w3 shop", "coffee coffee shop", "coffee shop", "tea shop", "w0 w1 w2 w3 w4 w5 w6 w7 w8"]
    N = len(docs)
    g = torch.Generator().manual_seed(3)
    terms = torch.from_numpy(lexical.term_rows(docs))
    assert torch.equal(terms[2], terms[3])
    qt = torch.from_numpy(lexical.term_rows([" ".join(words), "coffee coffee", "coffee", "tea w16"], 16))
    assert int((qt[0] != 0).sum()) == 16 and torch.equal(qt[1], qt[2])
    u, dw, r = _weights(terms, qt, 1.0)
    ids, sc, cnt = _search(_vectors(N, 8, g), torch.zeros(N, dtype=torch.int32), torch.zeros(N, dtype=torch.int64),
                           terms, _vectors(4, 8, g), _i32([0] * 4), _i64([0] * 4), _i32([N] * 4), N, qt, u, dw, r)
    score = {int(i): float(s) for i, s in zip(ids[0], sc[0])}
    assert score[0] == 0.0 and score[1] > 0.0 and score[5] > score[1]     # "w16" fell off the query
    assert torch.equal(ids[1], ids[2]) and torch.equal(sc[1].view(torch.int32), sc[2].view(torch.int32))
    assert ids[1, :2].tolist() == [2, 3] and float(sc[1, 0]) == float(sc[1, 1]) > 0.0 == float(sc[1, 2])
    assert ids[3, :2].tolist() == [0, 4] or ids[3, :2].tolist() == [4, 0]


@pytest.mark.parametrize("nq", [64, 65])
def test_hybrid_query_counts(nq):
    g = torch.Generator().manual_seed(nq)
    rng = np.random.default_rng(nq)
    N = 500
    terms = edge_terms(N, rng)
    users = torch.randint(0, 40, (N,), generator=g, dtype=torch.int32)
    dates = torch.randint(0, 1000, (N,), generator=g, dtype=torch.int64)
    qt = _qterms([[SPECIAL[i % 4]] + [POOL + int(x) for x in rng.permutation(200)[: i % 16]] for i in range(nq)])
    alpha = torch.tensor([(0.0, 0.5, 1.0, 0.3)[i % 4] for i in range(nq)])
    u, dw, r = _weights(terms, qt, alpha)
    q_user = (torch.arange(nq, dtype=torch.int32) * 7) % 43 - 1           # -1 and 40, 41: nobody
    q_floor = torch.where(torch.arange(nq) % 3 == 0, SENTINEL, torch.randint(0, 1000, (nq,), generator=g))
    ks = torch.randint(0, 13, (nq,), generator=g, dtype=torch.int32)
    _, _, cnt = _search(_vectors(N, 8, g), users, dates, terms, _vectors(nq, 8, g), q_user, q_floor.to(torch.int64),
                        ks, 8, qt, u, dw, r)
    assert cnt.shape == (nq,)


def many_candidates_case():
    """8,193 rows of one user at D = 8: one more than the select kernel sorts."""
    g = torch.Generator().manual_seed(41)
    N = 8400
    users = torch.full((N,), 9, dtype=torch.int32)
    users[torch.randperm(N, generator=g)[:8193]] = 0
    terms = edge_terms(N, np.random.default_rng(41))
    qt = _qterms([[TOP, POOL + 1, POOL + 2], [BKT, POOL + 3], SPECIAL])
    u, dw, r = _weights(terms, qt, torch.tensor([0.5, 1.0, 0.25]))
    return (_vectors(N, 8, g), users, torch.zeros(N, dtype=torch.int64), terms, _vectors(3, 8, g), _i32([0, 0, 9]),
            _i64([0, 0, 0]), _i32([10, 9000, 5]), 9000, qt, u, dw, r)


@pytest.mark.parametrize("cap", [65536, 8192], ids=["score_list", "full_recompute"])
def test_hybrid_more_candidates_than_the_sort_holds(cap):
    """Above SORT_CAP the host finishes from the device score list; with cap = 8192 the candidate list
    overflows too and the scores are recomputed in torch."""
    _, _, cnt = _search(*many_candidates_case(), cap=cap)
    assert cnt.tolist() == [10, 8193, 5]


@pytest.mark.parametrize("D", [1032, 12])
def test_hybrid_bad_width_raises_and_writes_nothing(D):
    g = torch.Generator().manual_seed(D)
    N = 64
    users, dates = torch.zeros(N, dtype=torch.int32), torch.zeros(N, dtype=torch.int64)
    terms = edge_terms(N, np.random.default_rng(D))
    qt = _qterms([[TOP], [ONE]])
    u, dw, r = _weights(terms, qt, 0.5)
    args = (_i32([0, 0]), _i64([0, 0]), _i32([4, 4]), 4, qt, u, dw, r)
    _search(_vectors(N, 8, g), users, dates, terms, _vectors(2, 8, g), *args)       # sizes the workspace for (2, N)
    ws = retrieval_ops._WS
    ws.counts.fill_(7), ws.cand.fill_(7), ws.scores.fill_(7.0)
    with pytest.raises(RuntimeError):
        ops.filtered_topk_hybrid(*_dev(_vectors(N, D, g), users, dates, terms, _vectors(2, D, g), *args[:3]), 4,
                                 *_dev(qt, u, dw, r))
    torch.cuda.synchronize()
    assert bool((ws.counts == 7).all()) and bool((ws.cand == 7).all()) and bool((ws.scores == 7.0).all())


@pytest.mark.parametrize("path", ["kernel", "host_list"])
def test_hybrid_is_bitwise_repeatable(path):
    if path == "kernel":
        g = torch.Generator().manual_seed(5)
        N = 257
        terms = edge_terms(N, np.random.default_rng(5))
        qt = _qterms(EDGE_QUERIES)
        u, dw, r = _weights(terms, qt, torch.tensor(EDGE_ALPHA))
        args = (_vectors(N, 768, g), torch.zeros(N, dtype=torch.int32), torch.zeros(N, dtype=torch.int64), terms,
                _vectors(6, 768, g), _i32([0] * 6), _i64([0] * 6), _i32([50] * 6), 64, qt, u, dw, r)
    else:
        args = many_candidates_case()
    dev_args = _dev(*args[:8]) + [args[8]] + _dev(*args[9:])
    a = ops.filtered_topk_hybrid(*dev_args)
    b = ops.filtered_topk_hybrid(*dev_args)
    for x, y in zip(a, b):
        assert torch.equal(x.cpu().view(torch.int32), y.cpu().view(torch.int32))


# ---- exact cases ------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [8, 520, 768])
def test_hybrid_alpha_zero_equals_the_dense_kernel_bit_for_bit(D):
    g = torch.Generator().manual_seed(D + 1)
    N = 257
    terms = edge_terms(N, np.random.default_rng(D))
    users = torch.randint(0, 2, (N,), generator=g, dtype=torch.int32)
    dates = torch.randint(0, 100, (N,), generator=g, dtype=torch.int64)
    qt = _qterms(EDGE_QUERIES[:4])
    u, dw, r = _weights(terms, qt, 0.0)
    assert not u.any() and dw.tolist() == [1.0] * 4
    base = (_vectors(N, D, g), users, dates)
    q = (_vectors(4, D, g), _i32([0, 1, 1, 0]), _i64([0, 50, SENTINEL, 99]), _i32([10, 200, 1, 64]))
    want = ops.filtered_topk(*_dev(*base, *q), 64)
    got = ops.filtered_topk_hybrid(*_dev(*base, terms, *q), 64, *_dev(qt, u, dw, r))
    for x, y in zip(got, want):
        assert x.dtype == y.dtype and torch.equal(x.cpu().view(torch.int32), y.cpu().view(torch.int32))


def dyadic_case():
    """alpha = 1 with weights that are small dyadic fractions and a dyadic r table: every sum is exact in
    float32 in any order, so the kernel must equal the torch reference exactly.  Many rows share a score."""
    g = torch.Generator().manual_seed(77)
    N = 300
    terms = edge_terms(N, np.random.default_rng(77))
    users = torch.randint(0, 2, (N,), generator=g, dtype=torch.int32)
    dates = torch.zeros(N, dtype=torch.int64)
    qt = _qterms([SPECIAL + [POOL + i for i in range(12)], [TOP, POOL + 7], [POOL + i for i in range(16)]])
    u = torch.zeros((3, 16))
    u[0] = 2.0 ** -torch.arange(1, 17).float()
    u[1, :2] = torch.tensor([0.75, 0.25])
    u[2] = 1 / 16
    dw = torch.zeros(3)
    r = 2.0 ** -(torch.arange(33) % 3).float()
    return (_vectors(N, 8, g), users, dates, terms, _vectors(3, 8, g), _i32([0, 1, 1]), _i64([0, 0, 0]),
            _i32([40, 300, 25]), 64, qt, u, dw, r)


def test_hybrid_alpha_one_dyadic_weights_are_exact_and_ties_come_back_by_row_id():
    args = dyadic_case()
    ids, sc, cnt = _search(*args)
    corpus, users, dates, terms, queries, q_user, q_floor, ks, kmax, qt, u, dw, r = args
    want = ops.filtered_topk_hybrid_ref(corpus, users, dates, terms, queries, q_user.tolist(), q_floor.tolist(),
                                        ks.tolist(), kmax, qt, u, dw, r)
    assert torch.equal(ids, want[0]) and torch.equal(cnt, want[2])
    assert torch.equal(sc.view(torch.int32), want[1].view(torch.int32))
    # ties: within a run of equal scores the ids ascend, and there are such runs
    runs = 0
    for qi in range(3):
        k = int(cnt[qi])
        same = sc[qi, 1:k] == sc[qi, :k - 1]
        runs += int(same.sum())
        assert bool((ids[qi, 1:k][same] > ids[qi, :k - 1][same]).all())
    assert runs > 20


# ---- df kernel --------------------------------------------------------------------------------------
def _df_rows(n, rng):
    rows = rng.integers(1, 1 << 32, size=(n, 32), dtype=np.uint64).astype(np.uint32)
    rows[rng.random((n, 32)) < 0.3] = 0
    rows[:, 0] = 0x811C0000 + 77                             # a field label: every row carries it
    rows[::3, 5] = BKT
    rows[1::3, 9] = BKT2                                     # lands in BKT's bucket
    return rows.view(np.int32)


@pytest.mark.parametrize("n", [1, 64, 65, 5000])
def test_lex_df_add_equals_bincount(n):
    rng = np.random.default_rng(n)
    a, b = _df_rows(n, rng), _df_rows(n // 2 + 1, rng)
    df = torch.zeros(1 << 20, dtype=torch.int32, device=DEV)
    ops.lex_df_add(torch.from_numpy(a).to(DEV), df)
    want = np.bincount(lexical.buckets(a), minlength=1 << 20)
    assert np.array_equal(df.cpu().numpy(), want)
    assert int(df[(0x811C0000 + 77) & 0xFFFFF]) >= n and int(df[BKT & 0xFFFFF]) >= len(a[::3]) + len(a[1::3])
    ops.lex_df_add(torch.from_numpy(b).to(DEV), df)          # a second call accumulates
    want = want + np.bincount(lexical.buckets(b), minlength=1 << 20)
    assert np.array_equal(df.cpu().numpy(), want)
    same = np.zeros((n, 32), np.int32)
    same[:, 31] = TOP                                        # every row carries one and the same term
    df.zero_()
    ops.lex_df_add(torch.from_numpy(same).to(DEV), df)
    assert int(df[5]) == n and int(df.sum()) == n


# ---- store ------------------------------------------------------------------------------------------
def test_device_store_agrees_with_numpy_store_on_the_gpu():
    docs, vecs, qtexts, qvecs, users, floors, limits = store_case()
    ref = NumpyVectorStore(64, lexical=True)
    dev = DeviceVectorStore(64, device=DEV, lexical=True)
    fill_case(ref, docs, vecs, batches=1)
    fill_case(dev, docs, vecs, batches=2)
    assert np.array_equal(dev.terms[: dev.size].cpu().numpy(), ref.terms)
    assert np.array_equal(dev.df.cpu().numpy(), ref.df) and dev.total_terms == ref.total_terms
    assert np.array_equal(dev.vectors[: dev.size].float().cpu().numpy(), ref.vectors)    # exact in bf16
    assert_topk_boundary_is_clear(ref, qvecs, qtexts, users, floors, limits, 0.5)
    want = ref.search_batch(qvecs, users, floors, limits, texts=qtexts, alpha=0.5)
    got = dev.search_batch(qvecs, users, floors, limits, texts=qtexts, alpha=0.5)
    assert [[h.id for h in hs] for hs in got] == [[h.id for h in hs] for hs in want]
    # both float32 scores lie within tol of fp64, and tol <= 32 * 2^-24 * (0.5 * 1 + 0.5 * r) < 2e-6 here
    np.testing.assert_allclose([h.score for hs in got for h in hs], [h.score for hs in want for h in hs],
                               rtol=0, atol=4e-6)
    dense = dev.search_batch(qvecs, users, floors, limits)
    again = dev.search_batch(qvecs, users, floors, limits, texts=qtexts, alpha=0.0)
    assert [[(h.id, h.score) for h in hs] for hs in again] == [[(h.id, h.score) for h in hs] for hs in dense]
