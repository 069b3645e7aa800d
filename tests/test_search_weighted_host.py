"""CPU tests of the weighted query terms (bm25_search_weighted,
bm25_score_docs_weighted and their device forms): the symbols are exported,
bound and documented, a NULL handle is rejected without a GPU, the Python
layers reject malformed shapes before any C call, and
bm25s_io.weighted_query_ids keeps ids and weights together.

The numpy reference of the GPU tests (tests/test_gpu_search_weighted.py) and
their weighted fixture live here, with two tests that guard them: with unit
weights the reference is the C oracle's dense row bit for bit, and on the
fixture a fused multiply-add reference differs from it — so a kernel that
contracts the multiply into the add cannot pass the GPU tests by luck."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle
from test_gpu_edges import TILE, _columns, _csc, _edge_index

SYMS = {"bm25_search_weighted": 11, "bm25_search_weighted_device": 12,
        "bm25_score_docs_weighted": 8, "bm25_score_docs_weighted_device": 9}


# ------------------------------------------------------------ the reference
def ref_scores(n_docs, ip, ix, dt, ids, weights, fused=False):
    """The dense fp32 row of one weighted query: for each valid (id, weight)
    in query order, s[docs of the term] += float32(weight) * values — the
    multiply and the add are separate float32 ufuncs (a column holds a
    document once, so the fancy-indexed update is the per-document fold).
    fused: every step as one multiply-add, rounded once (what a contracted
    kernel would compute)."""
    s = np.zeros(n_docs, np.float32)
    V = len(ip) - 1
    for t, w in zip(np.asarray(ids).tolist(), np.asarray(weights, np.float32)):
        if t < 0 or t >= V:
            continue
        seg = slice(int(ip[t]), int(ip[t + 1]))
        if fused:
            s[ix[seg]] = (np.float64(w) * dt[seg].astype(np.float64)
                          + s[ix[seg]].astype(np.float64)).astype(np.float32)
        else:
            s[ix[seg]] = s[ix[seg]] + np.float32(w) * dt[seg]
    return s


def ref_rows(n_docs, ip, ix, dt, q, w, fused=False):
    return [ref_scores(n_docs, ip, ix, dt, q[r], w[r], fused) for r in range(len(q))]


# ------------------------------------------------------------- the fixture
SHORT = 40          # first of the short terms of weighted_index
N_SHORT = 160


@functools.lru_cache(maxsize=None)
def weighted_index(n_docs):
    """_edge_index (40 signed quarter-step terms, an empty one and one of
    every document) followed by N_SHORT short terms of 1-3 postings per tile:
    several of them fit one 64-posting row, so rows span term boundaries."""
    rng = np.random.default_rng(7000 + n_docs)
    ip, ix, dt = _edge_index(rng, n_docs, SHORT, min(n_docs, 3000))
    cols = _columns(ip, ix, dt)
    ntiles = (n_docs + TILE - 1) // TILE
    for _ in range(N_SHORT):
        docs = []
        for tile in range(ntiles):
            lo, hi = tile * TILE, min((tile + 1) * TILE, n_docs)
            docs.append(rng.choice(np.arange(lo, hi), min(int(rng.integers(1, 4)), hi - lo),
                                   replace=False))
        docs = np.sort(np.concatenate(docs)).astype(np.int32)
        vals = (np.round(rng.uniform(-2.0, 3.0, len(docs)) * 8) / 8 + 0.0625).astype(np.float32)
        cols.append((docs, vals))
    ip, ix, dt = _csc(cols, np.float32)
    for a in (ip, ix, dt):
        a.setflags(write=False)
    return ip, ix, dt, SHORT + N_SHORT


def weighted_queries(n_docs, T, Q=6):
    """Q rows of T (id, weight) slots over weighted_index(n_docs): mostly
    short terms, some long ones and padding; random float32 weights of both
    signs with |w| in [2^-6, 2^6], the exact ones -2, 0.25, 1.5 mixed in, NaN
    on the padding slots, and in row 0 (T >= 2) one id twice with two
    different weights."""
    rng = np.random.default_rng(100 * n_docs + T)
    V = SHORT + N_SHORT
    q = rng.integers(SHORT, V, size=(Q, T)).astype(np.int32)
    long_ = rng.random((Q, T)) < 0.15
    q[long_] = rng.integers(0, SHORT, size=int(long_.sum()))
    q[rng.random((Q, T)) < 0.1] = -1
    mag = np.exp2(rng.uniform(-6.0, 6.0, (Q, T)))
    w = (mag * rng.choice([-1.0, 1.0], (Q, T))).astype(np.float32)
    exact = rng.random((Q, T)) < 0.15
    w[exact] = rng.choice(np.array([-2.0, 0.25, 1.5], np.float32), int(exact.sum()))
    if T >= 2:
        q[0, 0] = q[0, 1] = SHORT + 3
        w[0, 0], w[0, 1] = np.float32(1.7), np.float32(-0.3)
    else:
        q[0, 0] = SHORT + 3
    w[q < 0] = np.nan
    return q, w


def spanning_rows(n_docs, ip, ix, q):
    """(query, tile) pairs whose first 64 concatenated postings come from more
    than one term (the row of add_group that spans a term boundary)."""
    n = 0
    ntiles = (n_docs + TILE - 1) // TILE
    for row in q:
        for tile in range(ntiles):
            terms, left = 0, 64
            for t in row:
                if t < 0 or left <= 0:
                    continue
                col = ix[ip[t]:ip[t + 1]]
                c = int(np.searchsorted(col, (tile + 1) * TILE) - np.searchsorted(col, tile * TILE))
                if c:
                    terms += 1
                    left -= c
            n += terms > 1
    return n


# ------------------------------------------------- guards of the yardstick
def test_reference_with_unit_weights_is_the_oracle():
    rng = np.random.default_rng(3)
    N, V = 5000, 40
    ip, ix, dt = _edge_index(rng, N, V, 2500)
    assert (dt < 0).any()
    q = rng.integers(-1, V, size=(5, 9)).astype(np.int32)
    q[1, 3] = q[1, 4]  # a repeated id
    for row in q:
        got = ref_scores(N, ip, ix, dt, row, np.ones(9, np.float32))
        want = oracle.scores_dense_c(N, ip, ix, dt, row)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("T", [8, 65, 130])
@pytest.mark.parametrize("n_docs", [2047, 2049, 70_001])
def test_fused_reference_differs_on_the_fixture(n_docs, T):
    ip, ix, dt, V = weighted_index(n_docs)
    q, w = weighted_queries(n_docs, T)
    assert np.isnan(w[q < 0]).all() and np.isfinite(w[q >= 0]).all()
    assert (w[q >= 0] < 0).any() and (w[q >= 0] > 0).any()
    assert q[0, 0] == q[0, 1] and w[0, 0] != w[0, 1]
    assert spanning_rows(n_docs, ip, ix, q) > 0
    plain = np.stack(ref_rows(n_docs, ip, ix, dt, q, w))
    fused = np.stack(ref_rows(n_docs, ip, ix, dt, q, w, fused=True))
    assert np.isfinite(plain).all()
    pv = plain.view(np.uint32)
    assert (pv != fused.view(np.uint32)).any()
    assert not (pv == 0x80000000).any()
    # the tests stay out of the subnormal range
    assert not ((plain != 0) & (np.abs(plain) < np.float32(1.17549435e-38))).any()


def test_fixture_with_one_term():
    q, w = weighted_queries(2049, 1)
    assert q.shape == (6, 1) and (q >= -1).all()


# ------------------------------------------------------------- the C-ABI
def test_symbols_exported_bound_and_documented():
    from bm25mi import _capi
    syms = _capi.header_symbols()
    text = open(_capi.HEADER).read()
    for s, nargs in SYMS.items():
        assert s in syms, s
        f = getattr(_capi.lib, s)
        assert f.restype is ctypes.c_int and s in _capi._SIGS, s
        assert len(f.argtypes) == nargs, s
    doc = text[text.index("Weighted query terms:"):text.index("int bm25_search_weighted(")]
    for phrase in ("Replaces no reference call: BM25v.search takes no weights",
                   "(bm25_native.py:76-158)", "never an FMA", "rounded to fp32 on its own",
                   "1.0f", "0.0f", "same as padding", "must be finite", "BM25_EINVAL",
                   "tile-bound threshold", "negative", "8192", "no filter for every"):
        assert phrase in doc, phrase
    assert "8192 (a flag): the last search was weighted" in text
    assert _capi.abi_version() == 1  # additive: the ABI version stays
    assert "#define BM25MI_ABI_VERSION 1" in text


def test_null_handle_is_einval_without_gpu():
    from bm25mi._capi import BM25_EINVAL, lib
    q = np.zeros((1, 2), np.int32)
    w = np.ones((1, 2), np.float32)
    m = np.full((1, 1), 0xFFFFFFFF, np.uint32)
    qm = np.zeros(1, np.int32)
    docs = np.full((1, 3), 7, np.int32)
    scores = np.full((1, 3), 7.0, np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.bm25_search_weighted(None, p(q), p(w), 1, 2, 3, p(m), 1, p(qm), p(docs),
                                    p(scores)) == BM25_EINVAL
    assert b"NULL index" in lib.bm25_last_error()
    assert lib.bm25_search_weighted_device(None, p(q), p(w), 1, 2, 3, p(m), 1, p(qm), p(docs),
                                           p(scores), None) == BM25_EINVAL
    assert b"NULL index" in lib.bm25_last_error()
    assert lib.bm25_score_docs_weighted(None, p(q), p(w), 1, 2, p(docs), 3,
                                        p(scores)) == BM25_EINVAL
    assert b"NULL index" in lib.bm25_last_error()
    assert lib.bm25_score_docs_weighted_device(None, p(q), p(w), 1, 2, p(docs), 3, p(scores),
                                               None) == BM25_EINVAL
    assert b"NULL index" in lib.bm25_last_error()
    assert (docs == 7).all() and (scores == 7.0).all()


# ------------------------------------------------------- the Python layers
def _bare_index(n_docs=70):
    """A GpuIndex object without a handle: shape validation runs before the
    handle is touched, so it needs no device."""
    from bm25mi.index import GpuIndex
    g = GpuIndex.__new__(GpuIndex)
    g._h = None
    g.n_docs, g.n_terms, g.doc_offset = n_docs, 5, 0
    return g


def test_gpu_index_weighted_rejects_shapes_before_c():
    g = _bare_index(70)  # W = 3
    q = np.zeros((2, 3), np.int32)
    w = np.ones((2, 3), np.float32)
    with pytest.raises(ValueError, match="queries must be a 2-D"):
        g.search_weighted(np.zeros(3, np.int32), np.ones(3, np.float32), 1)
    with pytest.raises(ValueError, match="weights must be .* shape"):
        g.search_weighted(q, np.ones((2, 4), np.float32), 1)
    with pytest.raises(ValueError, match="weights must be .* shape"):
        g.search_weighted(q, np.ones(6, np.float32), 1)
    with pytest.raises(ValueError, match="weights must be .* shape"):
        g.search_weighted(q, np.ones((3, 2), np.float32), 1)
    with pytest.raises(ValueError, match=r"70 \(n_docs\) columns"):
        g.search_weighted(q, w, 1, np.ones((2, 69), bool))
    with pytest.raises(ValueError, match="3 .* words per row"):
        g.search_weighted(q, w, 1, np.zeros((2, 2), np.uint32))
    with pytest.raises(ValueError, match=r"one mask id per query \(2\)"):
        g.search_weighted(q, w, 1, np.ones((2, 70), bool), np.zeros(3, np.int32))
    with pytest.raises(ValueError, match=r"in \[-1, 2\)"):
        g.search_weighted(q, w, 1, np.ones((2, 70), bool), np.array([0, 2], np.int32))
    with pytest.raises(ValueError, match=r"in \[-1, 0\)"):
        g.search_weighted(q, w, 1, None, np.array([0, -1], np.int32))
    d = np.zeros((2, 2), np.int32)
    with pytest.raises(ValueError, match="queries must be a 2-D"):
        g.score_docs_weighted(np.zeros(3, np.int32), np.ones(3, np.float32), d)
    with pytest.raises(ValueError, match="weights must be .* shape"):
        g.score_docs_weighted(q, np.ones((2, 2), np.float32), d)
    with pytest.raises(ValueError, match="docs must be a 2-D"):
        g.score_docs_weighted(q, w, np.zeros(2, np.int32))
    with pytest.raises(ValueError, match="queries has 2 rows, docs has 3"):
        g.score_docs_weighted(q, w, np.zeros((3, 2), np.int32))


def test_gpu_index_weighted_device_rejects_shapes_before_c():
    import torch
    g = _bare_index(70)
    q = torch.zeros((2, 3), dtype=torch.int32)
    w = torch.ones((2, 3), dtype=torch.float32)
    m = torch.zeros((2, 3), dtype=torch.int32)
    qm = torch.zeros(2, dtype=torch.int32)
    d = torch.zeros((2, 4), dtype=torch.int32)
    s = torch.zeros((2, 4), dtype=torch.float32)
    with pytest.raises(ValueError, match="2-D"):
        g.search_weighted_device(q[0], w[0], 4, m, qm, d, s)
    with pytest.raises(ValueError, match="d_weights must be a float32"):
        g.search_weighted_device(q, w[:, :2], 4, m, qm, d, s)
    with pytest.raises(ValueError, match="d_weights must be a float32"):
        g.search_weighted_device(q, w.to(torch.float64), 4, m, qm, d, s)
    with pytest.raises(ValueError, match=r"packed \[M, 3\]"):
        g.search_weighted_device(q, w, 4, m[:, :2], qm, d, s)
    with pytest.raises(ValueError, match=r"one mask id per query \(2\)"):
        g.search_weighted_device(q, w, 4, m, torch.zeros(3, dtype=torch.int32), d, s)
    with pytest.raises(ValueError, match="2 x 4 results"):
        g.search_weighted_device(q, w, 4, None, None, d[:, :3], s)
    with pytest.raises(ValueError, match="d_weights must be a float32"):
        g.score_docs_weighted_device(q, w[:1], d, s)
    with pytest.raises(ValueError, match="2 x 4 scores"):
        g.score_docs_weighted_device(q, w, d, s[:, :3])


def test_bm25v_search_weighted_validation_before_gpu():
    import bm25_native
    m = bm25_native.BM25v()
    docs, scores = m.search_weighted([], [], 3)
    assert docs.shape == (0, 0) and scores.shape == (0, 0)
    with pytest.raises(ValueError, match="list of list"):
        m.search_weighted(np.array([1, 2], np.int32), np.ones(2, np.float32), 1)
    with pytest.raises(ValueError, match="list of list"):
        m.search_weighted(np.array([[1, 2]], np.int64), np.ones((1, 2), np.float32), 1)
    q = np.array([[0, -1]], np.int32)
    with pytest.raises(ValueError, match="weights must be .* shape"):
        m.search_weighted(q, np.ones((1, 3), np.float32), 1)
    with pytest.raises(ValueError, match="weights must be .* shape"):
        m.search_weighted(q, np.ones((2, 2), np.float32), 1)
    with pytest.raises(ValueError, match="negative dimensions"):
        m.search_weighted(q, np.ones((1, 2), np.float32), -1)
    with pytest.raises(ValueError, match=r"maximum token ID in the query \(5\)"):
        m.search_weighted(np.array([[5, -1]], np.int32), np.ones((1, 2), np.float32), 1)


def test_weighted_query_ids():
    from bm25mi.bm25s_io import query_ids, weighted_query_ids
    vocab = {"a": 0, "b": 1, "c": 2, "far": 9}
    queries = [[("c", 2.0), ("nope", 5.0), ("a", -0.5), ("far", 3.0), ("c", 0.25)],
               [],
               [("b", 1.5)]]
    ids, w = weighted_query_ids(queries, vocab, n_terms=3)
    assert ids.dtype == np.int32 and w.dtype == np.float32 and ids.shape == w.shape == (3, 3)
    assert ids.tolist() == [[2, 0, 2], [-1, -1, -1], [1, -1, -1]]
    assert w.tolist() == [[2.0, -0.5, 0.25], [0.0, 0.0, 0.0], [1.5, 0.0, 0.0]]
    # the drop rules of query_ids
    assert np.array_equal(ids, query_ids([[t for t, _ in q] for q in queries], vocab, 3))
    ids2, w2 = weighted_query_ids(queries, vocab, n_terms=3, width=2)
    assert ids2.tolist() == [[2, 0], [-1, -1], [1, -1]]
    assert w2.tolist() == [[2.0, -0.5], [0.0, 0.0], [1.5, 0.0]]
    ids5, w5 = weighted_query_ids(queries, vocab, n_terms=3, width=5)
    assert ids5.shape == w5.shape == (3, 5) and (ids5[:, 3:] == -1).all() and not w5[:, 3:].any()
    e_ids, e_w = weighted_query_ids([], vocab, 3)
    assert e_ids.shape == e_w.shape == (0, 1)
