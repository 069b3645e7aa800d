"""CPU tests of the cursor pagination (bm25_search_after,
bm25_search_after_device): the symbols are exported, bound and documented, a
NULL handle is rejected without a GPU, the Python layers reject malformed
shapes, dtypes and a one-sided ``after`` before any C call, and page_cursor
round-trips (padding column included).

The numpy reference of the GPU tests (tests/test_gpu_search_after.py), their
fixtures and their cursors live here, with the tests that guard them: pages
of the reference concatenated are the C oracle's top-(k P) bit for bit, and
every cursor the GPU tests place inside a tie really sits inside one — an
allowed document of equal score on either side of it, and an equal-score
pair across the tile boundary 2047 / 2048 — so a `>=` for `>` in the tie
rule or a slip at a tile edge cannot pass unseen."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle
from test_gpu_edges import FULL, TILE, _edge_index, _edge_queries
from test_search_weighted_host import ref_rows, weighted_index, weighted_queries

SYMS = {"bm25_search_after": 13, "bm25_search_after_device": 14}
AFTER_NONE = -2
PAD = 0xFFFFFFFF
PAGE_DOCS = (1, 33, 2047, 2048, 2049, 5000, 70_001)   # the paging test's n_docs
V = 40


# ------------------------------------------------------------ the reference
def score_keys(s):
    """The engine's order of fp32 scores as uint32 (csrc/bm25mi_internal.h,
    score_key): numeric order, -0.0 just below +0.0."""
    u = np.ascontiguousarray(s, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def ordered(row, allowed=None):
    """The ids of one dense score row in result order (score descending, doc
    ascending), restricted to ``allowed`` (bool [n_docs] or None)."""
    ids = np.arange(len(row)) if allowed is None else np.nonzero(allowed)[0]
    return ids[np.lexsort((ids, -score_keys(row[ids]).astype(np.int64)))]


def ref_after(rows, k, after=None, allow=None, query_mask=None, doc_offset=0):
    """rows: the queries' dense score rows; after: None or (scores [Q], docs
    [Q]) with global doc ids; allow: bool [M, n_docs] (or None: no masks);
    query_mask: per query its mask (-1: no filter; None: mask 0 when there
    are masks).  Each row: the allowed ids strictly after its cursor, in
    order, the first k, padded with doc -1 / score bits 0xFFFFFFFF."""
    Q = len(rows)
    docs = np.full((Q, k), -1, np.int32)
    bits = np.full((Q, k), PAD, np.uint32)
    for r, row in enumerate(rows):
        m = -1 if allow is None else 0 if query_mask is None else int(query_mask[r])
        ids = ordered(row, None if m < 0 else allow[m])
        if after is not None and int(after[1][r]) != AFTER_NONE:
            c = int(after[1][r])
            if c == -1:
                ids = ids[:0]
            else:
                assert c >= 0
                sk = score_keys(row[ids]).astype(np.int64)
                ck = int(score_keys(np.float32(after[0][r]).reshape(1))[0])
                ids = ids[(sk < ck) | ((sk == ck) & (ids.astype(np.int64) + doc_offset > c))]
        ids = ids[:k]
        docs[r, :len(ids)] = ids + doc_offset
        bits[r, :len(ids)] = row[ids].view(np.uint32)
    return docs, bits.view(np.float32)


def last_column(page):
    """What bm25mi.page_cursor gives, without the package."""
    return (np.ascontiguousarray(page[1][:, -1], np.float32),
            np.ascontiguousarray(page[0][:, -1], np.int32))


# ------------------------------------------------------------- the fixtures
@functools.lru_cache(maxsize=None)
def after_case(n_docs):
    """_edge_index (40 signed quarter-step terms: long tie runs, a positive, a
    zero-score and a negative region) with 7 queries of 8 slots (the last all
    padding) and their dense oracle rows.  Where they exist, documents 2047
    and 2048 hold the same value of the term of every document, so row 1
    (that term alone) ties across the first tile boundary."""
    rng = np.random.default_rng(500 + n_docs)
    ip, ix, dt = _edge_index(rng, n_docs, V, min(n_docs, 3000))
    if n_docs > TILE:
        dt[ip[FULL] + TILE] = dt[ip[FULL] + TILE - 1] = np.float32(1.25)
    q = np.concatenate([_edge_queries(rng, V, 8), np.full((1, 8), -1, np.int32)])
    rows = [oracle.scores_dense_c(n_docs, ip, ix, dt, row) for row in q]
    for a in (ip, ix, dt, q, *rows):
        a.setflags(write=False)
    return ip, ix, dt, q, rows


@functools.lru_cache(maxsize=None)
def position_masks(n_docs=5000):
    """Two masks of the 5000-document fixture (60 % and 30 %; both allow 2046
    .. 2049 and disallow document 5) and the queries' mask ids, mixing -1, 0
    and 1."""
    rng = np.random.default_rng(77)
    allow = np.stack([rng.random(n_docs) < 0.6, rng.random(n_docs) < 0.3])
    allow[:, TILE - 2:TILE + 2] = True
    allow[:, 5] = False
    qm = np.array([-1, 0, 1, 0, -1, 1, 0], np.int32)
    allow.setflags(write=False)
    qm.setflags(write=False)
    return allow, qm


def _allowed(allow, qm, r, n_docs):
    return np.ones(n_docs, bool) if allow is None or qm[r] < 0 else allow[qm[r]]


def tie_cursor(rows, allow, qm):
    """Per row a cursor inside a tie run: the middle one of the three allowed
    documents that come first in the longest run of equal scores."""
    s = np.zeros(len(rows), np.float32)
    d = np.zeros(len(rows), np.int32)
    for r, row in enumerate(rows):
        ids = ordered(row, _allowed(allow, qm, r, len(row)))
        sk = score_keys(row[ids])
        vals, start, cnt = np.unique(sk, return_index=True, return_counts=True)
        j = int(np.argmax(cnt))
        assert cnt[j] >= 3
        first = int(np.nonzero(sk == vals[j])[0][0])
        d[r] = ids[first + 1]
        s[r] = row[d[r]]
    return s, d


def position_cursors(rows, allow, qm, doc_offset=0):
    """The cursors of the GPU tests' position cases on one fixture, as (name,
    (scores [Q], docs [Q])); doc ids are global (doc_offset added)."""
    Q, N = len(rows), len(rows[0])
    order = [ordered(row, _allowed(allow, qm, r, N)) for r, row in enumerate(rows)]
    f32 = lambda v: np.array(v, np.float32)
    i32 = lambda v: (np.array(v, np.int64) + doc_offset).astype(np.int32)
    out = [("best key", (f32([rows[r][order[r][0]] for r in range(Q)]),
                         i32([order[r][0] for r in range(Q)]))),
           ("worst key", (f32([rows[r][order[r][-1]] for r in range(Q)]),
                          i32([order[r][-1] for r in range(Q)])))]
    ts, td = tie_cursor(rows, allow, qm)
    out.append(("inside a tie", (ts, i32(td))))
    out.append(("tile edge", (f32([rows[r][TILE - 1] for r in range(Q)]), i32([TILE - 1] * Q))))
    between = []
    for r in range(Q):   # halfway between the two best distinct scores (the best one: one score)
        u = np.unique(rows[r][order[r]])
        between.append((np.float64(u[-1]) + np.float64(u[-2])) / 2 if len(u) > 1 else u[-1])
    out.append(("between scores", (f32(between), i32([0] * Q))))
    out.append(("+inf", (f32([np.inf] * Q), i32([0] * Q))))
    out.append(("disallowed doc", (f32([rows[r][5] for r in range(Q)]), i32([5] * Q))))
    out.append(("doc past n_docs", (ts, i32([N + 5] * Q))))
    if doc_offset > 0:
        out.append(("doc below doc_offset", (ts, np.full(Q, doc_offset - 7, np.int32))))
    md = i32(td)
    ms = ts.copy()
    md[::2] = AFTER_NONE
    ms[::2] = np.nan       # (not read)
    md[3] = -1
    out.append(("mixed with AFTER_NONE and -1", (ms, md)))
    return out


def rank_cursor(rows, rank, allow=None, qm=None, doc_offset=0):
    """Per row the key of its ``rank``-th result (1-based) as a cursor."""
    ids = [ordered(row, _allowed(allow, qm, r, len(row)))[rank - 1] for r, row in enumerate(rows)]
    return (np.array([rows[r][d] for r, d in enumerate(ids)], np.float32),
            (np.array(ids, np.int64) + doc_offset).astype(np.int32))


def weighted_case(n_docs=5000, T=8):
    ip, ix, dt, _ = weighted_index(n_docs)
    q, w = weighted_queries(n_docs, T)
    return ip, ix, dt, q, w, ref_rows(n_docs, ip, ix, dt, q, w)


def zero_band_cursor(rows):
    """Per row a cursor inside the band of +0.0 scores (the documents no term
    touches, in the middle of the order under weights of both signs): the
    second of its documents."""
    d = np.array([np.nonzero(row.view(np.uint32) == 0)[0][1] for row in rows], np.int32)
    return np.zeros(len(rows), np.float32), d


# ------------------------------------------------- guards of the yardstick
def _concat(pages):
    return np.concatenate([p[0] for p in pages], 1), np.concatenate([p[1] for p in pages], 1)


def _same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32),
                                                         b[1].view(np.uint32))


# (k > n_docs is the reference's argpartition error)
PAGE_CASES = [(n, k) for n in PAGE_DOCS for k in (1, 10) if k <= n]


@pytest.mark.parametrize("n_docs,k", PAGE_CASES)
def test_reference_pages_are_the_oracle_prefix(n_docs, k):
    ip, ix, dt, q, rows = after_case(n_docs)
    P = min(6, n_docs // k)
    pages, after = [], None
    for _ in range(P):
        pages.append(ref_after(rows, k, after))
        after = last_column(pages[-1])
    want = oracle.search_c(n_docs, ip, ix, dt, q, k * P)
    assert _same(_concat(pages), want)
    assert (np.asarray(want[0]) >= 0).all()


def test_reference_pages_are_the_oracle_prefix_weighted_and_masked():
    ip, ix, dt, q, rows = after_case(5000)
    allow, qm = position_masks()
    k, P = 10, 6
    pages, after = [], None
    for _ in range(P):
        pages.append(ref_after(rows, k, after, allow, qm))
        after = last_column(pages[-1])
    whole = ref_after(rows, k * P, None, allow, qm)
    assert _same(_concat(pages), whole)
    for r in np.nonzero(qm < 0)[0]:   # the unmasked rows: the oracle's search
        want = oracle.search_c(5000, ip, ix, dt, q[r:r + 1], k * P)
        assert _same((whole[0][r:r + 1], whole[1][r:r + 1]), want)
    _, _, _, wq, ww, wrows = weighted_case()
    pages, after = [], None
    for _ in range(P):
        pages.append(ref_after(wrows, k, after))
        after = last_column(pages[-1])
    assert _same(_concat(pages), ref_after(wrows, k * P))


@pytest.mark.parametrize("doc_offset", [0, 10_000])
def test_tie_cursors_sit_inside_ties(doc_offset):
    ip, ix, dt, q, rows = after_case(5000)
    allow, qm = position_masks()
    cur = dict(position_cursors(rows, allow, qm, doc_offset))
    assert len(cur) == (10 if doc_offset else 9)
    for name in ("inside a tie", "doc past n_docs", "mixed with AFTER_NONE and -1"):
        s, d = cur[name]
        for r, row in enumerate(rows):
            if d[r] < 0 or name == "doc past n_docs":
                continue
            ok = _allowed(allow, qm, r, 5000)
            same = np.nonzero(ok & (score_keys(row) == score_keys(s[r:r + 1])[0]))[0]
            loc = int(d[r]) - doc_offset
            assert (same < loc).any() and (same > loc).any() and loc in same, (name, r)
    # the equal-score pair across the tile boundary, both allowed, on row 1
    s, d = cur["tile edge"]
    assert (d == TILE - 1 + doc_offset).all()
    assert rows[1][TILE - 1] == rows[1][TILE] == s[1]
    for m in (0, 1):
        assert allow[m, TILE - 1] and allow[m, TILE]
    want = ref_after(rows, 3, cur["tile edge"], allow, qm, doc_offset)
    assert want[0][1, 0] == TILE + doc_offset
    # the disallowed doc really is, on the masked rows; between-scores is no score of the row
    assert not allow[:, 5].any()
    s, _ = cur["between scores"]
    assert sum(s[r] not in rows[r] for r in range(len(rows))) >= 4
    # the regions the paging test runs through at n_docs <= 33
    rr = after_case(33)[4]
    assert (rr[1] > 0).any() and (rr[1] < 0).any()      # the term of every document
    assert any((x > 0).any() and (x == 0).any() for x in rr)
    assert any((x == 0).any() and (x < 0).any() for x in rr)


def test_weighted_zero_band_is_in_the_middle():
    _, _, _, q, w, rows = weighted_case()
    s, d = zero_band_cursor(rows)
    for r, row in enumerate(rows):
        assert (row > 0).any() and (row < 0).any() and (row.view(np.uint32) == 0).sum() >= 3
        assert row[d[r]] == 0 and not (row.view(np.uint32) == 0x80000000).any()


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
    doc = text[text.index("Cursor pagination"):text.index("int bm25_search_after(")]
    for phrase in ("Replaces no reference call: BM25v.search has no cursor",
                   "(bm25_native.py:76-158)", "#define BM25_AFTER_NONE (-2)", "exhausted",
                   "Returned scores are never", "-0.0f", "BM25_EINVAL", "16384", "doc_offset + d > c",
                   "bm25_merge_topk_device"):
        assert phrase in doc, phrase
    assert "16384 (a flag)" in text
    assert _capi.abi_version() == 1  # additive: the ABI version stays
    assert "#define BM25MI_ABI_VERSION 1" in text
    import bm25mi
    assert bm25mi.AFTER_NONE == AFTER_NONE
    from bm25mi.index import GpuIndex
    assert GpuIndex.KERNELS[16384] == "after"


def test_null_handle_is_einval_without_gpu():
    from bm25mi._capi import BM25_EINVAL, lib
    q = np.zeros((1, 2), np.int32)
    w = np.ones((1, 2), np.float32)
    a_s = np.zeros(1, np.float32)
    a_d = np.zeros(1, np.int32)
    docs = np.full((1, 3), 7, np.int32)
    scores = np.full((1, 3), 7.0, np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.bm25_search_after(None, p(q), p(w), 1, 2, 3, None, 0, None, p(a_s), p(a_d),
                                 p(docs), p(scores)) == BM25_EINVAL
    assert b"NULL index" in lib.bm25_last_error()
    assert lib.bm25_search_after_device(None, p(q), p(w), 1, 2, 3, None, 0, None, p(a_s), p(a_d),
                                        p(docs), p(scores), None) == BM25_EINVAL
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


def test_page_cursor_round_trips():
    import bm25mi
    docs = np.array([[4, 9, 2], [7, -1, -1]], np.int32)
    scores = np.array([[3.0, 1.5, 1.5], [0.25, 0, 0]], np.float32)
    scores.view(np.uint32)[1, 1:] = PAD
    s, d = bm25mi.page_cursor(docs, scores)
    assert s.dtype == np.float32 and d.dtype == np.int32 and s.shape == d.shape == (2,)
    assert s.flags.c_contiguous and d.flags.c_contiguous
    assert d.tolist() == [2, -1]
    assert s.view(np.uint32).tolist() == [np.float32(1.5).view(np.uint32), PAD]
    assert _same((d[:, None], s[:, None]), (docs[:, -1:], scores[:, -1:]))
    # the padding column is the "exhausted" cursor: the reference pads the row
    rows = [np.arange(5, dtype=np.float32), np.arange(5, dtype=np.float32)]
    nxt = ref_after(rows, 2, (s, d))
    assert nxt[0].tolist() == [[1, 0], [-1, -1]]
    import torch
    ts, td = bm25mi.page_cursor(torch.from_numpy(docs), torch.from_numpy(scores))
    assert ts.is_contiguous() and td.is_contiguous()
    assert td.tolist() == [2, -1] and ts.dtype == torch.float32 and td.dtype == torch.int32
    with pytest.raises(ValueError, match="2-D"):
        bm25mi.page_cursor(docs[0], scores[0])
    with pytest.raises(ValueError, match="2-D"):
        bm25mi.page_cursor(docs, scores[:, :2])
    with pytest.raises(ValueError, match="no cursor"):
        bm25mi.page_cursor(docs[:, :0], scores[:, :0])


def test_gpu_index_after_rejects_shapes_before_c():
    g = _bare_index(70)  # W = 3
    q = np.zeros((2, 3), np.int32)
    w = np.ones((2, 3), np.float32)
    s = np.zeros(2, np.float32)
    d = np.zeros(2, np.int32)
    with pytest.raises(ValueError, match="queries must be a 2-D"):
        g.search_after(np.zeros(3, np.int32), 1)
    with pytest.raises(ValueError, match="weights must be .* shape"):
        g.search_after(q, 1, None, np.ones((2, 4), np.float32))
    with pytest.raises(ValueError, match=r"70 \(n_docs\) columns"):
        g.search_after(q, 1, None, w, np.ones((2, 69), bool))
    with pytest.raises(ValueError, match="3 .* words per row"):
        g.search_after(q, 1, None, None, np.zeros((2, 2), np.uint32))
    with pytest.raises(ValueError, match=r"one mask id per query \(2\)"):
        g.search_after(q, 1, None, None, np.ones((2, 70), bool), np.zeros(3, np.int32))
    with pytest.raises(ValueError, match=r"in \[-1, 2\)"):
        g.search_after(q, 1, None, None, np.ones((2, 70), bool), np.array([0, 2], np.int32))
    with pytest.raises(ValueError, match=r"in \[-1, 0\)"):
        g.search_after(q, 1, None, None, None, np.array([0, -1], np.int32))
    with pytest.raises(ValueError, match="None or a pair"):
        g.search_after(q, 1, s)
    with pytest.raises(ValueError, match="None or a pair"):
        g.search_after(q, 1, (s, d, d))
    with pytest.raises(ValueError, match="both halves"):
        g.search_after(q, 1, (s, None))
    with pytest.raises(ValueError, match="both halves"):
        g.search_after(q, 1, (None, d))
    with pytest.raises(ValueError, match="float32 scores, int32 docs"):
        g.search_after(q, 1, (s.astype(np.float64), d))
    with pytest.raises(ValueError, match="float32 scores, int32 docs"):
        g.search_after(q, 1, (s, d.astype(np.int64)))
    with pytest.raises(ValueError, match="float32 scores, int32 docs"):
        g.search_after(q, 1, (d, s))   # the halves swapped
    with pytest.raises(ValueError, match=r"one cursor per query \(2\)"):
        g.search_after(q, 1, (s[:1], d[:1]))
    with pytest.raises(ValueError, match=r"one cursor per query \(2\)"):
        g.search_after(q, 1, (s[:, None], d[:, None]))
    with pytest.raises(ValueError, match=r">= AFTER_NONE \(-2\)"):
        g.search_after(q, 1, (s, np.array([0, -3], np.int32)))
    with pytest.raises(ValueError, match="must not be NaN"):
        g.search_after(q, 1, (np.array([0, np.nan], np.float32), d))


def test_gpu_index_after_device_rejects_shapes_before_c():
    import torch
    g = _bare_index(70)
    q = torch.zeros((2, 3), dtype=torch.int32)
    w = torch.ones((2, 3), dtype=torch.float32)
    m = torch.zeros((2, 3), dtype=torch.int32)
    qm = torch.zeros(2, dtype=torch.int32)
    a_s = torch.zeros(2, dtype=torch.float32)
    a_d = torch.zeros(2, dtype=torch.int32)
    d = torch.zeros((2, 4), dtype=torch.int32)
    s = torch.zeros((2, 4), dtype=torch.float32)
    with pytest.raises(ValueError, match="2-D"):
        g.search_after_device(q[0], 4, (a_s, a_d), w[0], m, qm, d, s)
    with pytest.raises(ValueError, match="d_weights must be a float32"):
        g.search_after_device(q, 4, (a_s, a_d), w[:, :2], m, qm, d, s)
    with pytest.raises(ValueError, match=r"packed \[M, 3\]"):
        g.search_after_device(q, 4, (a_s, a_d), w, m[:, :2], qm, d, s)
    with pytest.raises(ValueError, match=r"one mask id per query \(2\)"):
        g.search_after_device(q, 4, (a_s, a_d), w, m, torch.zeros(3, dtype=torch.int32), d, s)
    with pytest.raises(ValueError, match="None or a pair"):
        g.search_after_device(q, 4, a_s, None, None, None, d, s)
    with pytest.raises(ValueError, match="both halves"):
        g.search_after_device(q, 4, (a_s, None), None, None, None, d, s)
    with pytest.raises(ValueError, match="both halves"):
        g.search_after_device(q, 4, (None, a_d), None, None, None, d, s)
    with pytest.raises(ValueError, match=r"float32 \[2\], int32 \[2\]"):
        g.search_after_device(q, 4, (a_s[:1], a_d), None, None, None, d, s)
    with pytest.raises(ValueError, match=r"float32 \[2\], int32 \[2\]"):
        g.search_after_device(q, 4, (a_d, a_s), None, None, None, d, s)
    with pytest.raises(ValueError, match=r"float32 \[2\], int32 \[2\]"):
        g.search_after_device(q, 4, (a_s.to(torch.float64), a_d), None, None, None, d, s)
    with pytest.raises(ValueError, match="2 x 4 results"):
        g.search_after_device(q, 4, (a_s, a_d), None, None, None, d[:, :3], s)


def test_bm25v_search_after_validation_before_gpu():
    import bm25_native
    m = bm25_native.BM25v()
    docs, scores = m.search_after([], 3)
    assert docs.shape == (0, 0) and scores.shape == (0, 0)
    with pytest.raises(ValueError, match="list of list"):
        m.search_after(np.array([1, 2], np.int32), 1)
    with pytest.raises(ValueError, match="list of list"):
        m.search_after(np.array([[1, 2]], np.int64), 1)
    q = np.array([[0, -1]], np.int32)
    s = np.zeros(1, np.float32)
    d = np.zeros(1, np.int32)
    with pytest.raises(ValueError, match="weights must be .* shape"):
        m.search_after(q, 1, weights=np.ones((1, 3), np.float32))
    with pytest.raises(ValueError, match="allow must be"):
        m.search_after(q, 1, allow=np.ones((2, 4), bool))
    with pytest.raises(ValueError, match="None or a pair"):
        m.search_after(q, 1, after=(s, None))
    with pytest.raises(ValueError, match="None or a pair"):
        m.search_after(q, 1, after=s)
    with pytest.raises(ValueError, match=r"one cursor per query \(1\)"):
        m.search_after(q, 1, after=(np.zeros(2, np.float32), np.zeros(2, np.int32)))
    with pytest.raises(ValueError, match="negative dimensions"):
        m.search_after(q, -1, after=(s, d))
    with pytest.raises(ValueError, match=r"maximum token ID in the query \(5\)"):
        m.search_after(np.array([[5, -1]], np.int32), 1)
