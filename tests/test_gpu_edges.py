"""GPU parity at the size boundaries of the entry points beside the top-k
search: bm25_scores_dense, the float64 path (bm25_scores_dense_f64,
bm25_topn_f64), bm25_build_scores, the large merge and bm25_max_token_device
— and of the hand-written device sort and scan under them (bm25mi_sort.hip).

Every comparison is bit-exact against a plain CPU reference (the C oracle,
oracle.scores_f64 / topn_f64 — pinned to numpy itself in tests/test_oracle.py
— oracle.build_scores_numpy, a numpy lexsort); the one exception is the
suite's own: values built with the device-computed idf stay within 1 f32 ulp
of the numpy restatement.  The constants the shapes sit next to:

  2048   documents per tile (kDefaultTileShift = 11)
  4096   pairs per radix tile (kRsTile = 256 threads x 16 rounds)
  256    radix tiles per chunk of rs_scan_kernel (kRsT)
  1024   counts per chunk of exclusive_scan_u64 and of scan_bsum_kernel
         (kScanChunk)
  8, 128 numpy's pairwise sum: in order below 8 terms, 8 partial sums up to
         128, halves above
  256    rows per value pass of radix_sort_rows_desc (8 bits per pass)
  262144 threads of max_token_kernel's grid (1024 blocks x 256)"""
import ctypes

import numpy as np
import pytest

from oracle import oracle
from test_gpu_parity import _exact, _idx, _rand_index

pytestmark = pytest.mark.gpu

TILE = 2048       # documents per tile
NEG_ZERO32 = 0x80000000


def _columns(ip, ix, dt):
    return [(ix[ip[t]:ip[t + 1]], dt[ip[t]:ip[t + 1]]) for t in range(len(ip) - 1)]


def _csc(cols, dtype):
    """CSC (indptr int64, indices int32, data) of per-term (docs, values)."""
    ip = np.zeros(len(cols) + 1, np.int64)
    np.cumsum([len(d) for d, _ in cols], out=ip[1:])
    ix = np.concatenate([np.asarray(d, np.int32) for d, _ in cols]) if cols else np.zeros(0, np.int32)
    dt = np.concatenate([np.asarray(v, dtype) for _, v in cols]) if cols else np.zeros(0, dtype)
    return ip, ix.astype(np.int32), dt.astype(dtype)


def _quarter(rng, n, dtype):
    """Signed quarter steps in [-2, 3] (0.0 and -0.0 among them): sums tie
    and cancel exactly."""
    return (np.round(rng.uniform(-2.0, 3.0, n) * 4) / 4).astype(dtype)


EMPTY, FULL = 0, 1  # the terms _edge_index replaces


def _edge_index(rng, N, V, dfmax):
    """_rand_index(signed, coarse) with term EMPTY holding no posting and
    term FULL holding every document."""
    ip, ix, dt = _rand_index(rng, N, V, dfmax, signed=True, coarse=True)
    cols = _columns(ip, ix, dt)
    cols[EMPTY] = (np.zeros(0, np.int32), np.zeros(0, np.float32))
    cols[FULL] = (np.arange(N, dtype=np.int32), _quarter(rng, N, np.float32))
    return _csc(cols, np.float32)


def _edge_queries(rng, V, T):
    """Queries of T terms: random with padding, one term repeated, rows with
    the empty term and the term of every document, all padding."""
    if T == 0:
        return np.zeros((1, 0), np.int32)
    q = rng.integers(-1, V, size=(6, T)).astype(np.int32)
    q[0, :] = 7                      # one term T times
    q[1, :] = FULL                   # every document, T times
    q[2, :] = EMPTY                  # no posting at all
    q[3, T // 2:] = -1               # a padded tail
    q[3, 0] = FULL
    q[4, 0] = EMPTY
    q[4, -1] = FULL
    q[5, ::2] = -1                   # padding between terms
    return q


# ------------------------------------------------------- bm25_scores_dense
@pytest.mark.parametrize("n_docs", [1, 2047, 2048, 2049, 70_001])
@pytest.mark.parametrize("segments", ["dense", "sparse"])
def test_scores_dense_tile_edges(gpu, segments, n_docs):
    """scores_dense_kernel around the 2048-doc tile: one document, one short
    of a tile, exactly one tile (float4 stores only), one document into the
    second tile and 35 tiles with a partial last one (base + D > n_docs: the
    scalar stores), on both segment tables.  Signed quarter-step values with
    explicit -0.0 and exact cancellations; queries of 0, 1, 9, 65 and 200
    terms with padding, a repeated term, a term without postings and a term
    of every document — every score bit is the C oracle's, and none is -0.0
    (the accumulator starts at +0.0).  A doc-shard handle (doc_offset != 0)
    gives the same vector: it is indexed by local id."""
    rng = np.random.default_rng(n_docs)
    V = 300
    ip, ix, dt = _edge_index(rng, n_docs, V, 5000)
    assert (dt.view(np.uint32) == NEG_ZERO32).any() or n_docs == 1
    index = _idx(ip, ix, dt, n_docs, segments=segments)
    assert index.info()["sparse"] == (segments == "sparse")
    assert index.info()["n_tiles"] == (n_docs + TILE - 1) // TILE
    shard = _idx(ip, ix, dt, n_docs, doc_offset=5000, segments=segments)
    for T in (0, 1, 9, 65, 200):
        for row in _edge_queries(rng, V, T):
            want = oracle.scores_dense_c(n_docs, ip, ix, dt, row)
            for h in (index, shard):
                got = h.scores_dense(row)
                assert got.dtype == np.float32 and got.shape == (n_docs,)
                bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
                assert bad.size == 0, (T, row[:8], bad[:5], got[bad[:5]], want[bad[:5]])
                assert not (got.view(np.uint32) == NEG_ZERO32).any()
    index.close()
    shard.close()


def test_scores_dense_null_query(gpu):
    """bm25_scores_dense with a NULL query: EINVAL "NULL query" when T > 0
    (the host loop over query[i] must not run), accepted when T = 0."""
    from bm25mi._capi import BM25_EINVAL, BM25_OK, lib
    ip = np.array([0, 2, 3], np.int64)
    index = _idx(ip, np.array([0, 2, 1], np.int32), np.array([1.0, 2.0, 4.0], np.float32), 3)
    out = np.full(3, 7.0, np.float32)
    po = out.ctypes.data_as(ctypes.c_void_p)
    assert lib.bm25_scores_dense(index._h, None, 3, po) == BM25_EINVAL
    assert b"NULL query" in lib.bm25_last_error()
    assert out.tolist() == [7.0, 7.0, 7.0]
    assert lib.bm25_scores_dense(index._h, None, 0, po) == BM25_OK
    assert out.tolist() == [0.0, 0.0, 0.0]
    index.close()


# ------------------------------------------------ -0.0 values in the search
@pytest.mark.parametrize("signed", [True, False])
@pytest.mark.parametrize("segments", ["dense", "sparse"])
def test_search_negative_zero_values(gpu, segments, signed):
    """The top-k search on an index whose terms 0..9 hold only -0.0 values
    (the others signed quarter steps, or — signed = False — positive ones,
    where the index still counts as non-negative: -0.0 == 0): a document
    touched only by -0.0 scores +0.0 and ties with the untouched documents by
    id.  Queries of 1, 8, 17 and 65 terms (8, 32 term lanes of the flat
    kernel's cross-lane sums, and the wave kernel above 64), k = 1 and 50,
    both segment tables, bit-exact vs the C oracle."""
    rng = np.random.default_rng(5 + signed)
    N, V, Z = 40_000, 300, 10
    ip, ix, dt = _rand_index(rng, N, V, 8000, signed=signed, coarse=True)
    dt[:ip[Z]] = -0.0
    assert (dt[:ip[Z]].view(np.uint32) == NEG_ZERO32).all() and ip[Z] > 0
    index = _idx(ip, ix, dt, N, segments=segments)
    for T in (1, 8, 17, 65):
        q = rng.integers(-1, V, size=(12, T)).astype(np.int32)
        q[0, :] = 3                                    # one -0.0 term, T times
        q[1, :] = rng.integers(0, Z, T)                # -0.0 terms only
        q[2, :] = -1                                   # all padding: the same result
        q[3, :] = rng.integers(0, Z, T)
        q[3, -1] = 40                                  # -0.0 terms, then one real term
        q[4, :] = rng.integers(Z, V, T)
        q[4, 0] = 5                                    # a -0.0 term first
        for k in (1, 50):
            got = index.search(q, k)
            _exact(got, oracle.search_c(N, ip, ix, dt, q, k))
            assert not (got[1].view(np.uint32) == NEG_ZERO32).any()
            for r in (0, 1, 2):  # all scores +0.0: the smallest ids
                assert got[0][r].tolist() == list(range(k)) and not got[1][r].any()
    index.close()


# ------------------------------------------------------- the float64 path
def _f64_index(cols, n_docs, segments=None):
    """A GpuIndex of float32(data64) with the float64 values set beside it."""
    ip, ix, d64 = _csc(cols, np.float64)
    index = _idx(ip, ix, d64.astype(np.float32), n_docs, segments=segments)
    index.set_values_f64(d64)
    return index, ip, ix, d64


def _exact64(got, want):
    assert got.dtype == np.float64 and got.shape == want.shape
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    assert bad.size == 0, (bad[:5], got[bad[:5]], want[bad[:5]])


def _check_topn(index, scores, q, n):
    d, s = index.topn_f64(q, n)
    rd, rs = oracle.topn_f64(scores, n)
    assert d.dtype == np.int32 and np.array_equal(d, rd), (n, d[:8], rd[:8])
    _exact64(s, rs)


FIRST, MIDDLE, LAST = 2, 3, 4  # terms of one tile only (_f64_cols)


def _f64_cols(rng, N, V, values):
    """V terms over N documents: EMPTY, FULL, a term present only in the
    first tile, only in a middle tile, only in the last tile, the rest
    random.  values: "quarter" = signed quarter steps (ties), "mixed" =
    signed values of magnitudes 1e-8, 1, 1e8 that float32 does not hold (the
    order of the adds shows in the sum)."""
    def vals(n):
        if values == "quarter":
            return _quarter(rng, n, np.float64)
        return rng.uniform(-3.0, 3.0, n) * rng.choice([1e-8, 1.0, 1e8], n)

    ntiles = (N + TILE - 1) // TILE
    cols = []
    for t in range(V):
        if t == EMPTY:
            docs = np.zeros(0, np.int64)
        elif t == FULL:
            docs = np.arange(N)
        else:
            tile = {FIRST: 0, MIDDLE: ntiles // 2, LAST: ntiles - 1}.get(t)
            lo, hi = (0, N) if tile is None else (tile * TILE, min(N, (tile + 1) * TILE))
            df = int(rng.integers(1, min(hi - lo, 3000) + 1))
            docs = lo + np.sort(rng.choice(hi - lo, df, replace=False))
        cols.append((docs.astype(np.int32), vals(len(docs))))
    return cols


@pytest.mark.parametrize("values", ["quarter", "mixed"])
@pytest.mark.parametrize("n_docs", [2, 3, 9, 2049, 70_001])
@pytest.mark.parametrize("segments", ["dense", "sparse"])
def test_f64_scores_and_topn_multi_tile(gpu, segments, n_docs, values):
    """dense64_kernel on an arbitrary CSC through GpuIndex, both segment
    tables (the sparse branch is a binary search over the term's tile list,
    which bm25.BM25's default index never takes): 2, 3 and 9 documents (the
    smallest corpora numpy does not sum pairwise), 2049 (one document past
    the 2048-doc tile) and 70 001 (35 tiles, a partial last one), with terms
    present only in the first, a middle or the last tile, an empty term and
    a term of every document.  Queries of 0, 1, 8 and 40 terms: scores
    bit-exact vs oracle.scores_f64, bm25_topn_f64 at n = 1, n_docs // 2 and
    n_docs exact in documents and scores."""
    rng = np.random.default_rng(n_docs + (values == "mixed"))
    V = 60
    index, ip, ix, d64 = _f64_index(_f64_cols(rng, n_docs, V, values), n_docs, segments)
    assert index.info()["sparse"] == (segments == "sparse")
    queries = [np.zeros(0, np.int32)]
    queries += [np.array([t], np.int32) for t in (EMPTY, FULL, FIRST, MIDDLE, LAST, 17)]
    q8 = rng.integers(-1, V, size=(3, 8)).astype(np.int32)
    q8[0, :5] = [FIRST, LAST, MIDDLE, EMPTY, FULL]
    q8[1, :] = [LAST, -1, LAST, FIRST, -1, FIRST, MIDDLE, MIDDLE]
    q40 = rng.integers(-1, V, size=(3, 40)).astype(np.int32)
    q40[0, ::3] = FULL
    q40[1, 20:] = -1
    queries += list(q8) + list(q40)
    for q in queries:
        ids = [int(t) for t in q if t >= 0]
        want = oracle.scores_f64(n_docs, ip, ix, d64, ids)
        _exact64(index.scores_dense_f64(q), want)
        for n in sorted({1, n_docs // 2, n_docs}):
            _check_topn(index, want, q, n)
    index.close()


def test_f64_one_document_pairwise(gpu):
    """dense64_one_doc_kernel (numpy's pairwise sum of the one gathered row,
    restated with an explicit stack) on a one-document corpus of 40 terms:
    T = 0, 1, 7 (in order: fewer than 8 terms), 8, 9, 127, 128 (8 partial
    sums per block of <= 128), 129, 300, 1000 (the recursion into halves cut
    on a multiple of 8) — with duplicates, padding and terms without a
    posting, values of mixed sign and magnitude.  Compared with numpy's own
    np.sum over the gathered row, bit for bit; top-1 is the document."""
    rng = np.random.default_rng(41)
    V = 40
    v = rng.uniform(-3.0, 3.0, V) * rng.choice([1e-8, 1.0, 1e8], V)
    v[[4, 11, 30]] = 0.0  # no posting
    cols = [((np.zeros(1, np.int32), v[t:t + 1]) if v[t] != 0.0 else
             (np.zeros(0, np.int32), np.zeros(0))) for t in range(V)]
    index, ip, ix, d64 = _f64_index(cols, 1)
    for T in (0, 1, 7, 8, 9, 127, 128, 129, 300, 1000):
        for pad in (False, True):
            q = rng.integers(0, V, T).astype(np.int32)
            if T >= 7:
                q[T // 2] = q[0]           # a duplicate
                q[T // 3] = 11             # a term without a posting
            if pad and T:
                q[rng.random(T) < 0.2] = -1
                q[-1] = -1
            ids = q[q >= 0]
            want = np.sum(v[None, :][:, ids], axis=1)
            got = index.scores_dense_f64(q)
            _exact64(got, want)
            _exact64(got, oracle.scores_f64(1, ip, ix, d64, ids))
            _check_topn(index, want, q, 1)
    index.close()


@pytest.mark.parametrize("n_docs", [4095, 4096, 4097, 1_100_000])
def test_topn_f64_sort_boundaries(gpu, n_docs):
    """bm25_topn_f64's 64-bit descending stable radix sort at the radix tile
    of 4096 pairs (4095, 4096, 4097: a short tile, a full one, one pair into
    a second) and at 1 100 000 documents = 269 tiles, where rs_scan_kernel's
    scan of a digit's per-tile counts takes a second chunk of 256 tiles.
    Signed quarter-step values over 50 terms: negative keys, and tie groups
    of most of the corpus that the stable sort must leave in document
    order.  n = n_docs and n = 10."""
    rng = np.random.default_rng(n_docs)
    V = 50
    df = 6000 if n_docs > 100_000 else 400
    cols = []
    for t in range(V):
        docs = np.unique(rng.integers(0, n_docs, df)).astype(np.int32)
        cols.append((docs, _quarter(rng, len(docs), np.float64)))
    index, ip, ix, d64 = _f64_index(cols, n_docs)
    for q in (np.array([3, 9, 9, -1, 27, 41, 0, 12], np.int32), np.zeros(0, np.int32)):
        want = oracle.scores_f64(n_docs, ip, ix, d64, [int(t) for t in q if t >= 0])
        assert q.size == 0 or ((want < 0).any() and (want > 0).any())
        _exact64(index.scores_dense_f64(q), want)
        for n in (n_docs, 10):
            _check_topn(index, want, q, n)
    index.close()


# ------------------------------------------------------- bm25_build_scores
def _triples(rng, n_docs, n_terms, n, must=()):
    """About n distinct (doc, term) cells, shuffled, those of ``must``
    (pairs) among them; tf in 1..5."""
    d = np.concatenate([rng.integers(0, n_docs, n), [m[0] for m in must]]).astype(np.int64)
    t = np.concatenate([rng.integers(0, n_terms, n), [m[1] for m in must]]).astype(np.int64)
    cells = rng.permutation(np.unique(t * n_docs + d))
    docs, terms = (cells % n_docs).astype(np.int32), (cells // n_docs).astype(np.int32)
    return docs, terms, rng.integers(1, 6, len(cells)).astype(np.float32)


def _doc_len(rng, docs, tfs, n_docs):
    return (np.bincount(docs, weights=tfs, minlength=n_docs) +
            rng.integers(0, 4, n_docs)).astype(np.int32)


def _ulp32(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def _check_build(docs, terms, tfs, dl, n_terms, device_idf=True, k1=1.2, b=0.7):
    """bm25_build_scores vs oracle.build_scores_numpy, both methods: with the
    host idf indptr, indices and every f32 and f64 data bit; with the device
    idf indptr and indices exact and the f32 data within 1 ulp."""
    from bm25mi.scoring import build_scores
    dl = np.asarray(dl, np.int32)
    avgdl = float(np.mean(dl.tolist()))
    idf = oracle.idf_numpy(np.bincount(terms, minlength=n_terms), len(dl))
    csum = np.zeros(n_terms + 1, np.int64)
    np.cumsum(np.bincount(terms, minlength=n_terms), out=csum[1:])
    for method in ("lucene", "bm25py"):
        ref = oracle.build_scores_numpy(docs, terms, tfs, dl, n_terms, k1, b, method, avgdl,
                                        idf=idf)
        got = build_scores(docs, terms, tfs, dl, n_terms, k1=k1, b=b, method=method, avgdl=avgdl,
                           idf=idf, want_f64=True)
        assert np.array_equal(got[0], csum) and np.array_equal(ref[0], csum), method
        assert np.array_equal(got[1], ref[1]), method
        assert np.array_equal(got[2].view(np.uint32), ref[2].view(np.uint32)), method
        assert np.array_equal(got[3].view(np.uint64), ref[3].view(np.uint64)), method
        if device_idf:
            dev = build_scores(docs, terms, tfs, dl, n_terms, k1=k1, b=b, method=method,
                               avgdl=avgdl)
            assert np.array_equal(dev[0], csum) and np.array_equal(dev[1], ref[1]), method
            assert dev[2].size == 0 or _ulp32(dev[2], ref[2]).max() <= 1, method


@pytest.mark.parametrize("n", [1, 2, 4095, 4096, 4097, 8193])
def test_build_scores_triple_counts(gpu, n):
    """The build's key sort next to the radix tile of 4096 pairs: n = 1 (the
    early return of radix_sort_pairs), 2, 4095, 4096, 4097 (one pair into a
    second tile) and 8193 (one into a third), the triples given shuffled,
    already in CSC order and in reverse order (the payload carries each
    triple's tf to its sorted place)."""
    rng = np.random.default_rng(n)
    n_docs, V = 700, 90
    cells = rng.permutation(n_docs * V)[:n]
    docs, terms = (cells % n_docs).astype(np.int32), (cells // n_docs).astype(np.int32)
    tfs = rng.integers(1, 6, n).astype(np.float32)
    dl = _doc_len(rng, docs, tfs, n_docs)
    order = np.lexsort((docs, terms))
    for name, o in (("shuffled", np.arange(n)), ("sorted", order), ("reverse", order[::-1])):
        _check_build(docs[o], terms[o], tfs[o], dl, V, device_idf=name == "shuffled")


@pytest.mark.parametrize("n_terms", [1, 2, 255, 256, 257, 65_536])
def test_build_scores_vocabulary_end_bit(gpu, n_terms):
    """The sort's end_bit (32 + the bits of n_terms) at vocabularies of 1, 2,
    255, 256, 257 and 65 536 terms — a power of two starts a new key bit,
    and past 256 and 65 536 a new 8-bit pass — with triples in term 0 and in
    term n_terms - 1."""
    rng = np.random.default_rng(n_terms)
    n_docs = 500
    must = [(d, 0) for d in rng.choice(n_docs, 40, replace=False)]
    must += [(d, n_terms - 1) for d in rng.choice(n_docs, 40, replace=False)]
    docs, terms, tfs = _triples(rng, n_docs, n_terms, 3000, must)
    assert terms.min() == 0 and terms.max() == n_terms - 1
    _check_build(docs, terms, tfs, _doc_len(rng, docs, tfs, n_docs), n_terms)


@pytest.mark.parametrize("n_terms", [1023, 1024, 1025, 1_048_575, 1_048_576, 1_100_000])
def test_build_scores_scan_boundaries(gpu, n_terms):
    """exclusive_scan_u64 over the n_terms + 1 document frequencies in chunks
    of 1024: one chunk (1023), one count into a second (1024, 1025), exactly
    1024 chunks (1 048 575), and 1025 and 1075 chunks (1 048 576,
    1 100 000), where scan_bsum_kernel's scan of the chunk sums takes its
    second 1024-element iteration and carries the first's total.  About
    50 000 triples with the last term and the terms around 1 048 576
    non-empty; indptr is the cumulative sum of the frequencies."""
    rng = np.random.default_rng(n_terms)
    n_docs = 2000
    edge = [t for t in (0, 1022, 1023, 1024, 1_048_574, 1_048_575, 1_048_576, 1_048_577,
                        n_terms - 2, n_terms - 1) if 0 <= t < n_terms]
    must = [(int(d), t) for t in edge for d in rng.choice(n_docs, 3, replace=False)]
    docs, terms, tfs = _triples(rng, n_docs, n_terms, 50_000, must)
    assert terms.max() == n_terms - 1
    if n_terms > 1_048_576:
        assert (terms < 1_048_576).any() and (terms > 1_048_576).any()
    _check_build(docs, terms, tfs, _doc_len(rng, docs, tfs, n_docs), n_terms)


@pytest.mark.parametrize("case", ["one_term", "one_doc", "df_all"])
def test_build_scores_skew(gpu, case):
    """Skewed triples: every triple in one term (each radix digit of the term
    bits has one value: the whole wave matches in rs_match, one histogram
    bin takes every pair), every triple in one document (the same for the
    document bits), and a term whose df equals n_docs (the smallest idf)
    among random ones.  5000 triples: a second radix tile of 4096."""
    rng = np.random.default_rng(len(case))
    if case == "one_term":
        n_docs, V = 6000, 7
        docs = rng.permutation(n_docs)[:5000].astype(np.int32)
        terms = np.full(5000, 3, np.int32)
    elif case == "one_doc":
        n_docs, V = 9, 6000
        docs = np.full(5000, 5, np.int32)
        terms = rng.permutation(V)[:5000].astype(np.int32)
    else:
        n_docs, V = 3000, 40
        docs, terms, _ = _triples(rng, n_docs, V, 4000, [(d, 11) for d in range(n_docs)])
        assert np.bincount(terms, minlength=V)[11] == n_docs
    tfs = rng.integers(1, 6, len(docs)).astype(np.float32)
    _check_build(docs, terms, tfs, _doc_len(rng, docs, tfs, n_docs), V)


@pytest.mark.parametrize("case", ["all_zero", "mixed_zero", "tf_range"])
def test_build_scores_lengths_and_tf(gpu, case):
    """Document lengths of 0 everywhere (avgdl = 0: the norm is k1 (1 - b)),
    zero and non-zero lengths mixed, and fractional term frequencies with
    tf = 1e6 among them."""
    rng = np.random.default_rng(len(case) + 100)
    n_docs, V = 800, 120
    docs, terms, tfs = _triples(rng, n_docs, V, 5000)
    dl = _doc_len(rng, docs, tfs, n_docs)
    if case == "all_zero":
        dl[:] = 0
    elif case == "mixed_zero":
        dl[rng.random(n_docs) < 0.5] = 0
        assert (dl == 0).any() and (dl > 0).any()
    else:
        tfs = rng.uniform(0.01, 9.0, len(docs)).astype(np.float32)
        tfs[::17] = 1e6
    _check_build(docs, terms, tfs, dl, V)


# --------------------------------------------- the large merge, max token
def test_large_merge_more_than_256_rows(gpu):
    """bm25_merge_topk_device at W = 2, Q = 300, k = 4097: 300 rows of 8194
    keys in one radix_sort_rows_desc — more than 256 rows, so the row number
    takes a second 8-bit value pass after the 64 key bits.  Lists with tied
    scores and padded tails (doc -1, score bits ~0); the reference is a numpy
    lexsort by (score desc, doc asc)."""
    import torch
    from bm25mi.index import merge_topk_device
    rng = np.random.default_rng(19)
    W, Q, k = 2, 300, 4097
    docs = rng.permutation(W * Q * k * 2)[:W * Q * k].reshape(W, Q, k).astype(np.int32)
    scores = (np.round(rng.uniform(0, 3, (W, Q, k)) * 8) / 8).astype(np.float32)
    for w, q, n in ((1, 2, 100), (0, 255, 4000), (1, 256, 0), (0, 299, 1), (1, 299, 2000)):
        docs[w, q, n:] = -1
        scores.view(np.uint32)[w, q, n:] = 0xFFFFFFFF
    md = torch.empty((Q, k), dtype=torch.int32, device="cuda")
    ms = torch.empty((Q, k), dtype=torch.float32, device="cuda")
    merge_topk_device(0, torch.from_numpy(docs).cuda(), torch.from_numpy(scores).cuda(), W, Q, k,
                      md, ms, torch.cuda.current_stream())
    torch.cuda.synchronize()
    md, ms = md.cpu().numpy(), ms.cpu().numpy()
    rd = np.full((Q, k), -1, np.int32)
    rs = np.full((Q, k), np.uint32(0xFFFFFFFF).view(np.float32), np.float32)
    for qi in range(Q):
        d, s = docs[:, qi].ravel(), scores[:, qi].ravel()
        ok = d >= 0
        order = np.lexsort((d[ok], -s[ok].astype(np.float64)))[:k]
        rd[qi, :len(order)], rs[qi, :len(order)] = d[ok][order], s[ok][order]
    assert (rd[299] == -1).sum() == k - 2001  # the padded tail reaches the output
    _exact((md, ms), (rd, rs))


def test_max_token_device_sizes(gpu):
    """bm25_max_token_device on batches of 1 and 63 ids (shorter than one
    wave), 257 (one past a workgroup) and 300 000 (more than the grid's
    262 144 threads: the grid-stride loop takes a second step), the maximum
    in the first, the last and a middle element; a maximum of 2**31 - 1; an
    all-negative batch gives 0 (queries.max(initial=0))."""
    import torch
    index = _idx(np.array([0, 1], np.int32), np.array([0], np.int32),
                 np.array([1.0], np.float32), 1)
    rng = np.random.default_rng(2)
    for n in (1, 63, 257, 300_000):
        base = rng.integers(-1, 1000, n).astype(np.int32)
        for pos in sorted({0, n // 2, n - 1}):
            for top in (5000, 2**31 - 1):
                q = base.copy()
                q[pos] = top
                assert index.max_token_device(torch.from_numpy(q).cuda().view(1, n)) == top, (n, pos)
        shape = (n // 4, 4) if n % 4 == 0 else (1, n)
        neg = torch.from_numpy(rng.integers(-2**31, 0, n).astype(np.int32)).cuda().view(shape)
        assert index.max_token_device(neg) == 0, n
        assert index.max_token_device(torch.from_numpy(base).cuda().view(shape)) == \
            int(base.max(initial=0)), n
    index.close()


# ------------------------------------------- the host calls' shared staging
def test_host_calls_reject_token_ids_and_stay_usable(gpu):
    """Every synchronous host-pointer call goes through one staging helper
    (csrc/bm25mi_host.h).  On the 5-document, 3-term index of
    tests/asan/host_check.cpp: a token id of 3 (= n_terms) gives EINVAL with
    the reference's message from each call that takes token ids, a term id or
    a CSC the device rejects gives EINVAL from bm25_build_scores and
    bm25_index_create, and after each failure the same call with valid
    arguments is bit-exact against the CPU reference — the handle is left
    usable.  Then all 16 search options round-trip through
    bm25_index_set_option / bm25_index_get_option, and the search still
    matches."""
    from bm25mi.scoring import build_scores
    N, V = 5, 3
    ip = np.array([0, 2, 2, 5], np.int64)
    ix = np.array([0, 3, 1, 2, 4], np.int32)
    dt = np.array([1.0, 2.0, 0.5, 0.25, 3.0], np.float32)
    d64 = dt.astype(np.float64) + 1e-9
    index = _idx(ip, ix, dt, N)
    index.set_values_f64(d64)
    msg = (r"The maximum token ID in the query \(3\) is higher than the number of tokens in "
           r"the index\.")
    good = np.array([[0, 2], [2, -1], [1, 1]], np.int32)
    bad = good.copy()
    bad[1, 1] = V
    dense = np.stack([oracle.scores_dense_c(N, ip, ix, dt, r) for r in good])
    holds = np.zeros((V, N), bool)           # holds[t, d]: document d has term t
    for t in range(V):
        holds[t, ix[ip[t]:ip[t + 1]]] = True

    def pack(allow):                          # bool [M, N] -> uint32 [M, 1]
        return (allow.astype(np.uint32) << np.arange(N, dtype=np.uint32)).sum(1, keepdims=True) \
            .astype(np.uint32)

    def filtered_ref(allow, k):               # top-k among the allowed, padded
        rd = np.full((len(good), k), -1, np.int32)
        rs = np.full((len(good), k), np.uint32(0xFFFFFFFF).view(np.float32), np.float32)
        for i, row in enumerate(dense):
            docs = np.nonzero(allow[i])[0]
            order = docs[np.lexsort((docs, -row[docs].astype(np.float64)))][:k]
            rd[i, :len(order)], rs[i, :len(order)] = order, row[order]
        return rd, rs

    k = 3
    allow = np.array([[1, 1, 0, 1, 1], [0, 0, 1, 0, 1], [1, 0, 0, 0, 0]], bool)
    must, must_bad = [[0], [2], []], [[0], [V], []]
    not_, any_ = [[], [0], [2]], [[2, 0], [], [0, 1]]
    built = np.stack([(holds[0] | holds[2]) & holds[0],
                      holds[2] & ~holds[0],
                      (holds[0] | holds[1]) & ~holds[2]])
    assert built.any(1).all() and not built.all(1).any()
    cand = np.array([[0, 4, -1], [3, 3, 1], [2, 0, 4]], np.int32)
    cand_ref = np.where(cand >= 0, np.take_along_axis(dense, np.maximum(cand, 0), 1), 0) \
        .astype(np.float32)

    def same64(got, want):
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (got, want)

    f64_ref = oracle.scores_f64(N, ip, ix, d64, [0, 2])
    calls = [  # (the call with token ids `q` / clause `m`, the check of its valid result)
        (lambda q, m: index.search(q, k),
         lambda r: _exact(r, oracle.search_c(N, ip, ix, dt, good, k))),
        (lambda q, m: index.search_filtered(q, k, allow, np.arange(3, dtype=np.int32)),
         lambda r: _exact(r, filtered_ref(allow, k))),
        (lambda q, m: index.term_masks(must=m, any=any_, must_not=not_),
         lambda r: np.testing.assert_array_equal(r, pack(built))),
        (lambda q, m: index.search_boolean(q, k, must=must, any=any_, must_not=not_),
         lambda r: _exact(r, filtered_ref(built, k))),
        (lambda q, m: index.search_boolean(good, k, must=m, any=any_, must_not=not_),
         lambda r: _exact(r, filtered_ref(built, k))),
        (lambda q, m: index.scores_dense(q[1]),
         lambda r: np.testing.assert_array_equal(r.view(np.uint32), dense[1].view(np.uint32))),
        (lambda q, m: index.score_docs(q, cand),
         lambda r: np.testing.assert_array_equal(r.view(np.uint32), cand_ref.view(np.uint32))),
        (lambda q, m: index.scores_dense_f64(q[0] if q is good else q[1]),
         lambda r: same64(r, f64_ref)),
        (lambda q, m: index.topn_f64(q[0] if q is good else q[1], 4),
         lambda r: (np.testing.assert_array_equal(r[0], oracle.topn_f64(f64_ref, 4)[0]),
                    same64(r[1], oracle.topn_f64(f64_ref, 4)[1]))),
    ]
    for i, (call, check) in enumerate(calls):
        with pytest.raises(ValueError, match=msg):
            call(bad, must_bad)
        check(call(good, must))
        _exact(index.search(good, k), oracle.search_c(N, ip, ix, dt, good, k))

    # the two calls without a handle: the device's own checks, mid-call
    docs, terms = np.array([0, 1, 1], np.int32), np.array([0, 0, 2], np.int32)
    tfs, dl = np.array([1.0, 2.0, 1.0], np.float32), np.array([3, 4], np.int32)
    with pytest.raises(ValueError, match="doc or term id out of range"):
        build_scores(docs, np.array([0, 0, V], np.int32), tfs, dl, V)
    ref = oracle.build_scores_numpy(docs, terms, tfs, dl, V, 1.5, 0.75, "lucene", 3.5,
                                    idf=oracle.idf_numpy(np.bincount(terms, minlength=V), 2))
    got = build_scores(docs, terms, tfs, dl, V, k1=1.5, b=0.75, method="lucene", avgdl=3.5,
                       idf=oracle.idf_numpy(np.bincount(terms, minlength=V), 2))
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    assert np.array_equal(got[2].view(np.uint32), ref[2].view(np.uint32))
    with pytest.raises(ValueError, match="indices must be sorted, unique"):
        _idx(ip, np.array([3, 0, 1, 2, 4], np.int32), dt, N)
    for segments in ("dense", "sparse"):
        again = _idx(ip, ix, dt, N, segments=segments)
        _exact(again.search(good, k), oracle.search_c(N, ip, ix, dt, good, k))
        again.close()

    # all 16 options through the C-ABI: default, an accepted value, back
    options = {"flat": (1, 0), "flat_bw": (0, 4), "items_per_wave": (4, 9), "sample_p": (8, 2),
               "list_cap": (0, 4096), "claim_ch": (1, 3), "claim_m": (4, 8), "tile_bound": (1, 0),
               "theta_bound": (1, 0), "grid_pct": (100, 50), "count_skips": (0, 1),
               "large_lists": (1, 0), "rest_split": (0, 1), "bound_pool": (1, 0),
               "filter_tiles": (1, 0), "bool_chunk": (0, 2)}
    assert len(options) == 16
    fresh = _idx(ip, ix, dt, N)
    for name, (default, value) in options.items():
        assert fresh.get_option(name) == default, name
        fresh.set_option(name, value)
        assert fresh.get_option(name) == value, name
    with pytest.raises(ValueError, match="^unknown option 'x'$"):
        fresh.set_option("x", 1)
    with pytest.raises(ValueError, match="^grid_pct must be in 1..100$"):
        fresh.set_option("grid_pct", 0)
    _exact(fresh.search(good, k), oracle.search_c(N, ip, ix, dt, good, k))
    _exact(fresh.search_boolean(good, k, must=must, any=any_, must_not=not_),
           filtered_ref(built, k))
    fresh.close()
    index.close()
