"""GPU tests of bm25_score_docs / bm25_score_docs_device (bm25mi_lookup.hip):
the scores of given (query, document) pairs.

Every comparison is on uint32 views of the scores.  The expected value of
(q, d) is element d of the C oracle's dense row of q
(oracle.scores_dense_c), +0.0 where the doc id is padding; the shapes sit
next to

  2048            documents per tile (the lookup's tile and slot split)
  8, 16, 32, 64   term slots per pair (queries of up to 8, 16, 32, 64 terms;
                  longer ones in groups of 64 with the sum carried)
  1 .. 2048       postings of a (term, tile) segment (the binary search)"""
import numpy as np
import pytest

from oracle import oracle
from test_gpu_edges import EMPTY, FULL, NEG_ZERO32, TILE, _columns, _csc, _edge_index, _edge_queries
from test_gpu_parity import _doc_slice, _idx, _rand_index

pytestmark = pytest.mark.gpu


def _want(n_docs, ip, ix, dt, q, docs, doc_offset=0):
    """oracle.scores_dense_c(q[r])[docs[r] - doc_offset], +0.0 for padding."""
    out = np.zeros(docs.shape, np.float32)
    for r in range(len(q)):
        row = oracle.scores_dense_c(n_docs, ip, ix, dt, q[r])
        ok = docs[r] >= 0
        out[r, ok] = row[docs[r][ok] - doc_offset]
    return out


def _device(index, q, docs, stream=None):
    import torch
    dq = torch.from_numpy(np.ascontiguousarray(q, np.int32)).cuda()
    dd = torch.from_numpy(np.ascontiguousarray(docs, np.int32)).cuda()
    out = torch.full(docs.shape, 7.0, dtype=torch.float32, device="cuda")
    index.score_docs_device(dq, dd, out, stream or torch.cuda.current_stream())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _same_bits(got, want, what=""):
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad[0].size == 0, (what, f"{bad[0].size} mismatches, first at row {bad[0][0]} "
                              f"col {bad[1][0]}: gpu {got[bad][:5]} want {want[bad][:5]}")
    assert not (got.view(np.uint32) == NEG_ZERO32).any(), what


def _check(index, q, docs, want, what=""):
    """The host call and the device call both return ``want`` bit for bit."""
    _same_bits(index.score_docs(q, docs), want, (what, "host"))
    _same_bits(_device(index, q, docs), want, (what, "device"))


# ------------------------------------------------------------- 1. tile edges
@pytest.mark.parametrize("n_docs", [1, 2047, 2048, 2049, 70_001])
@pytest.mark.parametrize("segments", ["dense", "sparse"])
def test_tile_edges(gpu, segments, n_docs):
    """Documents at both ends of a tile — one document, one short of a tile,
    exactly one, one into the second, 35 tiles with a partial last one — on
    both segment tables.  Signed quarter-step values with -0.0 among them, an
    empty term and an every-document term; every document is a candidate
    (70 001: the tile-edge documents, 200 random ones and padding)."""
    rng = np.random.default_rng(n_docs)
    V = 40
    ip, ix, dt = _edge_index(rng, n_docs, V, min(n_docs, 3000))
    q = _edge_queries(rng, V, 8)
    if n_docs <= 2049:
        cand = np.arange(n_docs, dtype=np.int32)
    else:
        assert (dt.view(np.uint32) == NEG_ZERO32).any()
        edge = [0, 2047, 2048, 2049, 4095, 4096, n_docs - 1]
        cand = np.concatenate([edge, rng.integers(0, n_docs, 200), [-1, -1]]).astype(np.int32)
    docs = np.tile(cand, (len(q), 1))
    index = _idx(ip, ix, dt, n_docs, segments=segments)
    assert index.info()["sparse"] == (segments == "sparse")
    assert index.info()["n_tiles"] == (n_docs + TILE - 1) // TILE
    want = _want(n_docs, ip, ix, dt, q, docs)
    assert want[1].any() or n_docs == 1  # the every-document term scores
    _check(index, q, docs, want)
    index.close()


# ------------------------------------------------- 2. term-slot boundaries
ORDER_DOC = 1234       # holds 1e8, 1.0, -1e8 through the terms below
BIG, ONE, NEG = 2, 3, 4


@pytest.fixture(scope="module")
def slot_index(gpu):
    """5 000 documents, 60 terms of signed quarter steps; FULL holds every
    document; BIG, ONE, NEG hold ORDER_DOC alone with 1e8, 1.0, -1e8: in
    query order (1e8 + 1.0) - 1e8 = 0.0, in any other order 1.0."""
    rng = np.random.default_rng(77)
    N, V = 5000, 60
    cols = _columns(*_rand_index(rng, N, V, 2500, signed=True, coarse=True))
    cols[EMPTY] = (np.zeros(0, np.int32), np.zeros(0, np.float32))
    cols[FULL] = (np.arange(N, dtype=np.int32),
                  (np.round(rng.uniform(-2.0, 3.0, N) * 4) / 4).astype(np.float32))
    for t, v in ((BIG, 1e8), (ONE, 1.0), (NEG, -1e8)):
        cols[t] = (np.array([ORDER_DOC], np.int32), np.array([v], np.float32))
    ip, ix, dt = _csc(cols, np.float32)
    index = _idx(ip, ix, dt, N)
    yield index, N, V, ip, ix, dt
    index.close()


@pytest.mark.parametrize("T", [0, 1, 8, 9, 16, 17, 32, 33, 64, 65, 130])
def test_term_slot_boundaries(slot_index, T):
    """Queries of 0 .. 130 terms around the 8, 16, 32 and 64 term slots of a
    pair (and, past 64, the carried partial sum): one term T times, padding
    between terms, the every-document term T times, random rows, and — T >=
    3 — 1e8, 1.0, -1e8 on one document at the first, a middle and the last
    position, which any reordered sum turns from 0.0 into 1.0.  37
    candidates per row: no multiple of a wave's 8, 4, 2 or 1 pairs."""
    index, N, V, ip, ix, dt = slot_index
    rng = np.random.default_rng(T)
    C = 37
    q = rng.integers(-1, V, size=(6, T)).astype(np.int32)
    if T:
        q[0, :] = 7
        q[1, ::2] = -1
        q[2, :] = FULL
    docs = rng.integers(0, N, size=(6, C)).astype(np.int32)
    docs[:, 5] = -1
    docs[:, [0, 17, C - 1]] = ORDER_DOC
    if T >= 3:
        q[4, :] = -1
        q[4, [0, T // 2, T - 1]] = [BIG, ONE, NEG]
        q[5, [0, T // 2, T - 1]] = [BIG, ONE, NEG]
    want = _want(N, ip, ix, dt, q, docs)
    if T >= 3:
        assert (want[4, [0, 17, C - 1]] == 0.0).all()  # (1e8 + 1.0) - 1e8, in this order
    _check(index, q, docs, want, T)


# ---------------------------------------------------- 3. binary search edges
SEG_LENS = [1, 2, 3, 63, 64, 65, 2048]


@pytest.mark.parametrize("segments", ["dense", "sparse"])
def test_binary_search_edges(gpu, segments):
    """Three tiles; term i's segment in the middle tile holds SEG_LENS[i]
    postings (one, two, three, around a wave, the whole tile), chosen so
    that documents are absent below the first, above the last and between
    present ones; even terms also hold the documents just across both tile
    boundaries (2047, 4096) and a few more of the outer tiles, odd terms
    nothing outside the middle tile.  Candidates: each segment's first and
    last document, the absent neighbours, the middle tile's own first and
    last document and the outer tiles' boundary documents — per single-term
    query and for the query of all seven terms."""
    rng = np.random.default_rng(3)
    N = 3 * TILE
    cols, cand = [], {0, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, N - 1}
    for i, n in enumerate(SEG_LENS):
        if n == TILE:
            mid = np.arange(TILE)
        else:
            mid = np.sort(rng.choice(np.arange(5, 2040, 3), n, replace=False))
            cand |= {TILE + int(mid[0]) - 1, TILE + int(mid[-1]) + 1, TILE + int(mid[0]) + 1}
        mid = mid + TILE
        cand |= {int(mid[0]), int(mid[-1])}
        outer = np.zeros(0, np.int64)
        if i % 2 == 0:
            outer = np.array([3, 900, TILE - 1, 2 * TILE, 2 * TILE + 17, N - 1])
        d = np.sort(np.concatenate([mid, outer])).astype(np.int32)
        cols.append((d, rng.uniform(0.5, 3.0, len(d)).astype(np.float32)))  # distinct values
    ip, ix, dt = _csc(cols, np.float32)
    V = len(cols)
    q = np.full((V + 1, V), -1, np.int32)
    q[np.arange(V), 0] = np.arange(V)   # each term alone
    q[V, :] = np.arange(V)[::-1]        # all of them
    docs = np.tile(np.array(sorted(cand), np.int32), (V + 1, 1))
    index = _idx(ip, ix, dt, N, segments=segments)
    assert index.info()["sparse"] == (segments == "sparse") and index.info()["n_tiles"] == 3
    want = _want(N, ip, ix, dt, q, docs)
    for i in range(V):  # present and absent candidates both occur
        assert (want[i] != 0).any() and (want[i] == 0).any() or SEG_LENS[i] == TILE
    _check(index, q, docs, want)
    index.close()


# ------------------------------------------------ 4. padding and validation
def test_padding_and_validation(gpu):
    """An all-padding candidate row is all zero bits.  The host call rejects
    a doc id == n_docs (naming it) and a token id == n_terms (the
    reference's message); the device call scores both +0.0 and the rest of
    the batch stays exact.  Q == 0 and C == 0 give empty arrays."""
    import torch
    rng = np.random.default_rng(9)
    N, V = 3000, 30
    ip, ix, dt = _rand_index(rng, N, V, 1500, signed=True, coarse=True)
    index = _idx(ip, ix, dt, N)
    q = rng.integers(0, V, size=(4, 8)).astype(np.int32)
    docs = rng.integers(0, N, size=(4, 11)).astype(np.int32)
    docs[2, :] = -1
    want = _want(N, ip, ix, dt, q, docs)
    assert not want[2].view(np.uint32).any() and want[[0, 1, 3]].any()
    _check(index, q, docs, want)

    bad_docs = docs.copy()
    bad_docs[1, 4] = N
    with pytest.raises(ValueError, match=rf"doc id {N} "):
        index.score_docs(q, bad_docs)
    ok_docs = bad_docs.copy()
    ok_docs[1, 4] = -1
    _same_bits(_device(index, q, bad_docs), _want(N, ip, ix, dt, q, ok_docs), "doc id == n_docs")

    bad_q = q.copy()
    bad_q[3, 2] = V
    with pytest.raises(ValueError, match=rf"maximum token ID in the query \({V}\) is higher than "
                                         "the number of tokens in the index"):
        index.score_docs(bad_q, docs)
    ok_q = bad_q.copy()
    ok_q[3, 2] = -1
    _same_bits(_device(index, bad_q, docs), _want(N, ip, ix, dt, ok_q, docs), "token id == n_terms")

    for shape_q, shape_d in (((0, 8), (0, 11)), ((4, 8), (4, 0)), ((0, 0), (0, 0))):
        out = index.score_docs(np.zeros(shape_q, np.int32), np.zeros(shape_d, np.int32))
        assert out.shape == shape_d and out.dtype == np.float32
        dev = torch.empty(shape_d, dtype=torch.float32, device="cuda")
        index.score_docs_device(torch.zeros(shape_q, dtype=torch.int32, device="cuda"),
                                torch.zeros(shape_d, dtype=torch.int32, device="cuda"), dev)
    torch.cuda.synchronize()
    index.close()


# --------------------------------------------------- 5. agreement with search
@pytest.fixture(scope="module")
def nonneg_case(gpu):
    """50 000 documents, 300 non-negative terms, 64 queries of 8 terms with
    padding, and the oracle's top-50."""
    rng = np.random.default_rng(50)
    N, V = 50_000, 300
    ip, ix, dt = _rand_index(rng, N, V, 8000)
    assert ip.dtype == np.int64
    q = rng.integers(-1, V, size=(64, 8)).astype(np.int32)
    ref = oracle.search_c(N, ip, ix, dt, q, 50)
    return N, V, ip, ix, dt, q, ref


def test_agrees_with_search(nonneg_case):
    """score_docs(q, search(q, 50).docs) is search(q, 50).scores bit for bit,
    by the host call and by the device call."""
    N, V, ip, ix, dt, q, ref = nonneg_case
    index = _idx(ip, ix, dt, N)
    docs, scores = index.search(q, 50)
    assert np.array_equal(docs, ref[0])
    _same_bits(scores, ref[1], "search")
    _check(index, q, docs, scores)
    index.close()


# ------------------------------------------------------------ 6. shards add up
def test_shards_add_up(nonneg_case):
    """The index split at document 24 576 into two handles (doc_offset 0 and
    24 576), both given the same global candidate ids: each device call
    writes +0.0 for the other shard's documents, and the fp32 sum of the two
    outputs is the single index's output bit for bit.  The host call on the
    second shard takes ids >= 24 576 and rejects id 0."""
    N, V, ip, ix, dt, q, ref = nonneg_case
    cut = 24_576
    rng = np.random.default_rng(6)
    docs = rng.integers(0, N, size=(len(q), 40)).astype(np.int32)
    docs[:, 0], docs[:, 1], docs[:, 2], docs[:, 3] = cut - 1, cut, N - 1, -1
    want = _want(N, ip, ix, dt, q, docs)
    full = _idx(ip, ix, dt, N)
    one = _device(full, q, docs)
    _same_bits(one, want, "single index")
    parts = []
    for lo, hi in ((0, cut), (cut, N)):
        sh = _idx(*_doc_slice(ip, ix, dt, lo, hi), hi - lo, doc_offset=lo)
        got = _device(sh, q, docs)
        outside = (docs < lo) | (docs >= hi)
        assert not got.view(np.uint32)[outside].any()
        parts.append(got)
        if lo:
            mine = np.where(outside, -1, docs).astype(np.int32)
            _same_bits(sh.score_docs(q, mine), np.where(outside, np.float32(0), want), "shard 1 host")
            with pytest.raises(ValueError, match="doc id 0 "):
                sh.score_docs(q[:1], np.array([[cut, 0]], np.int32))
        sh.close()
    _same_bits(parts[0] + parts[1], one, "sum of the shards")
    full.close()


# ------------------------------------- 7. int64 indptr, stream, interleaving
def test_streams_interleaved_with_search(nonneg_case):
    """An index built from an int64 indptr.  Queries and candidates are
    uploaded on a non-default stream and scored there with no host
    synchronisation in between; a search of the same handle is enqueued on a
    second stream, then a second score_docs_device on the first.  After both
    streams synchronise all three results are exact: the lookup takes no
    part in the search workspace or its stream ordering."""
    import torch
    N, V, ip, ix, dt, q, ref = nonneg_case
    index = _idx(ip, ix, dt, N)
    rng = np.random.default_rng(70)
    docs = rng.integers(-1, N, size=(len(q), 100)).astype(np.int32)
    docs2 = np.ascontiguousarray(ref[0][:, ::-1])
    want, want2 = _want(N, ip, ix, dt, q, docs), _want(N, ip, ix, dt, q, docs2)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    hq, hd, hd2 = (torch.from_numpy(a).pin_memory() for a in (q, docs, docs2))
    with torch.cuda.stream(s1):
        dq = hq.to("cuda", non_blocking=True)
        dd = hd.to("cuda", non_blocking=True)
        dd2 = hd2.to("cuda", non_blocking=True)
        out1 = torch.full(docs.shape, 7.0, dtype=torch.float32, device="cuda")
        out2 = torch.full(docs2.shape, 7.0, dtype=torch.float32, device="cuda")
    index.score_docs_device(dq, dd, out1, s1)
    s2.wait_stream(s1)  # (the queries' upload)
    with torch.cuda.stream(s2):
        sd = torch.empty((len(q), 50), dtype=torch.int32, device="cuda")
        ss = torch.empty((len(q), 50), dtype=torch.float32, device="cuda")
    index.search_device(dq, 50, sd, ss, s2)
    index.score_docs_device(dq, dd2, out2, s1)
    s1.synchronize()
    s2.synchronize()
    _same_bits(out1.cpu().numpy(), want, "first lookup")
    _same_bits(out2.cpu().numpy(), want2, "second lookup")
    _same_bits(out2.cpu().numpy()[:, ::-1], ref[1], "the search's own scores")
    assert np.array_equal(sd.cpu().numpy(), ref[0])
    _same_bits(ss.cpu().numpy(), ref[1], "search")
    index.close()
