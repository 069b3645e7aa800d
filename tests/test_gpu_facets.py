"""GPU tests of the facet counts (bm25_mask_facets(_device),
bm25_search_boolean_facets; bm25mi_facets.hip).

The expected counts come from numpy (tests/facets_model.py: a row unpacked to
bool, np.bincount of the in-range groups of its allowed documents); they never
go through the code under test.  Every check runs through the host call and
through the device call (a non-default stream, the mask buffer one word off a
16-byte boundary), into int64 buffers pre-filled with -7 that carry 64 guard
entries.  The shapes sit next to

  32      documents per mask word
  256     documents of a wave's span (8 mask words)
  8192    kFacetBins: LDS bins of a workgroup; G = 8192 is the last LDS shape
          (one row per block), G = 8193 the first global-atomic shape
  64      kFacetMaxRows: R = min(64, 8192 / G) rows share a block (G = 64: 64)
  8192    documents of a chunk on the LDS route with few bins (8 per bin,
          rounded up to a multiple of 1024 — 3 rows of G = 1000: 24 000 ->
          24 576 — at least 8192 ...
  65536   ... and at most 65536: G = 8192)
  16384   documents of a chunk on the global route
  4       documents of a row in a 64-document step up to which they are added
          one by one; from 5 on the wave-aggregated add"""
import ctypes

import numpy as np
import pytest

from facets_model import facets_want, unpack_rows
from test_gpu_parity import _exact, _idx, _rand_index
from test_gpu_term_masks import _has_of, _want

pytestmark = pytest.mark.gpu

FILL = -7
GUARD = 64
BINS, MAXROWS, SPAN = 8192, 64, 256
CHUNK_MIN, CHUNK_MAX, CHUNK_GLOBAL = 8192, 65536, 16384


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None


@pytest.fixture(scope="module")
def make(gpu):
    """index_of(n_docs): a handle over n_docs documents (one term, one
    posting: the facet calls read the caller's masks and groups only)."""
    made = {}

    def index_of(n_docs):
        if n_docs not in made:
            made[n_docs] = _idx(np.array([0, 1], np.int64), np.zeros(1, np.int32),
                                np.ones(1, np.float32), n_docs)
        return made[n_docs]
    yield index_of
    for ix in made.values():
        ix.close()


def _host_raw(index, packed, groups, G):
    """bm25_mask_facets into a pre-filled buffer with guard entries."""
    from bm25mi._capi import check, lib
    M = packed.shape[0]
    buf = np.full(M * G + GUARD, FILL, np.int64)
    check(lib.bm25_mask_facets(index._h, _p(packed), M, _p(groups), G, _p(buf)))
    assert (buf[M * G:] == FILL).all(), "guard entries written"
    return buf[:M * G].reshape(M, G).copy()


def _device_raw(index, packed, groups, G, stream=None):
    """facets_device on a non-default stream: the masks start one word past a
    16-byte boundary, the counts are pre-filled and carry guard entries."""
    import torch
    M, W = packed.shape
    st = stream or torch.cuda.Stream()
    dm = torch.zeros(M * W + 1, dtype=torch.int32, device="cuda")
    dm[1:] = torch.from_numpy(np.ascontiguousarray(packed).view(np.int32).reshape(-1)).cuda()
    assert dm.data_ptr() % 16 == 0
    dg = torch.from_numpy(np.ascontiguousarray(groups, dtype=np.int32)).cuda()
    buf = torch.full((M * G + GUARD,), FILL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()  # (the uploads ran on the current stream)
    index.facets_device(dm[1:].view(M, W), dg, G, buf[:M * G].view(M, G), st)
    st.synchronize()
    got = buf.cpu().numpy()
    assert (got[M * G:] == FILL).all(), "guard entries written"
    return got[:M * G].reshape(M, G).copy()


def _check(index, packed, groups, G, what="", host=True):
    """Host call (unless the groups are out of range, which it rejects) and
    device call both give numpy's counts; returns them."""
    packed = np.ascontiguousarray(packed, dtype=np.uint32)
    groups = np.ascontiguousarray(groups, dtype=np.int32)
    want = facets_want(packed, groups, G)
    calls = [("device", _device_raw)] + ([("host", _host_raw)] if host else [])
    for name, call in calls:
        got = call(index, packed, groups, G)
        bad = np.nonzero(got != want)
        assert bad[0].size == 0, (what, name, f"{bad[0].size} counts differ, first row "
                                  f"{bad[0][0]} group {bad[1][0]}: got {got[bad][0]} "
                                  f"want {want[bad][0]}")
    return want


def _garbage_tail(packed, n_docs):
    """Sets every bit at or past n_docs of the last word."""
    if n_docs % 32:
        packed[:, -1] |= np.uint32((0xFFFFFFFF << (n_docs % 32)) & 0xFFFFFFFF)
    return packed


def _masks(rng, M, n_docs, p=0.5):
    """Packed random rows of density p; row M - 1 allows every document; the
    bits at or past n_docs are set (garbage that must be ignored)."""
    import bm25mi
    allow = rng.random((M, n_docs)) < p
    allow[M - 1] = True
    return _garbage_tail(bm25mi.pack_mask(allow), n_docs)


def _groups(rng, n_docs, G, negative=0.2):
    g = rng.integers(0, G, n_docs).astype(np.int32)
    g[rng.random(n_docs) < negative] = -1
    return g


# ------------------------------------------------------------ 1. the document axis
ROUTES = {"lds": (5, 3, CHUNK_MIN), "lds_mid": (1000, 3, 24 * 1024),
          "lds_wide": (BINS, 3, CHUNK_MAX), "global": (BINS + 1, 3, CHUNK_GLOBAL)}
WORDS = [1, 31, 32, 33, 63, 64, 65, 2047, 2048, 2049]


@pytest.mark.parametrize("route,n_docs", [(r, n) for r in ROUTES for n in WORDS] + [
    (r, n) for r, (_, _, c) in ROUTES.items() for n in (c - 1, c, c + 1, 2 * c + 1)])
def test_document_axis(make, route, n_docs):
    """Word, span and chunk edges of each route (M = 3 with an odd W leaves
    rows 1 and 2 misaligned, on top of the device buffer's one-word offset);
    garbage tail bits; a row of all ones counts every grouped document."""
    G, M, chunk = ROUTES[route]
    rng = np.random.default_rng(n_docs + G)
    groups = _groups(rng, n_docs, G)
    groups[-1] = G - 1                      # the last document and the last bin count
    want = _check(make(n_docs), _masks(rng, M, n_docs), groups, G, (route, n_docs))
    assert want[M - 1].sum() == (groups >= 0).sum() and want[M - 1, G - 1] >= 1


# --------------------------------------------------------------- 2. the group axis
@pytest.mark.parametrize("G", [1, 2, 63, 64, 65, 256, BINS, BINS + 1, 100_000])
def test_group_axis(make, G):
    """Each G at 5000 documents; G = 100 000: mostly empty bins, all written 0."""
    n_docs, M = 5000, 3
    rng = np.random.default_rng(G)
    want = _check(make(n_docs), _masks(rng, M, n_docs), _groups(rng, n_docs, G), G, G)
    assert want.sum() > 0 and (G < 100_000 or (want == 0).sum() > M * (G - n_docs))


# ------------------------------------------------------------------ 3. row blocks
@pytest.mark.parametrize("M", [MAXROWS - 1, MAXROWS, MAXROWS + 1, 2 * MAXROWS + 1])
def test_row_blocks(make, M):
    """G = 64 gives R = 64 rows per block: a block short of one row, full,
    one row over and two blocks and a row; the rows differ from each other."""
    n_docs, G = 3001, 64
    assert min(MAXROWS, BINS // G) == MAXROWS
    rng = np.random.default_rng(M)
    packed = _masks(rng, M, n_docs, 0.3)
    want = _check(make(n_docs), packed, _groups(rng, n_docs, G), G, M)
    assert len({w.tobytes() for w in want}) == M


def test_more_rows_than_65535(make):
    """70 000 rows of 2 words, G = 2."""
    n_docs, G, M = 50, 2, 70_000
    rng = np.random.default_rng(5)
    want = _check(make(n_docs), _masks(rng, M, n_docs), _groups(rng, n_docs, G), G)
    assert want[69_999].sum() > 0 and want[65_536:].sum() > 0


def test_empty_shapes_write_nothing(make):
    """M == 0 and G == 0 return without writing (host and device calls)."""
    import torch
    from bm25mi._capi import BM25_OK, lib
    index = make(70)
    packed = np.full((2, 3), 0xFFFFFFFF, np.uint32)
    groups = np.zeros(70, np.int32)
    buf = np.full(GUARD, FILL, np.int64)
    assert lib.bm25_mask_facets(index._h, _p(packed), 0, _p(groups), 4, _p(buf)) == BM25_OK
    assert lib.bm25_mask_facets(index._h, _p(packed), 2, _p(groups), 0, _p(buf)) == BM25_OK
    assert (buf == FILL).all()
    assert index.facets(packed, groups, 0).shape == (2, 0)
    assert index.facets(packed[:0], groups, 4).shape == (0, 4)
    st = torch.cuda.Stream()
    dm = torch.from_numpy(packed.view(np.int32)).cuda()
    dg = torch.from_numpy(groups).cuda()
    dbuf = torch.full((GUARD,), FILL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    index.facets_device(dm, dg, 0, dbuf[:0].view(2, 0), st)
    index.facets_device(dm[:0], dg, 4, dbuf[:0].view(0, 4), st)
    st.synchronize()
    assert (dbuf.cpu().numpy() == FILL).all()


# --------------------------------------------------------- 4. contention, content
@pytest.mark.parametrize("G,hot", [(1, 0), (7, 3), (BINS, BINS - 1), (BINS + 1, 8000)])
def test_every_document_in_one_group(make, G, hot):
    """An all-ones mask over documents of one group: 64 lanes on one bin.  That
    bin holds n_docs, every other one 0."""
    n_docs = 5000
    packed = _garbage_tail(np.full((2, (n_docs + 31) // 32), 0xFFFFFFFF, np.uint32), n_docs)
    want = _check(make(n_docs), packed, np.full(n_docs, hot, np.int32), G, (G, hot))
    assert (want[:, hot] == n_docs).all() and want.sum() == 2 * n_docs


@pytest.mark.parametrize("G", [3, 64, 1000, BINS + 1])
def test_cycling_and_random_groups(make, G):
    """Groups d % G, and random groups with 20 % negative, under random masks."""
    n_docs = 5000
    rng = np.random.default_rng(G)
    packed = _masks(rng, 3, n_docs)
    _check(make(n_docs), packed, np.arange(n_docs) % G, G, "cycle")
    groups = _groups(rng, n_docs, G)
    groups[::7] = np.iinfo(np.int32).min    # the most negative id is "no group" too
    _check(make(n_docs), packed, groups, G, "random")


@pytest.mark.parametrize("G", [1, 64, BINS + 1])
def test_groups_at_or_past_G(make, G):
    """5 % of the ids >= G (G itself and 2^31 - 1 among them): the device call
    counts them nowhere; the host call rejects the array, names the first such
    document and its value, and leaves the outputs untouched."""
    from bm25mi._capi import BM25_EINVAL, lib
    n_docs = 5000
    rng = np.random.default_rng(G + 1)
    packed = _masks(rng, 3, n_docs)
    groups = _groups(rng, n_docs, G)
    over = np.nonzero(rng.random(n_docs) < 0.05)[0]
    groups[over] = rng.integers(G, 2**31, len(over))
    groups[over[0]], groups[over[1]] = G, 2**31 - 1
    want = _check(make(n_docs), packed, groups, G, G, host=False)
    clean = np.where(groups >= G, -1, groups)
    assert np.array_equal(want, facets_want(packed, clean, G)) and want.sum() > 0
    buf = np.full(3 * G + GUARD, FILL, np.int64)
    index = make(n_docs)
    assert lib.bm25_mask_facets(index._h, _p(packed), 3, _p(groups), G, _p(buf)) == BM25_EINVAL
    msg = lib.bm25_last_error().decode()
    assert f"groups[{over[0]}] = {G}" in msg, msg
    assert (buf == FILL).all()
    with pytest.raises(ValueError, match=rf"groups\[{over[0]}\] = {G} "):
        index.facets(packed, groups, G)


# ------------------------------------------------------------------------ 5. masks
@pytest.mark.parametrize("G", [16, BINS + 1])
def test_mask_content(make, G):
    """All zeros, all ones, one bit at document 0, at n_docs - 1 and on each
    side of a word (32), span (256) and chunk boundary, and a 1 % random row;
    garbage bits at or past n_docs."""
    import bm25mi
    chunk = CHUNK_MIN if G <= BINS else CHUNK_GLOBAL
    n_docs = chunk + 100
    singles = [0, n_docs - 1, 31, 32, SPAN - 1, SPAN, chunk - 1, chunk]
    rng = np.random.default_rng(G)
    allow = np.zeros((len(singles) + 3, n_docs), bool)
    for r, d in enumerate(singles):
        allow[r, d] = True
    allow[-3] = rng.random(n_docs) < 0.01
    allow[-2] = True
    packed = _garbage_tail(bm25mi.pack_mask(allow), n_docs)
    groups = _groups(rng, n_docs, G, negative=0.0)
    want = _check(make(n_docs), packed, groups, G, G)
    for r, d in enumerate(singles):
        assert want[r].sum() == 1 and want[r, groups[d]] == 1
    assert want[-3].sum() == allow[-3].sum() > 0 and want[-2].sum() == n_docs
    assert want[-1].sum() == 0
    # all-zero masks alone (no bit set anywhere but in the ignored tail)
    zeros = _garbage_tail(np.zeros((2, packed.shape[1]), np.uint32), n_docs)
    assert _check(make(n_docs), zeros, groups, G, "zeros").sum() == 0


@pytest.mark.parametrize("G", [1, 3, BINS + 1])
def test_few_documents_in_a_step(make, G):
    """Rows with 1, 3, 4, 5, 6 and 64 documents inside one 64-document step
    (documents 64 .. 127, both of its mask words; 4 is the last count added
    one by one), next to neighbours of the other kind in the same row block,
    with groups that repeat, that are negative and (device call) that are >= G."""
    import bm25mi
    n_docs = 300
    picks = [[64], [64, 95, 96], [64, 95, 96, 127], [64, 95, 96, 127, 100],
             [70, 71, 72, 97, 98, 99], list(range(64, 128))]
    allow = np.zeros((2 * len(picks), n_docs), bool)
    for r, docs in enumerate(picks):
        allow[r, docs] = True
        allow[len(picks) + r, docs] = True
        allow[len(picks) + r, 200:200 + r] = True     # and another step of the same row
    packed = _garbage_tail(bm25mi.pack_mask(allow), n_docs)
    groups = (np.arange(n_docs) % G).astype(np.int32)
    groups[[95, 99]] = -1
    want = _check(make(n_docs), packed, groups, G, G)
    assert [int(w.sum()) for w in want[:len(picks)]] == [1, 2, 3, 4, 5, 62]
    groups[[96, 98]] = G, 2**31 - 1
    want = _check(make(n_docs), packed, groups, G, G, host=False)
    assert [int(w.sum()) for w in want[:len(picks)]] == [1, 1, 2, 3, 4, 60]


# ------------------------------------------------------------------- 6. identities
def test_sum_identity_with_mask_count(make):
    """facets.sum(1) + allowed documents without a group == mask_count."""
    n_docs, G = 5000, 37
    rng = np.random.default_rng(6)
    packed = _masks(rng, 5, n_docs, 0.3)
    groups = _groups(rng, n_docs, G)
    index = make(n_docs)
    got = index.facets(packed, groups, G)
    assert got.dtype == np.int64 and np.array_equal(got, facets_want(packed, groups, G))
    no_group = (unpack_rows(packed, n_docs) & (groups < 0)).sum(axis=1)
    assert no_group.sum() > 0
    assert np.array_equal(got.sum(axis=1) + no_group, index.mask_count(packed))


def test_doc_shards_add_up(make):
    """Handles over [0, 2048) and [2048, 5000) of one collection: their [M, G]
    outputs add up element-wise to the whole index's."""
    import bm25mi
    n, h, G = 5000, 2048, 37
    rng = np.random.default_rng(7)
    allow = rng.random((4, n)) < 0.4
    groups = _groups(rng, n, G)
    whole = _check(make(n), bm25mi.pack_mask(allow), groups, G, "whole")
    lo = _check(make(h), bm25mi.pack_mask(allow[:, :h]), groups[:h], G, "lo")
    hi = _check(make(n - h), bm25mi.pack_mask(allow[:, h:]), groups[h:], G, "hi")
    assert lo.sum() > 0 and hi.sum() > 0 and np.array_equal(lo + hi, whole)


# ------------------------------------------------------------- 7. one-call search
@pytest.fixture(scope="module")
def facet_case(gpu):
    """6000 documents (3 tiles), 60 terms, 7 queries with a clause row each,
    the masks by numpy, 11 groups with documents that have none."""
    rng = np.random.default_rng(41)
    N, nt, G = 6000, 60, 11
    ip, ix, dt = _rand_index(rng, N, nt, 3000)
    by_df = np.argsort(-np.diff(ip))
    a, b, c, d = (int(x) for x in by_df[:4])
    has = _has_of(ip, ix, nt, N)
    q = rng.integers(-1, nt, size=(7, 8)).astype(np.int32)
    mu = [[a], [a, b], [], [], [c], [b, b], [-1]]
    an = [[], [c, d], [a, d], [], [a, b], [], [-1, -1]]
    mn = [[b], [], [c], [a], [d], [b], []]
    masks = _want(has, mu, an, mn, 7)
    groups = _groups(rng, N, G)
    index = _idx(ip, ix, dt, N)
    yield index, q, mu, an, mn, masks, groups, G
    index.close()


def test_search_boolean_with_facets(facet_case):
    """search_boolean(facets=..., total_hits=True): docs, scores and totals
    bit-equal to the call without facets=, the facet rows equal to numpy's over
    the numpy-built masks and to index.facets(index.term_masks(...)), whatever
    bool_chunk (0 = automatic, 1, 3 on the 7-query batch); k = 0 returns the
    totals and facets alone; without facets= the return value has today's shape."""
    index, q, mu, an, mn, masks, groups, G = facet_case
    want = facets_want(masks, groups, G)
    assert want.sum() > 0 and not want[5].any()      # (row 5: the empty mask)
    built = index.term_masks(mu, an, mn)
    assert np.array_equal(built, masks)
    assert np.array_equal(index.facets(built, groups, G), want)
    plain = index.search_boolean(q, 10, mu, an, mn, total_hits=True)
    assert len(plain) == 3 and len(index.search_boolean(q, 10, mu, an, mn)) == 2
    try:
        for chunk in (0, 1, 3):
            index.set_option("bool_chunk", chunk)
            got = index.search_boolean(q, 10, mu, an, mn, total_hits=True, facets=(groups, G))
            assert len(got) == 4 and got[3].dtype == np.int64 and got[3].shape == (7, G)
            _exact(got[:2], plain[:2])
            assert np.array_equal(got[2], plain[2]) and np.array_equal(got[3], want), chunk
            got = index.search_boolean(q, 10, mu, an, mn, facets=(groups.astype(np.int64), G))
            assert len(got) == 3 and np.array_equal(got[2], want)
            _exact(got[:2], plain[:2])
            got = index.search_boolean(q, 0, mu, an, mn, total_hits=True, facets=(groups, G))
            assert got[0].shape == (7, 0) and got[1].shape == (7, 0)
            assert np.array_equal(got[2], plain[2]) and np.array_equal(got[3], want), chunk
            got = index.search_boolean(q, 0, mu, an, mn, facets=(groups, G))
            assert len(got) == 3 and np.array_equal(got[2], want), chunk
    finally:
        index.set_option("bool_chunk", 0)
    with pytest.raises(ValueError, match=r"groups\[17\] = 11 is not below G = 11"):
        bad = groups.copy()
        bad[17] = G
        index.search_boolean(q, 10, mu, an, mn, facets=(bad, G))


def test_search_boolean_facets_pointer_pairs(facet_case):
    """The C call: groups without out_facets (and the reverse) with G > 0 is
    EINVAL and writes nothing; with neither, it is bm25_search_boolean_min_match."""
    from bm25mi._capi import BM25_EINVAL, BM25_OK, lib
    from test_gpu_term_masks import _pad
    index, q, mu, an, mn, masks, groups, G = facet_case
    cl = [_pad(c, 7) for c in (mu, an, mn)]
    docs = np.full((7, 5), 7, np.int32)
    scores = np.full((7, 5), 7.0, np.float32)
    totals = np.full(7, FILL, np.int64)
    fac = np.full((7, G), FILL, np.int64)
    call = lambda gr, g, out: lib.bm25_search_boolean_facets(
        index._h, _p(q), 7, 8, 5, _p(cl[0]), cl[0].shape[1], _p(cl[1]), cl[1].shape[1], _p(cl[2]),
        cl[2].shape[1], None, None, 0, gr, g, _p(docs), _p(scores), _p(totals), out)
    assert call(_p(groups), G, None) == BM25_EINVAL
    assert call(None, G, _p(fac)) == BM25_EINVAL
    assert (docs == 7).all() and (totals == FILL).all() and (fac == FILL).all()
    assert call(None, 0, None) == BM25_OK
    want = index.search_boolean(q, 5, mu, an, mn, total_hits=True)
    _exact((docs, scores), want[:2])
    assert np.array_equal(totals, want[2]) and (fac == FILL).all()


# -------------------------------------------------------------------- 8. not a search
def test_not_a_search(facet_case):
    """After a search, facets (host and device calls) leave last_dispatch(),
    search_stats() and filtered_stats() as they were."""
    index, q, mu, an, mn, masks, groups, G = facet_case
    index.search_filtered(q, 10, masks, np.arange(7, dtype=np.int32))
    before = (index.last_dispatch(), index.search_stats(), index.filtered_stats())
    _check(index, masks, groups, G)
    assert (index.last_dispatch(), index.search_stats(), index.filtered_stats()) == before


def test_beside_a_search_on_another_stream(facet_case):
    """facets_device enqueued on its own stream right after a search_device on
    another stream of the same handle: both are exact."""
    import torch
    index, q, mu, an, mn, masks, groups, G = facet_case
    want = index.search(q, 50)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    dq = torch.from_numpy(q).cuda()
    dd = torch.full((7, 50), 99, dtype=torch.int32, device="cuda")
    ds = torch.full((7, 50), 7.5, dtype=torch.float32, device="cuda")
    dm = torch.from_numpy(masks.view(np.int32)).cuda()
    dg = torch.from_numpy(groups).cuda()
    dc = torch.full((7, G), FILL, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    index.search_device(dq, 50, dd, ds, s1)
    index.facets_device(dm, dg, G, dc, s2)
    s1.synchronize()
    s2.synchronize()
    _exact((dd.cpu().numpy(), ds.cpu().numpy()), want)
    assert np.array_equal(dc.cpu().numpy(), facets_want(masks, groups, G))
