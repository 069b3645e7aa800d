"""GPU tests of the cursor pagination (bm25_search_after /
bm25_search_after_device; cursor_keys_kernel of bm25mi_filter.hip, the cursor
instantiations of the filter passes in bm25mi_kernels.hip and of the radix
selection in bm25mi_large.hip).

The expected rows come from tests/test_search_after_host.py (ref_after: the
C oracle's dense rows — the weighted numpy fold for weighted rows — ordered by
(score descending, doc ascending), restricted to the mask and to the keys
strictly after the cursor, the first k, padded), whose guards run on the CPU.
Docs compare exactly and scores on their uint32 views, by the host call and
by the device call (a non-default stream, outputs pre-filled with garbage).
The shapes sit next to

  2048   documents per tile (a cursor on 2047 with its equal at 2048)
  4096   largest k of the tile passes (above: the dense path and its clamp)"""
import numpy as np
import pytest

from test_gpu_edges import NEG_ZERO32, TILE
from test_gpu_parity import _doc_slice, _exact, _idx
from test_search_after_host import (AFTER_NONE, PAD, PAGE_CASES, after_case, position_cursors,
                                    position_masks, rank_cursor, ref_after, tie_cursor,
                                    weighted_case, zero_band_cursor)

pytestmark = pytest.mark.gpu


def _pack(allow):
    import bm25mi
    return None if allow is None else bm25mi.pack_mask(allow)


def _device(index, q, k, after=None, weights=None, packed=None, query_mask=None):
    import torch
    st = torch.cuda.Stream()
    up = lambda a, t: None if a is None else torch.from_numpy(np.array(a, t)).cuda()
    dq = up(q, np.int32)
    dw = up(weights, np.float32)
    dm = None if packed is None else torch.from_numpy(
        np.ascontiguousarray(packed).view(np.int32)).cuda()
    dqm = up(query_mask, np.int32)
    da = None if after is None else (up(after[0], np.float32), up(after[1], np.int32))
    dd = torch.full((len(q), k), 123456789, dtype=torch.int32, device="cuda")
    ds = torch.full((len(q), k), 7.5, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()  # (the uploads ran on the current stream)
    index.search_after_device(dq, k, da, dw, dm, dqm, dd, ds, st)
    st.synchronize()
    return dd.cpu().numpy(), ds.cpu().numpy()


def _check(index, q, k, want, after=None, weights=None, packed=None, query_mask=None, what=""):
    """The host call and the device call both return ``want`` bit for bit."""
    got = index.search_after(q, k, after, weights, packed, query_mask)
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32, what
    assert got[0].shape == (len(q), k), what
    _exact(got, want)
    _exact(_device(index, q, k, after, weights, packed, query_mask), want)
    assert not (got[1].view(np.uint32) == NEG_ZERO32).any(), what
    return got


def _oracle_rows(ip, ix, dt, q, n_docs):
    from oracle import oracle
    return [oracle.scores_dense_c(n_docs, ip, ix, dt, row) for row in q]


def _all_padding(page, rows):
    return (page[0][rows] == -1).all() and (page[1][rows].view(np.uint32) == PAD).all()


# ---------------------------------------------------------- 1. paging identity
@pytest.mark.parametrize("segments", ["dense", "sparse"])
@pytest.mark.parametrize("n_docs,k", PAGE_CASES)
def test_paging_identity(gpu, segments, n_docs, k):
    """Pages of k fed back through page_cursor until a row is exhausted or 6
    pages are taken: every page is the reference's, the concatenation is
    index.search(q, k P) where k P <= n_docs, and the call after a padded page
    returns all padding.  At n_docs <= 33 and k = 10 the pages run through the
    positive, the zero-score and the negative region into padding."""
    import bm25mi
    ip, ix, dt, q, rows = after_case(n_docs)
    index = _idx(ip, ix, dt, n_docs, segments=segments)
    assert index.info()["sparse"] == (segments == "sparse")
    pages, after = [], None
    while len(pages) < 6:
        want = ref_after(rows, k, after)
        pages.append(_check(index, q, k, want, after, what=(n_docs, k, len(pages))))
        after = bm25mi.page_cursor(*pages[-1])
        _exact((after[1][:, None], after[0][:, None]), (want[0][:, -1:], want[1][:, -1:]))
        if (after[1] == -1).any():
            break
    P = len(pages)
    cat = (np.concatenate([p[0] for p in pages], 1), np.concatenate([p[1] for p in pages], 1))
    _exact(cat, ref_after(rows, k * P))
    if k * P <= n_docs:
        _exact(cat, index.search(q, k * P))
        assert (cat[0] >= 0).all()
    else:   # the list ran out inside the last page
        assert n_docs <= 33 and (cat[0][:, :n_docs] >= 0).all() and (cat[0][:, n_docs:] == -1).all()
    done = np.nonzero(after[1] == -1)[0]
    if done.size:
        nxt = _check(index, q, k, ref_after(rows, k, after), after)
        assert _all_padding(nxt, done)
    if k * 6 >= n_docs:
        assert done.size == len(q)   # (these fixtures are paged to their end)
    index.close()


# --------------------------------------------------------- 2. cursor positions
@pytest.fixture(scope="module")
def pos_case(gpu):
    """The 5000-document fixture (3 tiles) with two masks and mask ids mixing
    -1, 0 and 1; one handle at doc_offset 0 and one at 10 000."""
    ip, ix, dt, q, rows = after_case(5000)
    allow, qm = position_masks()
    handles = {off: _idx(ip, ix, dt, 5000, doc_offset=off) for off in (0, 10_000)}
    yield q, rows, allow, qm, _pack(allow), handles
    for h in handles.values():
        h.close()


@pytest.mark.parametrize("doc_offset", [0, 10_000])
def test_cursor_positions(pos_case, doc_offset):
    """The best key (everything but one document left), the worst (nothing
    left), inside a tie run, on doc 2047 with its equal at 2048, a score
    between two present ones, +inf, a doc id the mask disallows, a doc id past
    n_docs and (doc_offset = 10 000) one below doc_offset, AFTER_NONE and -1
    mixed with cursors in one batch."""
    q, rows, allow, qm, packed, handles = pos_case
    index = handles[doc_offset]
    k = 10
    first = ref_after(rows, k, None, allow, qm, doc_offset)
    cursors = position_cursors(rows, allow, qm, doc_offset)
    assert len(cursors) == (10 if doc_offset else 9)
    for name, after in cursors:
        want = ref_after(rows, k, after, allow, qm, doc_offset)
        got = _check(index, q, k, want, after, None, packed, qm, what=name)
        if name == "best key":    # rank 2 onwards
            _exact((got[0][:, :-1], got[1][:, :-1]), (first[0][:, 1:], first[1][:, 1:]))
        elif name == "worst key":
            assert _all_padding(got, slice(None))
        elif name == "+inf":
            _exact(got, first)
        elif name == "tile edge":
            assert got[0][1, 0] == TILE + doc_offset and got[1][1, 0] == after[0][1]
        elif name == "inside a tie":   # the next document of the run, not the cursor's own
            assert (got[1][:, 0] == after[0]).all() and (got[0][:, 0] > after[1]).all()
        elif name == "doc below doc_offset":   # the whole run of equal scores is still there
            tie = dict(cursors)["inside a tie"]
            assert (got[1][:, 0] == after[0]).all() and (got[0][:, 0] < tie[1]).all()
        elif name == "doc past n_docs":        # none of the equal scores is
            assert (got[1][:, 0].view(np.uint32) != after[0].view(np.uint32)).all()
        elif name.startswith("mixed"):
            _exact((got[0][::2], got[1][::2]), (first[0][::2], first[1][::2]))
            assert _all_padding(got, [3])
    kinds = index.last_dispatch()["kernels"]
    assert "after" in kinds and "weighted" not in kinds


# ------------------------------------------------- 3. every route, the same bits
def test_routes_agree(pos_case):
    """The position cursors through the tile passes, with list_cap small (the
    rows with more than list_cap eligible documents overflow to the dense
    path), and with filter_tiles = 0: identical bits, the dispatch flags and
    the dense rows counted."""
    q, rows, allow, qm, packed, handles = pos_case
    index = handles[0]
    k, cap = 10, 4
    try:
        for name, after in position_cursors(rows, allow, qm):
            want = ref_after(rows, k, after, allow, qm)
            left = (ref_after(rows, 5000, after, allow, qm)[0] >= 0).sum(1)
            index.set_option("filter_tiles", 1)
            index.set_option("list_cap", 0)
            _check(index, q, k, want, after, None, packed, qm, what=(name, "tiles"))
            assert {"after", "filtered"} <= index.last_dispatch()["kernels"]
            index.set_option("list_cap", cap)
            _check(index, q, k, want, after, None, packed, qm, what=(name, "overflow"))
            over = int((left > cap).sum())
            assert index.filtered_stats()[0] == over, name
            assert {"after", "filtered"} | ({"large_k"} if over else set()) == \
                index.last_dispatch()["kernels"], name
            index.set_option("filter_tiles", 0)
            _check(index, q, k, want, after, None, packed, qm, what=(name, "dense"))
            assert index.last_dispatch()["kernels"] == {"after", "large_k"}
            assert index.filtered_stats() == (len(q), 0, 0)
    finally:
        index.set_option("filter_tiles", 1)
        index.set_option("list_cap", 0)


@pytest.mark.parametrize("left", [4900, 4097, 3000, 1, 0])
def test_dense_clamp_at_large_k(pos_case, left):
    """k = 4097 (the dense path) on the 5000-document fixture with every row's
    cursor at the rank that leaves more than, exactly and fewer than 4097
    eligible documents: the row holds min(4097, left) documents and the rest is
    padding — counted against the reference, not a prefix compared."""
    q, rows, allow, qm, packed, handles = pos_case
    index = handles[0]
    k = 4097
    after = rank_cursor(rows, 5000 - left)
    want = ref_after(rows, k, after)
    assert ((want[0] == -1).sum(1) == k - min(k, left)).all()
    got = _check(index, q, k, want, after, what=left)
    assert ((got[0] == -1).sum(1) == k - min(k, left)).all()
    assert ((got[1].view(np.uint32) == PAD).sum(1) == k - min(k, left)).all()
    assert index.last_dispatch()["kernels"] == {"after", "large_k"}
    assert index.filtered_stats() == (len(q), 0, 0)
    # ... and under the masks, where the census bounds a row before the cursor does
    for name, cur in position_cursors(rows, allow, qm)[2:4]:
        _check(index, q, k, ref_after(rows, k, cur, allow, qm), cur, None, packed, qm, what=name)


# ------------------------------------------------------------- 4. composition
def test_weights_of_both_signs(gpu):
    """The weighted fixture (the zero-score band in the middle of the order):
    pages through a cursor inside the band, a tie cursor, and the identities
    all-1.0f weights == weights None and after None == search_weighted /
    search_filtered / search."""
    import bm25mi
    ip, ix, dt, q, w, rows = weighted_case()
    N, k = 5000, 10
    index = _idx(ip, ix, dt, N)
    after = zero_band_cursor(rows)
    for _ in range(3):
        page = _check(index, q, k, ref_after(rows, k, after), after, w, what="zero band")
        assert (page[1] <= 0).all()
        after = bm25mi.page_cursor(*page)
    assert {"after", "weighted"} <= index.last_dispatch()["kernels"]
    # from inside the positive region down into the band
    npos = [int((r > 0).sum()) for r in rows]
    assert min(npos) >= 4
    each = [rank_cursor(rows[r:r + 1], npos[r] - 3) for r in range(len(rows))]
    after = (np.concatenate([e[0] for e in each]), np.concatenate([e[1] for e in each]))
    page = _check(index, q, k, ref_after(rows, k, after), after, w, what="into the band")
    assert (page[1][:, 0] > 0).all() and (page[1][:, -1] == 0).all()
    # masks with weights
    allow, qm = position_masks()
    qm = qm[:len(q)]
    ta = tie_cursor(rows, allow, qm)
    _check(index, q, k, ref_after(rows, k, ta, allow, qm), ta, w, _pack(allow), qm, "masked")
    # after None is the search without a cursor, bit for bit
    _exact(index.search_after(q, k, None, w), index.search_weighted(q, w, k))
    _exact(index.search_after(q, k, None, w, _pack(allow), qm),
           index.search_weighted(q, w, k, _pack(allow), qm))
    _exact(index.search_after(q, k, None, None, _pack(allow), qm),
           index.search_filtered(q, k, _pack(allow), qm))
    _exact(index.search_after(q, k), index.search(q, k))
    none = (np.full(len(q), np.nan, np.float32), np.full(len(q), AFTER_NONE, np.int32))
    _exact(index.search_after(q, k, none, w), index.search_weighted(q, w, k))
    _exact(_device(index, q, k, none, w), index.search_weighted(q, w, k))
    # all-1.0f weights are weights None
    plain = ref_after(_oracle_rows(ip, ix, dt, q, N), k, ta, allow, qm)
    ones = np.ones(q.shape, np.float32)
    a = _check(index, q, k, plain, ta, ones, _pack(allow), qm, "unit weights")
    b = _check(index, q, k, plain, ta, None, _pack(allow), qm, "no weights")
    _exact(a, b)
    index.close()


# --------------------------------------------------------------- 5. doc shards
def test_doc_shards_compose(gpu):
    """Two handles over the halves [0, 2048) and [2048, 5000) of the fixture
    with their doc_offsets, the same global cursor on both, the lists merged by
    merge_topk_device: the single index's page — for a cursor inside a tie,
    the cursor on doc 2047 (the last of shard 0: below shard 1's doc_offset)
    and a deep rank whose doc lies in either shard."""
    import torch
    from bm25mi.index import merge_topk_device
    ip, ix, dt, q, rows = after_case(5000)
    allow, qm = position_masks()
    N, cut, k = 5000, TILE, 40
    cur = dict(position_cursors(rows, allow, qm))
    cursors = [("inside a tie", cur["inside a tie"]), ("tile edge", cur["tile edge"]),
               ("rank 700", rank_cursor(rows, 700, allow, qm))]
    assert (cursors[2][1][1] < cut).any() and (cursors[2][1][1] >= cut).any()
    shards = [(_idx(*_doc_slice(ip, ix, dt, lo, hi), hi - lo, doc_offset=lo), lo, hi)
              for lo, hi in ((0, cut), (cut, N))]
    dq = torch.from_numpy(np.array(q)).cuda()
    dqm = torch.from_numpy(np.array(qm)).cuda()
    for name, after in cursors:
        want = ref_after(rows, k, after, allow, qm)
        da = (torch.from_numpy(after[0]).cuda(), torch.from_numpy(after[1]).cuda())
        outs_d = torch.full((2, len(q), k), 99, dtype=torch.int32, device="cuda")
        outs_s = torch.full((2, len(q), k), 7.5, dtype=torch.float32, device="cuda")
        for r, (sh, lo, hi) in enumerate(shards):
            dm = torch.from_numpy(_pack(allow[:, lo:hi]).view(np.int32)).cuda()
            sh.search_after_device(dq, k, da, None, dm, dqm, outs_d[r], outs_s[r],
                                   torch.cuda.current_stream())
            torch.cuda.synchronize()
            _exact((outs_d[r].cpu().numpy(), outs_s[r].cpu().numpy()),
                   ref_after([x[lo:hi] for x in rows], k, after, allow[:, lo:hi], qm, lo))
        md = torch.empty((len(q), k), dtype=torch.int32, device="cuda")
        ms = torch.empty((len(q), k), dtype=torch.float32, device="cuda")
        merge_topk_device(0, outs_d, outs_s, 2, len(q), k, md, ms, torch.cuda.current_stream())
        torch.cuda.synchronize()
        _exact((md.cpu().numpy(), ms.cpu().numpy()), want)
    for sh, _, _ in shards:
        sh.close()


# ------------------------------------------------------------- 6. handle state
def test_cursor_search_between_ordinary_searches(pos_case):
    """A cursor search between ordinary searches of one handle (other shapes,
    other paths) leaves their results as they were, and is itself unchanged
    by them."""
    q, rows, allow, qm, packed, handles = pos_case
    index = handles[0]
    after = tie_cursor(rows, allow, qm)
    want = ref_after(rows, 10, after, allow, qm)
    s1 = index.search(q, 25)
    f1 = index.search_filtered(q[:4], 7, packed, qm[:4])
    _check(index, q, 10, want, after, None, packed, qm)
    _exact(index.search(q, 25), s1)
    assert "after" not in index.last_dispatch()["kernels"]
    _check(index, q, 10, want, after, None, packed, qm)
    _exact(index.search_filtered(q[:4], 7, packed, qm[:4]), f1)
    assert "after" not in index.last_dispatch()["kernels"]
    big = index.search(q[:2], 4500)
    _check(index, q, 10, want, after, None, packed, qm)
    _exact(index.search(q[:2], 4500), big)


# ------------------------------------------------------- 7. the host call's checks
def test_host_call_rejects_bad_cursors(pos_case):
    """bm25_search_after itself (below the Python layer): an after_docs entry
    < -2, a NaN cursor score on a row that names a document and a one-sided
    cursor are EINVAL, naming row and value; the outputs stay untouched and
    the handle stays usable.  A NaN beside AFTER_NONE or -1 is not read."""
    import ctypes
    from bm25mi._capi import BM25_EINVAL, lib
    q, rows, allow, qm, packed, handles = pos_case
    index = handles[0]
    Q, T = q.shape
    qq = np.array(q)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    docs = np.full((Q, 5), 7, np.int32)
    scores = np.full((Q, 5), 7.0, np.float32)

    def call(a_s, a_d):
        return lib.bm25_search_after(index._h, p(qq), None, Q, T, 5, None, 0, None,
                                     None if a_s is None else p(a_s),
                                     None if a_d is None else p(a_d), p(docs), p(scores))
    a_s = np.zeros(Q, np.float32)
    a_d = np.zeros(Q, np.int32)
    a_d[4] = -3
    assert call(a_s, a_d) == BM25_EINVAL
    assert b"after_docs[4] = -3" in lib.bm25_last_error()
    a_d[4] = 0
    a_s[2] = np.nan
    assert call(a_s, a_d) == BM25_EINVAL
    assert b"after_scores[2] = nan" in lib.bm25_last_error()
    assert call(a_s, None) == BM25_EINVAL and b"both" in lib.bm25_last_error()
    assert call(None, a_d) == BM25_EINVAL and b"both" in lib.bm25_last_error()
    assert (docs == 7).all() and (scores == 7.0).all()
    a_d[2] = AFTER_NONE
    a_s[5] = np.nan
    a_d[5] = -1
    assert call(a_s, a_d) == 0
    _exact((docs, scores), ref_after(rows, 5, (np.nan_to_num(a_s), a_d)))
