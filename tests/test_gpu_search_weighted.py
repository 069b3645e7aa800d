"""GPU tests of the weighted query terms (bm25_search_weighted,
bm25_score_docs_weighted and their device forms; the weighted instantiations
of add_item's kernels in bm25mi_kernels.hip and of score_docs_kernel in
bm25mi_lookup.hip).

The expected row of a query comes from the numpy reference of
tests/test_search_weighted_host.py (float32 multiply, then float32 add, per
term in query order), selected as the filtered search's tests select: the
allowed ids by (score descending, doc ascending), the first k, padded with
doc -1 / score bits 0xFFFFFFFF.  Docs compare exactly and scores on their
uint32 views, by the host call and by the device call (a non-default stream,
outputs pre-filled with garbage).  The shapes sit next to

  32     documents per mask word
  2048   documents per tile
  64     terms per add_item group, postings per row
  4096   largest k of the tile passes (above: the dense path)"""
import numpy as np
import pytest

from test_gpu_edges import NEG_ZERO32, TILE, _edge_index, _edge_queries
from test_gpu_parity import _doc_slice, _exact, _idx, _rand_index
from test_gpu_search_filtered import PAD, _pack, _want
from test_search_weighted_host import (SHORT, ref_rows, spanning_rows, weighted_index,
                                       weighted_queries)

pytestmark = pytest.mark.gpu


def _device(index, q, w, k, packed=None, query_mask=None):
    import torch
    st = torch.cuda.Stream()
    dq = torch.from_numpy(np.ascontiguousarray(q, np.int32)).cuda()
    dw = torch.from_numpy(np.ascontiguousarray(w, np.float32)).cuda()
    dm = None if packed is None else torch.from_numpy(
        np.ascontiguousarray(packed).view(np.int32)).cuda()
    dqm = None if query_mask is None else torch.from_numpy(
        np.ascontiguousarray(query_mask, np.int32)).cuda()
    dd = torch.full((len(q), k), 123456789, dtype=torch.int32, device="cuda")
    ds = torch.full((len(q), k), 7.5, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()  # (the uploads ran on the current stream)
    index.search_weighted_device(dq, dw, k, dm, dqm, dd, ds, st)
    st.synchronize()
    return dd.cpu().numpy(), ds.cpu().numpy()


def _none(Q):
    return np.full(Q, -1, np.int32)


def _check(index, q, w, k, want, packed=None, query_mask=None, device=True, what=""):
    """The host call (and the device call) return ``want`` bit for bit."""
    got = index.search_weighted(q, w, k, packed, query_mask)
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32, what
    _exact(got, want)
    if device:
        _exact(_device(index, q, w, k, packed, query_mask), want)
    assert not (got[1].view(np.uint32) == NEG_ZERO32).any(), what
    return got


def _want_all(rows, k, doc_offset=0):
    return _want(rows, k, None, _none(len(rows)), doc_offset)


# -------------------------------------------- 1. unit weights: the plain search
@pytest.mark.parametrize("n_docs", [1, 33, 2049, 70_001])
@pytest.mark.parametrize("segments", ["dense", "sparse"])
def test_unit_weights_are_the_unweighted_search(gpu, segments, n_docs):
    """Weights of 1.0f give p == v: the rows of search_filtered without a
    filter, bit for bit, and the numpy reference's, on both segment tables."""
    rng = np.random.default_rng(200 + n_docs)
    V = 40
    ip, ix, dt = _edge_index(rng, n_docs, V, min(n_docs, 3000))
    q = np.concatenate([_edge_queries(rng, V, 8), np.full((1, 8), -1, np.int32)])
    w = np.ones(q.shape, np.float32)
    rows = ref_rows(n_docs, ip, ix, dt, q, w)
    index = _idx(ip, ix, dt, n_docs, segments=segments)
    assert index.info()["sparse"] == (segments == "sparse")
    none_masks = np.zeros((0, (n_docs + 31) // 32), np.uint32)
    for k in (1, 10):
        if k > n_docs:
            with pytest.raises(ValueError, match="out of bounds"):
                index.search_weighted(q, w, k)
            continue
        got = _check(index, q, w, k, _want_all(rows, k), what=(n_docs, k))
        _exact(got, index.search_filtered(q, k, none_masks, _none(len(q))))
        _exact(got, index.search(q, k))
    index.close()


# ------------------------------------------------- 2. zero weight is padding
@pytest.mark.parametrize("zero", [0.0, -0.0])
def test_zero_weight_is_padding(gpu, zero):
    """A slot of weight +0.0f or -0.0f changes nothing: the result of the same
    query with those ids replaced by -1, and no score is -0.0f."""
    n_docs, T = 2049, 8
    ip, ix, dt, V = weighted_index(n_docs)
    q, w = weighted_queries(n_docs, T)
    rng = np.random.default_rng(12)
    off = (rng.random(q.shape) < 0.4) & (q >= 0)
    off[1, :] = q[1, :] >= 0  # a whole row of zero weights
    assert off.any() and (~off & (q >= 0)).any()
    wz = w.copy()
    wz[off] = np.float32(zero)
    assert (wz[off].view(np.uint32) == (0x80000000 if np.signbit(zero) else 0)).all()
    qp = q.copy()
    qp[off] = -1
    index = _idx(ip, ix, dt, n_docs)
    for k in (1, 10, 300):
        want = _want_all(ref_rows(n_docs, ip, ix, dt, qp, w), k)
        got = _check(index, q, wz, k, want)
        _exact(got, index.search_weighted(qp, w, k))
    index.close()


# ------------------------------------------------ 3. signed, inexact weights
_CASE3 = {}


def _case3(n_docs, T):
    """The index, the queries and the reference rows of case 3 (shared with
    cases 7 and 8; computed once per shape)."""
    if (n_docs, T) not in _CASE3:
        ip, ix, dt, V = weighted_index(n_docs)
        q, w = weighted_queries(n_docs, T)
        _CASE3[(n_docs, T)] = (ip, ix, dt, q, w, ref_rows(n_docs, ip, ix, dt, q, w))
    return _CASE3[(n_docs, T)]


@pytest.mark.parametrize("T", [1, 8, 65, 130])
@pytest.mark.parametrize("n_docs", [2047, 2049, 70_001])
def test_signed_inexact_weights(gpu, n_docs, T):
    """Random float32 weights of both signs beside exact ones, NaN on the
    padding slots, a repeated id with two weights, queries of 1 term, inside
    one 64-term group, and across it (65, 130: the second group's weights
    start at weights + 64), rows that span term boundaries."""
    ip, ix, dt, q, w, rows = _case3(n_docs, T)
    if T > 1:
        assert spanning_rows(n_docs, ip, ix, q) > 0
        assert q[0, 0] == q[0, 1] and w[0, 0] != w[0, 1]
    index = _idx(ip, ix, dt, n_docs)
    for k in (1, 10, min(n_docs, 300)):
        _check(index, q, w, k, _want_all(rows, k), what=(n_docs, T, k))
    index.close()


# --------------------------- 4. all-negative weights on a non-negative index
def test_all_negative_weights_zero_fill(gpu):
    """Every touched document goes below zero: the untouched ones come first
    at +0.0f (the k smallest untouched ids), the touched ones follow by (score
    desc, doc asc).  Zero-score thresholds overflow the candidate lists, so
    the dense path serves queries — weighted."""
    rng = np.random.default_rng(4)
    N, V = 3 * TILE + 5, 30
    ip, ix, dt = _rand_index(rng, N, V, 400)
    assert (dt > 0).all()
    q = rng.integers(-1, V, size=(4, 6)).astype(np.int32)
    q[0, 0] = 2
    w = -np.exp2(rng.uniform(-3.0, 3.0, q.shape)).astype(np.float32)
    rows = ref_rows(N, ip, ix, dt, q, w)
    untouched = [np.nonzero(r == 0)[0] for r in rows]
    n_un = min(len(u) for u in untouched)
    assert all((r <= 0).all() and (r < 0).any() for r in rows) and n_un > 100
    index = _idx(ip, ix, dt, N)
    for k in (5, n_un):
        got = _check(index, q, w, k, _want_all(rows, k))
        for r in range(len(q)):
            assert got[0][r].tolist() == untouched[r][:k].tolist()
        assert not got[1].view(np.uint32).any()
    k = N
    got = _check(index, q, w, k, _want_all(rows, k))
    for r in range(len(q)):
        nu = len(untouched[r])
        assert got[0][r, :nu].tolist() == untouched[r].tolist()
        assert (got[1][r, nu:] < 0).all() and (np.diff(got[1][r, nu:]) <= 0).all()
    # the zero-fill overflow route of the tile passes
    index.set_option("list_cap", 64)
    k = min(n_un + 50, 4096)
    _check(index, q, w, k, _want_all(rows, k))
    assert index.filtered_stats()[0] > 0
    kernels = index.last_dispatch()["kernels"]
    assert {"filtered", "large_k", "weighted"} <= kernels
    index.close()


# --------------------------------------------------- 5. every route, same bits
@pytest.fixture(scope="module")
def small_case(gpu):
    """5 000 documents (3 tiles), 60 signed terms, 5 weighted queries."""
    rng = np.random.default_rng(21)
    N, V = 5000, 60
    ip, ix, dt = _rand_index(rng, N, V, 2500, signed=True, coarse=True)
    q = rng.integers(-1, V, size=(5, 8)).astype(np.int32)
    w = (np.exp2(rng.uniform(-6.0, 6.0, q.shape)) * rng.choice([-1.0, 1.0], q.shape)).astype(
        np.float32)
    return N, V, ip, ix, dt, q, w, ref_rows(N, ip, ix, dt, q, w)


@pytest.mark.parametrize("k", [1, 100, 4096, 4097, 5000])
def test_every_route_gives_the_same_bits(small_case, k):
    """The default route, the dense path for every query (filter_tiles = 0)
    and lists forced to overflow into the dense path (list_cap small)."""
    N, V, ip, ix, dt, q, w, rows = small_case
    want = _want_all(rows, k)
    index = _idx(ip, ix, dt, N)
    _check(index, q, w, k, want, what="default")
    kernels = index.last_dispatch()["kernels"]
    assert "weighted" in kernels and ("filtered" in kernels) == (k <= 4096)
    index.set_option("filter_tiles", 0)
    _check(index, q, w, k, want, what="dense")
    assert index.last_dispatch()["kernels"] == {"large_k", "weighted"}
    assert index.filtered_stats() == (len(q), 0, 0)
    index.set_option("filter_tiles", 1)
    index.set_option("list_cap", 4)
    _check(index, q, w, k, want, what="overflow")
    if 4 < k <= 4096:
        assert index.filtered_stats()[0] > 0
    index.close()


# ------------------------------------------------------------- 6. with masks
def test_with_masks(gpu):
    """Three masks (random 50 %, one tile only, all zeros) and query_mask
    mixing 0, 1, 2 and -1; M == 0 with query_mask None is no filter; a fully
    disallowed row is all padding; bits past n_docs never give a document."""
    n_docs, T = 70_001, 8
    ip, ix, dt, q, w, rows = _case3(n_docs, T)
    rng = np.random.default_rng(6)
    allow = np.zeros((3, n_docs), bool)
    allow[0] = rng.random(n_docs) < 0.5
    allow[1, 5 * TILE:6 * TILE] = True
    qm = np.array([0, 1, 2, -1, 1, 0], np.int32)
    assert len(q) == len(qm)
    packed = _pack(allow)
    index = _idx(ip, ix, dt, n_docs)
    for k in (1, 25, 3000):
        got = _check(index, q, w, k, _want(rows, k, allow, qm), packed, qm, what=k)
        assert (got[0][2] == -1).all() and (got[1][2].view(np.uint32) == PAD).all()
        in_tile = got[0][[1, 4]]
        assert ((in_tile == -1) | ((in_tile >= 5 * TILE) & (in_tile < 6 * TILE))).all()
    # query_mask None with masks: mask 0 for every query
    _check(index, q, w, 25, _want(rows, 25, allow, np.zeros(len(q), np.int32)), packed, None)
    # no masks at all: no filter, with and without the mask ids
    free = _want_all(rows, 25)
    _check(index, q, w, 25, free)
    _check(index, q, w, 25, free, np.zeros((0, packed.shape[1]), np.uint32), _none(len(q)))
    _check(index, q, w, 25, free, packed, _none(len(q)))
    # bits at and past n_docs of the last word set
    assert n_docs % 32
    ones = _pack(np.ones((1, n_docs), bool))
    ones[0, -1] = 0xFFFFFFFF
    last = np.zeros((1, n_docs), bool)
    last[0, n_docs - 40:] = True
    tail = _pack(last)
    tail[0, -1] = 0xFFFFFFFF
    _check(index, q, w, 25, free, ones)
    got = _check(index, q, w, 64, _want(rows, 64, last), tail)
    assert got[0].max() < n_docs and (got[0][:, 40:] == -1).all()
    index.close()


# ------------------------------------- 7. score_docs_weighted agrees with it
def _score_device(index, q, w, docs):
    import torch
    st = torch.cuda.Stream()
    dq = torch.from_numpy(np.ascontiguousarray(q, np.int32)).cuda()
    dw = torch.from_numpy(np.ascontiguousarray(w, np.float32)).cuda()
    dd = torch.from_numpy(np.ascontiguousarray(docs, np.int32)).cuda()
    out = torch.full(docs.shape, 7.5, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    index.score_docs_weighted_device(dq, dw, dd, out, st)
    st.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("T", [1, 8, 65, 130])
@pytest.mark.parametrize("segments", ["dense", "sparse"])
def test_score_docs_weighted_agrees_with_the_search(gpu, segments, T):
    """The documents case 3 returns, scored with the same weights: the bits of
    the search's scores and of the reference; a negative doc id and (device
    call) a doc outside the handle's range score +0.0f; two doc shards'
    device outputs add element-wise to the single-index output."""
    n_docs, k = 2049, 50
    ip, ix, dt, q, w, rows = _case3(n_docs, T)
    index = _idx(ip, ix, dt, n_docs, segments=segments)
    docs, scores = index.search_weighted(q, w, k)
    docs = np.concatenate([docs, np.full((len(q), 1), -1, np.int32),
                           np.tile(np.array([[0, n_docs - 1, TILE - 1, TILE]], np.int32),
                                   (len(q), 1))], axis=1)
    want = np.stack([np.where(docs[r] >= 0, rows[r][np.maximum(docs[r], 0)], np.float32(0))
                     for r in range(len(q))]).astype(np.float32)
    got = index.score_docs_weighted(q, w, docs)
    assert got.dtype == np.float32 and got.shape == docs.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[:, :k].view(np.uint32), scores.view(np.uint32))
    assert np.array_equal(_score_device(index, q, w, docs).view(np.uint32), want.view(np.uint32))
    # unit weights: bm25_score_docs
    ones = np.where(q >= 0, np.float32(1), np.float32(np.nan)).astype(np.float32)
    assert np.array_equal(index.score_docs_weighted(q, ones, docs).view(np.uint32),
                          index.score_docs(q, docs).view(np.uint32))
    # outside the handle's range: the device call scores +0.0f, the host call rejects
    far = docs.copy()
    far[:, 0] = n_docs + 7
    dev = _score_device(index, q, w, far)
    assert not dev[:, 0].view(np.uint32).any()
    assert np.array_equal(dev[:, 1:].view(np.uint32), want[:, 1:].view(np.uint32))
    with pytest.raises(ValueError, match="outside the index's documents"):
        index.score_docs_weighted(q, w, far)
    # two doc shards add up
    cut = TILE
    parts = []
    for lo, hi in ((0, cut), (cut, n_docs)):
        sh = _idx(*_doc_slice(ip, ix, dt, lo, hi), hi - lo, doc_offset=lo, segments=segments)
        parts.append(_score_device(sh, q, w, docs))
        sh.close()
    total = parts[0] + parts[1]
    assert np.array_equal(total.view(np.uint32), want.view(np.uint32))
    index.close()


# --------------------------------------------------------- 8. doc shards merge
def test_doc_shards_merge(gpu):
    """A 3-way split of the 70 001-document index: each shard's
    search_weighted_device list (padded where the shard holds fewer than k
    candidates under its mask) merged by merge_topk_device equals the
    single-index result."""
    import torch
    from bm25mi.index import merge_topk_device
    n_docs, T, k = 70_001, 65, 40
    ip, ix, dt, q, w, rows = _case3(n_docs, T)
    # a mask that leaves the last shard fewer than k documents
    cuts = [0, 11 * TILE, 30 * TILE, n_docs]
    rng = np.random.default_rng(8)
    allow = rng.random((1, n_docs)) < 0.6
    allow[0, cuts[2]:] = False
    allow[0, rng.choice(np.arange(cuts[2], n_docs), 17, replace=False)] = True
    want = _want(rows, k, allow)
    dq = torch.from_numpy(q).cuda()
    dw = torch.from_numpy(w).cuda()
    outs_d = torch.full((3, len(q), k), 99, dtype=torch.int32, device="cuda")
    outs_s = torch.full((3, len(q), k), 7.5, dtype=torch.float32, device="cuda")
    shards = []
    for r in range(3):
        lo, hi = cuts[r], cuts[r + 1]
        sh = _idx(*_doc_slice(ip, ix, dt, lo, hi), hi - lo, doc_offset=lo)
        shards.append(sh)
        dm = torch.from_numpy(_pack(allow[:, lo:hi]).view(np.int32)).cuda()
        sh.search_weighted_device(dq, dw, k, dm, None, outs_d[r], outs_s[r],
                                  torch.cuda.current_stream())
    torch.cuda.synchronize()
    third = outs_d[2].cpu().numpy()
    assert (third[:, :17] >= cuts[2]).all() and (third[:, 17:] == -1).all()
    md = torch.empty((len(q), k), dtype=torch.int32, device="cuda")
    ms = torch.empty((len(q), k), dtype=torch.float32, device="cuda")
    merge_topk_device(0, outs_d, outs_s, 3, len(q), k, md, ms, torch.cuda.current_stream())
    torch.cuda.synchronize()
    _exact((md.cpu().numpy(), ms.cpu().numpy()), want)
    for sh in shards:
        sh.close()


# ------------------------------------------------ 9. validation, live handle
def test_validation_on_a_live_handle(gpu):
    n_docs, T = 2049, 8
    ip, ix, dt, q, w, rows = _case3(n_docs, T)
    V = len(ip) - 1
    index = _idx(ip, ix, dt, n_docs)
    docs = np.zeros((len(q), 2), np.int32)
    r, c = map(int, np.argwhere(q >= 0)[5])
    for bad in (np.nan, np.inf, -np.inf):
        wb = w.copy()
        wb[r, c] = bad
        for call in (lambda: index.search_weighted(q, wb, 5),
                     lambda: index.score_docs_weighted(q, wb, docs)):
            with pytest.raises(ValueError, match=rf"weights\[{r}\]\[{c}\] = .* is not finite"):
                call()
    # NaN on a padding slot is accepted (the fixture has them)
    assert np.isnan(w[q < 0]).any()
    index.search_weighted(q, w, 5)
    index.score_docs_weighted(q, w, docs)
    qb = q.copy()
    qb[2, 1] = V
    with pytest.raises(ValueError, match=rf"maximum token ID in the query \({V}\)"):
        index.search_weighted(qb, w, 5)
    with pytest.raises(ValueError, match=rf"maximum token ID in the query \({V}\)"):
        index.score_docs_weighted(qb, w, docs)
    with pytest.raises(ValueError, match="out of bounds"):
        index.search_weighted(q, w, n_docs + 1)
    # the device call: ids >= n_terms are padding, their weights ignored
    wd = w.copy()
    wd[2, 1] = np.nan
    qp = q.copy()
    qp[2, 1] = -1
    want = _want_all(ref_rows(n_docs, ip, ix, dt, qp, w), 10)
    _exact(_device(index, qb, wd, 10), want)
    got = _score_device(index, qb, wd, want[0])
    assert np.array_equal(got.view(np.uint32), want[1].view(np.uint32))
    index.close()


# ------------------------------------------------------------- 10. dispatch
def test_dispatch_flag(gpu):
    n_docs, T = 2049, 8
    ip, ix, dt, q, w, rows = _case3(n_docs, T)
    index = _idx(ip, ix, dt, n_docs)
    index.search_weighted(q, w, 5)
    assert {"filtered", "weighted"} <= index.last_dispatch()["kernels"]
    import ctypes
    from bm25mi._capi import check, lib
    km = ctypes.c_uint32()
    check(lib.bm25_search_dispatch(index._h, ctypes.byref(km), None, None, None))
    assert km.value & 4096 and km.value & 8192
    qv = np.where(q >= SHORT, q, -1).astype(np.int32)
    index.search(qv, 5)
    check(lib.bm25_search_dispatch(index._h, ctypes.byref(km), None, None, None))
    assert not km.value & (4096 | 8192)
    assert not {"filtered", "weighted"} & index.last_dispatch()["kernels"]
    index.close()
