"""GPU tests of the filtered search (bm25_search_filtered /
bm25_search_filtered_device; bm25mi_filter.hip, the filter passes of
bm25mi_kernels.hip and the masked radix selection of bm25mi_large.hip).

The expected row of a query is computed here: the C oracle's dense scores
(oracle.scores_dense_c), the allowed ids kept, ordered by (score descending,
doc ascending), the first k, padded with doc -1 / score bits 0xFFFFFFFF.  Docs
compare exactly and scores on their uint32 views, by the host call and by the
device call (a non-default stream, outputs pre-filled with garbage).  The
shapes sit next to

  32     documents per mask word
  2048   documents per tile (64 mask words; a lane's 8 nibbles)
  4096   largest k of the tile passes (above: the dense path)"""
import numpy as np
import pytest

from oracle import oracle
from test_gpu_edges import FULL, NEG_ZERO32, TILE, _columns, _edge_index, _edge_queries
from test_gpu_parity import _doc_slice, _exact, _idx, _rand_index
from test_gpu_score_docs import BIG, NEG, ONE, ORDER_DOC, slot_index  # noqa: F401 (a fixture)

pytestmark = pytest.mark.gpu

PAD = 0xFFFFFFFF


def _pack(allow):
    import bm25mi
    return bm25mi.pack_mask(allow)


def _dense_rows(n_docs, ip, ix, dt, q):
    return [oracle.scores_dense_c(n_docs, ip, ix, dt, row) for row in q]


def _want(rows, k, allow, query_mask=None, doc_offset=0):
    """rows: the queries' dense score rows; allow: bool [M, n_docs];
    query_mask: per query its mask (-1: no filter; None: mask 0)."""
    Q = len(rows)
    docs = np.full((Q, k), -1, np.int32)
    bits = np.full((Q, k), PAD, np.uint32)
    for r, row in enumerate(rows):
        m = 0 if query_mask is None else int(query_mask[r])
        ids = np.arange(len(row)) if m < 0 else np.nonzero(allow[m])[0]
        s = row[ids]
        order = np.lexsort((ids, -s.astype(np.float64)))[:k]   # score desc, then doc asc
        docs[r, :len(order)] = ids[order] + doc_offset
        bits[r, :len(order)] = s[order].view(np.uint32)
    return docs, bits.view(np.float32)


def _device(index, q, k, packed, query_mask=None):
    import torch
    st = torch.cuda.Stream()
    dq = torch.from_numpy(np.ascontiguousarray(q, np.int32)).cuda()
    dm = torch.from_numpy(np.ascontiguousarray(packed).view(np.int32)).cuda()
    dqm = None if query_mask is None else torch.from_numpy(
        np.ascontiguousarray(query_mask, np.int32)).cuda()
    dd = torch.full((len(q), k), 123456789, dtype=torch.int32, device="cuda")
    ds = torch.full((len(q), k), 7.5, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()  # (the uploads ran on the current stream)
    index.search_filtered_device(dq, k, dm, dqm, dd, ds, st)
    st.synchronize()
    return dd.cpu().numpy(), ds.cpu().numpy()


def _check(index, q, k, packed, want, query_mask=None, what=""):
    """The host call and the device call both return ``want`` bit for bit."""
    got = index.search_filtered(q, k, packed, query_mask)
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32, what
    _exact(got, want)
    _exact(_device(index, q, k, packed, query_mask), want)
    assert not (got[1].view(np.uint32) == NEG_ZERO32).any(), what
    return got


# ------------------------------------------------------ 1. word and tile edges
@pytest.mark.parametrize("n_docs", [1, 31, 32, 33, 2047, 2048, 2049, 70_001])
@pytest.mark.parametrize("segments", ["dense", "sparse"])
def test_word_and_tile_edges(gpu, segments, n_docs):
    """Around the 32-document mask word and the 2048-document tile (one
    document ... 35 tiles with a partial last word and tile), both segment
    tables, signed quarter-step values with -0.0 among the inputs.  Masks, one
    after the other: all ones, all zeros (a fully padded row), a single
    document at each end of a word and of a tile, random 50 % and 1 %, the
    documents of one tile only, and all ones with the bits past n_docs of the
    last word set (they never produce a document).  k = 1 and 10 (k > n_docs
    is the reference's argpartition error)."""
    rng = np.random.default_rng(100 + n_docs)
    V = 40
    ip, ix, dt = _edge_index(rng, n_docs, V, min(n_docs, 3000))
    if n_docs > 2049:
        assert (dt.view(np.uint32) == NEG_ZERO32).any()
    q = np.concatenate([_edge_queries(rng, V, 8), np.full((1, 8), -1, np.int32)])
    rows = _dense_rows(n_docs, ip, ix, dt, q)
    index = _idx(ip, ix, dt, n_docs, segments=segments)
    assert index.info()["sparse"] == (segments == "sparse")
    ntiles = (n_docs + TILE - 1) // TILE
    W = (n_docs + 31) // 32

    masks = [("ones", np.ones(n_docs, bool)), ("zeros", np.zeros(n_docs, bool))]
    for d in sorted({0, 31, 32, 63, TILE - 1, TILE, n_docs - 1}):
        if d < n_docs:
            a = np.zeros(n_docs, bool)
            a[d] = True
            masks.append((f"doc {d}", a))
    masks.append(("half", rng.random(n_docs) < 0.5))
    masks.append(("1 %", rng.random(n_docs) < 0.01))
    t = min(1, ntiles - 1)
    a = np.zeros(n_docs, bool)
    a[t * TILE:(t + 1) * TILE] = True
    masks.append((f"tile {t}", a))
    for name, allow in masks:
        packed = _pack(allow)
        assert packed.shape == (1, W)
        for k in (1, 10):
            if k > n_docs:
                with pytest.raises(ValueError, match="out of bounds"):
                    index.search_filtered(q, k, packed)
                continue
            _check(index, q, k, packed, _want(rows, k, allow[None, :]), what=(name, k))
    if n_docs % 32:
        packed = _pack(np.ones(n_docs, bool))
        packed[0, -1] = 0xFFFFFFFF  # bits at and past n_docs set
        for k in (1, min(10, n_docs)):
            got = _check(index, q, k, packed, _want(rows, k, np.ones((1, n_docs), bool)),
                         what=("past n_docs", k))
            assert got[0].max() < n_docs
    # a fully padded row: every doc -1, every score bit set
    got = index.search_filtered(q, 1, _pack(np.zeros(n_docs, bool)))
    assert (got[0] == -1).all() and (got[1].view(np.uint32) == PAD).all()
    index.close()


# ------------------------------------------------ 2. k against the allowed count
@pytest.fixture(scope="module")
def small_case(gpu):
    """5 000 documents (3 tiles), 60 signed terms, 5 queries, a mask allowing
    300 documents."""
    rng = np.random.default_rng(21)
    N, V = 5000, 60
    ip, ix, dt = _rand_index(rng, N, V, 2500, signed=True, coarse=True)
    q = rng.integers(-1, V, size=(5, 8)).astype(np.int32)
    allow = np.zeros((1, N), bool)
    allow[0, rng.choice(N, 300, replace=False)] = True
    return N, V, ip, ix, dt, q, allow, _dense_rows(N, ip, ix, dt, q)


@pytest.mark.parametrize("k", [0, 299, 300, 301, 4096, 4097, 5000])
def test_k_against_allowed_count(small_case, k):
    """k below, at and above the 300 allowed documents, and across the 4096
    boundary of the tile passes: the padding starts exactly at column 300;
    k >= 4097 takes the dense path (dispatch bit 64), k = 301 the tile passes
    (bit 4096)."""
    N, V, ip, ix, dt, q, allow, rows = small_case
    index = _idx(ip, ix, dt, N)
    want = _want(rows, k, allow)
    got = _check(index, q, k, _pack(allow), want)
    assert got[0].shape == (len(q), k)
    if k > 300:
        assert (got[0][:, :300] >= 0).all() and (got[0][:, 300:] == -1).all()
        assert (got[1][:, 300:].view(np.uint32) == PAD).all()
        assert (got[1][:, :300].view(np.uint32) != PAD).all()
    elif k:
        assert (got[0] >= 0).all()
    kernels = index.last_dispatch()["kernels"]
    if k >= 4097:
        assert "large_k" in kernels and "filtered" not in kernels
        assert index.filtered_stats()[0] == len(q)
    elif k == 301:
        assert "filtered" in kernels
    index.close()


# ------------------------------------------------ 3. zero fill, signed scores
def test_zero_fill_and_signed_scores(small_case):
    """An all-padding query returns its k smallest allowed ids at score bits
    0x00000000; on a signed index the allowed documents no term touches (and
    those whose sum is 0) outrank the allowed documents of negative sums."""
    N, V, ip, ix, dt, q, allow, _ = small_case
    index = _idx(ip, ix, dt, N)
    packed = _pack(allow)
    ids = np.nonzero(allow[0])[0]
    pad_q = np.full((2, 8), -1, np.int32)
    for k in (1, 10, 300):
        docs, scores = index.search_filtered(pad_q, k, packed)
        assert docs.tolist() == [ids[:k].tolist()] * 2
        assert not scores.view(np.uint32).any()
        _exact(_device(index, pad_q, k, packed), (docs, scores))
    # one short term of negative values: most allowed documents stay at zero
    cols = _columns(ip, ix, dt)
    neg_term = next(t for t in range(V) if len(cols[t][0]) and (cols[t][1] < 0).any())
    qn = np.full((1, 8), -1, np.int32)
    qn[0, 3] = neg_term
    rows = _dense_rows(N, ip, ix, dt, qn)
    allow2 = allow.copy()
    allow2[0, np.nonzero(rows[0] < 0)[0][:40]] = True  # negative documents among the allowed
    hit = allow2[0] & (rows[0] < 0)
    assert hit.sum() >= 40
    k = int(allow2[0].sum())
    want = _want(rows, k, allow2)
    first_neg = int(np.argmax(want[1][0] < 0))
    assert first_neg > 0 and (want[1][0][:first_neg] >= 0).all() and (want[1][0][first_neg:] < 0).all()
    _check(index, qn, k, _pack(allow2), want)
    _check(index, qn, first_neg + 5, _pack(allow2), _want(rows, first_neg + 5, allow2))
    index.close()


# ----------------------------------------------------------- 4. rounding order
@pytest.mark.parametrize("T", [3, 65])
def test_rounding_order(slot_index, T):
    """1e8, 1.0, -1e8 on one allowed document, in this query order: its score
    is (1e8 + 1.0) - 1e8 = 0.0 — any reordered sum gives 1.0 — by the tile
    passes and by the dense path."""
    index, N, V, ip, ix, dt = slot_index
    q = np.full((2, T), -1, np.int32)
    q[0, [0, T // 2, T - 1]] = [BIG, ONE, NEG]
    q[1, [0, T // 2, T - 1]] = [BIG, ONE, NEG]
    q[1, 1] = FULL
    rows = _dense_rows(N, ip, ix, dt, q)
    assert rows[0][ORDER_DOC] == 0.0
    allow = np.zeros((1, N), bool)
    allow[0, [5, ORDER_DOC, 4000]] = True
    want = _want(rows, 3, allow)
    assert want[0][0].tolist() == [5, ORDER_DOC, 4000] and not want[1][0].view(np.uint32).any()
    for tiles in (1, 0):
        index.set_option("filter_tiles", tiles)
        _check(index, q, 3, _pack(allow), want, what=(T, tiles))
    index.set_option("filter_tiles", 1)


# ------------------------------------------------------------- 5. several masks
def test_several_masks(gpu):
    """Q = 7 queries over M = 3 masks, query_mask = [0, 2, -1, 1, 1, -1, 0]:
    the -1 rows equal index.search's rows bit for bit; query_mask = None
    equals all-zero entries; M = 0 serves a batch of -1 entries only."""
    rng = np.random.default_rng(5)
    N, V = 9000, 80
    ip, ix, dt = _rand_index(rng, N, V, 3000, signed=True, coarse=True)
    q = rng.integers(-1, V, size=(7, 9)).astype(np.int32)
    rows = _dense_rows(N, ip, ix, dt, q)
    allow = np.stack([rng.random(N) < 0.5, rng.random(N) < 0.02, np.arange(N) >= 2 * TILE + 7])
    qm = np.array([0, 2, -1, 1, 1, -1, 0], np.int32)
    index = _idx(ip, ix, dt, N)
    packed = _pack(allow)
    plain = index.search(q, 25)
    got = _check(index, q, 25, packed, _want(rows, 25, allow, qm), qm)
    for r in (2, 5):
        assert np.array_equal(got[0][r], plain[0][r])
        assert np.array_equal(got[1][r].view(np.uint32), plain[1][r].view(np.uint32))
    _check(index, q, 25, packed, _want(rows, 25, allow, np.zeros(7, np.int32)), None)
    _exact(index.search_filtered(q, 25, packed, np.zeros(7, np.int32)),
           index.search_filtered(q, 25, packed))
    none = np.full(7, -1, np.int32)
    _exact(index.search_filtered(q, 25, np.zeros((0, (N + 31) // 32), np.uint32), none), plain)
    with pytest.raises(ValueError, match=r"outside \[-1, 3\)"):
        from bm25mi._capi import check, lib
        import ctypes
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        bad = np.array([0, 3, -1, 1, 1, -1, 0], np.int32)
        d, s = np.zeros((7, 25), np.int32), np.zeros((7, 25), np.float32)
        check(lib.bm25_search_filtered(index._h, p(q), 7, 9, 25, p(packed), 3, p(bad), p(d), p(s)))
    index.close()


# --------------------------------------------------------------- 6. paths agree
def test_paths_agree(gpu):
    """The same inputs by the tile passes, by the dense path (filter_tiles =
    0) and with list_cap small enough that the lists overflow and the queries
    go to the dense path on their own (filtered_stats()[0] > 0): identical
    bits.  The all-ones mask at k = 100 equals index.search."""
    rng = np.random.default_rng(6)
    N, V = 40 * TILE + 77, 200  # 41 tiles: 164 pass-A keys per query, more than k
    ip, ix, dt = _rand_index(rng, N, V, 12_000)
    q = rng.integers(-1, V, size=(16, 8)).astype(np.int32)
    q[3, :] = -1
    rows = _dense_rows(N, ip, ix, dt, q)
    allow = np.stack([rng.random(N) < 0.3, np.ones(N, bool)])
    qm = (np.arange(16) % 2).astype(np.int32)
    want = _want(rows, 100, allow, qm)
    packed = _pack(allow)
    index = _idx(ip, ix, dt, N)
    a = _check(index, q, 100, packed, want, qm, "tiles")
    assert "filtered" in index.last_dispatch()["kernels"]
    served = index.filtered_stats()
    assert served[0] < 16 and served[2] > 0
    index.set_option("filter_tiles", 0)
    b = _check(index, q, 100, packed, want, qm, "dense")
    assert index.last_dispatch()["kernels"] == {"large_k"}
    assert index.filtered_stats() == (16, 0, 0)
    index.set_option("filter_tiles", 1)
    index.set_option("list_cap", 4)
    c = _check(index, q, 100, packed, want, qm, "overflow")
    assert index.filtered_stats()[0] > 0
    assert {"filtered", "large_k"} <= index.last_dispatch()["kernels"]
    _exact(a, b)
    _exact(a, c)
    index.set_option("list_cap", 0)
    ones = np.ones(16, np.int32)
    _exact(index.search_filtered(q, 100, packed, ones), index.search(q, 100))
    _exact(_device(index, q, 100, packed, ones), index.search(q, 100))
    index.close()


# --------------------------------------------------------------- 7. census skip
def test_census_skip(gpu):
    """20 tiles, a mask that allows only documents of tile 3: pass A skips the
    other 19 tiles of every query (filtered_stats()[1] == Q * 19) and the
    results are exact."""
    rng = np.random.default_rng(7)
    N, V = 20 * TILE, 100
    ip, ix, dt = _rand_index(rng, N, V, 5000)
    q = rng.integers(-1, V, size=(9, 8)).astype(np.int32)
    rows = _dense_rows(N, ip, ix, dt, q)
    allow = np.zeros((1, N), bool)
    allow[0, 3 * TILE:4 * TILE] = rng.random(TILE) < 0.7
    allow[0, [3 * TILE, 4 * TILE - 1]] = True
    index = _idx(ip, ix, dt, N)
    assert index.info()["n_tiles"] == 20
    got = _check(index, q, 50, _pack(allow), _want(rows, 50, allow))
    assert ((got[0] >= 3 * TILE) & (got[0] < 4 * TILE)).all()
    stats = index.filtered_stats()
    assert stats[1] == len(q) * 19, stats
    assert stats[2] <= len(q)
    index.close()


# ---------------------------------------------------------- 8. doc shards compose
def test_doc_shards_compose(gpu):
    """One index split at document 4096 into two shards (doc_offset), the
    second allowing fewer than k documents: each shard's filtered list from
    its slice of the mask, merged by the existing merge_topk_device, equals
    the single index's filtered result."""
    import torch
    from bm25mi.index import merge_topk_device
    rng = np.random.default_rng(8)
    N, V, cut, k = 9000, 80, 2 * TILE, 40
    ip, ix, dt = _rand_index(rng, N, V, 3000, signed=True, coarse=True)
    q = rng.integers(-1, V, size=(6, 8)).astype(np.int32)
    rows = _dense_rows(N, ip, ix, dt, q)
    allow = np.zeros((1, N), bool)
    allow[0, :cut] = rng.random(cut) < 0.2
    allow[0, rng.choice(np.arange(cut, N), 17, replace=False)] = True   # 17 < k
    want = _want(rows, k, allow)
    full = _idx(ip, ix, dt, N)
    _check(full, q, k, _pack(allow), want)
    dq = torch.from_numpy(q).cuda()
    outs_d = torch.full((2, len(q), k), 99, dtype=torch.int32, device="cuda")
    outs_s = torch.full((2, len(q), k), 7.5, dtype=torch.float32, device="cuda")
    shards = []
    for r, (lo, hi) in enumerate(((0, cut), (cut, N))):
        sh = _idx(*_doc_slice(ip, ix, dt, lo, hi), hi - lo, doc_offset=lo)
        shards.append(sh)
        dm = torch.from_numpy(_pack(allow[:, lo:hi]).view(np.int32)).cuda()
        sh.search_filtered_device(dq, k, dm, None, outs_d[r], outs_s[r],
                                  torch.cuda.current_stream())
    torch.cuda.synchronize()
    second = outs_d[1].cpu().numpy()
    assert (second[:, :17] >= cut).all() and (second[:, 17:] == -1).all()
    md = torch.empty((len(q), k), dtype=torch.int32, device="cuda")
    ms = torch.empty((len(q), k), dtype=torch.float32, device="cuda")
    merge_topk_device(0, outs_d, outs_s, 2, len(q), k, md, ms, torch.cuda.current_stream())
    torch.cuda.synchronize()
    _exact((md.cpu().numpy(), ms.cpu().numpy()), want)
    for sh in shards:
        sh.close()
    full.close()
