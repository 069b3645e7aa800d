"""CPU tests of tests/wide_cases.py: the sparse reference the wide GPU tests
(tests/test_gpu_wide.py) compare with, and the generator of their indexes.

ref_search and its siblings equal, bit for bit, what the suite already trusts
at the widths those references reach — oracle.search_c for the plain search,
and the dense numpy references of the filtered, weighted, cursor, term-mask,
min-match, hit-count and score_docs tests — on wide_csc and on
test_gpu_parity._rand_index data, signed and non-negative, at k around the
number of touched documents, with all-padding rows, duplicate terms, zero-fill
rows and stored -0.0f.

The 30 720-tile case of the GPU tests must stay on the tile-bound threshold
through a whole sweep: a search whose candidate lists overflow turns that
threshold off for the handle's next searches (bound_weak).
test_cap_case_lists_fit_their_capacity checks with the bounds model that, for
every query of that sweep, fewer documents reach the threshold than a list
holds."""
import functools

import numpy as np
import pytest

import mask_model as mm
import select_cases
import wide_cases as wc
from oracle import oracle
from test_bounds_model import _f16_down
from test_gpu_min_match import _bits as dense_bits
from test_gpu_min_match import _want as dense_min_match
from test_gpu_parity import _rand_index
from test_gpu_score_docs import _want as dense_score_docs
from test_gpu_search_filtered import _want as dense_filtered
from test_gpu_term_masks import _has_of
from test_gpu_term_masks import _want as dense_term_masks
from test_search_after_host import ref_after as dense_after
from test_search_weighted_host import ref_rows as dense_weighted_rows

N_DOCS = (1, 33, 2049, 70_001)
KINDS = [("wide", False), ("wide", True), ("rand", False), ("rand", True)]
NEG_ZERO = 0x80000000


def _same(got, want, what=""):
    assert got[0].shape == want[0].shape, what
    assert np.array_equal(got[0], want[0]), (what, got[0], want[0])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), (what, got[1], want[1])


@functools.lru_cache(maxsize=None)
def case(n_docs, kind, signed):
    """(indptr, indices, data, queries [Q, 8]) read-only.  Queries: an
    all-padding row, one term in every slot, a term twice among others, ids
    past the vocabulary, a row of the rarest terms (zero fill)."""
    if kind == "wide":
        ip, ix, dt = wc.wide_csc(n_docs, 11 + n_docs, signed)
        q = np.concatenate([wc.wide_queries(8), wc.wide_queries(8, seed=1)[6:]])
        q[-1, 5] = q[-1, 4]                       # a repeated id among others
        q[-2, 7] = wc.V + 3                       # an id past the vocabulary: padding
    else:
        rng = np.random.default_rng(50 + n_docs + signed)
        nv = 40
        ip, ix, dt = _rand_index(rng, n_docs, nv, min(n_docs, 3000), signed=signed, coarse=True)
        dt[::7] = np.float32(-0.0)                # stored -0.0f: touched, and it adds nothing
        q = rng.integers(-1, nv, size=(9, 8)).astype(np.int32)
        q[0, :] = -1
        q[1, :] = 5
        q[2, 3] = q[2, 6] = 9
        q[3, :] = np.argsort(np.diff(ip))[:8]     # the rarest terms: zero fill
        q[4, 1] = nv + 1
    for a in (ip, ix, dt, q):
        a.setflags(write=False)
    return ip, ix, dt, q


def _ks(n_touched, n_docs, cap=None):
    ks = {1, 10, n_touched - 1, n_touched, n_touched + 1, n_docs}
    return sorted(k for k in ks if 1 <= k <= (cap or n_docs))


# ---------------------------------------------------------------- the search
@pytest.mark.parametrize("kind,signed", KINDS)
@pytest.mark.parametrize("n_docs", N_DOCS)
def test_plain_search_is_the_oracle(n_docs, kind, signed):
    ip, ix, dt, q = case(n_docs, kind, signed)
    assert (dt.view(np.uint32) == NEG_ZERO).any() or (kind, signed) == ("wide", False)
    assert signed == bool((dt < 0).any())
    rows = wc.ref_rows(ip, ix, dt, q)
    assert len(rows[0][0]) == 0                   # the all-padding row touches nothing
    seen_fill = False
    for r in range(len(q)):
        ids, sc = rows[r]
        dense = oracle.scores_dense_c(n_docs, ip, ix, dt, np.where(q[r] < len(ip) - 1, q[r], -1))
        assert np.array_equal(dense[ids].view(np.uint32), sc.view(np.uint32))
        assert not (sc.view(np.uint32) == NEG_ZERO).any()
        seen_fill |= 0 < len(ids) < min(10, n_docs)
        qr = np.where(q[r:r + 1] < len(ip) - 1, q[r:r + 1], -1)   # (the C oracle rejects such ids)
        for k in _ks(len(ids), n_docs):
            got = wc.ref_search(n_docs, ip, ix, dt, q[r:r + 1], k)
            _same(got, oracle.search_c(n_docs, ip, ix, dt, qr, k), (r, k))
            _same(wc.ref_search(n_docs, ip, ix, dt, q[r:r + 1], k, rows=rows[r:r + 1]), got)
    assert seen_fill or n_docs < 10 or kind == "rand"
    # the batch form: every row at once
    qq = np.where(q < len(ip) - 1, q, -1)
    k = min(10, n_docs)
    _same(wc.ref_search(n_docs, ip, ix, dt, q, k), oracle.search_c(n_docs, ip, ix, dt, qq, k))


def _masks(n_docs, seed):
    """bool [6, n_docs]: half, only the last document, only document 0, every
    third, every document, a range."""
    rng = np.random.default_rng(seed)
    d = np.arange(n_docs)
    return np.stack([rng.random(n_docs) < 0.5, d == n_docs - 1, d == 0, d % 3 == 0,
                     np.ones(n_docs, bool), (d >= n_docs // 3) & (d < n_docs // 3 + 40)])


@pytest.mark.parametrize("kind,signed", KINDS)
@pytest.mark.parametrize("n_docs", N_DOCS)
def test_filtered_search_is_the_dense_reference(n_docs, kind, signed):
    import bm25mi
    ip, ix, dt, q = case(n_docs, kind, signed)
    qq = np.where(q < len(ip) - 1, q, -1)
    dense = [oracle.scores_dense_c(n_docs, ip, ix, dt, row) for row in qq]
    allow = _masks(n_docs, n_docs)
    packed = bm25mi.pack_mask(allow)
    assert np.array_equal(packed[4], wc.all_ones(n_docs))
    assert np.array_equal(packed[5], wc.range_words(n_docs, n_docs // 3, n_docs // 3 + 40))
    assert np.array_equal(packed[3], wc.ids_to_words(n_docs, np.arange(0, n_docs, 3)))
    rows = wc.ref_rows(ip, ix, dt, q)
    for m in range(len(allow)):
        n_allowed = int(allow[m].sum())
        garbage = packed[m].copy()
        if n_docs % 32:
            garbage[-1] |= np.uint32((0xFFFFFFFF << (n_docs % 32)) & 0xFFFFFFFF)
        for k in _ks(n_allowed, n_docs, cap=n_allowed + 1) + [n_allowed + 12]:
            want = dense_filtered(dense, k, allow[m:m + 1])
            _same(wc.ref_search(n_docs, ip, ix, dt, q, k, allow=packed[m], rows=rows), want, (m, k))
            _same(wc.ref_search(n_docs, ip, ix, dt, q, k, allow=garbage, rows=rows), want, (m, k))
            _same(wc.ref_search(n_docs, ip, ix, dt, q, k, allow=lambda i, a=allow[m]: a[i],
                                rows=rows), want, (m, k))
    # one mask per query, None among them
    per = [None if r % 3 == 0 else packed[r % len(packed)] for r in range(len(q))]
    qm = np.array([-1 if r % 3 == 0 else r % len(packed) for r in range(len(q))], np.int32)
    k = min(10, n_docs)
    _same(wc.ref_search(n_docs, ip, ix, dt, q, k, allow=per, rows=rows),
          dense_after(dense, k, None, allow, qm))


def _weights(q, seed):
    rng = np.random.default_rng(seed)
    w = (np.exp2(rng.uniform(-3.0, 3.0, q.shape)) * rng.choice([-1.0, 1.0], q.shape))
    w = w.astype(np.float32)
    w[rng.random(q.shape) < 0.15] = 0.0            # a weight of 0.0 is padding
    w[q < 0] = np.nan                              # (not read)
    return w


def _cursors(dense, allow, qm, k, doc_offset):
    """Cursor vectors (scores [Q], docs [Q]) over the dense rows: the key of
    rank 1, of rank k, of the last allowed document; inside the +0.0 band; a
    score no document has; +inf; a document below doc_offset; exhausted and
    AFTER_NONE mixed in."""
    first = dense_after(dense, k, None, allow, qm, doc_offset)
    Q, n = len(dense), len(dense[0])
    f32, i32 = (lambda v: np.array(v, np.float32)), (lambda v: np.array(v, np.int32))
    col = lambda j: (f32([first[1][r, min(j, k - 1)] for r in range(Q)]),
                     i32([first[0][r, min(j, k - 1)] for r in range(Q)]))
    whole = dense_after(dense, n, None, allow, qm, doc_offset)
    last = [int((whole[0][r] >= 0).sum()) - 1 for r in range(Q)]
    out = [col(0), col(k - 1),
           (f32([whole[1][r, max(last[r], 0)] for r in range(Q)]),
            i32([whole[0][r, max(last[r], 0)] for r in range(Q)])),
           (np.zeros(Q, np.float32), i32([doc_offset + n // 2] * Q)),
           (f32([0.0103] * Q), i32([doc_offset] * Q)),
           (f32([np.inf] * Q), i32([doc_offset] * Q)),
           (col(0)[0], i32([max(doc_offset - 7, 0)] * Q))]
    s, d = col(1)
    d = d.copy()
    d[::3] = wc.AFTER_NONE
    d[1::3] = -1
    out.append((s, d))
    # a page that ended in padding: its last column is (NaN bits, -1), the exhausted cursor
    out.append((np.full(Q, np.nan, np.float32), np.full(Q, -1, np.int32)))
    return out


@pytest.mark.parametrize("kind,signed", KINDS)
@pytest.mark.parametrize("n_docs", N_DOCS)
def test_weighted_and_cursor_search_is_the_dense_reference(n_docs, kind, signed):
    import bm25mi
    ip, ix, dt, q = case(n_docs, kind, signed)
    qq = np.where(q < len(ip) - 1, q, -1)
    allow = _masks(n_docs, 3 * n_docs)[[0, 3]]
    packed = bm25mi.pack_mask(allow)
    qm = np.array([(-1, 0, 1)[r % 3] for r in range(len(q))], np.int32)
    per = [None if m < 0 else packed[m] for m in qm]
    k = min(10, n_docs)
    for weighted in (False, True):
        w = _weights(q, n_docs) if weighted else None
        dense = (dense_weighted_rows(n_docs, ip, ix, dt, qq, w) if weighted else
                 [oracle.scores_dense_c(n_docs, ip, ix, dt, row) for row in qq])
        rows = wc.ref_rows(ip, ix, dt, q, w)
        for r, (ids, sc) in enumerate(rows):
            assert np.array_equal(dense[r][ids].view(np.uint32), sc.view(np.uint32))
        for off in (0, 2 ** 31 - n_docs):
            for al, am, aq in ((None, None, None), (per, allow, qm)):
                kw = dict(weights=w, allow=al, doc_offset=off, rows=rows)
                # pages: each page's last column is the next one's cursor
                after = None
                for _ in range(4):
                    got = wc.ref_search(n_docs, ip, ix, dt, q, k, after=after, **kw)
                    _same(got, dense_after(dense, k, after, am, aq, off), (weighted, off))
                    after = (np.ascontiguousarray(got[1][:, -1]), np.ascontiguousarray(got[0][:, -1]))
                for i, cur in enumerate(_cursors(dense, am, aq, k, off)):
                    if off and i == 6:
                        assert (cur[1] < off).all()
                    live = cur[1] >= 0
                    if np.isnan(cur[0][live]).any():
                        continue
                    got = wc.ref_search(n_docs, ip, ix, dt, q, k, after=cur, **kw)
                    _same(got, dense_after(dense, k, cur, am, aq, off), (weighted, off, i))
                    if off:
                        assert int(got[0].max()) <= wc.INT32_MAX


# ---------------------------------------------------------------- the siblings
@pytest.mark.parametrize("kind,signed", [("wide", False), ("rand", True)])
@pytest.mark.parametrize("n_docs", N_DOCS)
def test_term_masks_min_match_and_counts_are_the_dense_references(n_docs, kind, signed):
    import bm25mi
    ip, ix, dt, _ = case(n_docs, kind, signed)
    nv = len(ip) - 1
    has = _has_of(ip, ix, nv, n_docs)
    big = int(np.argmax(np.diff(ip)))
    must = [[big], [0, 1], [], [], [2], [-1, -1], [nv + 2], [], [3, 3]]
    any_ = [[], [], [4, 5, 6], [7, 7, 8, 9], [10, 11, 12], [-1], [], [nv + 2, 4], [4, 5, 5, 6]]
    mnot = [[], [2], [], [0], [13, 14], [-1], [], [], [big]]
    M = len(must)
    base_b = _masks(n_docs, 9)[[0]]
    base = bm25mi.pack_mask(base_b)
    for b_b, b in ((None, None), (base_b, base)):
        want = dense_term_masks(has, must, any_, mnot, M, b_b)
        got = wc.ref_term_masks(n_docs, ip, ix, must, any_, mnot, b)
        assert np.array_equal(got, want)
        for need in (np.array([0, 1, 2, 2, 3, 1, 1, 1, 3]), 2):
            mmv = np.broadcast_to(np.asarray(need), (M,))
            want = dense_min_match(has, must, any_, mnot, mmv, M, b_b)
            got = wc.ref_term_masks(n_docs, ip, ix, must, any_, mnot, b, min_match=need)
            assert np.array_equal(got, want)
    rows = wc.ref_term_masks(n_docs, ip, ix, [[t] for t in range(nv)])
    assert np.array_equal(wc.ref_mask_count(n_docs, rows), np.diff(ip))
    assert np.array_equal(wc.ref_mask_count(n_docs, want), dense_bits(want, n_docs))
    tail = wc.all_ones(n_docs, garbage_tail=True)
    assert (tail == 0xFFFFFFFF).all()
    assert wc.ref_mask_count(n_docs, tail)[0] == n_docs == wc.ref_mask_count(
        n_docs, wc.all_ones(n_docs))[0]
    assert np.array_equal(wc.ref_mask_count(n_docs, np.stack([tail, rows[0]])),
                          dense_bits(np.stack([tail, rows[0]]), n_docs))


@pytest.mark.parametrize("kind,signed", KINDS)
@pytest.mark.parametrize("n_docs", N_DOCS)
def test_score_docs_is_the_dense_reference(n_docs, kind, signed):
    ip, ix, dt, q = case(n_docs, kind, signed)
    qq = np.where(q < len(ip) - 1, q, -1)
    rng = np.random.default_rng(n_docs)
    for off in (0, 2 ** 31 - n_docs):
        docs = rng.integers(0, n_docs, size=(len(q), 12)).astype(np.int64) + off
        docs[:, 0], docs[:, 1] = off, off + n_docs - 1
        docs[:, 2] = -1                                         # padding
        for r, (ids, _) in enumerate(wc.ref_rows(ip, ix, dt, q)):
            docs[r, 3:3 + min(len(ids), 4)] = ids[:4] + off     # touched documents
        docs = docs.astype(np.int32)
        want = dense_score_docs(n_docs, ip, ix, dt, qq, docs, off)
        got = wc.ref_score_docs(n_docs, ip, ix, dt, q, docs, doc_offset=off)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # ids of another shard score +0.0
    out = np.array([[n_docs, n_docs + 5]] * len(q), np.int64)
    if n_docs + 5 <= wc.INT32_MAX:
        assert not wc.ref_score_docs(n_docs, ip, ix, dt, q, out).view(np.uint32).any()


# ---------------------------------------------------------------- the generator
@pytest.mark.parametrize("signed", [False, True])
@pytest.mark.parametrize("n_docs", [wc.CAP, wc.CAP1, wc.C5, wc.MAX1, wc.MAX, 70_001, 2049, 33, 1])
def test_wide_csc_carries_the_edges(n_docs, signed):
    ip, ix, dt = wc.wide_csc(n_docs, 3, signed)
    nt = wc.n_tiles(n_docs)
    assert len(ip) == wc.V + 1 and ip[-1] <= 2_100_000 and ix.dtype == np.int32
    assert int(ix.min()) == 0 and int(ix.max()) == n_docs - 1
    col = lambda t: ix[ip[t]:ip[t + 1]].astype(np.int64)
    for t in range(wc.V):
        assert (np.diff(col(t)) > 0).all(), t            # canonical: sorted, no repeats
    edges = wc.edge_docs(n_docs)
    want = {0, n_docs - 1, min(wc.TILE, n_docs) - 1, (nt - 1) * wc.TILE}
    if nt > wc.BOUND_MAX_TILES:
        want |= {wc.CAP - wc.TILE, wc.CAP - 1, wc.CAP, min(wc.CAP + wc.TILE, n_docs) - 1}
    assert want <= set(edges.tolist())
    if nt >= 8:   # both sides of a pooled-group boundary
        t = edges // wc.TILE
        assert any(a % wc.POOL == wc.POOL - 1 and a + 1 in t for a in t.tolist())
    for t in (0, wc.EDGE_LO, wc.EDGE_HI):
        assert np.isin(edges, col(t)).all(), t
    assert n_docs - 1 in col(wc.ZFILL) and ip[wc.ZFILL + 1] - ip[wc.ZFILL] == min(7, n_docs)
    assert (np.diff(ip)[:wc.N_COMMON] >= min(n_docs // 4, 140_000)).all()
    neg = float((dt < 0).mean())
    assert (0.3 < neg < 0.37 or n_docs < 100) if signed else neg == 0
    assert bool((dt.view(np.uint32) == NEG_ZERO).any()) == signed
    if signed or len(edges) < 2 * wc.N_TOP:
        return
    # the tie runs at the two ends of the id space, ranked by id
    q = wc.wide_queries(8)
    k = len(edges)
    d, s = wc.ref_search(n_docs, ip, ix, dt, q[1:3], k)
    assert (s[:, :wc.N_TOP] == 7.0).all() and (s[:, wc.N_TOP:] == 3.0).all()
    assert d[0, 0] == 0 and d[0, -1] == n_docs - 1 and (np.diff(d[0]) > 0).all()
    assert d[1, wc.N_TOP - 1] == n_docs - 1 and d[1, wc.N_TOP] == 0
    assert (np.diff(d[1, :wc.N_TOP]) > 0).all() and (np.diff(d[1, wc.N_TOP:]) > 0).all()
    d, s = wc.ref_search(n_docs, ip, ix, dt, q[3:4], 10)
    assert (s[0, :7] > 0).all() and d[0, 7:].tolist() == [0, 1, 2] and not s[0, 7:].any()


def list_capacity(k: int) -> int:
    """A query's candidate-list capacity at the handle's default list_cap = 0
    (list_cap_for): 64 k within 2048 .. 65 536."""
    return min(65_536, max(2048, 64 * k))


@functools.lru_cache(maxsize=None)
def cap_case():
    ip, ix, dt = wc.wide_csc(wc.CAP, 1)
    for a in (ip, ix, dt):
        a.setflags(write=False)
    return ip, ix, dt


CAP_T = (1, 8, 12)   # the query widths of the sweep that the tile-bound threshold serves


def test_cap_case_lists_fit_their_capacity():
    """For every query of the GPU sweep at 30 720 tiles and k in {1, 10, 30, 100}:
    the documents at or above the tile-bound threshold — per tile and pooled
    over groups of 4 — are fewer than the candidate list holds, so no search
    of the sweep overflows and the handle keeps the bound path (bound_weak
    stays off).  The threshold is the bounds model's (mask_model.theta_bound
    over f16 maxima rounded down)."""
    ip, ix, dt = cap_case()
    assert wc.n_tiles(wc.CAP) == wc.BOUND_MAX_TILES
    bmax, _ = mm.tables(ip, ix, dt, wc.CAP)
    # the tables' f16 maxima are the bounds model's, on a term with postings in few tiles
    col = lambda t: (ix[ip[t]:ip[t + 1]], dt[ip[t]:ip[t + 1]])
    for t in (0, wc.EDGE_HI, wc.RARE0):
        m = np.zeros(wc.BOUND_MAX_TILES, np.float32)
        np.maximum.at(m, col(t)[0] // wc.TILE, col(t)[1])
        lb = bmax[t].view(np.float16).astype(np.float32)
        assert np.array_equal(_f16_down(m), lb)
        assert np.array_equal(select_cases.tile_bounds(*col(t), wc.BOUND_MAX_TILES), lb)
    worst = 0.0
    for T in CAP_T:
        q = wc.wide_queries(T)
        rows = wc.ref_rows(ip, ix, dt, q)
        for k in (1, 10, 30, 100):   # (30: the k of the paging test's whole list)
            cap = list_capacity(k)
            for r in range(len(q)):
                sc = rows[r][1]
                for pool in (False, True):
                    theta = mm.theta_bound(bmax, q[r], k, pool)
                    n = int((sc >= theta).sum())
                    worst = max(worst, n / cap)
                    if T == 1 and r:     # one term: the selection model's list length
                        assert n == select_cases.list_count(col(int(q[r].max())), k,
                                                            wc.BOUND_MAX_TILES, pool), (r, k, pool)
                    assert n < cap, (T, k, r, pool, float(theta), n, cap)
                # the pooled threshold is the looser one, and both are lower bounds
                assert mm.theta_bound(bmax, q[r], k, True) <= mm.theta_bound(bmax, q[r], k, False)
                if len(sc) >= k:
                    assert mm.theta_bound(bmax, q[r], k, False) <= np.sort(sc)[-k]
    print(f"  fullest list: {worst:.2f} of its capacity")
    assert wc.BOUND_MAX_TILES >= 16 * 100 and (wc.BOUND_MAX_TILES + 3) // 4 >= 8 * 100
