"""The document axis at its limits, on the GPU: the tile-bound threshold's
last width (30 720 tiles) and the first one past it, config 5's collection on
one handle, the widest index (65 536 tiles: tile id 65 535 in the sparse
table's u16, mask rows of 4 194 304 words) and doc ids up to 2^31 - 1.

Every result is compared bit for bit with the sparse reference of
tests/wide_cases.py (held to the C oracle by tests/test_wide_model.py); the
indexes are wide_csc's — about 2 M postings whatever the width — built once
per (n_docs, segment table, doc_offset) and shared by the tests of this
module."""
import functools
import itertools

import numpy as np
import pytest

import wide_cases as wc
from test_gpu_parity import _exact, _idx, _world_bounds_search

pytestmark = pytest.mark.gpu

TILE = wc.TILE
WIDTHS = {"cap": wc.CAP, "cap+1": wc.CAP1, "c5": wc.C5, "max-1": wc.MAX1, "max": wc.MAX}
TILES = {"cap": 30_720, "cap+1": 30_721, "c5": 48_829, "max-1": 65_536, "max": 65_536}
SEGMENTS = ("dense", "sparse")
SEED = 1                       # (tests/test_wide_model.py checks the cap case of this seed)
SMALL = 70_001
OPTS = ("theta_bound", "tile_bound", "bound_pool", "tile_mask", "seg_skip")


# ------------------------------------------------------------ shared state
@functools.lru_cache(maxsize=None)
def _csc(n_docs):
    arrays = wc.wide_csc(n_docs, SEED)
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _rows(n_docs, T):
    q = wc.wide_queries(T)
    q.setflags(write=False)
    return q, wc.ref_rows(*_csc(n_docs), q)


@functools.lru_cache(maxsize=None)
def _ref(n_docs, T, k):
    q, rows = _rows(n_docs, T)
    return wc.ref_search(n_docs, *_csc(n_docs), q, k, rows=rows)


class _Pool:
    """GpuIndex handles by (n_docs, segments, doc_offset), closed with the module."""

    def __init__(self):
        self.handles = {}

    def get(self, n_docs, segments, doc_offset=0):
        key = (n_docs, segments, doc_offset)
        if key not in self.handles:
            self.handles[key] = _idx(*_csc(n_docs), n_docs, doc_offset=doc_offset,
                                     segments=segments)
        return self.handles[key]

    def close(self):
        for h in self.handles.values():
            h.close()
        self.handles.clear()


@pytest.fixture(scope="module")
def pool(gpu):
    p = _Pool()
    yield p
    p.close()


def _bits(a, b, what=""):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    bad = np.flatnonzero(np.ascontiguousarray(a).view(np.uint32).ravel()
                         != np.ascontiguousarray(b).view(np.uint32).ravel())
    assert bad.size == 0, (what, f"{bad.size} words differ, first at {bad[0]}")


# ---------------------------------------------------------- 1. create limits
def test_create_limits(pool):
    """65 537 tiles and a doc id past 2^31 - 1 are rejected with the reason;
    the next create works; every width reports the tiles it should."""
    from bm25mi.index import GpuIndex
    ip, ix, dt = _csc(SMALL)
    q = wc.wide_queries(8)
    want = wc.ref_search(SMALL, ip, ix, dt, q, 10)
    one = (np.array([0, 1], np.int64), np.zeros(1, np.int32), np.ones(1, np.float32))
    with pytest.raises(ValueError, match=r"65537 tiles"):
        GpuIndex(*one, wc.MAX + 1)
    index = _idx(ip, ix, dt, SMALL)
    _exact(index.search(q, 10), want)
    index.close()
    off = 2 ** 31 - SMALL
    with pytest.raises(ValueError, match=r"doc_offset"):
        GpuIndex(ip, ix, dt, SMALL, doc_offset=off + 1)
    with pytest.raises(ValueError, match=r"int32"):
        GpuIndex(*one, 2 ** 31)
    index = _idx(ip, ix, dt, SMALL, doc_offset=off)
    got = index.search(q, 10)
    _exact(got, wc.ref_search(SMALL, ip, ix, dt, q, 10, doc_offset=off))
    assert int(got[0].max()) == wc.INT32_MAX
    index.close()
    for name, n in WIDTHS.items():
        info = pool.get(n, "dense").info()
        assert info["n_tiles"] == TILES[name] == wc.n_tiles(n) and info["n_docs"] == n, (name, info)
        assert info["tile_bounds"] and not info["sparse"], (name, info)


# ----------------------------------------------------------- 2. plain search
def _dispatch_ok(index, name, segments, T, theta_bound, pool_opt):
    d = index.last_dispatch()
    assert "bound_off" not in d["kernels"], (name, d)
    bound = name == "cap" and segments == "dense" and theta_bound and T <= 16
    if bound:
        assert d["sample_p"] == 0 and "bound_keys" in d["kernels"], (name, T, d)
        assert ("bound_pool" in d["kernels"]) == bool(pool_opt), (name, T, pool_opt, d)
    else:
        assert d["sample_p"] > 1 and "bound_keys" not in d["kernels"], (name, T, d)
        assert "bound_pool" not in d["kernels"], (name, T, d)
    return d


@pytest.mark.parametrize("segments", SEGMENTS)
@pytest.mark.parametrize("name", list(WIDTHS))
def test_plain_search(pool, name, segments):
    """k in {1, 10, 100} at every width: the reference's bits under every
    setting of the threshold and tile-bound options, the tile-bound threshold
    (bound_keys, pooled and per tile) at 30 720 tiles and the sampled one at
    every wider index, and never a threshold the handle turned off."""
    n = WIDTHS[name]
    index = pool.get(n, segments)
    assert index.get_option("list_cap") == 0      # (the capacity test_wide_model.py assumes)
    q, _ = _rows(n, 8)
    combos = list(itertools.product((1, 0), repeat=len(OPTS))) if segments == "dense" else [(1,) * 5]
    for k in (1, 10, 100):
        want = _ref(n, 8, k)
        for combo in combos:
            for o, v in zip(OPTS, combo):
                index.set_option(o, v)
            _exact(index.search(q, k), want)
            d = _dispatch_ok(index, name, segments, 8, combo[0], combo[2])
            if segments == "dense" and d["sample_p"] == 0:
                assert d["tile_skip"] == bool(combo[1]), (combo, d)
    for o in OPTS:
        index.set_option(o, 1)


@pytest.mark.parametrize("segments", SEGMENTS)
@pytest.mark.parametrize("T", [1, 12, 70])
@pytest.mark.parametrize("name", ["cap", "max"])
def test_plain_search_query_widths(pool, name, segments, T):
    """T = 1 and 12 (the flat kernel at 8 and 16 term lanes) and 70 (the wave
    kernel); T = 8 is test_plain_search's."""
    n = WIDTHS[name]
    index = pool.get(n, segments)
    q, _ = _rows(n, T)
    for k in (10, 100):
        _exact(index.search(q, k), _ref(n, T, k))
        d = _dispatch_ok(index, name, segments, T, 1, 1)
        flat = {"flat_rest", "flat_all"} <= d["kernels"]
        wave = {"wave_rest", "wave_all"} <= d["kernels"]
        assert (flat, wave) == (T <= 64, T > 64), (T, d)
        if T <= 16:
            assert d["term_lanes"] == (8 if T <= 8 else 16), d


def test_skipped_tiles_are_counted(pool):
    """count_skips at 30 720 tiles (the tile-bound threshold) and at 65 536
    (a sampled threshold of stride 64 with two keys per sample tile, so REST
    reads the pre-pass's bits rather than the sample keys): the pre-pass ran
    and REST skipped (query, tile) pairs by its bits."""
    for name, k, opts in (("cap", 10, {}), ("max", 600, {"sample_p": 64})):
        n = WIDTHS[name]
        index = pool.get(n, "dense")
        q, _ = _rows(n, 8)
        sample_p = index.get_option("sample_p")
        for o, v in dict(opts, count_skips=1).items():
            index.set_option(o, v)
        try:
            _exact(index.search(q, k), _ref(n, 8, k))
            d, st = index.last_dispatch(), index.search_stats()
            print(f"  {name}: k={k} dispatch {d} stats {st}")
            assert d["tile_skip"] and "bound_off" not in d["kernels"], d
            assert d["sample_p"] == (0 if name == "cap" else 64), d
            assert 0 < st["bound_skipped_tiles"] <= len(q) * TILES[name], st
            assert st["bound_skipped_postings"] > 0, st
        finally:
            index.set_option("count_skips", 0)
            index.set_option("sample_p", sample_p)
        _exact(index.search(q, k), _ref(n, 8, k))


# --------------------------------------------------------------- 3. large k
@pytest.mark.parametrize("segments", SEGMENTS)
def test_large_k(pool, segments):
    """k = 4097 and 5000 on config 5's 100 M documents: the list path, then
    the dense rows (large_lists = 0: a row stride of 48 829 tiles x 2048
    floats); a row with fewer than k touched documents zero-fills."""
    n = wc.C5
    index = pool.get(n, segments)
    q8, rows8 = _rows(n, 8)
    pick = [5, 6]
    q = np.ascontiguousarray(q8[pick])
    rows = [rows8[r] for r in pick]
    assert len(rows[0][0]) < 4097 < len(rows[1][0])
    for k in (4097, 5000):
        want = wc.ref_search(n, *_csc(n), q, k, rows=rows)
        assert (want[1][0, -1] == 0) and want[1][1, -1] > 0
        for lists in (1, 0):
            index.set_option("large_lists", lists)
            try:
                _exact(index.search(q, k), want)
                d, st = index.last_dispatch(), index.search_stats()
                assert "large_k" in d["kernels"], d
                if lists:
                    assert 0 <= st["large_dense_queries"] <= len(q), st
                    assert "flat_rest" in d["kernels"], d
                else:
                    assert st["large_dense_queries"] == -1, st
                    assert "flat_rest" not in d["kernels"], d
            finally:
                index.set_option("large_lists", 1)


# -------------------------------------------------------- 4. filtered search
def _wide_masks(n):
    """uint32 [6, W] built as words: every document; only the last; only
    document 0; a range across tiles 30 719 | 30 720; every 97th document;
    every document with the bits past n_docs set too.  And the documents each
    allows."""
    lo, hi = wc.CAP - 1000, min(wc.CAP + 1000, n)
    m = np.stack([wc.all_ones(n), wc.ids_to_words(n, [n - 1]), wc.ids_to_words(n, [0]),
                  wc.range_words(n, lo, hi), wc.ids_to_words(n, np.arange(0, n, 97)),
                  wc.all_ones(n, garbage_tail=True)])
    allowed = [n, 1, 1, hi - lo, (n + 96) // 97, n]
    return m, allowed


@functools.lru_cache(maxsize=None)
def _masks_of(n):
    m, allowed = _wide_masks(n)
    m.setflags(write=False)
    return m, tuple(allowed)


@pytest.mark.parametrize("segments", SEGMENTS)
@pytest.mark.parametrize("name", ["cap+1", "max-1"])
def test_filtered_search(pool, name, segments):
    """Six masks built as words, two queries under each in one batch: the tile
    passes and the dense path (filter_tiles = 0) give the reference's bits at
    k = 1, 100 and around the small masks' allowed counts; the census skips
    every tile the range mask leaves empty."""
    n = WIDTHS[name]
    index = pool.get(n, segments)
    masks, allowed = _masks_of(n)
    assert n % 32 and (masks[5, -1] >> np.uint32(n % 32)) != 0 and masks[0, -1] != masks[5, -1]
    assert np.array_equal(wc.ref_mask_count(n, masks), allowed)
    q8, rows8 = _rows(n, 8)
    pick = [2, 6]                                  # EDGE_HI alone (the last ids); common + rare
    M = len(masks)
    q = np.ascontiguousarray(np.concatenate([q8[pick]] * M + [q8[pick]]))
    rows = [rows8[r] for r in pick] * (M + 1)
    qm = np.concatenate([np.repeat(np.arange(M), 2), [-1, -1]]).astype(np.int32)
    allow = [None if m < 0 else masks[m] for m in qm]
    assert len(q) <= 16
    ks = sorted({1, 100} | {a + d for a in allowed if a < 10_000 for d in (-1, 0, 1) if a + d >= 1})
    assert ks == ([1, 2, 100, 1999, 2000, 2001] if name == "max-1" else
                  [1, 2, 100, 1000, 1001, 1002]), ks
    for k in ks:
        want = wc.ref_search(n, *_csc(n), q, k, allow=allow, rows=rows)
        got = index.search_filtered(q, k, masks, qm)
        _exact(got, want)
        assert "filtered" in index.last_dispatch()["kernels"]
        _exact((got[0][0:2], got[1][0:2]), (got[0][10:12], got[1][10:12]))   # the garbage tail
        if k in (1, 100, allowed[3]):
            index.set_option("filter_tiles", 0)
            try:
                _exact(index.search_filtered(q, k, masks, qm), want)
                assert "large_k" in index.last_dispatch()["kernels"]
                assert index.filtered_stats()[0] >= 2 * M and index.filtered_stats()[1] == 0
            finally:
                index.set_option("filter_tiles", 1)
    # the range mask alone: the census leaves two tiles
    got = index.search_filtered(q[:2], 100, masks[3:4])
    _exact(got, wc.ref_search(n, *_csc(n), q[:2], 100, allow=masks[3], rows=rows[:2]))
    stats = index.filtered_stats()
    assert stats[0] == 0 and stats[1] == 2 * (TILES[name] - 2), stats


# ------------------------------------- 5. term masks, min-match, hit counts
CLAUSES = dict(
    must=[[0], [wc.EDGE_LO], [], [1, 2], [wc.ZFILL], []],
    any=[[], [2, 3], [4, 5, 6, wc.RARE0], [wc.RARE0 + 1, wc.RARE0 + 2], [], [7, 8, 8, 9]],
    must_not=[[], [wc.EDGE_HI], [0], [], [3], [wc.RARE0 + 4]],
)
NEED = np.array([0, 1, 2, 1, 1, 3], np.int32)
COUNT_TERMS = [0, 1, 11, wc.EDGE_LO, wc.EDGE_HI, wc.RARE0, 30, wc.ZFILL]


@pytest.mark.parametrize("segments", SEGMENTS)
@pytest.mark.parametrize("name", ["cap+1", "max-1", "max"])
def test_term_masks_and_counts(pool, name, segments):
    """term_masks and its min-match form equal the word-array model over the
    whole row (4 194 304 words at the widest); mask_count of every document
    is n_docs (2^27 at the widest index: no wider total exists), with or
    without garbage past n_docs, and a term's mask counts its postings."""
    n = WIDTHS[name]
    index = pool.get(n, segments)
    ip, ix, dt = _csc(n)
    base = np.stack([wc.range_words(n, 5, n - 3)])
    for b in (None, base):
        _bits(index.term_masks(base=b, **CLAUSES), wc.ref_term_masks(n, ip, ix, base=b, **CLAUSES),
              (name, "term_masks"))
        _bits(index.term_masks(base=b, min_match=NEED, **CLAUSES),
              wc.ref_term_masks(n, ip, ix, base=b, min_match=NEED, **CLAUSES), (name, "min_match"))
    ones = np.stack([wc.all_ones(n), wc.all_ones(n, garbage_tail=True)])
    assert index.mask_count(ones).tolist() == [n, n]
    assert n < 2 ** 27 or name == "max"
    tm = index.term_masks(must=[[t] for t in COUNT_TERMS])
    assert index.mask_count(tm).tolist() == np.diff(ip)[COUNT_TERMS].tolist()
    _bits(tm[3], wc.term_words(n, ip, ix, wc.EDGE_LO))
    assert wc.bits_of(tm[3], [0, n - 1]).all() and wc.bits_of(tm[7], [n - 1]).all()


@pytest.mark.parametrize("segments", SEGMENTS)
@pytest.mark.parametrize("name", ["cap+1", "max-1"])
def test_boolean_search_with_totals(pool, name, segments):
    """search_boolean(total_hits=True) is the filtered search under the same
    masks, and its totals are their counts."""
    n = WIDTHS[name]
    index = pool.get(n, segments)
    ip, ix, dt = _csc(n)
    q8, rows8 = _rows(n, 8)
    M = len(NEED)
    pick = [1, 2, 4, 5, 6, 7]
    q = np.ascontiguousarray(q8[pick])
    rows = [rows8[r] for r in pick]
    masks = wc.ref_term_masks(n, ip, ix, min_match=NEED, **CLAUSES)
    for k in (10, 100):
        want = wc.ref_search(n, ip, ix, dt, q, k, allow=list(masks), rows=rows)
        docs, scores, totals = index.search_boolean(q, k, min_match=NEED, total_hits=True, **CLAUSES)
        _exact((docs, scores), want)
        assert totals.tolist() == wc.ref_mask_count(n, masks).tolist()
        _exact(index.search_filtered(q, k, masks, np.arange(M, dtype=np.int32)), want)


# ------------------------------------------------------------ 6. score_docs
@pytest.mark.parametrize("segments", SEGMENTS)
def test_score_docs(pool, segments):
    """Given documents at both ends of the id space and on the edges of tiles
    0 | 1 and 30 719 | 30 720 of the widest index, absent ones and padding:
    the reference's sums, and the bits the search reports for its results."""
    n = wc.MAX
    index = pool.get(n, segments)
    q, rows = _rows(n, 8)
    fixed = [0, TILE - 1, TILE, wc.CAP - 1, wc.CAP, n - 1, -1, 12_345_679, n - 2, -7]
    docs = np.array([fixed] * len(q), np.int64)
    top = _ref(n, 8, 10)
    docs = np.concatenate([docs, top[0].astype(np.int64)], axis=1).astype(np.int32)
    want = wc.ref_score_docs(n, *_csc(n), q, docs, rows=rows)
    assert (want[1:3, :6] > 0).all() and not want[1:6, 6:10].any()   # the edge terms' documents
    _bits(index.score_docs(q, docs), want)
    got = index.search(q, 10)
    _exact(got, top)
    s = index.score_docs(q, got[0])
    _bits(s, got[1])


# ---------------------------------------------------------- 7. search_after
def _last_positive(rows):
    """Per row the cursor on its last-ranked positive document (AFTER_NONE
    for a row without one)."""
    s = np.zeros(len(rows), np.float32)
    d = np.full(len(rows), wc.AFTER_NONE, np.int32)
    for r, (ids, sc) in enumerate(rows):
        pos = sc > 0
        if pos.any():
            s[r] = sc[pos].min()
            d[r] = ids[pos & (sc == s[r])].max()
    return s, d


def _cursor_on(rows, doc, doc_offset=0):
    """Per row the cursor (the row's score of ``doc``, doc)."""
    s = np.zeros(len(rows), np.float32)
    for r, (ids, sc) in enumerate(rows):
        hit = np.flatnonzero(ids == doc)
        if hit.size:
            s[r] = sc[hit[0]]
    return s, np.full(len(rows), doc + doc_offset, np.int32)


@pytest.mark.parametrize("segments", SEGMENTS)
@pytest.mark.parametrize("name", ["cap", "max"])
def test_search_after(pool, name, segments):
    """Three pages of 10 are the search of 30 (the edge terms' tie runs cross
    the page edges); cursors on the last positive document and on document
    n_docs - 1 inside its tie run; the same with weights of both signs and
    under a mask."""
    n = WIDTHS[name]
    index = pool.get(n, segments)
    ip, ix, dt = _csc(n)
    q, rows = _rows(n, 8)
    k = 10
    whole = index.search(q, 3 * k)
    _exact(whole, _ref(n, 8, 3 * k))
    assert whole[1][1, 9] == whole[1][1, 10] == 3.0      # a tie run across the first page edge
    assert whole[1][4, 19] == whole[1][4, 20] > 0        # ... and across the second
    rng = np.random.default_rng(8)
    w = (np.exp2(rng.uniform(-2, 2, q.shape)) * rng.choice([-1.0, 1.0], q.shape)).astype(np.float32)
    w[1:6] = np.abs(w[1:6])                         # the fixed rows keep their order
    wrows = wc.ref_rows(ip, ix, dt, q, w)
    assert any((sc < 0).any() and (sc > 0).any() for _, sc in wrows)
    mask = wc.ids_to_words(n, np.concatenate([np.arange(0, n, 97), wc.edge_docs(n)]))[None, :]
    for weights, masks, rr in ((None, None, rows), (w, None, wrows), (w, mask, wrows)):
        kw = dict(weights=weights, allow=None if masks is None else masks[0], rows=rr)
        pages, after = [], None
        for _ in range(3):
            got = index.search_after(q, k, after, weights=weights, masks=masks)
            _exact(got, wc.ref_search(n, ip, ix, dt, q, k, after=after, **kw))
            assert "after" in index.last_dispatch()["kernels"]
            pages.append(got)
            after = (np.ascontiguousarray(got[1][:, -1]), np.ascontiguousarray(got[0][:, -1]))
        cat = (np.concatenate([p[0] for p in pages], 1), np.concatenate([p[1] for p in pages], 1))
        _exact(cat, wc.ref_search(n, ip, ix, dt, q, 3 * k, **kw))
        if weights is None:
            _exact(cat, whole)
        for cur in (_last_positive(rr), _cursor_on(rr, n - 1)):
            got = index.search_after(q, k, cur, weights=weights, masks=masks)
            _exact(got, wc.ref_search(n, ip, ix, dt, q, k, after=cur, **kw))
    # document n_docs - 1 ends the 7.0 run of EDGE_HI: the 3.0 run follows, from document 0
    got = index.search_after(q, k, _cursor_on(rows, n - 1))
    assert got[1][2, 0] == 3.0 and got[0][2, 0] == 0 and (got[0][0] == -1).all()


# ------------------------------------------------------------ 8. scores_dense
@pytest.mark.parametrize("segments", SEGMENTS)
def test_scores_dense(pool, segments):
    """One query's 134 217 728 sums: non-zero exactly on the reference's
    touched documents, with its bits, the last element among them."""
    n = wc.MAX
    index = pool.get(n, segments)
    ip, ix, dt = _csc(n)
    row = np.array([0, wc.EDGE_LO, wc.EDGE_HI, wc.RARE0 + 5, 3, -1, 7, wc.ZFILL], np.int32)
    ids, sc = wc.touched(ip, ix, dt, row)
    out = index.scores_dense(row)
    assert out.shape == (n,) and out.dtype == np.float32
    nz = np.flatnonzero(out.view(np.uint32))
    assert np.count_nonzero(out) == len(ids) == len(nz)
    assert np.array_equal(nz, ids)
    _bits(out[nz], sc)
    assert out[n - 1] == sc[-1] == np.float32(1.0 + 3.0 + 7.0 + 2.5) and ids[-1] == n - 1
    assert out[0] == sc[0] and ids[0] == 0


# -------------------------------------------------- 9. the top of the id space
@pytest.mark.parametrize("segments", SEGMENTS)
@pytest.mark.parametrize("n", [SMALL, wc.MAX])
def test_ids_up_to_int32_max(pool, n, segments):
    """doc_offset = 2^31 - n_docs: the last document is INT32_MAX.  Plain,
    filtered and weighted search, score_docs on global ids, and cursors at
    (score, INT32_MAX) inside a tie run, below doc_offset and exhausted."""
    off = 2 ** 31 - n
    index = pool.get(n, segments, doc_offset=off)
    ip, ix, dt = _csc(n)
    q, rows = _rows(n, 8)
    kw = dict(doc_offset=off, rows=rows)
    for k in (10, 100):
        got = index.search(q, k)
        _exact(got, wc.ref_search(n, ip, ix, dt, q, k, **kw))
    assert got[0][2, wc.N_TOP - 1] == wc.INT32_MAX and got[0].min() >= off
    mask = wc.ids_to_words(n, np.concatenate([np.arange(0, n, 97), wc.edge_docs(n)]))[None, :]
    _exact(index.search_filtered(q, 10, mask), wc.ref_search(n, ip, ix, dt, q, 10, allow=mask[0], **kw))
    rng = np.random.default_rng(9)
    w = (np.exp2(rng.uniform(-2, 2, q.shape)) * rng.choice([-1.0, 1.0], q.shape)).astype(np.float32)
    wrows = wc.ref_rows(ip, ix, dt, q, w)
    _exact(index.search_weighted(q, w, 10),
           wc.ref_search(n, ip, ix, dt, q, 10, weights=w, doc_offset=off, rows=wrows))
    docs = np.array([[off, off + TILE - 1, off + TILE, wc.INT32_MAX, wc.INT32_MAX - 1, -1,
                      off + n // 2]] * len(q), np.int32)
    want = wc.ref_score_docs(n, ip, ix, dt, q, docs, **kw)
    assert want[2, 3] == 7.0 and want[1, 0] == 7.0
    _bits(index.score_docs(q, docs), want)
    # cursors
    top = _cursor_on(rows, n - 1, off)
    assert (top[1] == wc.INT32_MAX).all() and top[0][2] == 7.0
    below = (np.full(len(q), 7.0, np.float32), np.full(len(q), off - 5, np.int32))
    done = (np.zeros(len(q), np.float32), np.full(len(q), -1, np.int32))
    zero_top = (np.zeros(len(q), np.float32), np.full(len(q), wc.INT32_MAX, np.int32))
    for cur in (top, below, done, zero_top):
        got = index.search_after(q, 10, cur)
        _exact(got, wc.ref_search(n, ip, ix, dt, q, 10, after=cur, **kw))
        assert (got[0] >= off).all() or (got[0][got[0] < off] == -1).all()
    got = index.search_after(q, 10, top)
    assert got[1][2, 0] == 3.0 and got[0][2, 0] == off          # nothing at 7.0 follows INT32_MAX
    assert (index.search_after(q, 10, zero_top)[0] == -1).all()  # ... and nothing at +0.0
    got = index.search_after(q, 10, below)
    assert got[0][2, :wc.N_TOP].tolist() == (wc.edge_docs(n)[-wc.N_TOP:] + off).tolist()


def test_shards_merge_at_int32_max(gpu):
    """Two doc shards, the upper one ending at INT32_MAX: their lists merged
    by merge_topk_device and merge_sorted_device are the collection's result,
    ties across the shard edge ranked by global id."""
    import torch
    from bm25mi.index import merge_sorted_device, merge_topk_device
    n, cut = 2 * SMALL, SMALL
    base = 2 ** 31 - n
    ip, ix, dt = _csc(n)
    q, rows = _rows(n, 8)
    shards = [_idx(*wc.doc_slice(ip, ix, dt, lo, hi), hi - lo, doc_offset=base + lo)
              for lo, hi in ((0, cut), (cut, n))]
    Q = len(q)
    for k in (10, 100):
        want = wc.ref_search(n, ip, ix, dt, q, k, doc_offset=base, rows=rows)
        assert (want[0][2] < base + cut).any() and (want[0][2] >= base + cut).any()
        assert want[1][2, wc.N_TOP] == want[1][2, 9] == 3.0       # a tie run below the upper shard's
        parts = [s.search(q, k) for s in shards]
        d = torch.from_numpy(np.stack([p[0] for p in parts])).cuda()
        s = torch.from_numpy(np.stack([p[1] for p in parts])).cuda()
        for merge in ("topk", "sorted"):
            od = torch.empty((Q, k), dtype=torch.int32, device="cuda")
            os_ = torch.empty((Q, k), dtype=torch.float32, device="cuda")
            if merge == "topk":
                merge_topk_device(0, d, s, 2, Q, k, od, os_)
            else:
                merge_sorted_device(0, d, s, 2, Q, k, Q * k, od, os_)
            torch.cuda.synchronize()
            _exact((od.cpu().numpy(), os_.cpu().numpy()), want)
        assert int(want[0].max()) == wc.INT32_MAX
    for s in shards:
        s.close()


# ------------------------------------------------ 10. world bounds at the cap
@pytest.mark.parametrize("name", ["cap", "cap+1"])
def test_world_bounds_at_the_cap(gpu, name):
    """Two doc shards under the world's tile bounds.  15 360 + 15 360 tiles:
    the collection's 30 720 tiles take the world threshold (bound_keys over
    both shards' rows, pooled and per tile).  15 360 + 15 361: one tile too
    many for the world threshold — each shard falls back to its own geometry
    (its own tile-bound threshold).  Both merge to the reference."""
    import torch
    n = WIDTHS[name]
    cut = 15_360 * TILE
    ip, ix, dt = _csc(n)
    q, _ = _rows(n, 8)
    shards = [_idx(*wc.doc_slice(ip, ix, dt, lo, hi), hi - lo, doc_offset=lo, segments="dense")
              for lo, hi in ((0, cut), (cut, n))]
    assert [s.info()["n_tiles"] for s in shards] == [15_360, TILES[name] - 15_360]
    dq = torch.from_numpy(q.copy()).cuda()
    for k in (10, 100):
        for pool_opt in (1, 0):
            for s in shards:
                s.set_option("bound_pool", pool_opt)
            _exact(_world_bounds_search(shards, dq, k), _ref(n, 8, k))
            for s in shards:
                d = s.last_dispatch()
                assert d["sample_p"] == 0 and "bound_keys" in d["kernels"], (name, d)
                assert "bound_off" not in d["kernels"], (name, d)
                assert ("bound_pool" in d["kernels"]) == bool(pool_opt), (name, pool_opt, d)
    for s in shards:
        s.close()


# ------------------------------------------- 11. handles of different widths
def test_handles_across_widths(gpu):
    """One process: the widest index, a small one, the widest again — each
    created after the one before it is destroyed, each searched plain,
    filtered and at a k that grows the candidate buffers."""
    for n in (wc.MAX, SMALL, wc.MAX):
        ip, ix, dt = _csc(n)
        q, rows = _rows(n, 8)
        index = _idx(ip, ix, dt, n, segments="dense")
        for k in (10, 1000, 10):
            want = _ref(n, 8, k)
            _exact(index.search(q, k), want)
        mask = wc.ids_to_words(n, np.arange(0, n, 97))[None, :]
        _exact(index.search_filtered(q, 10, mask),
               wc.ref_search(n, ip, ix, dt, q, 10, allow=mask[0], rows=rows))
        _exact(index.search(q, 100), _ref(n, 8, 100))
        index.close()
