"""GPU tests of the sort-by-field search (bm25_sort_ranks(_device),
bm25_search_sorted(_device), bm25_search_boolean_sorted; bm25mi_sorted.hip).

The expected orders and rows come from numpy (tests/sorted_model.py: np.lexsort
for the order, the unpacked mask AND rank > after for the rows); they never go
through the code under test, and every comparison is exact.  Every selection
runs through the host call and through the device call — a non-default stream,
outputs pre-filled with a marker between guard words, scratch of exactly
bm25_search_sorted_scratch's size with marked guard bytes behind it.  The
constants as built (bm25mi_internal.h) and the shapes that sit next to them:

  32      documents per mask word: n_docs 31, 32, 33
  64      documents of a step (one ballot): n_docs 63, 64, 65
  256     kSortedSpanDocs, documents of a wave's span: n_docs 255, 256, 257
  1024    kSortedRoundDocs, a workgroup's round, and the slice of documents of
          a workgroup at these sizes (a slice is whole rounds; it only grows
          past 8 workgroups per CU): n_docs 1023, 1024, 1025
  2048    kSortedWmax, the interval width that is collected: n_docs 2047 and
          2048 take no level, 2049 takes one
  256     kSortedBins, automatic bins per level: 256 x 2048 = 524 288 documents
          take one level, 524 289 take two; "sorted_bins" 2, 3 and 64 at 5000
          documents take 2, 1 and 1 levels
  32      kSortedRows, mask rows of a row block: M 1, 32, 33, 64, 65; M =
          65 537 at 40 documents passes a 16-bit grid
  4096    the largest k, at 5000 documents: a list of up to 5000 ranks sorted
          in LDS (kSortedSortP = 8192)
  4096    pairs of a radix-sort tile (the rank build): n_docs 4095, 4097"""
import ctypes

import numpy as np
import pytest

from facets_model import facets_want, unpack_rows
from range_model import pack_rows, range_allowed
from sorted_model import order_want, select_want
from test_gpu_parity import _idx, _rand_index
from test_gpu_term_masks import _has_of, _want

pytestmark = pytest.mark.gpu

MARK_I32 = 0xA5A5A5A5 - (1 << 32)
GUARD = 64


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None


@pytest.fixture(scope="module")
def make(gpu):
    """index_of(n_docs): a handle over n_docs documents (one term, one
    posting: the sorted calls read the caller's buffers only)."""
    made = {}

    def index_of(n_docs, doc_offset=0):
        if (n_docs, doc_offset) not in made:
            made[n_docs, doc_offset] = _idx(np.array([0, 1], np.int64), np.zeros(1, np.int32),
                                            np.ones(1, np.float32), n_docs, doc_offset=doc_offset)
        return made[n_docs, doc_offset]
    yield index_of
    for ix in made.values():
        ix.close()


def _garbage_tail(packed, n_docs):
    """Every bit at or past n_docs set (garbage that must not count)."""
    packed = packed.copy()
    if n_docs % 32:
        packed[:, -1] |= np.uint32((0xFFFFFFFF << (n_docs % 32)) & 0xFFFFFFFF)
    return packed


def _host_raw(index, masks, M, ranks, perm, k, after):
    """bm25_search_sorted into marked buffers with guard entries."""
    from bm25mi._capi import check, lib
    docs = np.full(M * k + GUARD, MARK_I32, np.int32)
    out = np.full(M * k + GUARD, MARK_I32, np.int32)
    check(lib.bm25_search_sorted(index._h, _p(masks), M, _p(ranks), _p(perm), k, _p(after),
                                 _p(docs), _p(out)))
    assert (docs[M * k:] == MARK_I32).all() and (out[M * k:] == MARK_I32).all(), "guards written"
    return docs[:M * k].reshape(M, k).copy(), out[:M * k].reshape(M, k).copy()


def _device_raw(index, masks, M, ranks, perm, k, after):
    """search_sorted_device on a non-default stream: marked outputs between
    guard words, scratch of exactly the reported size with guard bytes behind."""
    import torch
    st = torch.cuda.Stream()
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dm = None if masks is None else dev(masks.view(np.int32))
    dr, dp, da = dev(ranks), dev(perm), dev(after)
    bufs = [torch.full((GUARD + M * k + GUARD,), MARK_I32, dtype=torch.int32, device="cuda")
            for _ in range(2)]
    need = index.sorted_scratch_bytes(M, k)
    n = index.n_docs
    assert need == 4 * M * (4 + 1 + 256 + min(k + 2048, n))
    scratch = torch.full((need + 256,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # (the uploads ran on the current stream)
    index.search_sorted_device(dm, dr, dp, k, da, bufs[0][GUARD:GUARD + M * k].view(M, k),
                               bufs[1][GUARD:GUARD + M * k].view(M, k),
                               scratch[:need] if masks is not None else None, st)
    st.synchronize()
    assert (scratch[need:] == 0x5A).all().item(), "bytes behind the scratch written"
    got = []
    for b in bufs:
        a = b.cpu().numpy()
        assert (a[:GUARD] == MARK_I32).all() and (a[GUARD + M * k:] == MARK_I32).all(), \
            "guard words written"
        got.append(a[GUARD:GUARD + M * k].reshape(M, k).copy())
    return tuple(got)


def _check(index, allowed, order, k, after=None, what="", tail=True):
    """Host call and device call both give the model's rows; returns them.
    allowed: bool [M, n_docs], or an int M (masks = NULL)."""
    ranks, perm = order
    n = index.n_docs
    if isinstance(allowed, (int, np.integer)):
        masks, M = None, int(allowed)
    else:
        masks = pack_rows(allowed)
        if tail:
            masks = _garbage_tail(masks, n)
        M = masks.shape[0]
    after = None if after is None else np.ascontiguousarray(after, dtype=np.int32)
    want = select_want(allowed, ranks, perm, k, after, index.doc_offset)
    for name, call in (("device", _device_raw), ("host", _host_raw)):
        got = call(index, masks, M, ranks, perm, k, after)
        for g, w, part in zip(got, want, ("docs", "ranks")):
            bad = np.nonzero(g != w)
            assert bad[0].size == 0, (what, name, part, f"{bad[0].size} entries differ, first row "
                                      f"{bad[0][0]} col {bad[1][0]}: got {g[bad][0]} want "
                                      f"{w[bad][0]}")
    return want


def _order(rng, n, kind=np.int32, span=None):
    """A random column with ties and its model order."""
    v = rng.integers(0, span or max(2, n // 3), size=n).astype(kind)
    return order_want(v, bool(rng.integers(0, 2)))


# ------------------------------------------------------------------ 1. rank build
def _build_both(index, values, descending):
    import torch
    got = [index.sort_ranks(values, descending)]
    st = torch.cuda.Stream()
    dv = torch.from_numpy(values).cuda()
    n = values.shape[0]
    dr = torch.full((n + GUARD,), MARK_I32, dtype=torch.int32, device="cuda")
    dp = torch.full((n + GUARD,), MARK_I32, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    index.sort_ranks_device(dv, dr[:n], dp[:n], descending, st)
    a, b = dr.cpu().numpy(), dp.cpu().numpy()   # (the call synchronised its stream)
    assert (a[n:] == MARK_I32).all() and (b[n:] == MARK_I32).all(), "guard words written"
    got.append((a[:n].copy(), b[:n].copy()))
    return got


def _rank_cases(dtype):
    rng = np.random.default_rng(11)
    nan, inf = np.float32("nan"), np.float32("inf")
    if np.dtype(dtype).kind == "f":
        special = np.array([nan, inf, -inf, 0.0, -0.0, 1.0, -1.0, np.float32(1e-45),
                            np.float32(-1e-45), np.float32(3.4e38), nan], np.float32)
        yield "nan inf zero mixed", special[rng.integers(0, special.size, 4097)]
        yield "random", rng.standard_normal(5000).astype(np.float32).round(1)
        yield "all nan", np.full(70, nan, np.float32)
    else:
        info = np.iinfo(dtype)
        lim = np.array([info.min, info.max, info.min + 1, info.max - 1, 0, -1, 1], dtype)
        yield "limits", lim[rng.integers(0, lim.size, 4095)]
        yield "random", rng.integers(-50, 50, 5000).astype(dtype)
        if dtype == np.int64:
            a = 2 ** 53
            yield "2^53", np.array([a + 1, a, a + 1, a, -a, -a - 1, a + 2] * 10, np.int64)
            yield "high words", (rng.integers(-3, 3, 600).astype(np.int64) << 40) + rng.integers(0, 3, 600)
    yield "all equal", np.full(300, 7).astype(dtype)
    yield "two values", (rng.integers(0, 2, 1025) * 5 - 2).astype(dtype)
    yield "one document", np.array([3]).astype(dtype)


@pytest.mark.parametrize("dtype", [np.int32, np.float32, np.int64])
def test_rank_build(make, dtype):
    """The three kinds, both directions, host and device calls: perm and ranks
    equal the model's, and ranks[perm] == arange."""
    for what, values in _rank_cases(dtype):
        index = make(values.shape[0])
        for desc in (False, True):
            want = order_want(values, desc)
            for got in _build_both(index, values, desc):
                assert got[0].dtype == np.int32 and got[1].dtype == np.int32
                assert np.array_equal(got[1], want[1]), (what, desc, "perm")
                assert np.array_equal(got[0], want[0]), (what, desc, "ranks")
                assert np.array_equal(got[0][got[1]], np.arange(values.shape[0])), (what, desc)


# ------------------------------------------------------------ 2. the document axis
@pytest.mark.parametrize("n_docs", [1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025,
                                    2047, 2048, 2049, 4097])
def test_document_axis(make, n_docs):
    """Word, step, span, round and Wmax edges; rows: random at three
    densities, all ones, all zeros, only the last document; garbage in the
    tail bits; k = 1, 7 (or n_docs) and n_docs (capped at 4096)."""
    rng = np.random.default_rng(n_docs)
    order = _order(rng, n_docs)
    allowed = np.stack([rng.random(n_docs) < 0.5, rng.random(n_docs) < 0.05,
                        rng.random(n_docs) < 0.9, np.ones(n_docs, bool), np.zeros(n_docs, bool),
                        np.arange(n_docs) == n_docs - 1])
    for k in sorted({1, min(7, n_docs), min(n_docs, 4096)}):
        want = _check(make(n_docs), allowed, order, k, what=(n_docs, k))
        assert (want[0][4] == -1).all() and want[0][5][0] == n_docs - 1
        assert np.array_equal(want[0][3], order[1][:k])
    _check(make(n_docs), 3, order, min(n_docs, 9), [-2, min(4, n_docs - 1), -1], "no masks")


@pytest.mark.parametrize("n_docs", [524_288, 524_289])
def test_two_automatic_levels(make, n_docs):
    """256 bins x 2048 ranks: one level up to 524 288 documents, two past it.
    A column that grows with the doc id (a step's documents share a bin), a
    random one, and the rows that stress a level: exactly k and k - 1 allowed
    documents, one contiguous rank interval in the middle."""
    rng = np.random.default_rng(n_docs)
    k = 100
    for v in ((np.arange(n_docs) // 3).astype(np.int32), rng.integers(0, 1000, n_docs).astype(np.int32)):
        order = order_want(v, True)
        ranks = order[0]
        exact = np.zeros((2, n_docs), bool)
        exact[0, rng.choice(n_docs, k, replace=False)] = True
        exact[1, rng.choice(n_docs, k - 1, replace=False)] = True
        mid = (ranks >= 200_000) & (ranks < 300_001)
        allowed = np.vstack([rng.random((2, n_docs)) < [[0.5], [0.001]], exact, mid[None, :]])
        want = _check(make(n_docs), allowed, order, k, [-2, -2, -2, -2, 250_000], n_docs)
        assert (want[1][2] >= 0).all() and want[1][3][-1] == -1 and want[1][3][-2] >= 0
        assert np.array_equal(want[1][4], np.arange(250_001, 250_001 + k))


# --------------------------------------------------------------------- 3. the rows
@pytest.mark.parametrize("M", [1, 32, 33, 64, 65])
def test_row_blocks(make, M):
    """A single row, a full block, a row over, two blocks and one row, at 2500
    documents (one level; W = 79, odd); every row has its own density and
    cursor."""
    n_docs, k = 2500, 20
    rng = np.random.default_rng(M)
    order = _order(rng, n_docs)
    allowed = rng.random((M, n_docs)) < rng.random((M, 1))
    after = rng.integers(-2, n_docs, M)
    want = _check(make(n_docs), allowed, order, k, after, M)
    assert M < 3 or len({w.tobytes() for w in want[0]}) > M // 2


def test_more_rows_than_65535(make):
    """65 537 rows at 40 documents, with and without masks."""
    n_docs, M, k = 40, 65_537, 5
    rng = np.random.default_rng(5)
    order = _order(rng, n_docs)
    allowed = rng.random((M, n_docs)) < 0.3
    after = rng.integers(-2, n_docs, M)
    want = _check(make(n_docs), allowed, order, k, after)
    assert (want[0][65_536:] >= 0).any() and (want[0][:65_536] >= 0).any()
    _check(make(n_docs), M, order, k, after, "no masks")


def test_largest_k(make):
    """k = 4096 at 5000 documents: dense rows (the list holds all 5000 ranks'
    worth), a row with exactly k and one with k - 1 allowed documents."""
    n_docs, k = 5000, 4096
    rng = np.random.default_rng(6)
    order = _order(rng, n_docs)
    allowed = np.ones((4, n_docs), bool)
    allowed[1] = rng.random(n_docs) < 0.95
    allowed[2] = False
    allowed[2, rng.choice(n_docs, k, replace=False)] = True
    allowed[3] = False
    allowed[3, rng.choice(n_docs, k - 1, replace=False)] = True
    want = _check(make(n_docs), allowed, order, k, what="k 4096")
    assert (want[1][2] >= 0).all() and want[1][3][-1] == -1 and want[1][3][-2] >= 0
    _check(make(n_docs), allowed, order, k, [700, 100, 30, -1], "k 4096 with cursors")


# ------------------------------------------------------------------ 4. paging
def test_pages_concatenate(make):
    """Pages of 1, 7 and k, each continued from the last ranks column, equal
    the one-shot list; a padded page's cursor gives an all-padding row; -2 is
    no cursor."""
    n_docs, total = 3000, 42
    rng = np.random.default_rng(7)
    index = make(n_docs, 1000)
    order = _order(rng, n_docs)
    allowed = np.stack([rng.random(n_docs) < 0.3, rng.random(n_docs) < 0.01, np.ones(n_docs, bool)])
    allowed[1, np.flatnonzero(allowed[1])[30:]] = False       # 30 allowed: the list ends early
    one = _check(index, allowed, order, total, what="one shot")
    assert (one[0][0] >= 1000).all() and one[0][1][30] == -1 and one[0][1][29] >= 1000
    for page in (1, 7, total):
        after = np.full(3, -2, np.int32)
        docs, ranks = [], []
        for _ in range(total // page):
            d, r = _check(index, allowed, order, page, after, ("page", page))
            docs.append(d)
            ranks.append(r)
            after = r[:, -1]
        assert np.array_equal(np.hstack(docs), one[0]) and np.array_equal(np.hstack(ranks), one[1])
    d, r = index.search_sorted(allowed, order, 5, np.array([-1, -2, -1]))
    assert (d[[0, 2]] == -1).all() and (r[[0, 2]] == -1).all()
    assert np.array_equal(d[1], one[0][1][:5])


# ------------------------------------------------------------------ 5. the option
def test_sorted_bins(make):
    """"sorted_bins" 2, 3 and 64 at 5000 documents (2, 1 and 1 levels against
    the automatic 1) give the automatic result bit for bit."""
    n_docs, k = 5000, 50
    rng = np.random.default_rng(8)
    index = make(n_docs)
    order = _order(rng, n_docs)
    allowed = rng.random((40, n_docs)) < rng.random((40, 1))
    after = rng.integers(-2, n_docs // 2, 40)
    assert index.get_option("sorted_bins") == 0
    auto = _check(index, allowed, order, k, after, "automatic")
    try:
        for bins in (2, 3, 64, 256):
            index.set_option("sorted_bins", bins)
            got = _check(index, allowed, order, k, after, bins)
            assert np.array_equal(got[0], auto[0]) and np.array_equal(got[1], auto[1])
        with pytest.raises(ValueError, match="sorted_bins must be in 0..256"):
            index.set_option("sorted_bins", 257)
    finally:
        index.set_option("sorted_bins", 0)


# ------------------------------------------------------------ 6. errors of the C calls
def test_c_calls_reject_and_leave_outputs(make):
    """Every BM25_EINVAL the C calls find before device work, with the value
    named; the outputs stay as they were."""
    from bm25mi._capi import BM25_EINVAL, BM25_OK, lib
    n = 70
    index = make(n)
    h = index._h
    v = np.arange(n, dtype=np.int32)
    ranks, perm = order_want(v, True)
    masks = np.full((2, 3), 0xFFFFFFFF, np.uint32)
    docs = np.full((2, 3), 7, np.int32)
    out = np.full((2, 3), 7, np.int32)
    r2, p2 = np.full(n, 7, np.int32), np.full(n, 7, np.int32)
    nbytes = ctypes.c_int64(-7)

    def bad(rc, text):
        assert rc == BM25_EINVAL
        assert text in lib.bm25_last_error().decode(), lib.bm25_last_error()

    bad(lib.bm25_sort_ranks(h, _p(v), 3, 0, _p(r2), _p(p2)), "kind = 3: BM25_FIELD_I32 (0)")
    bad(lib.bm25_sort_ranks_device(h, _p(v), -1, 0, _p(r2), _p(p2), None), "kind = -1")
    bad(lib.bm25_sort_ranks(h, None, 0, 0, _p(r2), _p(p2)), "NULL values")
    bad(lib.bm25_sort_ranks(h, _p(v), 0, 0, None, _p(p2)), "NULL output")
    bad(lib.bm25_sort_ranks_device(h, _p(v), 0, 0, _p(r2), None, None), "NULL output")
    s = lambda m=masks, M=2, r=ranks, p=perm, k=3, a=None, d=docs, o=out: lib.bm25_search_sorted(
        h, _p(m), M, _p(r), _p(p), k, _p(a), _p(d), _p(o))
    bad(s(k=4097), "k = 4097: a sorted search returns at most 4096")
    bad(s(k=71), "k = 71 is above the index's 70 documents")
    bad(s(k=-1), "negative dimensions")
    bad(s(M=-1), "negative mask shape")
    bad(s(r=None), "NULL ranks or perm")
    bad(s(d=None), "NULL output")
    r = ranks.copy()
    r[5], r[9] = 70, -1
    bad(s(r=r), "ranks[5] = 70 is outside [0, 70)")
    r = ranks.copy()
    r[11] = r[40]
    bad(s(r=r), f"ranks[11] = {ranks[40]} but perm[{ranks[40]}] = 40: ranks and perm are not "
                "inverse permutations")
    bad(s(a=np.array([-2, -3], np.int32)), "after_ranks[1] = -3 is below BM25_AFTER_NONE (-2)")
    bad(lib.bm25_search_sorted_scratch(h, 2, 4097, ctypes.byref(nbytes)), "k = 4097")
    bad(lib.bm25_search_sorted_scratch(h, 2, 3, None), "NULL output")
    dev = lambda k=3, sc=None, nb=0, r=ranks: lib.bm25_search_sorted_device(
        h, _p(masks), 2, _p(r), _p(perm), k, None, _p(docs), _p(out), sc, nb, None)
    bad(dev(k=4097), "k = 4097")
    bad(dev(r=None), "NULL ranks or perm")
    need = index.sorted_scratch_bytes(2, 3)
    bad(dev(sc=ctypes.c_void_p(256), nb=need - 1), f"scratch of {need - 1} bytes: "
        f"bm25_search_sorted_scratch asks for {need}")
    bad(dev(), f"scratch of 0 bytes: bm25_search_sorted_scratch asks for {need}")
    # the one-call search
    q = np.zeros((2, 2), np.int32)
    anyc = np.zeros((2, 2), np.int32)
    scores = np.full((2, 3), 7.0, np.float32)
    b = lambda k=3, r=ranks, p=perm, a=None, o=out: lib.bm25_search_boolean_sorted(
        h, _p(q), 2, 2, k, None, 0, _p(anyc), 2, None, 0, None, None, 0, None, 0, None, 0, 0, None,
        None, None, 0, _p(docs), _p(scores), None, None, _p(r), _p(p), _p(a), _p(o))
    bad(b(p=None), "NULL perm")
    bad(b(o=None), "NULL output")
    r = ranks.copy()
    r[0] = r[1]
    bad(b(r=r), f"ranks[0] = {ranks[1]} but perm[{ranks[1]}] = 1")
    bad(b(a=np.array([-9, 0], np.int32)), "after_ranks[0] = -9")
    assert (docs == 7).all() and (out == 7).all() and (scores == 7.0).all()
    assert (r2 == 7).all() and (p2 == 7).all() and nbytes.value == -7
    # k == 0 and M == 0 return without device work or writes
    assert s(k=0) == BM25_OK and s(M=0) == BM25_OK and dev(k=0) == BM25_OK
    assert (docs == 7).all() and (out == 7).all()
    # a cursor below -2 is "no cursor" in the device call; ranks outside
    # [0, n_docs) are never eligible there
    r = ranks.copy()
    r[[3, 4]] = [n, -5]
    got = _device_raw(index, masks, 2, r, perm, 3, np.array([-7, -2], np.int32))
    elig = np.sort(r[(r >= 0) & (r < n)])[:3]
    assert np.array_equal(got[1], np.stack([elig, elig]))


# --------------------------------------------------------------- 7. one-call search
@pytest.fixture(scope="module")
def bool_case(gpu):
    """6000 documents, 60 terms, 7 queries with a term clause row and a range
    clause row each (the case of test_gpu_range_masks), the masks by numpy, on
    a handle with doc_offset 0 and one with 4000."""
    import bm25mi
    rng = np.random.default_rng(43)
    N, nt, G = 6000, 60, 11
    ip, ix, dt = _rand_index(rng, N, nt, 3000)
    by_df = np.argsort(-np.diff(ip))
    a, b, c, d = (int(x) for x in by_df[:4])
    has = _has_of(ip, ix, nt, N)
    q = rng.integers(-1, nt, size=(7, 8)).astype(np.int32)
    mu = [[a], [a, b], [], [], [c], [b, b], [-1]]
    an = [[], [c, d], [a, d], [], [a, b], [], [-1, -1]]
    mn = [[b], [], [c], [a], [d], [b], []]
    values = np.stack([rng.integers(1990, 2025, N), rng.integers(0, 500, N)]).astype(np.int32)
    rows = [{"year": (2000, 2010)}, {"price": (None, 250)}, {"year": (2015, None), "price": (100, 400)},
            {}, {"year": (2030, None)}, {"price": (0, 499)}, {"year": (1995, 2020), "price": (50, None)}]
    fields, lo, hi = bm25mi.range_rows(rows, ["year", "price"], np.int32)
    base = rng.random((1, N)) < 0.9
    terms = unpack_rows(_want(has, mu, an, mn, 7, base), N)
    allowed = terms & range_allowed(values, fields, lo, hi)
    allowed[3, np.flatnonzero(allowed[3])[6:]] = False
    base5 = np.broadcast_to(base, (7, N)).copy()
    base5[3] = allowed[3]              # query 3 keeps 6 documents: a padded row
    groups = rng.integers(-1, G, N).astype(np.int32)
    indexes = [_idx(ip, ix, dt, N), _idx(ip, ix, dt, N, doc_offset=4000)]
    yield indexes, q, (mu, an, mn), base5, (values, fields, lo, hi), allowed, groups, G
    for index in indexes:
        index.close()


def test_search_boolean_sorted(bool_case):
    """search_boolean(sort=...) rows equal the model on the numpy mask, scores
    equal score_docs' bits, tails are 0xFFFFFFFF / -1, totals and facets are
    unchanged by sort=, sort=None equals today's call, doc_offset gives global
    ids; once with bool_chunk = 1 (and 3: a short last chunk), once automatic."""
    indexes, q, (mu, an, mn), base, rng4, allowed, groups, G = bool_case
    price = rng4[0][1].astype(np.float32) / 4
    price[::17] = np.nan
    k = 10
    for index in indexes:
        order = index.sort_ranks(price, descending=True)
        assert np.array_equal(order[1], order_want(price, True)[1])
        after = np.array([-2, 40, -2, 3000, -2, -2, -1], np.int32)
        plain = index.search_boolean(q, k, mu, an, mn, base, total_hits=True, facets=(groups, G),
                                     ranges=rng4)
        assert np.array_equal(plain[2], allowed.sum(axis=1))
        assert np.array_equal(plain[3], facets_want(pack_rows(allowed), groups, G))
        try:
            for chunk in (1, 3, 0):
                index.set_option("bool_chunk", chunk)
                for aft in (None, after):
                    want = select_want(allowed, order[0], order[1], k, aft, index.doc_offset)
                    got = index.search_boolean(q, k, mu, an, mn, base, total_hits=True,
                                               facets=(groups, G), ranges=rng4, sort=order,
                                               after_ranks=aft)
                    assert len(got) == 5 and got[2].dtype == np.int32
                    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[1])
                    pad = want[0] < 0
                    if aft is None:  # 6 hits and a tail; no hit at all
                        assert pad[3, 6:].all() and not pad[3, :6].any() and pad[4].all()
                    sc = index.score_docs(q, np.where(pad, index.doc_offset, want[0]))
                    bits = np.where(pad, np.uint32(0xFFFFFFFF), sc.view(np.uint32))
                    assert np.array_equal(got[1].view(np.uint32), bits), chunk
                    assert np.array_equal(got[3], plain[2]) and np.array_equal(got[4], plain[3])
                got = index.search_boolean(q, k, mu, an, mn, base, sort=order, ranges=rng4)
                want = select_want(allowed, order[0], order[1], k, None, index.doc_offset)
                assert len(got) == 3 and np.array_equal(got[0], want[0])
        finally:
            index.set_option("bool_chunk", 0)
        # sort=None: today's call; k = 0 with sort: the counts alone
        again = index.search_boolean(q, k, mu, an, mn, base, total_hits=True, facets=(groups, G),
                                     ranges=rng4, sort=None)
        assert all(np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x,
                                  y.view(np.uint32) if y.dtype == np.float32 else y)
                   for x, y in zip(again, plain))
        got = index.search_boolean(q, 0, mu, an, mn, base, total_hits=True, ranges=rng4, sort=order)
        assert got[0].shape == (7, 0) and got[2].shape == (7, 0) and np.array_equal(got[3], plain[2])
        with pytest.raises(ValueError, match="k = 4097"):
            index.search_boolean(q, 4097, mu, an, mn, base, sort=order)


def test_native_passes_sort_through(bool_case):
    """bm25_native.BM25v.search_boolean passes sort= and after_ranks= on."""
    import bm25_native
    indexes, q, (mu, an, mn), base, rng4, allowed, groups, G = bool_case
    index = indexes[0]
    m = bm25_native.BM25v()
    m._gpu = index
    order = order_want(rng4[0][0], False)
    qq = np.where(q < 0, 0, q).astype(bm25_native.TokId)
    got = m.search_boolean(qq, 5, mu, an, mn, base, ranges=rng4, sort=order,
                           after_ranks=np.full(7, 10, np.int32))
    want = select_want(allowed, order[0], order[1], 5, np.full(7, 10))
    assert len(got) == 3 and np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[1])


# -------------------------------------------------------------------- 8. not a search
def test_not_a_search(bool_case):
    """After a search, sort_ranks and search_sorted (host and device calls)
    leave last_dispatch(), search_stats() and filtered_stats() as they were."""
    indexes, q, _, base, rng4, allowed, groups, G = bool_case
    index = indexes[0]
    index.search_filtered(q, 10, pack_rows(allowed), np.arange(7, dtype=np.int32))
    before = (index.last_dispatch(), index.search_stats(), index.filtered_stats())
    order = index.sort_ranks(rng4[0][0].astype(np.int64))
    _check(index, allowed, order, 10)
    assert (index.last_dispatch(), index.search_stats(), index.filtered_stats()) == before
