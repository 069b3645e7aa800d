"""GPU tests of the numeric range filters (bm25_range_masks(_device),
bm25_search_boolean_ranges; bm25mi_range.hip).

The expected masks come from numpy (tests/range_model.py: (v >= lo) & (v <= hi)
per clause in the column's dtype, ANDed with the unpacked base, packed with the
tail bits cleared); they never go through the code under test.  Every check
runs through the host call and through the device call (a non-default stream,
the out and base buffers one word off a 16-byte boundary), into word buffers
pre-filled with a marker that carry 64 guard words.  The kernel's constants as
built (bm25mi_internal.h) and the shapes that sit next to them:

  32      documents per mask word: n_docs 31, 32, 33
  64      documents of a step (one ballot): n_docs 63, 64, 65
  256     kRangeSpanDocs, documents of a wave's span (8 words a lane): n_docs
          255, 256, 257; a base row of zeros over documents 256 .. 511 skips a
          whole span of that row
  4096    kRangeChunkDocs, documents of a workgroup's chunk (4 waves x 4
          spans): n_docs 4095, 4097; 70 001 is 18 chunks, the last one short
  64      kRangeRows, mask rows of a row block (a lane per row): M 1, 64, 65,
          131 = 2 x 64 + 3; M = 65 537 at 40 documents passes a 16-bit grid
  2       kRangeCache, columns of a step kept in registers: rows that walk 3
          and more fields, and neighbours that name other fields, miss it
  8       kRangeRegClauses: up to 8 clauses a row stay in the lanes' registers,
          in kernels built for 1, 2, 4 and 8 of them (C 0 and 1; 2; 3 and 4;
          5 and 8); C = 9 and 70 take the kernel that reads them from memory"""
import ctypes

import numpy as np
import pytest

from facets_model import unpack_rows
from range_model import edge_case, pack_rows, range_allowed, range_want
from test_gpu_parity import _exact, _idx, _rand_index
from test_gpu_term_masks import _has_of, _want

pytestmark = pytest.mark.gpu

MARK = 0xA5A5A5A5
MARK_I32 = MARK - (1 << 32)
GUARD = 64
ROWS, SPAN, CHUNK = 64, 256, 4096


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None


@pytest.fixture(scope="module")
def make(gpu):
    """index_of(n_docs): a handle over n_docs documents (one term, one
    posting: the range calls read the caller's buffers only)."""
    made = {}

    def index_of(n_docs):
        if n_docs not in made:
            made[n_docs] = _idx(np.array([0, 1], np.int64), np.zeros(1, np.int32),
                                np.ones(1, np.float32), n_docs)
        return made[n_docs]
    yield index_of
    for ix in made.values():
        ix.close()


def _kind(values):
    return {np.dtype(np.int32): 0, np.dtype(np.float32): 1, np.dtype(np.int64): 2}[values.dtype]


def _host_raw(index, values, fields, lo, hi, base):
    """bm25_range_masks into a marked buffer with guard words."""
    from bm25mi._capi import check, lib
    M, C = fields.shape
    W = (index.n_docs + 31) // 32
    buf = np.full(M * W + GUARD, MARK, np.uint32)
    check(lib.bm25_range_masks(index._h, _p(values), _kind(values), values.shape[0], _p(fields),
                               _p(lo), _p(hi), C, M, _p(base), 0 if base is None else len(base),
                               _p(buf)))
    assert (buf[M * W:] == MARK).all(), "guard words written"
    return buf[:M * W].reshape(M, W).copy()


def _device_raw(index, values, fields, lo, hi, base, stream=None):
    """range_masks_device on a non-default stream: out and base start one word
    past a 16-byte boundary; out is marked and sits between guard words."""
    import torch
    M, C = fields.shape
    W = (index.n_docs + 31) // 32
    st = stream or torch.cuda.Stream()
    dv = torch.from_numpy(values).cuda()
    df, dlo, dhi = (torch.from_numpy(a).cuda() for a in (fields, lo, hi))
    buf = torch.full((1 + M * W + GUARD,), MARK_I32, dtype=torch.int32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    db = None
    if base is not None:
        bb = torch.zeros(1 + base.size, dtype=torch.int32, device="cuda")
        bb[1:] = torch.from_numpy(np.ascontiguousarray(base).view(np.int32).reshape(-1)).cuda()
        assert bb.data_ptr() % 16 == 0
        db = bb[1:].view(base.shape[0], W)
    torch.cuda.synchronize()  # (the uploads ran on the current stream)
    index.range_masks_device(dv, df, dlo, dhi, buf[1:1 + M * W].view(M, W), db, st)
    st.synchronize()
    got = buf.cpu().numpy().view(np.uint32)
    assert got[0] == MARK and (got[1 + M * W:] == MARK).all(), "guard words written"
    return got[1:1 + M * W].reshape(M, W).copy()


def _check(index, values, fields, lo, hi, base=None, what="", host=True):
    """Host call (unless a field id is out of range, which it rejects) and
    device call both give numpy's masks; returns them."""
    values = np.ascontiguousarray(values if values.ndim == 2 else values[None, :])
    fields = np.ascontiguousarray(fields, dtype=np.int32)
    lo, hi = np.ascontiguousarray(lo), np.ascontiguousarray(hi)
    want = range_want(values, fields, lo, hi, base)
    calls = [("device", _device_raw)] + ([("host", _host_raw)] if host else [])
    for name, call in calls:
        got = call(index, values, fields, lo, hi, base)
        bad = np.nonzero(got != want)
        assert bad[0].size == 0, (what, name, f"{bad[0].size} words differ, first row "
                                  f"{bad[0][0]} word {bad[1][0]}: got {got[bad][0]:#x} "
                                  f"want {want[bad][0]:#x}")
    return want


def _bits(packed):
    return np.unpackbits(packed.view(np.uint8), axis=1).sum(axis=1)


def _base(rng, M, n_docs, p=0.7):
    """Packed random base rows of density p with every bit at or past n_docs
    set (garbage that must come out 0)."""
    b = pack_rows(rng.random((M, n_docs)) < p)
    if n_docs % 32:
        b[:, -1] |= np.uint32((0xFFFFFFFF << (n_docs % 32)) & 0xFFFFFFFF)
    return b


def _clauses(rng, M, C, F, dtype, span=100):
    """Random clause rows over values in [-span, span): about a tenth of the
    slots padding, widths from a point to the whole range."""
    fields = rng.integers(0, F, size=(M, C)).astype(np.int32)
    fields[rng.random((M, C)) < 0.1] = -1
    a = rng.integers(-span, span, size=(M, C))
    w = rng.integers(0, 2 * span, size=(M, C))
    return fields, a.astype(dtype), (a + w).astype(dtype)


# ------------------------------------------------------------ 1. the document axis
@pytest.mark.parametrize("n_docs", [1, 31, 32, 33, 63, 64, 65, SPAN - 1, SPAN, SPAN + 1,
                                    CHUNK - 1, CHUNK + 1, 70_001])
def test_document_axis(make, n_docs):
    """Word, step, span and chunk edges (M = 3 with an odd W leaves rows 1 and
    2 misaligned, on top of the device buffers' one-word offset); a base per
    row with garbage tail bits; the last row is open: it gives base's documents."""
    rng = np.random.default_rng(n_docs)
    M, C, F = 3, 2, 2
    values = rng.integers(-100, 100, size=(F, n_docs)).astype(np.int32)
    fields, lo, hi = _clauses(rng, M, C, F, np.int32)
    fields[M - 1] = [0, 1]
    lo[M - 1], hi[M - 1] = -2**31, 2**31 - 1
    base = _base(rng, M, n_docs)
    want = _check(make(n_docs), values, fields, lo, hi, base, n_docs)
    assert np.array_equal(want[M - 1], pack_rows(unpack_rows(base, n_docs))[M - 1])
    full = _check(make(n_docs), values, fields, lo, hi, None, n_docs)   # no base: all ones
    assert _bits(full)[M - 1] == n_docs


# --------------------------------------------------------------------- 2. the rows
@pytest.mark.parametrize("M", [1, ROWS, ROWS + 1, 2 * ROWS + 3])
def test_row_blocks(make, M):
    """A single row, a full block, a row over, two blocks and three rows, at
    333 documents (W = 11, odd); the rows differ from each other."""
    n_docs, C, F = 333, 2, 3
    rng = np.random.default_rng(M)
    values = rng.integers(-100, 100, size=(F, n_docs)).astype(np.int32)
    fields, lo, hi = _clauses(rng, M, C, F, np.int32)
    want = _check(make(n_docs), values, fields, lo, hi, _base(rng, M, n_docs, 0.9), M)
    assert M < 3 or len({w.tobytes() for w in want}) > M // 2


def test_more_rows_than_65535(make):
    """65 537 rows of 2 words at 40 documents."""
    n_docs, M = 40, 65_537
    rng = np.random.default_rng(5)
    values = rng.integers(-100, 100, size=(1, n_docs)).astype(np.int32)
    fields, lo, hi = _clauses(rng, M, 1, 1, np.int32)
    want = _check(make(n_docs), values, fields, lo, hi, _base(rng, 1, n_docs, 0.9))
    assert want[65_536:].any() and want[:65_536].any()


def test_empty_shapes_write_nothing(make):
    """M == 0 returns without writing (host and device calls)."""
    import torch
    from bm25mi._capi import BM25_OK, lib
    index = make(70)
    values = np.zeros((1, 70), np.int32)
    z = np.zeros((2, 1), np.int32)
    buf = np.full(GUARD, MARK, np.uint32)
    assert lib.bm25_range_masks(index._h, _p(values), 0, 1, _p(z), _p(z), _p(z), 1, 0, None, 0,
                                _p(buf)) == BM25_OK
    assert (buf == MARK).all()
    assert index.range_masks(values, z[:0], z[:0], z[:0]).shape == (0, 3)
    st = torch.cuda.Stream()
    dbuf = torch.full((GUARD,), MARK_I32, dtype=torch.int32, device="cuda")
    dz = torch.zeros((0, 1), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    index.range_masks_device(torch.from_numpy(values).cuda(), dz, dz, dz, dbuf[:0].view(0, 3),
                             None, st)
    st.synchronize()
    assert (dbuf.cpu().numpy() == MARK_I32).all()


# ------------------------------------------------------------------ 3. the clauses
@pytest.mark.parametrize("C", [0, 1, 2, 3, 4, 5, 8, 9, 70])
def test_clause_axis(make, C):
    """Clause widths (each kernel's last width and the first of the next) at
    1000 documents, 6 fields, 9 rows: random rows (a row of 5 or 70 clauses
    walks more fields than the register cache holds, and
    neighbours name other fields), then rows made by hand: every clause on one
    field (the cache always hits), fields cycling 0, 1, 2 (it always misses),
    all padding, and one padding slot among real ones."""
    n_docs, M, F = 1000, 9, 6
    rng = np.random.default_rng(C)
    values = rng.integers(-100, 100, size=(F, n_docs)).astype(np.int32)
    fields, lo, hi = _clauses(rng, M, C, F, np.int32)
    if C >= 5:   # wide rows are ANDs of many clauses: keep them from being all empty
        lo[:], hi[:] = -90, 90
        lo[:, 0], hi[:, 0] = -30, 60
    if C:
        fields[3] = 4
        fields[4] = np.arange(C) % 3
        fields[5] = -1
        fields[6] = np.arange(C) % F
        fields[6, C // 2] = -7
        fields[7] = (np.arange(C) + 3) % F    # the neighbour of row 6 starts on another field
    base = _base(rng, M, n_docs, 0.95)
    want = _check(make(n_docs), values, fields, lo, hi, base, C)
    assert want.any()
    if C:        # the all-padding row: base, tail bits cleared
        assert np.array_equal(want[5], pack_rows(unpack_rows(base, n_docs))[5])
    if C == 0:   # no clause: base, tail bits cleared
        again = _check(make(n_docs), values, fields, lo, hi, None, C)
        assert (_bits(again) == n_docs).all()


# -------------------------------------------------------------------- 4. the kinds
@pytest.mark.parametrize("dtype", [np.int32, np.float32, np.int64])
def test_edge_values(make, dtype):
    """The edge values of the CPU model case, at 70 documents and spread over
    4500 (past a chunk): NaN, +-inf and signed zeros (float32), +-2^53 + 1 and
    the int64 limits (int64, which a float compare would get wrong), with and
    without a base."""
    values, fields, lo, hi = edge_case(dtype, 70)
    rng = np.random.default_rng(1)
    want = _check(make(70), values, fields, lo, hi, None, dtype)
    assert not want[4].any() and _bits(want)[5] == 70
    _check(make(70), values, fields, lo, hi, _base(rng, len(fields), 70), dtype)
    n = 4500
    wide = np.ascontiguousarray(values[:, rng.integers(0, 70, n)])
    want = _check(make(n), wide, fields, lo, hi, _base(rng, 1, n, 0.9), dtype)
    assert want[0].any() and want[7].any() and want[8].any() and not want[4].any()


@pytest.mark.parametrize("dtype", [np.int32, np.float32, np.int64])
def test_sorted_column(make, dtype):
    """A column sorted ascending: every range is one contiguous run of
    documents; the runs start and end on each side of word, step, span and
    chunk edges, and the rows' run lengths come out exactly."""
    n = 2 * CHUNK + 300
    step = {np.int32: 3, np.float32: 0.25, np.int64: 2**40 + 1}[dtype]
    col = (np.arange(n, dtype=np.int64) - n // 2).astype(dtype) * dtype(step)
    assert (np.diff(col) > 0).all()
    edges = [0, 31, 32, 63, 64, SPAN - 1, SPAN, CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK, n - 1]
    runs = [(a, b) for a in edges for b in edges if a <= b][::3] + [(0, n - 1), (CHUNK, CHUNK)]
    fields = np.zeros((len(runs), 1), np.int32)
    lo = np.array([[col[a]] for a, _ in runs], dtype)
    hi = np.array([[col[b]] for _, b in runs], dtype)
    want = _check(make(n), col[None, :], fields, lo, hi, None, dtype)
    assert _bits(want).tolist() == [b - a + 1 for a, b in runs]


# --------------------------------------------------------------------- 5. the base
@pytest.mark.parametrize("sel", [0.0, 0.01, 1.0])
def test_base_rows(make, sel):
    """Mb = 0, 1 and M at 0 %, about 1 % and 100 % selectivity; base rows with
    documents 256 .. 511 (a whole span) or a whole chunk cleared, so that
    (step, row) pairs are skipped; garbage tail bits come out 0."""
    n, M = CHUNK + 777, 5
    rng = np.random.default_rng(int(sel * 100))
    values = rng.integers(0, 1000, size=(2, n)).astype(np.int32)
    fields = np.tile(np.array([[0, 1]], np.int32), (M, 1))
    width = {0.0: -1, 0.01: 99, 1.0: 999}[sel]     # field 0 in [0, width], field 1 in [0, 99]
    lo = np.zeros((M, 2), np.int32)
    hi = np.tile(np.array([[width, 999 if sel == 1.0 else 99]], np.int32), (M, 1))
    allow = rng.random((M, n)) < 0.8
    allow[0, SPAN:2 * SPAN] = False
    allow[1, :CHUNK] = False
    allow[2] = False
    allow[3] = True
    base = pack_rows(allow)
    base[:, -1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)
    for b in (None, base[3:4], base[:1], base):
        want = _check(make(n), values, fields, lo, hi, b, sel)
        if sel == 0.0:
            assert not want.any()
        elif sel == 1.0 and b is None:
            assert (_bits(want) == n).all()
        elif sel == 1.0 and len(b) == M:
            assert np.array_equal(want, pack_rows(allow))
    if sel == 0.01:
        frac = _bits(_check(make(n), values, fields, lo, hi, None, sel))[0] / n
        assert 0.005 < frac < 0.02


# ------------------------------------------------------------ 6. unknown field ids
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_unknown_field(make, dtype):
    """A field id == F and one of 2^31 - 1: the device call gives an empty row
    (and the guard words are intact: nothing out of bounds was touched); the
    host call rejects the array, names row, column and value, and leaves the
    outputs untouched.  A float32 NaN bound is rejected by the host call too."""
    from bm25mi._capi import BM25_EINVAL, lib
    n, F = 5000, 2
    rng = np.random.default_rng(9)
    values = rng.integers(-100, 100, size=(F, n)).astype(dtype)
    low, high = np.iinfo(dtype).min, np.iinfo(dtype).max
    fields = np.array([[0, 1], [0, F], [2**31 - 1, 1], [1, -1]], np.int32)
    lo = np.full((4, 2), low, dtype)
    hi = np.full((4, 2), high, dtype)
    want = _check(make(n), values, fields, lo, hi, None, dtype, host=False)
    assert _bits(want).tolist() == [n, 0, 0, n]
    index = make(n)
    W = (n + 31) // 32
    buf = np.full(4 * W + GUARD, MARK, np.uint32)
    kind = 0 if dtype == np.int32 else 2
    assert lib.bm25_range_masks(index._h, _p(values), kind, F, _p(fields), _p(lo), _p(hi), 2, 4,
                                None, 0, _p(buf)) == BM25_EINVAL
    msg = lib.bm25_last_error().decode()
    assert f"fields[1][1] = {F} is not below F = {F}" in msg, msg
    assert (buf == MARK).all()
    fv = values.astype(np.float32)
    flo, fhi = np.full((4, 2), -np.inf, np.float32), np.full((4, 2), np.inf, np.float32)
    ok_fields = np.array([[0, 1], [0, 1], [1, -1], [1, -1]], np.int32)
    fhi[2, 0] = np.nan
    flo[3, 1] = np.nan            # (a padding slot: its bounds are not looked at)
    assert lib.bm25_range_masks(index._h, _p(fv), 1, F, _p(ok_fields), _p(flo), _p(fhi), 2, 4,
                                None, 0, _p(buf)) == BM25_EINVAL
    assert "hi[2][0] is NaN" in lib.bm25_last_error().decode()
    assert (buf == MARK).all()
    # the device call takes the NaN bound: the comparison matches nothing
    want = _check(make(n), fv, ok_fields, flo, fhi, None, "nan bound", host=False)
    assert _bits(want).tolist() == [n, n, 0, n]
    with pytest.raises(ValueError, match=r"fields\[1\]\[1\] = 2 is not below F = 2"):
        index.range_masks(values, fields, lo, hi)


# ------------------------------------------------------------------- 7. identities
@pytest.mark.parametrize("dtype", [np.int32, np.float32, np.int64])
def test_buckets_partition_the_base(make, dtype):
    """M bucket rows that partition a column's range (a histogram): the
    mask_count of the rows sums to the count of base, row by row to numpy's
    histogram of the allowed documents."""
    n, M = 9000, 37
    rng = np.random.default_rng(12)
    col = rng.integers(0, 370, n).astype(dtype)
    if dtype == np.int64:
        col = col * dtype(2**45)
    cuts = [int(x) for x in np.linspace(0, 370, M + 1)]
    scale = 2**45 if dtype == np.int64 else 1
    lo = np.array([[c * scale] for c in cuts[:-1]], dtype)
    hi = np.array([[(c - 1) * scale if dtype != np.float32 else np.nextafter(
        np.float32(c), np.float32(-1))] for c in cuts[1:]], dtype)
    base = _base(rng, 1, n, 0.6)
    index = make(n)
    got = index.range_masks(col, None, lo[:, 0], hi[:, 0], base)
    assert np.array_equal(got, range_want(col[None, :], np.zeros((M, 1), np.int32), lo, hi, base))
    counts = index.mask_count(got)
    allowed = unpack_rows(base, n)[0]
    assert counts.sum() == allowed.sum() == index.mask_count(base)[0]
    hist = np.histogram(col[allowed].astype(np.float64) / scale, bins=cuts)[0]
    assert np.array_equal(counts, hist)


def test_doc_shards_concatenate(make):
    """Handles over [0, 2048) and [2048, 5000) of one collection: their masks,
    side by side, are the whole index's (2048 is a whole number of words)."""
    n, h, M = 5000, 2048, 4
    rng = np.random.default_rng(7)
    values = rng.integers(-100, 100, size=(2, n)).astype(np.int64)
    fields, lo, hi = _clauses(rng, M, 2, 2, np.int64)
    allow = rng.random((M, n)) < 0.6
    whole = _check(make(n), values, fields, lo, hi, pack_rows(allow), "whole")
    a = _check(make(h), np.ascontiguousarray(values[:, :h]), fields, lo, hi,
               pack_rows(allow[:, :h]), "lo")
    b = _check(make(n - h), np.ascontiguousarray(values[:, h:]), fields, lo, hi,
               pack_rows(allow[:, h:]), "hi")
    assert a.any() and b.any() and np.array_equal(np.hstack([a, b]), whole)


# ------------------------------------------------------------- 8. one-call search
@pytest.fixture(scope="module")
def range_case(gpu):
    """6000 documents (3 tiles), 60 terms, 7 queries with a term clause row and
    a range clause row each; the masks by numpy."""
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
    groups = rng.integers(-1, G, N).astype(np.int32)
    index = _idx(ip, ix, dt, N)
    yield (index, q, (mu, an, mn), base, (values, fields, lo, hi), pack_rows(allowed), groups, G,
           terms)
    index.close()


def test_search_boolean_with_ranges(range_case):
    """search_boolean(ranges=..., total_hits=True, facets=...) equals, bit for
    bit, search_filtered under pack_mask(range model AND term-clause model);
    the totals and facets are that mask's; once with bool_chunk = 1, once
    automatic.  ranges=None equals the call without it."""
    import bm25mi
    from facets_model import facets_want
    index, q, (mu, an, mn), base, rng4, masks, groups, G, terms = range_case
    want = index.search_filtered(q, 10, masks, np.arange(7, dtype=np.int32))
    totals = _bits(masks)
    assert totals[4] == 0 and (totals[[0, 1, 2, 3, 6]] > 0).all()
    fac = facets_want(masks, groups, G)
    try:
        for chunk in (1, 0):
            index.set_option("bool_chunk", chunk)
            got = index.search_boolean(q, 10, mu, an, mn, base, total_hits=True,
                                       facets=(groups, G), ranges=rng4)
            assert len(got) == 4
            _exact(got[:2], want)
            assert np.array_equal(got[2], totals) and np.array_equal(got[3], fac), chunk
            got = index.search_boolean(q, 10, mu, an, mn, base, ranges=rng4)
            assert len(got) == 2
            _exact(got, want)
            got = index.search_boolean(q, 0, mu, an, mn, base, total_hits=True, ranges=rng4)
            assert got[0].shape == (7, 0) and np.array_equal(got[2], totals)
    finally:
        index.set_option("bool_chunk", 0)
    # one field as a triple, int64: the year clause alone
    year = rng4[0][0].astype(np.int64)
    lo1, hi1 = np.full(7, 2000, np.int64), np.full(7, 2010, np.int64)
    only = pack_rows(terms & ((year >= 2000) & (year <= 2010)))
    got = index.search_boolean(q, 10, mu, an, mn, base, ranges=(year, lo1, hi1))
    _exact(got, index.search_filtered(q, 10, only, np.arange(7, dtype=np.int32)))
    # ranges=None: today's output
    plain = index.search_boolean(q, 10, mu, an, mn, base, total_hits=True)
    got = index.search_boolean(q, 10, mu, an, mn, base, total_hits=True, ranges=None)
    _exact(got[:2], plain[:2])
    assert np.array_equal(got[2], plain[2])
    # a row without a range clause anywhere (C == 0): the call without ranges
    f0 = np.zeros((7, 0), np.int32)
    got = index.search_boolean(q, 10, mu, an, mn, base, total_hits=True,
                               ranges=(rng4[0], f0, f0.copy(), f0.copy()))
    _exact(got[:2], plain[:2])
    with pytest.raises(ValueError, match=r"fields\[2\]\[0\] = 2 is not below F = 2"):
        bad = rng4[1].copy()
        bad[2, 0] = 2
        index.search_boolean(q, 10, mu, an, mn, base, ranges=(rng4[0], bad, rng4[2], rng4[3]))


def test_device_chain(range_case):
    """range_masks_device -> term_masks_device(d_base=...) ->
    search_filtered_device on one stream gives the same rows."""
    import torch
    import bm25mi
    index, q, (mu, an, mn), base, (values, fields, lo, hi), masks, groups, G, _ = range_case
    want = index.search_filtered(q, 10, masks, np.arange(7, dtype=np.int32))
    W = (index.n_docs + 31) // 32
    st = torch.cuda.Stream()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dv, df, dlo, dhi = dev(values), dev(fields), dev(lo), dev(hi)
    dbase = dev(bm25mi.pack_mask(base).view(np.int32))
    dmu, dan, dmn = (dev(bm25mi.pad_clause(c)) for c in (mu, an, mn))
    dr = torch.full((7, W), MARK_I32, dtype=torch.int32, device="cuda")
    dm = torch.full((7, W), MARK_I32, dtype=torch.int32, device="cuda")
    dq, dqm = dev(q), dev(np.arange(7, dtype=np.int32))
    dd = torch.full((7, 10), 99, dtype=torch.int32, device="cuda")
    ds = torch.full((7, 10), 7.5, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    index.range_masks_device(dv, df, dlo, dhi, dr, dbase, st)
    index.term_masks_device(dmu, dan, dmn, dr, dm, st)
    index.search_filtered_device(dq, 10, dm, dqm, dd, ds, st)
    st.synchronize()
    assert np.array_equal(dm.cpu().numpy().view(np.uint32), masks)
    _exact((dd.cpu().numpy(), ds.cpu().numpy()), want)


# -------------------------------------------------------------------- 9. not a search
def test_not_a_search(range_case):
    """After a search, range_masks (host and device calls) leave
    last_dispatch(), search_stats() and filtered_stats() as they were."""
    index, q, _, base, (values, fields, lo, hi), masks, groups, G, _ = range_case
    index.search_filtered(q, 10, masks, np.arange(7, dtype=np.int32))
    before = (index.last_dispatch(), index.search_stats(), index.filtered_stats())
    _check(index, values, fields, lo, hi, pack_rows(base))
    assert (index.last_dispatch(), index.search_stats(), index.filtered_stats()) == before
