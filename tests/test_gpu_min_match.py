"""GPU tests of minimum-should-match and the hit counts
(bm25_term_masks_min_match(_device), bm25_mask_count(_device),
bm25_search_boolean_min_match; bm25mi_termmask.hip).

The expected masks are computed here from a bool has[n_terms, n_docs] by the
formula of include/bm25mi.h, row by row, and packed with bm25mi.pack_mask; they
never go through the code under test.  Masks compare word for word, by the host
call and by the device call (a non-default stream), into buffers pre-filled
with 0xA5A5A5A5 that carry 64 guard words.  The shapes sit next to

  32     documents per mask word
  2048   documents per tile (64 mask words: one per lane of the item's wave)
  64     terms of a clause looked up per step
  1024   mask words per row up to which the count runs a wave per row"""
import ctypes

import numpy as np
import pytest

from test_gpu_parity import _doc_slice, _exact, _idx, _rand_index
from test_gpu_term_masks import (DOC0, EMPTY, FIFTH, FILL, FULL, GUARD, HALF, LASTDOC, NEGV, P1, P5,
                                 ROWS, SLOT0, SLOTL, TILE, V, ZEROV, _has_of, _pad, _term_index)
from test_gpu_term_masks import _device_raw as _old_device_raw
from test_gpu_term_masks import _want as _old_want

pytestmark = pytest.mark.gpu


def _allowed(has, must, any_, must_not, min_match, M, base=None):
    """The formula, row by row -> bool [M, n_docs].  min_match: int [M] or
    None (every row needs one term); base: bool [1 or M, n_docs] or None; an
    id >= n_terms is a term that no document has."""
    n_terms, n_docs = has.shape
    none = np.zeros(n_docs, bool)
    col = lambda t: has[t] if t < n_terms else none
    mu, an, mn = _pad(must, M), _pad(any_, M), _pad(must_not, M)
    ok = np.ones((M, n_docs), bool)
    for m in range(M):
        if base is not None:
            ok[m] &= base[0 if len(base) == 1 else m]
        for t in mu[m][mu[m] >= 0]:
            ok[m] &= col(t)
        ids = an[m][an[m] >= 0]
        need = 1 if min_match is None else int(min_match[m])
        if len(ids) and need > 0:           # n_any == 0: absent; need <= 0: optional
            count = np.zeros(n_docs, np.int64)
            for t in ids:                   # every slot is a clause of its own
                count += col(t)
            ok[m] &= count >= need
        for t in mn[m][mn[m] >= 0]:
            ok[m] &= ~col(t)
    return ok


def _want(has, must, any_, must_not, min_match, M, base=None):
    import bm25mi
    return bm25mi.pack_mask(_allowed(has, must, any_, must_not, min_match, M, base))


def _bits(packed, n_docs):
    """Set bits of each packed row among bits 0 .. n_docs - 1."""
    b = np.unpackbits(np.ascontiguousarray(packed).view(np.uint8), axis=1, bitorder="little")
    return b[:, :n_docs].sum(axis=1, dtype=np.int64)


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None


def _host_raw(index, must, any_, must_not, min_match, M, base=None):
    """bm25_term_masks_min_match into a pre-filled buffer with guard words."""
    from bm25mi._capi import check, lib
    W = (index.n_docs + 31) // 32
    mu, an, mn = _pad(must, M), _pad(any_, M), _pad(must_not, M)
    mm = None if min_match is None else np.ascontiguousarray(min_match, dtype=np.int32)
    buf = np.full(M * W + GUARD, FILL, np.uint32)
    Mb = 0 if base is None else len(base)
    check(lib.bm25_term_masks_min_match(index._h, _p(mu), mu.shape[1], _p(an), an.shape[1], _p(mn),
                                        mn.shape[1], _p(mm), M, _p(base), Mb, _p(buf)))
    assert (buf[M * W:] == FILL).all(), "guard words written"
    return buf[:M * W].reshape(M, W).copy()


def _device_raw(index, must, any_, must_not, min_match, M, base=None):
    """term_masks_device(d_min_match=...) on a non-default stream, pre-filled,
    guard words."""
    import torch
    W = (index.n_docs + 31) // 32
    st = torch.cuda.Stream()
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    args = [None if c is None else up(_pad(c, M)) for c in (must, any_, must_not)]
    db = None if base is None else up(base.view(np.int32))
    dmm = up(np.ascontiguousarray(min_match, dtype=np.int32))
    buf = torch.full((M * W + GUARD,), FILL - (1 << 32), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # (the uploads ran on the current stream)
    index.term_masks_device(args[0], args[1], args[2], db, buf[:M * W].view(M, W), st,
                            d_min_match=dmm)
    st.synchronize()
    got = buf.cpu().numpy().view(np.uint32)
    assert (got[M * W:] == FILL).all(), "guard words written"
    return got[:M * W].reshape(M, W).copy()


def _check(index, want, must, any_, must_not, min_match, M, base=None, what=""):
    """Host call and device call both give ``want`` word for word; the bits
    at or past n_docs are 0."""
    for name, got in (("host", _host_raw(index, must, any_, must_not, min_match, M, base)),
                      ("device", _device_raw(index, must, any_, must_not, min_match, M, base))):
        bad = np.nonzero(got != want)
        assert bad[0].size == 0, (what, name, f"{bad[0].size} words differ, first row "
                                  f"{bad[0][0]} word {bad[1][0]}: got {got[bad][0]:#x} "
                                  f"want {want[bad][0]:#x}")
        r = index.n_docs % 32
        if r:
            assert not (got[:, -1] >> np.uint32(r)).any(), (what, name, "bits past n_docs")


def _differs(want, lo, mid, hi):
    """Row ``mid`` is non-empty and differs from rows ``lo`` and ``hi``."""
    return bool(want[mid].any() and not np.array_equal(want[mid], want[lo])
                and not np.array_equal(want[mid], want[hi]))


# the rows of the edge test: (must, any, must_not, need)
FOUR = [HALF, FIFTH, P5, ZEROV]
EDGE_ROWS = [([], FOUR, [], need) for need in range(6)] + [   # rows 0..5: need 0..5
    ([], [HALF, HALF], [], 2),                     # duplicates count: has(HALF, .)
    ([], [SLOT0, SLOTL, DOC0, LASTDOC], [], 2),    # most tiles: fewer than 2 terms have a segment
    ([], [FULL, EMPTY, -1, HALF], [], 2),          # padding and an empty term between ids
    ([], [FULL, EMPTY, -1, HALF], [], 3),          # ... n_any = 3, at most 2 can hit
    ([], [-1, -1], [], 3),                         # an absent clause: every document
    ([FULL], [HALF, FIFTH, ZEROV], [NEGV], 2),     # all three clauses (and a base row below)
    ([EMPTY], [HALF, FIFTH], [], 2),               # must empties the row before the any clause
    ([], [HALF, FIFTH], [], 1),                    # a neighbour on the shared-bitmap path
]


# ------------------------------------------------------ 1. word and tile edges
@pytest.mark.parametrize("n_docs", [1, 31, 32, 33, 2047, 2048, 2049, 70_001])
@pytest.mark.parametrize("segments", ["dense", "sparse"])
def test_word_and_tile_edges(gpu, segments, n_docs):
    """Around the 32-document mask word and the 2048-document tile, both
    segment tables; the rows above in one call (neighbouring items take
    different branches), without a base and with a base row per mask."""
    has, ip, ix, dt = _term_index(n_docs, 300 + n_docs)
    index = _idx(ip, ix, dt, n_docs, segments=segments)
    assert index.info()["sparse"] == (segments == "sparse")
    M = len(EDGE_ROWS)
    mu, an, mn, mm = ([r[i] for r in EDGE_ROWS] for i in range(4))
    want = _want(has, mu, an, mn, mm, M)
    ok = _allowed(has, mu, an, mn, mm, M)
    assert ok[0].all() and ok[10].all()                    # optional / absent: every document
    assert not ok[5].any() and not ok[9].any() and not ok[12].any()  # need > n_any, 3 of 2, must
    assert np.array_equal(ok[6], has[HALF]) and np.array_equal(ok[8], has[HALF])
    assert np.array_equal(ok[1], has[FOUR].any(axis=0))
    if n_docs >= 2047:  # non-vacuity: need 2 is neither need 1 nor need 3
        assert _differs(want, 1, 2, 3)
    # SLOT0 and DOC0 meet on document 0; LASTDOC meets SLOTL or SLOT0 where the last document
    # sits in the last or the first slot of its tile
    assert ok[7, 0] and ok[7].sum() == 1 + (n_docs > 1 and n_docs % TILE in (0, 1))
    _check(index, want, mu, an, mn, mm, M, what="no base")
    assert np.array_equal(index.term_masks(mu, an, mn, min_match=mm), want)
    rng = np.random.default_rng(n_docs)
    base = rng.random((M, n_docs)) < 0.7
    import bm25mi
    packed = bm25mi.pack_mask(base)
    if n_docs % 32:  # garbage in the base's bits past n_docs
        packed[:, -1] |= np.uint32((0xFFFFFFFF << (n_docs % 32)) & 0xFFFFFFFF)
    _check(index, _want(has, mu, an, mn, mm, M, base), mu, an, mn, mm, M, packed, what="base")
    index.close()


def test_document_zero_meets_two_sparse_terms(gpu):
    """SLOT0 and DOC0 both hold document 0, SLOTL and LASTDOC the last
    document of three full tiles: need 2 keeps exactly those two; in the
    middle tile two terms have a segment and no document has both."""
    n_docs = 3 * TILE
    has, ip, ix, dt = _term_index(n_docs, 11)
    index = _idx(ip, ix, dt, n_docs)
    an = [[SLOT0, SLOTL, DOC0, LASTDOC]] * 3
    mm = [1, 2, 3]
    ok = _allowed(has, None, an, None, mm, 3)
    assert np.nonzero(ok[1])[0].tolist() == [0, n_docs - 1] and not ok[2].any()
    _check(index, _want(has, None, an, None, mm, 3), None, an, None, mm, 3)
    index.close()


# -------------------------------------- 2. carry chains, clauses wider than a wave
CARRY_N = [3, 4, 7, 8, 15, 16, 17, 64, 65, 130]


@pytest.mark.parametrize("segments", ["dense", "sparse"])
def test_carry_chains_and_wide_clauses(gpu, segments):
    """any = [FULL] * n with need n - 1, n and n + 1 (every document twice,
    then none), and [FULL] * (n - 1) + [HALF], where the last increment decides
    per document: need n is has(HALF, .).  n crosses the counter's plane
    counts (2^P - 1, 2^P) and the 64 terms looked up per step.  Non-vacuity
    here: need n is non-empty and differs from need n - 1 and need n + 1."""
    n_docs = 2049
    has, ip, ix, dt = _term_index(n_docs, 21)
    index = _idx(ip, ix, dt, n_docs, segments=segments)
    an, mm = [], []
    for n in CARRY_N:
        for row in ([FULL] * n, [FULL] * (n - 1) + [HALF]):
            for need in (n - 1, n, n + 1):
                an.append(row)
                mm.append(need)
    M = len(an)
    ok = _allowed(has, None, an, None, mm, M)
    want = _want(has, None, an, None, mm, M)
    for i in range(len(CARRY_N)):
        a = 6 * i
        assert ok[a].all() and ok[a + 1].all() and not ok[a + 2].any()
        assert ok[a + 3].all() and np.array_equal(ok[a + 4], has[HALF]) and not ok[a + 5].any()
        assert _differs(want, a + 3, a + 4, a + 5)
    _check(index, want, None, an, None, mm, M)
    index.close()


# ------------------------------------------------------------- 3. device only
def test_device_ids_past_the_vocabulary_and_negative_need(gpu):
    """In the device call an id >= n_terms counts in n_any and never in
    count; a min_match entry of -3 behaves as 0.  The host call rejects both."""
    n_docs = 4100
    has, ip, ix, dt = _term_index(n_docs, 5)
    index = _idx(ip, ix, dt, n_docs)
    an = [[HALF, V + 3, FIFTH], [HALF, V + 3, FIFTH], [V, V + 1], [EMPTY], [V, -1], [HALF, V]]
    mm = [2, 3, 1, -3, 2, -3]
    ok = _allowed(has, None, an, None, mm, 6)
    assert np.array_equal(ok[0], has[HALF] & has[FIFTH]) and ok[0].any()
    assert not ok[1].any() and not ok[2].any() and ok[3].all() and not ok[4].any() and ok[5].all()
    want = _want(has, None, an, None, mm, 6)
    assert np.array_equal(_device_raw(index, None, an, None, mm, 6), want)
    with pytest.raises(ValueError, match=r"maximum token ID in the query \(15\) is higher"):
        _host_raw(index, None, [[HALF, V + 3]], None, [1], 1)
    with pytest.raises(ValueError, match=r"min_match\[1\] = -3 is negative"):
        _host_raw(index, None, [[HALF], [HALF]], None, [1, -3], 2)
    index.close()


def test_clause_wider_than_the_counter(gpu):
    """B > 65535 with a min_match pointer is EINVAL in both calls (a shape);
    without one the clause is as wide as it likes."""
    import torch
    has, ip, ix, dt = _term_index(40, 6)
    index = _idx(ip, ix, dt, 40)
    wide = np.full((1, 65536), -1, np.int32)
    wide[0, -1] = HALF
    with pytest.raises(ValueError, match="B = 65536 slots, at most 65535"):
        index.term_masks(any=wide, min_match=1)
    out = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError, match="B = 65536 slots, at most 65535"):
        index.term_masks_device(None, torch.from_numpy(wide).cuda(), None, None, out,
                                d_min_match=torch.ones(1, dtype=torch.int32, device="cuda"))
    assert np.array_equal(index.term_masks(any=wide), _old_want(has, None, [[HALF]], None, 1))
    ok = index.term_masks(any=wide[:, 1:], min_match=1)
    assert np.array_equal(ok, _old_want(has, None, [[HALF]], None, 1))
    index.close()


# ------------------------------------------------------------- 4. random rows
def test_random_rows(gpu):
    """64 rows at 70 001 documents (35 tiles): clause widths 0..12 drawn from
    the 12 terms with padding sprinkled in, need from 0..width + 1, a random
    base on half of the rows (ones on the others)."""
    n_docs, M = 70_001, 64
    has, ip, ix, dt = _term_index(n_docs, 31)
    index = _idx(ip, ix, dt, n_docs)
    rng = np.random.default_rng(32)
    an, mm = [], []
    for m in range(M):
        width = m % 13
        row = rng.integers(0, V, size=width)
        row[rng.random(width) < 0.15] = -1
        an.append([int(t) for t in row])
        mm.append(int(rng.integers(0, width + 2)))
    mu = [[HALF] if m % 7 == 3 else [] for m in range(M)]
    mn = [[P5] if m % 5 == 2 else [] for m in range(M)]
    base = np.ones((M, n_docs), bool)
    base[::2] = rng.random((M // 2, n_docs)) < 0.6
    want = _want(has, mu, an, mn, mm, M, base)
    # non-vacuity: some row's clause gives three different masks at need 1, 2, 3
    hit = False
    for m in range(M):
        w = _want(has, None, [an[m]] * 3, None, [1, 2, 3], 3)
        hit = hit or _differs(w, 0, 1, 2)
    assert hit and want.any()
    import bm25mi
    _check(index, want, mu, an, mn, mm, M, bm25mi.pack_mask(base))
    index.close()


# ---------------------------------------------------------------- 5. identity
@pytest.mark.parametrize("segments", ["dense", "sparse"])
def test_identity_with_term_masks(gpu, segments):
    """With min_match NULL and with all ones the new calls equal
    bm25_term_masks(_device) word for word on the sibling's ROWS."""
    from bm25mi._capi import check, lib
    n_docs = 5000
    has, ip, ix, dt = _term_index(n_docs, 77)
    index = _idx(ip, ix, dt, n_docs, segments=segments)
    M = len(ROWS)
    mu, an, mn = ([r[i] for r in ROWS] for i in range(3))
    old = index.term_masks(mu, an, mn)
    assert np.array_equal(old, _old_want(has, mu, an, mn, M))
    assert np.array_equal(_old_device_raw(index, mu, an, mn, M), old)
    ones = np.ones(M, np.int32)
    assert np.array_equal(_host_raw(index, mu, an, mn, None, M), old)     # NULL pointer
    assert np.array_equal(_host_raw(index, mu, an, mn, ones, M), old)
    assert np.array_equal(_device_raw(index, mu, an, mn, ones, M), old)
    assert np.array_equal(index.term_masks(mu, an, mn, min_match=1), old)
    # the device symbol with a NULL d_min_match
    import torch
    W = old.shape[1]
    cl = [torch.from_numpy(_pad(c, M)).cuda() for c in (mu, an, mn)]
    buf = torch.full((M, W), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    check(lib.bm25_term_masks_min_match_device(
        index._h, vp(cl[0]), cl[0].shape[1], vp(cl[1]), cl[1].shape[1], vp(cl[2]), cl[2].shape[1],
        None, M, None, 0, vp(buf), ctypes.c_void_p(st.cuda_stream)))
    st.synchronize()
    assert np.array_equal(buf.cpu().numpy().view(np.uint32), old)
    index.close()


# -------------------------------------------------------------- 6. mask_count
def _tiny_index(n_docs):
    """One term on document 0: the count reads the caller's masks only."""
    return _idx(np.array([0, 1], np.int64), np.zeros(1, np.int32), np.ones(1, np.float32), n_docs)


def _count_both(index, masks, offset=0):
    """bm25_mask_count (pre-filled output, guard entries) and
    bm25_mask_count_device on a non-default stream (garbage in the output
    buffer; the masks start ``offset`` words into their allocation)."""
    import torch
    from bm25mi._capi import check, lib
    M, W = masks.shape
    out = np.full(M + 8, -7, np.int64)
    check(lib.bm25_mask_count(index._h, _p(masks), M, _p(out)))
    assert (out[M:] == -7).all(), "guard entries written"
    dm = torch.zeros(offset + M * W + GUARD, dtype=torch.int32, device="cuda")
    dm[offset:offset + M * W] = torch.from_numpy(masks.view(np.int32).reshape(-1)).cuda()
    dc = torch.full((M + 8,), 0x5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    index.mask_count_device(dm[offset:offset + M * W].view(M, W), dc[:M], st)
    st.synchronize()
    got = dc.cpu().numpy()
    assert (got[M:] == 0x5A5A5A5A5A5A).all(), "guard entries written"
    assert np.array_equal(index.mask_count(masks), out[:M])
    return out[:M].copy(), got[:M].copy()


@pytest.mark.parametrize("n_docs", [1, 31, 32, 33, 2047, 2048, 2049, 70_001, 32_839, 140_050])
def test_mask_count(gpu, n_docs):
    """Rows all zero, all ones, random, one whose last word has every bit
    past n_docs set and one straight from term_masks, against numpy's bit
    counts.  W is 65 at 2049 and 1027 at 32 839 (odd: unaligned row starts, a
    wave per row and a workgroup per row); 140 050 documents are 4377 words
    (odd, two chunks per row: the atomics).  The device masks start 0 and 1
    words into a 16-byte-aligned allocation."""
    has, ip, ix, dt = _term_index(n_docs, 40 + n_docs)
    index = _idx(ip, ix, dt, n_docs)
    W = (n_docs + 31) // 32
    rng = np.random.default_rng(n_docs)
    rand = rng.integers(0, 2**32, size=(3, W), dtype=np.uint64).astype(np.uint32)
    r = n_docs % 32
    past = np.uint32((0xFFFFFFFF << r) & 0xFFFFFFFF) if r else np.uint32(0)
    tailed = rand[:1].copy()
    tailed[0, -1] |= past                       # every bit past n_docs set
    built = index.term_masks(any=[[HALF, FIFTH, ZEROV]], must_not=[[P1]], min_match=2)
    masks = np.concatenate([np.zeros((1, W), np.uint32), np.full((1, W), 0xFFFFFFFF, np.uint32),
                            rand, tailed, built])
    want = _bits(masks, n_docs)
    assert want[0] == 0 and want[1] == n_docs
    if n_docs in (2049, 32_839, 140_050):
        assert W % 2 == 1
    assert want[6] == _allowed(has, None, [[HALF, FIFTH, ZEROV]], [[P1]], [2], 1).sum()
    for offset in (0, 1):
        host, dev = _count_both(index, masks, offset)
        assert host.dtype == np.int64 and np.array_equal(host, want), (offset, host, want)
        assert np.array_equal(dev, want), (offset, dev, want)
    assert np.array_equal(index.mask_count(np.ones((2, n_docs), bool)), [n_docs, n_docs])
    assert index.mask_count(np.zeros((0, W), np.uint32)).shape == (0,)
    index.close()


def test_mask_count_many_rows(gpu):
    """M = 70 000 rows of 2 words (n_docs = 33): past 65 535 rows."""
    index = _tiny_index(33)
    rng = np.random.default_rng(8)
    masks = rng.integers(0, 2**32, size=(70_000, 2), dtype=np.uint64).astype(np.uint32)
    want = _bits(masks, 33)
    assert want.min() < want.max() <= 33
    host, dev = _count_both(index, masks, 1)
    assert np.array_equal(host, want) and np.array_equal(dev, want)
    index.close()


def test_mask_count_one_long_row(gpu):
    """M = 1 at n_docs = 10 000 001 (312 501 words, 77 chunks), random words
    from the host, on a handle of that many documents and one posting."""
    n_docs = 10_000_001
    index = _tiny_index(n_docs)
    rng = np.random.default_rng(9)
    masks = rng.integers(0, 2**32, size=(1, (n_docs + 31) // 32), dtype=np.uint64).astype(np.uint32)
    masks[0, -1] = 0xFFFFFFFF                   # one document in the last word
    want = _bits(masks, n_docs)
    assert 4_900_000 < want[0] < 5_100_000
    host, dev = _count_both(index, masks, 3)
    assert np.array_equal(host, want) and np.array_equal(dev, want)
    index.close()


# ---------------------------------------------------------- 7. one-call search
@pytest.fixture(scope="module")
def mm_case(gpu):
    """6000 documents (3 tiles), 60 terms, 7 queries with a clause row and a
    need each; the masks and their counts by numpy."""
    rng = np.random.default_rng(41)
    N, nt = 6000, 60
    ip, ix, dt = _rand_index(rng, N, nt, 3000)
    by_df = np.argsort(-np.diff(ip))
    a, b, c, d, e = (int(x) for x in by_df[:5])
    has = _has_of(ip, ix, nt, N)
    q = rng.integers(-1, nt, size=(7, 8)).astype(np.int32)
    mu = [[], [a], [], [], [c], [], [-1]]
    an = [[a, b, c, d, e], [b, c, d], [a, d], [a, b, c], [a, b, a], [a, b], [-1, -1]]
    mn = [[], [], [c], [], [d], [], []]
    mm = [4, 2, 2, 0, 3, 3, 2]
    ok = _allowed(has, mu, an, mn, mm, 7)
    masks = _want(has, mu, an, mn, mm, 7)
    totals = ok.sum(axis=1).astype(np.int64)
    assert 10 < totals[0] < 4096 and totals[3] == N and totals[5] == 0 and totals[6] == N
    assert np.array_equal(totals, _bits(masks, N))
    index = _idx(ip, ix, dt, N)
    yield index, q, mu, an, mn, mm, masks, totals, (ip, ix, dt, N, nt)
    index.close()


@pytest.mark.parametrize("k", [1, 10, "hits-1", "hits", "hits+1"])
def test_search_with_min_match_and_totals(mm_case, k):
    """search_boolean(min_match=..., total_hits=True) equals search_filtered
    under the numpy masks bit for bit, padding included, with k below, at and
    above row 0's hits, under bool_chunk 1, 3 and 0; totals are numpy's."""
    index, q, mu, an, mn, mm, masks, totals, _ = mm_case
    hits = int(totals[0])
    if isinstance(k, str):
        k = hits + {"hits-1": -1, "hits": 0, "hits+1": 1}[k]
    want = index.search_filtered(q, k, masks, np.arange(7, dtype=np.int32))
    assert (want[0][5] == -1).all()
    if k > hits:
        assert (want[0][0][:hits] >= 0).all() and (want[0][0][hits:] == -1).all()
    try:
        for chunk in (1, 3, 0):
            index.set_option("bool_chunk", chunk)
            docs, scores, tot = index.search_boolean(q, k, mu, an, mn, min_match=mm,
                                                     total_hits=True)
            _exact((docs, scores), want)
            assert tot.dtype == np.int64 and np.array_equal(tot, totals), chunk
            _exact(index.search_boolean(q, k, mu, an, mn, min_match=mm), want)
    finally:
        index.set_option("bool_chunk", 0)


def test_search_totals_alone_defaults_and_bm25v(mm_case):
    """k = 0 returns the totals alone; min_match None with totals counts
    bm25_search_boolean's masks; the defaults are the old call; BM25v passes
    both keywords through; a percentage works end to end."""
    import bm25_native
    import scipy.sparse as sp
    index, q, mu, an, mn, mm, masks, totals, (ip, ix, dt, N, nt) = mm_case
    has = _has_of(ip, ix, nt, N)
    for chunk in (3, 0):
        index.set_option("bool_chunk", chunk)
        docs, scores, tot = index.search_boolean(q, 0, mu, an, mn, min_match=mm, total_hits=True)
        assert docs.shape == (7, 0) and scores.shape == (7, 0) and np.array_equal(tot, totals)
    qm = np.arange(7, dtype=np.int32)
    old_masks = _old_want(has, mu, an, mn, 7)
    want = index.search_filtered(q, 10, old_masks, qm)
    docs, scores, tot = index.search_boolean(q, 10, mu, an, mn, total_hits=True)
    _exact((docs, scores), want)
    assert np.array_equal(tot, _bits(old_masks, N))
    _exact(index.search_boolean(q, 10, mu, an, mn), want)
    _exact(index.search_boolean(q, 10, mu, an, mn, min_match=1), want)
    import bm25mi
    pct = bm25mi.min_match_rows(an, "75%")
    assert pct.tolist() == [3, 2, 1, 2, 2, 1, 0]
    m75 = _want(has, mu, an, mn, pct, 7)
    _exact(index.search_boolean(q, 10, mu, an, mn, min_match="75%"),
           index.search_filtered(q, 10, m75, qm))
    model = bm25_native.BM25v()
    model.index(sp.csc_matrix((dt, ix, ip), shape=(N, nt)), np.ones(N, np.float32))
    want = index.search_filtered(q, 10, masks, qm)
    docs, scores, tot = model.search_boolean(q, 10, must=mu, any=an, must_not=mn, min_match=mm,
                                             total_hits=True)
    _exact((docs, scores), want)
    assert np.array_equal(tot, totals)
    _exact(model.search_boolean(q, 10, must=mu, any=an, must_not=mn, min_match=mm), want)


# ---------------------------------------------------------------- 8. doc shards
def test_doc_shards(mm_case):
    """The index split at document 4096 into two shards: each shard's mask
    equals its slice of the collection's, and the shards' counts sum to the
    collection's."""
    index, q, mu, an, mn, mm, masks, totals, (ip, ix, dt, N, nt) = mm_case
    has = _has_of(ip, ix, nt, N)
    assert np.array_equal(index.term_masks(mu, an, mn, min_match=mm), masks)
    total = np.zeros(7, np.int64)
    for lo, hi in ((0, 2 * TILE), (2 * TILE, N)):
        sh = _idx(*_doc_slice(ip, ix, dt, lo, hi), hi - lo, doc_offset=lo)
        want = _want(has[:, lo:hi], mu, an, mn, mm, 7)
        _check(sh, want, mu, an, mn, mm, 7, what=f"shard {lo}")
        host, dev = _count_both(sh, want)
        assert np.array_equal(host, dev)
        total += dev
        sh.close()
    assert np.array_equal(total, totals) and np.array_equal(index.mask_count(masks), totals)


# -------------------------------------------------------------- 9. not a search
def test_not_a_search(mm_case):
    """After a search, term_masks(min_match=...) and mask_count (host and
    device calls) leave last_dispatch(), search_stats() and filtered_stats()
    as they were."""
    index, q, mu, an, mn, mm, masks, totals, _ = mm_case
    index.search_filtered(q, 10, masks, np.arange(7, dtype=np.int32))
    before = (index.last_dispatch(), index.search_stats(), index.filtered_stats())
    assert np.array_equal(index.term_masks(mu, an, mn, min_match=mm), masks)
    assert np.array_equal(_device_raw(index, mu, an, mn, mm, 7), masks)
    host, dev = _count_both(index, masks)
    assert np.array_equal(host, totals) and np.array_equal(dev, totals)
    assert (index.last_dispatch(), index.search_stats(), index.filtered_stats()) == before
