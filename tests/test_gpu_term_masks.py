"""GPU tests of the boolean term filters (bm25_term_masks /
bm25_term_masks_device / bm25_search_boolean; bm25mi_termmask.hip).

The expected masks are computed here from the CSC arrays: a bool
has[n_terms, n_docs], the formula of include/bm25mi.h applied row by row, packed
with bm25mi.pack_mask.  Masks compare word for word, by the host call and by
the device call (a non-default stream), into buffers pre-filled with
0xA5A5A5A5 that carry 64 guard words.  The shapes sit next to

  32     documents per mask word
  2048   documents per tile (64 mask words: one per lane of the item's wave)"""
import ctypes

import numpy as np
import pytest

from test_gpu_parity import _doc_slice, _exact, _idx, _rand_index

pytestmark = pytest.mark.gpu

FILL = 0xA5A5A5A5
GUARD = 64
TILE = 2048

# the terms of _term_index
FULL, EMPTY, SLOT0, SLOTL, ZEROV, NEGV, HALF, FIFTH, P5, P1, LASTDOC, DOC0 = range(12)
V = 12


def _term_index(n_docs, seed):
    """12 terms: on every document (full 2048-posting segments), without a
    posting, on slot 0 / on the last slot of every tile only, with stored
    0.0f, with negative values, four random densities, on the last document
    and on document 0 only.  Returns has [V, n_docs] and the CSC arrays."""
    rng = np.random.default_rng(seed)
    d = np.arange(n_docs)
    has = np.zeros((V, n_docs), bool)
    has[FULL] = True
    has[SLOT0] = d % TILE == 0
    has[SLOTL] = d % TILE == TILE - 1
    has[ZEROV] = rng.random(n_docs) < 0.3
    has[NEGV] = rng.random(n_docs) < 0.1
    for t, p in ((HALF, 0.5), (FIFTH, 0.2), (P5, 0.05), (P1, 0.01)):
        has[t] = rng.random(n_docs) < p
    has[HALF, 0] = has[FIFTH, 0] = True  # (so the one-document index has hits)
    has[LASTDOC, n_docs - 1] = True
    has[DOC0, 0] = True
    val = np.full(V, 1.25, np.float32)
    val[ZEROV], val[NEGV] = 0.0, -1.5
    ip, ix, dt = [0], [], []
    for t in range(V):
        ids = np.nonzero(has[t])[0].astype(np.int32)
        ix.append(ids)
        dt.append(np.full(len(ids), val[t], np.float32))
        ip.append(ip[-1] + len(ids))
    return has, np.array(ip, np.int64), np.concatenate(ix), np.concatenate(dt)


def _has_of(ip, ix, n_terms, n_docs):
    has = np.zeros((n_terms, n_docs), bool)
    for t in range(n_terms):
        has[t, ix[ip[t]:ip[t + 1]]] = True
    return has


def _pad(rows, M):
    import bm25mi
    return np.zeros((M, 0), np.int32) if rows is None else bm25mi.pad_clause(rows)


def _want(has, must, any_, must_not, M, base=None):
    """The formula, row by row -> packed uint32 [M, W].  base: bool [Mb, n_docs]
    (Mb 1 or M) or None; an id >= n_terms is a term that no document has."""
    import bm25mi
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
        if len(ids):
            some = np.zeros(n_docs, bool)
            for t in ids:
                some |= col(t)
            ok[m] &= some
        for t in mn[m][mn[m] >= 0]:
            ok[m] &= ~col(t)
    return bm25mi.pack_mask(ok)


def _host_raw(index, must, any_, must_not, M, base=None):
    """bm25_term_masks into a pre-filled buffer with guard words."""
    from bm25mi._capi import check, lib
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None
    W = (index.n_docs + 31) // 32
    mu, an, mn = _pad(must, M), _pad(any_, M), _pad(must_not, M)
    buf = np.full(M * W + GUARD, FILL, np.uint32)
    Mb = 0 if base is None else len(base)
    check(lib.bm25_term_masks(index._h, p(mu), mu.shape[1], p(an), an.shape[1], p(mn),
                              mn.shape[1], M, p(base), Mb, p(buf)))
    assert (buf[M * W:] == FILL).all(), "guard words written"
    return buf[:M * W].reshape(M, W).copy()


def _device_raw(index, must, any_, must_not, M, base=None, stream=None):
    """term_masks_device on a non-default stream, pre-filled, guard words."""
    import torch
    W = (index.n_docs + 31) // 32
    st = stream or torch.cuda.Stream()
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    args = [None if c is None else up(_pad(c, M)) for c in (must, any_, must_not)]
    db = None if base is None else up(base.view(np.int32))
    buf = torch.full((M * W + GUARD,), FILL - (1 << 32), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()  # (the uploads ran on the current stream)
    index.term_masks_device(args[0], args[1], args[2], db, buf[:M * W].view(M, W), st)
    st.synchronize()
    got = buf.cpu().numpy().view(np.uint32)
    assert (got[M * W:] == FILL).all(), "guard words written"
    return got[:M * W].reshape(M, W).copy()


def _check(index, want, must, any_, must_not, M, base=None, what=""):
    """Host call and device call both give ``want`` word for word; the bits
    at or past n_docs are 0."""
    for name, got in (("host", _host_raw(index, must, any_, must_not, M, base)),
                      ("device", _device_raw(index, must, any_, must_not, M, base))):
        bad = np.nonzero(got != want)
        assert bad[0].size == 0, (what, name, f"{bad[0].size} words differ, first row "
                                  f"{bad[0][0]} word {bad[1][0]}: got {got[bad][0]:#x} "
                                  f"want {want[bad][0]:#x}")
        r = index.n_docs % 32
        if r:
            assert not (got[:, -1] >> np.uint32(r)).any(), (what, name, "bits past n_docs")


# the clause rows of the edge tests: (must, any, must_not)
ROWS = [
    ([FULL], [], []),                          # must of 1: every document
    ([FULL, HALF, ZEROV], [], []),             # must of 3 (a stored 0.0f counts)
    ([], [SLOT0, SLOTL], []),                  # any of 2: slot 0 or the last slot of a tile
    ([], [], [HALF]),                          # must_not alone
    ([HALF], [FIFTH, P5], [NEGV]),             # all three clauses at once
    ([FIFTH], [], [FIFTH]),                    # the same term in must and must_not: empty
    ([HALF, HALF], [ZEROV, ZEROV], []),        # duplicate ids
    ([-1, -1], [-1], [-1, -1, -1]),            # all padding: every document
    ([EMPTY], [], []),                         # a term with no posting: empty
    ([], [EMPTY], []),                         # ... in any: active, matches nothing
    ([], [], [EMPTY]),                         # ... in must_not: removes nothing
    ([-1, SLOT0], [], [-1, DOC0]),             # padding before the ids
    ([LASTDOC], [], []),
    ([], [DOC0, LASTDOC], [P1]),
    ([NEGV, FULL], [HALF], [SLOTL]),
]


# ------------------------------------------------------ 1. word and tile edges
@pytest.mark.parametrize("n_docs", [1, 31, 32, 33, 2047, 2048, 2049, 70_001])
@pytest.mark.parametrize("segments", ["dense", "sparse"])
def test_word_and_tile_edges(gpu, segments, n_docs):
    """Around the 32-document mask word and the 2048-document tile (one
    document ... 35 tiles with a partial last word and tile), both segment
    tables; the clause rows above in one call of three clauses, then must,
    any and must_not each alone (the other clauses of width 0), and no clause
    at all (every document)."""
    has, ip, ix, dt = _term_index(n_docs, 300 + n_docs)
    index = _idx(ip, ix, dt, n_docs, segments=segments)
    info = index.info()
    assert info["sparse"] == (segments == "sparse") and info["tile_docs"] == TILE
    M = len(ROWS)
    mu, an, mn = ([r[i] for r in ROWS] for i in range(3))
    want = _want(has, mu, an, mn, M)
    full = np.nonzero(has[FULL])[0]
    assert len(full) == n_docs and want[5].any() == False and want[8].any() == False  # noqa: E712
    _check(index, want, mu, an, mn, M, what="three clauses")
    assert np.array_equal(index.term_masks(mu, an, mn), want)
    for i, name in enumerate(("must", "any", "must_not")):
        cl = [None, None, None]
        cl[i] = [r[i] for r in ROWS]
        _check(index, _want(has, *cl, M), *cl, M, what=name + " alone")
    ones = _want(has, None, None, None, 3)
    assert int(np.unpackbits(ones.view(np.uint8)).sum()) == 3 * n_docs
    got = _device_raw(index, None, None, None, 3)
    assert np.array_equal(got, ones)
    index.close()


# --------------------------------------------------------------- 2. base masks
@pytest.mark.parametrize("segments", ["dense", "sparse"])
def test_base_masks(gpu, segments):
    """5000 documents (3 tiles, 8 documents in the last word): a base of one
    row for every mask and a base row per mask; packed rows with garbage bits
    past n_docs; a base whose words are zero for the whole of tile 1; a base
    of all ones; a base alone (no clause) is returned with its tail cleared."""
    import bm25mi
    n_docs = 5000
    has, ip, ix, dt = _term_index(n_docs, 77)
    index = _idx(ip, ix, dt, n_docs, segments=segments)
    rng = np.random.default_rng(78)
    M = len(ROWS)
    mu, an, mn = ([r[i] for r in ROWS] for i in range(3))
    one = rng.random((1, n_docs)) < 0.6
    per = rng.random((M, n_docs)) < 0.5
    per[3, TILE:2 * TILE] = False        # a whole tile of zero words
    per[4] = True                        # all ones
    per[7, :] = False                    # an all-zero base under an all-padding row
    hole = np.ones((1, n_docs), bool)
    hole[0, TILE:2 * TILE] = False
    for name, base in (("one row", one), ("row per mask", per), ("tile hole", hole),
                       ("all ones", np.ones((1, n_docs), bool))):
        want = _want(has, mu, an, mn, M, base)
        packed = bm25mi.pack_mask(base)
        _check(index, want, mu, an, mn, M, packed, what=name)
        garbage = packed.copy()
        garbage[:, -1] |= np.uint32(0xFFFFFF00)  # bits 8.. of the last word: past n_docs
        _check(index, want, mu, an, mn, M, garbage, what=name + " + garbage")
        assert np.array_equal(index.term_masks(mu, an, mn, base=base), want)
    # a base alone: M comes from the base
    garbage = bm25mi.pack_mask(per)
    garbage[:, -1] |= np.uint32(0xFFFFFF00)
    assert np.array_equal(index.term_masks(base=garbage), bm25mi.pack_mask(per))
    assert np.array_equal(_device_raw(index, None, None, None, M, garbage), bm25mi.pack_mask(per))
    index.close()


# -------------------------------------------------------- 3. out-of-range ids
def test_out_of_range_ids(gpu):
    """Host calls reject an id >= n_terms with the reference's message; in the
    device call it is a term that no document has: in must a zero row, in any
    (alone, or beside a real term) an active clause, in must_not no change."""
    n_docs = 4100
    has, ip, ix, dt = _term_index(n_docs, 5)
    index = _idx(ip, ix, dt, n_docs)
    for kw in ({"must": [[V]]}, {"any": [[HALF, V + 3]]}, {"must_not": [[V + 100]]}):
        with pytest.raises(ValueError, match=r"maximum token ID in the query \(1\d+\) is higher"):
            index.term_masks(**kw)
    q = np.array([[HALF, FIFTH]], np.int32)
    with pytest.raises(ValueError, match=r"maximum token ID in the query \(12\) is higher"):
        index.search_boolean(q, 3, must=[[V]])
    with pytest.raises(ValueError, match=r"maximum token ID in the query \(40\) is higher"):
        index.search_boolean(np.array([[40, FIFTH]], np.int32), 3, must=[[HALF]])
    mu = [[HALF, V + 3], [], [], [HALF], [2**31 - 1]]
    an = [[], [V], [V, FIFTH], [], []]
    mn = [[], [], [], [V + 100, P5], []]
    want = _want(has, mu, an, mn, 5)
    assert not want[0].any() and not want[1].any() and not want[4].any()
    assert np.array_equal(want[2], _want(has, None, [[FIFTH]], None, 1)[0])
    assert np.array_equal(want[3], _want(has, [[HALF]], None, [[P5]], 1)[0])
    assert np.array_equal(_device_raw(index, mu, an, mn, 5), want)
    index.close()


@pytest.mark.parametrize("segments", ["dense", "sparse"])
def test_clauses_wider_than_a_wave(gpu, segments):
    """The kernel looks a clause's terms up 64 at a step: clause rows of 64,
    65 and 130 ids whose deciding terms sit past the first 64 (behind padding,
    duplicates and terms without postings)."""
    n_docs = 4100
    has, ip, ix, dt = _term_index(n_docs, 9)
    index = _idx(ip, ix, dt, n_docs, segments=segments)
    mu = [[FULL] * 64 + [HALF], [-1] * 64 + [FIFTH, -1, HALF], [FULL] * 63 + [P5],
          [HALF] * 129 + [EMPTY]]
    an = [[EMPTY] * 64 + [P5, P1], [-1] * 129 + [SLOT0], [-1] * 64, [FULL]]
    mn = [[-1] * 64 + [NEGV], [EMPTY] * 70 + [LASTDOC], [ZEROV] * 64, []]
    want = _want(has, mu, an, mn, 4)
    assert want[0].any() and want[1].any() and want[2].any() and not want[3].any()
    assert not np.array_equal(want[0], _want(has, [[FULL]], [[EMPTY]], None, 1)[0])
    _check(index, want, mu, an, mn, 4)
    index.close()


# ------------------------------------- 4. boolean search equals filtered search
@pytest.fixture(scope="module")
def bool_case(gpu):
    """6000 documents (3 tiles), 60 terms, 7 queries with a clause row each;
    the masks by numpy and the allowed documents of row 0."""
    rng = np.random.default_rng(41)
    N, nt = 6000, 60
    ip, ix, dt = _rand_index(rng, N, nt, 3000)
    df = np.diff(ip)
    by_df = np.argsort(-df)
    a, b, c, d = (int(x) for x in by_df[:4])
    has = _has_of(ip, ix, nt, N)
    q = rng.integers(-1, nt, size=(7, 8)).astype(np.int32)
    mu = [[a], [a, b], [], [], [c], [b, b], [-1]]
    an = [[], [c, d], [a, d], [], [a, b], [], [-1, -1]]
    mn = [[b], [], [c], [a], [d], [b], []]
    masks = _want(has, mu, an, mn, 7)
    allowed = int(np.unpackbits(masks[0].view(np.uint8)).sum())
    assert 10 < allowed < 4096 and not masks[5].any()
    index = _idx(ip, ix, dt, N)
    yield index, q, mu, an, mn, masks, allowed, (ip, ix, dt, N, nt)
    index.close()


@pytest.mark.parametrize("k", [1, 10, "allowed-1", "allowed", "allowed+1", 4097])
def test_boolean_search_equals_filtered_search(bool_case, k):
    """search_boolean's rows equal search_filtered's over the numpy-built
    masks bit for bit (docs, and scores on their uint32 view), with k below,
    at and above row 0's allowed documents (padding) and past 4096 (the dense
    path), whatever bool_chunk (0 = automatic, 1, 3 on the 7-query batch)."""
    index, q, mu, an, mn, masks, allowed, _ = bool_case
    if isinstance(k, str):
        k = allowed + {"allowed-1": -1, "allowed": 0, "allowed+1": 1}[k]
    want = index.search_filtered(q, k, masks, np.arange(7, dtype=np.int32))
    assert (want[0][5] == -1).all()          # the empty mask: a fully padded row
    if k > allowed:
        assert (want[0][0][:allowed] >= 0).all() and (want[0][0][allowed:] == -1).all()
    try:
        for chunk in (0, 1, 3):
            index.set_option("bool_chunk", chunk)
            assert index.get_option("bool_chunk") == chunk
            got = index.search_boolean(q, k, mu, an, mn)
            assert got[0].dtype == np.int32 and got[1].dtype == np.float32
            _exact(got, want)
    finally:
        index.set_option("bool_chunk", 0)


def test_boolean_search_base_and_bm25v(bool_case):
    """A base of one row and of a row per query under the clauses, and the
    BM25v method on the same CSC matrix."""
    import bm25mi
    import bm25_native
    import scipy.sparse as sp
    index, q, mu, an, mn, masks, allowed, (ip, ix, dt, N, nt) = bool_case
    rng = np.random.default_rng(42)
    has = _has_of(ip, ix, nt, N)
    for base in (rng.random((1, N)) < 0.7, rng.random((7, N)) < 0.7):
        m2 = _want(has, mu, an, mn, 7, base)
        want = index.search_filtered(q, 25, m2, np.arange(7, dtype=np.int32))
        for chunk in (0, 3):
            index.set_option("bool_chunk", chunk)
            _exact(index.search_boolean(q, 25, mu, an, mn, base=base), want)
            _exact(index.search_boolean(q, 25, mu, an, mn, base=bm25mi.pack_mask(base)), want)
        index.set_option("bool_chunk", 0)
    model = bm25_native.BM25v()
    model.index(sp.csc_matrix((dt, ix, ip), shape=(N, nt)), np.ones(N, np.float32))
    want = index.search_filtered(q, 10, masks, np.arange(7, dtype=np.int32))
    _exact(model.search_boolean(q, 10, must=mu, any=an, must_not=mn), want)


# ---------------------------------------------------------- 5. doc shards compose
def test_doc_shards_compose(bool_case):
    """The index split at document 4096 into two shards (doc_offset): each
    shard builds its masks from its own postings on the device and searches
    filtered; the lists merged by merge_topk_device equal the single index's
    search_boolean."""
    import torch
    from bm25mi.index import merge_topk_device
    index, q, mu, an, mn, masks, allowed, (ip, ix, dt, N, nt) = bool_case
    cut, k = 2 * TILE, 40
    want = index.search_boolean(q, k, mu, an, mn)
    has = _has_of(ip, ix, nt, N)
    dq = torch.from_numpy(q).cuda()
    cl = [torch.from_numpy(_pad(c, 7)).cuda() for c in (mu, an, mn)]
    qm = torch.arange(7, dtype=torch.int32, device="cuda")
    outs_d = torch.full((2, 7, k), 99, dtype=torch.int32, device="cuda")
    outs_s = torch.full((2, 7, k), 7.5, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream()
    shards = []
    for r, (lo, hi) in enumerate(((0, cut), (cut, N))):
        sh = _idx(*_doc_slice(ip, ix, dt, lo, hi), hi - lo, doc_offset=lo)
        shards.append(sh)
        dm = torch.full((7, (hi - lo + 31) // 32), -1, dtype=torch.int32, device="cuda")
        sh.term_masks_device(cl[0], cl[1], cl[2], None, dm, st)
        torch.cuda.synchronize()
        assert np.array_equal(dm.cpu().numpy().view(np.uint32),
                              _want(has[:, lo:hi], mu, an, mn, 7))
        sh.search_filtered_device(dq, k, dm, qm, outs_d[r], outs_s[r], st)
    torch.cuda.synchronize()
    md = torch.empty((7, k), dtype=torch.int32, device="cuda")
    ms = torch.empty((7, k), dtype=torch.float32, device="cuda")
    merge_topk_device(0, outs_d, outs_s, 2, 7, k, md, ms, st)
    torch.cuda.synchronize()
    _exact((md.cpu().numpy(), ms.cpu().numpy()), want)
    for sh in shards:
        sh.close()


# ------------------------------------------- 6. independence from the workspace
def test_independent_of_the_search_workspace(bool_case):
    """term_masks_device enqueued on its own stream right after a
    search_device on another stream of the same handle: both are exact."""
    import torch
    index, q, mu, an, mn, masks, allowed, _ = bool_case
    want = index.search(q, 50)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    dq = torch.from_numpy(q).cuda()
    dd = torch.full((7, 50), 99, dtype=torch.int32, device="cuda")
    ds = torch.full((7, 50), 7.5, dtype=torch.float32, device="cuda")
    cl = [torch.from_numpy(_pad(c, 7)).cuda() for c in (mu, an, mn)]
    dm = torch.full((7, masks.shape[1]), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    index.search_device(dq, 50, dd, ds, s1)
    index.term_masks_device(cl[0], cl[1], cl[2], None, dm, s2)
    s1.synchronize()
    s2.synchronize()
    _exact((dd.cpu().numpy(), ds.cpu().numpy()), want)
    assert np.array_equal(dm.cpu().numpy().view(np.uint32), masks)
