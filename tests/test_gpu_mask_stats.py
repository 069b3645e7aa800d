"""GPU tests of the field statistics (bm25_mask_stats(_device);
bm25mi_stats.hip).

The expected values come from tests/stats_model.py (rows unpacked to bool,
count / min / max by numpy, wrapping int64 sums, the float sum by 32 Python-int
bins, a carry loop and one rounding — bit-equal to math.fsum); they never go
through the code under test.  Every check runs through the host call and
through the device call (a non-default stream, the mask buffer one word off a
16-byte boundary), into buffers pre-filled with -7 that carry 64 guard entries,
and compares bit for bit.  The shapes sit next to

  32      documents per mask word
  64      documents of a step, 256 of a wave's span (8 mask words)
  8192    kStatsChunk: documents of a workgroup's chunk, on both routes
  4608    kStatsLdsSlots: u64 LDS slots of a workgroup; a float32 record is 36
          slots, an integer record 4, so
  128     float32 buckets (1152 integer buckets) are the last LDS shape, 129
          (1153) the first global-atomic shape
  64      kStatsMaxRows: R = min(64, 128 / B) float32 rows share a block
          (ungrouped and G = 2: 64; G = 7: 18)"""
import ctypes
import itertools

import numpy as np
import pytest

import stats_model as sm
from facets_model import unpack_rows
from test_gpu_parity import _exact, _idx, _rand_index

pytestmark = pytest.mark.gpu

FILL = -7
GUARD = 64
CHUNK, MAXROWS = 8192, 64
LDS_F32, LDS_INT = 128, 1152
FLT_MAX = np.float32(3.4028234663852886e38)
KEYS = ("count", "min", "max", "sum")


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None and a.size else None


@pytest.fixture(scope="module")
def make(gpu):
    """index_of(n_docs): a handle over n_docs documents (one term, one
    posting: the stats calls read the caller's buffers only)."""
    made = {}

    def index_of(n_docs):
        if n_docs not in made:
            made[n_docs] = _idx(np.array([0, 1], np.int64), np.zeros(1, np.int32),
                                np.ones(1, np.float32), n_docs)
        return made[n_docs]
    yield index_of
    for ix in made.values():
        ix.close()


def _dtypes(values):
    return {"count": np.dtype(np.int64), "min": values.dtype, "max": values.dtype,
            "sum": np.dtype(np.float64 if values.dtype.kind == "f" else np.int64)}


def _host_raw(index, packed, values, groups, G, outs=KEYS):
    """bm25_mask_stats into pre-filled buffers with guard entries; the outputs
    not named in outs are passed as NULL."""
    from bm25mi._capi import check, lib
    from bm25mi.index import _SORT_KINDS
    M, B = packed.shape[0], G or 1
    bufs = {k: np.full(M * B + GUARD, FILL, dt) for k, dt in _dtypes(values).items() if k in outs}
    pg = None if groups is None else groups.ctypes.data_as(ctypes.c_void_p)
    check(lib.bm25_mask_stats(index._h, _p(packed), M, _p(values), _SORT_KINDS[values.dtype], pg,
                              G, *[_p(bufs.get(k)) for k in KEYS]))
    for k, b in bufs.items():
        assert (b[M * B:] == FILL).all(), ("guard entries written", k)
    return {k: b[:M * B].reshape(M, B).copy() for k, b in bufs.items()}


def _device_raw(index, packed, values, groups, G, outs=KEYS, stream=None):
    """stats_device on a non-default stream: the masks start one word past a
    16-byte boundary, the outputs are pre-filled and carry guard entries, the
    scratch is the caller's, of exactly stats_scratch_bytes."""
    import torch
    M, W = packed.shape
    B = G or 1
    st = stream or torch.cuda.Stream()
    dm = torch.zeros(M * W + 1, dtype=torch.int32, device="cuda")
    dm[1:] = torch.from_numpy(np.ascontiguousarray(packed).view(np.int32).reshape(-1)).cuda()
    assert dm.data_ptr() % 16 == 0
    dv = torch.from_numpy(values).cuda()
    dg = None if groups is None else torch.from_numpy(groups).cuda()
    bufs = {k: torch.full((M * B + GUARD,), FILL, dtype=getattr(torch, dt.name), device="cuda")
            for k, dt in _dtypes(values).items() if k in outs}
    nbytes = index.stats_scratch_bytes(values.dtype, M, G)
    assert nbytes == 8 * M * B * (36 if values.dtype.kind == "f" else 4) <= 288 * M * B
    scr = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda")   # (not cleared)
    torch.cuda.synchronize()  # (the uploads ran on the current stream)
    view = lambda k: bufs[k][:M * B].view(M, B) if k in bufs else None
    index.stats_device(dm[1:].view(M, W), dv, view("count"), view("min"), view("max"),
                       view("sum"), dg, G, scr, st)
    st.synchronize()
    got = {}
    for k, b in bufs.items():
        a = b.cpu().numpy()
        assert (a[M * B:] == FILL).all(), ("guard entries written", k)
        got[k] = a[:M * B].reshape(M, B).copy()
    return got


def _compare(got, want, what):
    for k in got:
        if sm.same_bits(got[k], want[k]):
            continue
        bad = np.nonzero(got[k].view(np.uint8).reshape(got[k].shape + (-1,)) !=
                         want[k].view(np.uint8).reshape(want[k].shape + (-1,)))
        m, b = int(bad[0][0]), int(bad[1][0])
        raise AssertionError((what, k, f"row {m} bucket {b}: got {got[k][m, b]!r} "
                                       f"want {want[k][m, b]!r}"))


def _check(index, packed, values, groups=None, G=0, what="", host=True, want=None):
    """Host call (unless the groups are out of range, which it rejects) and
    device call both give the model's count, min, max and sum, bit for bit."""
    packed = np.ascontiguousarray(packed, dtype=np.uint32)
    values = np.ascontiguousarray(values)
    groups = None if groups is None else np.ascontiguousarray(groups, dtype=np.int32)
    if want is None:
        want = sm.stats_want(packed, values, groups, G)
    calls = [("device", _device_raw)] + ([("host", _host_raw)] if host else [])
    for name, call in calls:
        _compare(call(index, packed, values, groups, G), want, (what, name))
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


def _column(rng, n_docs, dtype):
    """A random column: float32 over 60 binades with NaN, -0.0 and both signs;
    integers over the whole range of the dtype."""
    dt = np.dtype(dtype)
    if dt.kind == "f":
        v = (10.0 ** rng.uniform(-9, 9, n_docs) * rng.choice([-1.0, 1.0], n_docs)).astype(dt)
        v[rng.random(n_docs) < 0.05] = np.nan
        v[rng.random(n_docs) < 0.05] = -0.0
        return v
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, n_docs, dtype=dt, endpoint=True)


# ------------------------------------------------------------ 1. the document axis
ROUTES = {"lds_f32": (np.float32, 0), "lds_i64_g7": (np.int64, 7),
          "global_f32": (np.float32, LDS_F32 + 1), "global_i32": (np.int32, LDS_INT + 1)}
DOCS = [1, 31, 32, 33, 64, 65, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 5]


@pytest.mark.parametrize("route,n_docs", [(r, n) for r in ROUTES for n in DOCS])
def test_document_axis(make, route, n_docs):
    """Word, step, span and chunk edges of each route (M = 3 with an odd W
    leaves rows 1 and 2 misaligned, on top of the device buffer's one-word
    offset); garbage tail bits; the last document counts in the all-ones row."""
    dtype, G = ROUTES[route]
    rng = np.random.default_rng(n_docs + G)
    values = _column(rng, n_docs, dtype)
    values[-1] = 3
    groups = _groups(rng, n_docs, G) if G else None
    if G:
        groups[-1] = G - 1
    want = _check(make(n_docs), _masks(rng, 3, n_docs), values, groups, G, (route, n_docs))
    assert want["count"][2, -1] >= 1
    if not G and dtype is not np.float32:
        assert want["count"][2, 0] == n_docs


# --------------------------------------------------------------------- 2. row blocks
def _row_kinds(rng, M, n_docs):
    """Random rows, with an empty row, a full row and a row of one document per
    64-document step among them (as far as M allows)."""
    import bm25mi
    allow = rng.random((M, n_docs)) < 0.3
    allow[M - 1] = True
    if M > 2:
        allow[0] = False
        allow[1] = False
        starts = np.arange(0, n_docs, 64)
        allow[1, np.minimum(starts + rng.integers(0, 64, len(starts)), n_docs - 1)] = True
    return _garbage_tail(bm25mi.pack_mask(allow), n_docs)


@pytest.mark.parametrize("G", [0, 2, 7])
@pytest.mark.parametrize("M", [1, MAXROWS - 1, MAXROWS, MAXROWS + 1])
def test_row_blocks(make, M, G):
    """Ungrouped and G = 2 give R = 64 float32 rows per block: one row, a block
    short of one row, full, and one row over; G = 7: R = 18, several blocks."""
    n_docs = 3001
    rng = np.random.default_rng(M + G)
    packed = _row_kinds(rng, M, n_docs)
    values = _column(rng, n_docs, np.float32)
    want = _check(make(n_docs), packed, values, _groups(rng, n_docs, G) if G else None, G, (M, G))
    if M > 2:
        assert want["count"][0].sum() == 0 and want["sum"][0].tobytes() == bytes(8 * (G or 1))
        assert 0 < want["count"][1].sum() <= 47
    _check(make(n_docs), packed, _column(rng, n_docs, np.int64), None, 0, (M, "i64"))


def test_more_rows_than_65535(make):
    """70 000 rows of 2 words over 33 documents, ungrouped float32 and G = 2
    int32: 64 distinct rows repeated (the model runs on the distinct ones)."""
    n_docs, M = 33, 70_000
    rng = np.random.default_rng(5)
    distinct = _masks(rng, 64, n_docs)
    pick = rng.integers(0, 64, M)
    pick[[0, 65_536, M - 1]] = 63, 62, 63
    packed = np.ascontiguousarray(distinct[pick])
    for dtype, G in ((np.float32, 0), (np.int32, 2)):
        values = _column(rng, n_docs, dtype)
        groups = _groups(rng, n_docs, G) if G else None
        small = sm.stats_want(distinct, values, groups, G)
        want = {k: np.ascontiguousarray(v[pick]) for k, v in small.items()}
        _check(make(n_docs), packed, values, groups, G, dtype, want=want)
        assert want["count"][65_536:].sum() > 0 and want["count"][M - 1].sum() > 0


def test_no_rows_is_ok_and_writes_nothing(make):
    """M == 0 returns BM25_OK without writing (host and device calls)."""
    import torch
    from bm25mi._capi import BM25_OK, lib
    index = make(70)
    packed = np.full((2, 3), 0xFFFFFFFF, np.uint32)
    values = np.ones(70, np.float32)
    buf = np.full(GUARD, FILL, np.int64)
    assert lib.bm25_mask_stats(index._h, _p(packed), 0, _p(values), 1, None, 0, _p(buf), _p(buf),
                               _p(buf), _p(buf)) == BM25_OK
    assert (buf == FILL).all()
    got = index.stats(packed[:0], values)
    assert all(got[k].shape == (0, 1) for k in ("count", "min", "max", "sum", "mean"))
    dbuf = torch.full((GUARD,), FILL, dtype=torch.int64, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    index.stats_device(torch.zeros((0, 3), dtype=torch.int32, device="cuda"),
                       torch.from_numpy(values).cuda(), dbuf[:0].view(0, 1), stream=st)
    st.synchronize()
    assert (dbuf.cpu().numpy() == FILL).all()


# ----------------------------------------------------------------- 3. the bucket axis
@pytest.mark.parametrize("dtype,G", [(np.float32, g) for g in (1, 7, LDS_F32, LDS_F32 + 1)] +
                         [(np.int64, g) for g in (1, 7, LDS_INT, LDS_INT + 1)] +
                         [(np.int32, 7), (np.int32, LDS_INT + 1)])
def test_bucket_axis(make, dtype, G):
    """Each G at 5000 documents, 20 % of them without a group (negative ids,
    INT_MIN among them): the last LDS shape and the first global one per kind."""
    n_docs = 5000
    rng = np.random.default_rng(G)
    groups = _groups(rng, n_docs, G)
    groups[::11] = np.iinfo(np.int32).min
    want = _check(make(n_docs), _masks(rng, 3, n_docs), _column(rng, n_docs, dtype), groups, G,
                  (dtype, G))
    assert want["count"].sum() > 0 and want["count"][2].sum() <= (groups >= 0).sum()


@pytest.mark.parametrize("dtype", [np.float32, np.int64])
def test_100_000_buckets(make, dtype):
    """G = 100 000 at 257 documents: mostly empty buckets, all written as 0."""
    n_docs, G = 257, 100_000
    rng = np.random.default_rng(8)
    want = _check(make(n_docs), _masks(rng, 2, n_docs), _column(rng, n_docs, dtype),
                  _groups(rng, n_docs, G), G, dtype)
    assert (want["count"] == 0).sum() > 2 * (G - n_docs) and want["count"].sum() > 0


@pytest.mark.parametrize("G,hot", [(1, 0), (7, 3), (LDS_F32, LDS_F32 - 1), (LDS_F32 + 1, 100)])
def test_every_document_in_one_group(make, G, hot):
    """All-ones masks over documents of one group: 64 lanes on one record."""
    n_docs = 5000
    rng = np.random.default_rng(G)
    packed = _garbage_tail(np.full((2, (n_docs + 31) // 32), 0xFFFFFFFF, np.uint32), n_docs)
    groups = np.full(n_docs, hot, np.int32)
    for dtype in (np.float32, np.int64):
        values = _column(rng, n_docs, dtype)
        want = _check(make(n_docs), packed, values, groups, G, (G, hot, dtype))
        number = n_docs if dtype is np.int64 else int((~np.isnan(values)).sum())
        assert (want["count"][:, hot] == number).all() and want["count"].sum() == 2 * number


@pytest.mark.parametrize("dtype,G", [(np.float32, 1), (np.float32, 7), (np.int64, LDS_INT + 1)])
def test_groups_at_or_past_G(make, dtype, G):
    """5 % of the ids >= G (G itself and 2^31 - 1 among them): the device call
    puts them in no bucket; the host call rejects the array, names the first
    such document and its value, and leaves the outputs untouched."""
    from bm25mi._capi import BM25_EINVAL, lib
    from bm25mi.index import _SORT_KINDS
    n_docs = 5000
    rng = np.random.default_rng(G + 1)
    packed = _masks(rng, 3, n_docs)
    values = _column(rng, n_docs, dtype)
    groups = _groups(rng, n_docs, G)
    over = np.nonzero(rng.random(n_docs) < 0.05)[0]
    groups[over] = rng.integers(G, 2**31, len(over))
    groups[over[0]], groups[over[1]] = G, 2**31 - 1
    want = _check(make(n_docs), packed, values, groups, G, G, host=False)
    clean = np.where(groups >= G, -1, groups).astype(np.int32)
    _compare(want, sm.stats_want(packed, values, clean, G), "clean")
    bufs = [np.full(3 * G + GUARD, FILL, dt) for dt in _dtypes(values).values()]
    index = make(n_docs)
    assert lib.bm25_mask_stats(index._h, _p(packed), 3, _p(values), _SORT_KINDS[values.dtype],
                               _p(groups), G, *[_p(b) for b in bufs]) == BM25_EINVAL
    msg = lib.bm25_last_error().decode()
    assert f"groups[{over[0]}] = {G}" in msg, msg
    assert all((b == FILL).all() for b in bufs)
    with pytest.raises(ValueError, match=rf"groups\[{over[0]}\] = {G} "):
        index.stats(packed, values, groups, G)


def test_groups_and_G_come_together(make):
    """Exactly one of (groups == NULL, G == 0) is EINVAL, outputs untouched."""
    from bm25mi._capi import BM25_EINVAL, lib
    index = make(70)
    packed = np.full((2, 3), 0xFFFFFFFF, np.uint32)
    values = np.ones(70, np.int32)
    groups = np.zeros(70, np.int32)
    buf = np.full(GUARD, FILL, np.int64)
    for pg, G in ((None, 4), (_p(groups), 0)):
        assert lib.bm25_mask_stats(index._h, _p(packed), 2, _p(values), 0, pg, G, _p(buf), None,
                                   None, None) == BM25_EINVAL
        assert b"groups and G come together" in lib.bm25_last_error()
    assert lib.bm25_mask_stats(index._h, _p(packed), 2, _p(values), 3, None, 0, _p(buf), None,
                               None, None) == BM25_EINVAL   # a bad kind
    assert (buf == FILL).all()


# -------------------------------------------------------------- 4. float32 columns
def _float_columns(n):
    rng = np.random.default_rng(23)
    big = np.where(np.arange(n) % 2 == 0, 1e30, -1e30).astype(np.float32)
    big[rng.random(n) < 0.3] = 1e-40
    bits = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
    mixed = _column(rng, n, np.float32)
    mixed[rng.random(n) < 0.4] = np.nan
    one = lambda x: np.where(np.arange(n) == n // 2, x, rng.standard_normal(n)).astype(np.float32)
    return {
        "nan_everywhere": np.full(n, np.nan, np.float32),
        "nan_mixed_in": mixed,
        "zeros_of_both_signs": np.where(rng.random(n) < 0.5, 0.0, -0.0).astype(np.float32),
        "negative_zeros": np.full(n, -0.0, np.float32),
        "subnormals": (rng.integers(1, 2**23, n).astype(np.uint32)
                       | (rng.integers(0, 2, n).astype(np.uint32) << 31)).view(np.float32),
        "big_pairs_and_tiny": big,
        "all_flt_max": np.full(n, FLT_MAX, np.float32),
        "all_minus_flt_max": np.full(n, -FLT_MAX, np.float32),
        "plus_inf": one(np.inf), "minus_inf": one(-np.inf),
        "both_infs": np.where(np.arange(n) == 3, -np.inf, one(np.inf)).astype(np.float32),
        "random_bits": bits,
    }


@pytest.mark.parametrize("name", list(_float_columns(8)))
def test_float_columns(make, name):
    """One chunk and 77 documents (8269) of each column, ungrouped and G = 5,
    under an all-ones row (a chunk of FLT_MAX stresses the partial
    accumulators: 8192 x FLT_MAX in one record), a random row and an empty one."""
    n_docs = CHUNK + 77
    values = _float_columns(n_docs)[name]
    rng = np.random.default_rng(len(name))
    packed = _masks(rng, 3, n_docs)
    packed[0] = 0
    _garbage_tail(packed, n_docs)
    index = make(n_docs)
    for groups, G in ((None, 0), (_groups(rng, n_docs, 5), 5)):
        want = _check(index, packed, values, groups, G, (name, G))
        assert want["count"][0].sum() == 0
        full = want["count"][2].sum()
        if name == "nan_everywhere":
            assert want["count"].sum() == 0
            assert all(want[k].tobytes() == bytes(want[k].nbytes) for k in KEYS)
        elif name in ("zeros_of_both_signs", "negative_zeros"):
            assert full > 0
            assert all(want[k].tobytes() == bytes(want[k].nbytes) for k in ("min", "max", "sum"))
        elif name == "all_flt_max" and not G:
            assert want["sum"][2, 0] == n_docs * float(FLT_MAX) and want["min"][2, 0] == FLT_MAX
        elif name == "plus_inf" and not G:
            assert want["sum"][2, 0] == np.inf and want["max"][2, 0] == np.inf
        elif name == "minus_inf" and not G:
            assert want["sum"][2, 0] == -np.inf and want["min"][2, 0] == -np.inf
        elif name == "both_infs" and not G:
            assert np.isnan(want["sum"][2, 0]) and want["count"][2, 0] == n_docs
        elif name == "big_pairs_and_tiny" and not G:
            assert 0 < abs(want["sum"][2, 0]) < 1e-30 or abs(want["sum"][2, 0]) >= 1e29


# --------------------------------------------------------------- 5. integer columns
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
@pytest.mark.parametrize("G", [0, 5, LDS_INT + 1])
def test_integer_columns(make, dtype, G):
    """INT_MIN / INT_MAX extremes (alone, and mixed), sums that wrap int64, and
    all-equal values."""
    n_docs = 5000
    info = np.iinfo(dtype)
    rng = np.random.default_rng(G + info.bits)
    packed = _masks(rng, 3, n_docs)
    groups = _groups(rng, n_docs, G) if G else None
    index = make(n_docs)
    ends = rng.choice(np.array([info.min, info.max], dtype), n_docs)
    ends[:100] = info.max   # (so the two ends do not cancel)
    want = _check(index, packed, ends, groups, G, "extremes")
    if dtype is np.int64 and not G:
        exact = int((ends == info.max).sum()) * info.max + int((ends == info.min).sum()) * info.min
        assert exact != int(want["sum"][2, 0]) == (exact + 2**63) % 2**64 - 2**63   # it wrapped
        assert want["min"][2, 0] == info.min and want["max"][2, 0] == info.max
    for value in (info.min, info.max, 0, -1, 12345):
        _check(index, packed, np.full(n_docs, value, dtype), groups, G, ("equal", value))
    _check(index, packed, _column(rng, n_docs, dtype), groups, G, "random")


# ------------------------------------------------------------------ 6. NULL outputs
@pytest.mark.parametrize("dtype,G", [(np.float32, 0), (np.int64, 5), (np.float32, LDS_F32 + 1)])
def test_null_outputs(make, dtype, G):
    """out_min / out_max / out_sum NULL in every combination: the outputs that
    are asked for are the full call's."""
    n_docs = 3001
    rng = np.random.default_rng(G)
    packed = _masks(rng, 3, n_docs)
    values = _column(rng, n_docs, dtype)
    groups = _groups(rng, n_docs, G) if G else None
    index = make(n_docs)
    want = sm.stats_want(packed, values, groups, G)
    for n in range(4):
        for extra in itertools.combinations(("min", "max", "sum"), n):
            outs = ("count",) + extra
            for call in (_host_raw, _device_raw):
                got = call(index, packed, values, groups, G, outs)
                assert set(got) == set(outs)
                _compare(got, want, (outs, call.__name__))


def test_scratch_too_small_is_einval(make):
    """scratch_bytes one below bm25_mask_stats_scratch, a NULL scratch and a
    misaligned one: EINVAL before any launch, the outputs untouched."""
    import torch
    from bm25mi._capi import BM25_EINVAL, BM25_OK, lib
    n_docs, M = 300, 3
    index = make(n_docs)
    rng = np.random.default_rng(1)
    packed = _masks(rng, M, n_docs)
    values = _column(rng, n_docs, np.float32)
    need = index.stats_scratch_bytes(np.float32, M, 0)
    assert need == M * 288 and index.stats_scratch_bytes(np.int64, M, 7) == M * 7 * 32
    dm = torch.from_numpy(packed.view(np.int32)).cuda()
    dv = torch.from_numpy(values).cuda()
    dc = torch.full((M + GUARD,), FILL, dtype=torch.int64, device="cuda")
    scr = torch.zeros(need + 8, dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    call = lambda sp, sb: lib.bm25_mask_stats_device(
        index._h, vp(dm), M, vp(dv), 1, None, 0, vp(dc), None, None, None, sp, sb,
        ctypes.c_void_p(st.cuda_stream))
    assert call(vp(scr), need - 1) == BM25_EINVAL
    assert b"scratch_bytes" in lib.bm25_last_error()
    assert call(None, need) == BM25_EINVAL
    assert call(ctypes.c_void_p(scr.data_ptr() + 4), need) == BM25_EINVAL
    assert b"8-byte aligned" in lib.bm25_last_error()
    st.synchronize()
    assert (dc.cpu().numpy() == FILL).all()
    assert call(vp(scr), need) == BM25_OK
    st.synchronize()
    assert np.array_equal(dc.cpu().numpy()[:M], sm.stats_want(packed, values)["count"][:, 0])
    with pytest.raises(ValueError, match="d_scratch must be"):
        index.stats_device(dm.view(M, -1), dv, dc[:M].view(M, 1), d_scratch=scr[:need - 8],
                           stream=st)


# -------------------------------------------------------------------- 7. identities
def test_identities_with_mask_count_and_facets(make):
    """No NaN in the column: ungrouped count == mask_count, grouped count ==
    facets; integer kinds: sum over groups + the sum of the allowed documents
    without a group == the ungrouped sum, in wrapping int64.  GpuIndex.stats
    returns the five keys, mean = sum / count and NaN where count is 0."""
    n_docs, G = 5000, 37
    rng = np.random.default_rng(6)
    packed = _masks(rng, 5, n_docs, 0.3)
    packed[0] = 0
    groups = _groups(rng, n_docs, G)
    index = make(n_docs)
    for dtype in (np.float32, np.int32, np.int64):
        values = _column(rng, n_docs, dtype)
        if dtype is np.float32:
            values[np.isnan(values)] = 1.5
        flat = index.stats(packed, values)
        by_g = index.stats(packed, values, groups, G)
        assert tuple(flat) == ("count", "min", "max", "sum", "mean")
        _compare({k: flat[k] for k in KEYS}, sm.stats_want(packed, values), "flat")
        _compare({k: by_g[k] for k in KEYS}, sm.stats_want(packed, values, groups, G), "by_g")
        assert np.array_equal(flat["count"][:, 0], index.mask_count(packed))
        assert np.array_equal(by_g["count"], index.facets(packed, groups, G))
        assert flat["mean"].dtype == np.float64 and np.isnan(flat["mean"][0, 0])
        some = flat["count"] > 0
        assert np.array_equal(flat["mean"][some],
                              flat["sum"][some].astype(np.float64) / flat["count"][some])
        if dtype is not np.float32:
            allowed = unpack_rows(packed, n_docs)
            with np.errstate(over="ignore"):
                rest = np.array([values[a & (groups < 0)].astype(np.int64).sum(dtype=np.int64)
                                 for a in allowed])
                total = by_g["sum"].sum(axis=1, dtype=np.int64) + rest
            assert np.array_equal(total, flat["sum"][:, 0])


def test_doc_shards_combine(make):
    """Handles over [0, 2048) and [2048, 5000) of one collection: counts add,
    min and max combine, integer sums add (wrapping)."""
    import bm25mi
    n, h, G = 5000, 2048, 5
    rng = np.random.default_rng(7)
    allow = rng.random((4, n)) < 0.4
    groups = _groups(rng, n, G)
    values = _column(rng, n, np.int64)
    whole = _check(make(n), bm25mi.pack_mask(allow), values, groups, G, "whole")
    lo = _check(make(h), bm25mi.pack_mask(allow[:, :h]), values[:h], groups[:h], G, "lo")
    hi = _check(make(n - h), bm25mi.pack_mask(allow[:, h:]), values[h:], groups[h:], G, "hi")
    assert np.array_equal(lo["count"] + hi["count"], whole["count"])
    with np.errstate(over="ignore"):
        assert np.array_equal(lo["sum"] + hi["sum"], whole["sum"])
    both = (lo["count"] > 0) & (hi["count"] > 0)
    assert both.any()
    assert np.array_equal(np.minimum(lo["min"], hi["min"])[both], whole["min"][both])
    assert np.array_equal(np.maximum(lo["max"], hi["max"])[both], whole["max"][both])


# ------------------------------------------------------ 8. scheduling independence
@pytest.mark.parametrize("G", [0, 7, LDS_F32 + 1])
def test_same_bits_whatever_the_schedule(make, G):
    """The same float32 call twice, on two streams, and with the rows of the
    same masks in another order (other row blocks, other items): identical
    bits every time."""
    import torch
    n_docs, M = 2 * CHUNK + 5, 70
    rng = np.random.default_rng(G + 3)
    packed = _masks(rng, M, n_docs, 0.4)
    values = (10.0 ** rng.uniform(-20, 20, n_docs) * rng.choice([-1.0, 1.0], n_docs)
              ).astype(np.float32)
    groups = _groups(rng, n_docs, G) if G else None
    index = make(n_docs)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    first = _device_raw(index, packed, values, groups, G, stream=s1)
    _compare(first, sm.stats_want(packed, values, groups, G), "model")
    _compare(_device_raw(index, packed, values, groups, G, stream=s1), first, "again")
    _compare(_device_raw(index, packed, values, groups, G, stream=s2), first, "other stream")
    perm = rng.permutation(M)
    moved = _device_raw(index, np.ascontiguousarray(packed[perm]), values, groups, G, stream=s2)
    _compare(moved, {k: np.ascontiguousarray(v[perm]) for k, v in first.items()}, "row order")
    _compare(_host_raw(index, packed, values, groups, G), first, "host call")


# ----------------------------------------------------------------- 9. not a search
@pytest.fixture(scope="module")
def search_case(gpu):
    """6000 documents (3 tiles), 60 terms, 7 queries and 7 random masks."""
    rng = np.random.default_rng(41)
    N, nt = 6000, 60
    ip, ix, dt = _rand_index(rng, N, nt, 3000)
    q = rng.integers(-1, nt, size=(7, 8)).astype(np.int32)
    masks = _masks(rng, 7, N, 0.3)
    values = _column(rng, N, np.float32)
    groups = _groups(rng, N, 11)
    index = _idx(ip, ix, dt, N)
    yield index, q, masks, values, groups, 11
    index.close()


def test_not_a_search(search_case):
    """After a search_filtered, stats (host and device calls) leave
    last_dispatch() and filtered_stats() as they were."""
    index, q, masks, values, groups, G = search_case
    index.search_filtered(q, 10, masks, np.arange(7, dtype=np.int32))
    before = (index.last_dispatch(), index.search_stats(), index.filtered_stats())
    _check(index, masks, values, groups, G)
    _check(index, masks, values)
    assert (index.last_dispatch(), index.search_stats(), index.filtered_stats()) == before


def test_beside_a_search_on_another_stream(search_case):
    """stats_device enqueued on its own stream right after a search_device on
    another stream of the same handle: both are exact."""
    import torch
    index, q, masks, values, groups, G = search_case
    want = index.search(q, 50)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    dq = torch.from_numpy(q).cuda()
    dd = torch.full((7, 50), 99, dtype=torch.int32, device="cuda")
    ds = torch.full((7, 50), 7.5, dtype=torch.float32, device="cuda")
    dm = torch.from_numpy(masks.view(np.int32)).cuda()
    dv = torch.from_numpy(values).cuda()
    dg = torch.from_numpy(groups).cuda()
    out = {"count": torch.full((7, G), FILL, dtype=torch.int64, device="cuda"),
           "min": torch.full((7, G), FILL, dtype=torch.float32, device="cuda"),
           "max": torch.full((7, G), FILL, dtype=torch.float32, device="cuda"),
           "sum": torch.full((7, G), FILL, dtype=torch.float64, device="cuda")}
    scr = torch.empty(index.stats_scratch_bytes(np.float32, 7, G), dtype=torch.uint8,
                      device="cuda")
    torch.cuda.synchronize()
    index.search_device(dq, 50, dd, ds, s1)
    index.stats_device(dm, dv, out["count"], out["min"], out["max"], out["sum"], dg, G, scr, s2)
    s1.synchronize()
    s2.synchronize()
    _exact((dd.cpu().numpy(), ds.cpu().numpy()), want)
    _compare({k: v.cpu().numpy() for k, v in out.items()},
             sm.stats_want(masks, values, groups, G), "beside a search")
