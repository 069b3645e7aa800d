"""CPU tests of the sort-by-field search over doc shards
(bm25_sort_keys_device, bm25_sort_cursor_device, bm25_merge_sort_keys_device,
their Python wrappers, bm25mi.sort_keys / sort_key_values and
bm25mi.dist.sharded_search_sorted).

The model (tests/sorted_shards_model.py) is held against the single index
(tests/sorted_model.py): the keyed lists of 2, 3 and 5 doc shards of a
5000-document column, merged on (key, doc), are select_want over the whole —
and merged by their local ranks they are not, which is why the calls exist.
The C calls' argument checks precede any device call, so every BM25_EINVAL and
its message are tested here without a GPU; and sharded_search_sorted runs its
protocol (cursor translation, packing, a short shard's padding, one all-gather,
the merge's stride, the score sum) through a real 3-rank gloo group with numpy
stand-ins for the GPU calls."""
import ctypes

import numpy as np
import pytest

from facets_model import unpack_rows
from merge_collapse_model import CUTS
from range_model import pack_rows
from sorted_model import order_want, select_want
from sorted_shards_model import (PAD_KEY, cursor_rank_want, join, key_want, keys_of_docs,
                                 merge_want, planes, select_after_want, seven_valued,
                                 shard_sorted_lists)
from test_gpu_edges import TILE
from test_search_after_host import after_case, position_masks

SYMS = {"bm25_sort_keys_device": 9, "bm25_sort_cursor_device": 11,
        "bm25_merge_sort_keys_device": 12}
DTYPES = (np.int32, np.float32, np.int64)


# ------------------------------------------------------------- the bindings
def test_symbols_exported_bound_and_documented():
    from bm25mi import _capi
    text = open(_capi.HEADER).read()
    for sym, arity in SYMS.items():
        assert sym in _capi.header_symbols()
        f = getattr(_capi.lib, sym)
        assert f.restype is ctypes.c_int and sym in _capi._SIGS and len(f.argtypes) == arity
    doc = text[text.index("Sort-by-field search over doc shards: order keys"):
               text.index("int bm25_sort_keys_device(")]
    flat = " ".join(" ".join(line.strip().lstrip("*") for line in doc.splitlines()).split())
    for phrase in ("u = (uint32)v ^ 0x80000000", "NaN gives 1 << 32 in both directions",
                   "+-0.0 become bits 0", "u = sign ? ~bits : bits | 0x80000000",
                   "descending: (uint32)~u", "u = (uint64)v ^ (1 << 63)",
                   "(K ascending, global doc id ascending)",
                   "exactly the order bm25_sort_ranks builds", "same kind and direction",
                   "two uint32 planes", "never as an 8-byte word", "[3][Q][k]",
                   "Padding is doc -1 with key_hi = key_lo = 0xFFFFFFFF",
                   "recognised by the doc id, never by the key", "INT64_MAX",
                   "never synchronise", "take no scratch and retain nothing",
                   "no atomics on global memory", "are not searches",
                   "not ordered against the handle's searches",
                   "Every argument check runs before any device call",
                   "reads no value", "Nothing past n elements is written",
                   "(the doc of a padding slot: exhausted) -> -1",
                   "(no cursor) -> BM25_AFTER_NONE (-2)",
                   "c == 0 gives -2", "not -1, which would end the row", "otherwise c - 1",
                   "compared in 64 bits", "strictly after the cursor",
                   "need not name an existing document", "one binary search per row over d_perm",
                   "M may pass 65535", "makes that row unspecified",
                   "no value outside the column is read", "takes no handle",
                   "w * rank_stride + q * k", "3 * Q * k", "strictly ascending by (key, doc)",
                   "never read into a result", "unique across the lists",
                   "every output slot is written", "W = 1 returns its input",
                   "next page's collection cursor", "W > 64: merge in stages", "k > 4096",
                   "Q may pass 65535", "the kernel ends", "W k log k",
                   "Replaces no reference call"):
        assert phrase in flat, phrase
    block = text[text.index("Sort-by-field search:"):text.index("int bm25_sort_ranks(")]
    assert "Sort-by-field search over doc shards" in block   # the old block points here
    assert _capi.abi_version() == 1  # additive: the ABI version stays
    import bm25mi
    from bm25mi import dist, index
    assert bm25mi.merge_sort_keys_device is index.merge_sort_keys_device
    assert bm25mi.sort_keys is index.sort_keys and bm25mi.sort_key_values is index.sort_key_values
    assert callable(index.GpuIndex.sort_keys_device) and callable(index.GpuIndex.sort_cursor_device)
    assert callable(dist.sharded_search_sorted)


def _merge_call(W=2, Q=3, k=4, stride=None, null=()):
    from bm25mi._capi import lib
    n = max(W, 1) * max(Q, 1) * max(k, 1)
    bufs = {"docs": np.zeros(n, np.int32), "hi": np.zeros(n, np.uint32),
            "lo": np.zeros(n, np.uint32), "od": np.full(n, 7, np.int32),
            "oh": np.full(n, 7, np.uint32), "ol": np.full(n, 7, np.uint32)}
    p = lambda name: None if name in null else bufs[name].ctypes.data_as(ctypes.c_void_p)
    rc = lib.bm25_merge_sort_keys_device(0, p("docs"), p("hi"), p("lo"), W, Q, k,
                                         Q * k if stride is None else stride, p("od"), p("oh"),
                                         p("ol"), None)
    assert all((bufs[o] == 7).all() for o in ("od", "oh", "ol"))
    return rc, lib.bm25_last_error()


@pytest.mark.parametrize("kwargs,message", [
    (dict(W=0), b"W=0"), (dict(W=-3), b"W=-3"), (dict(W=65), b"W=65"),
    (dict(Q=-1, stride=0), b"Q=-1"), (dict(k=-1, stride=0), b"k=-1"),
    (dict(k=4097), b"k=4097"), (dict(stride=11), b"rank_stride=11"),
    (dict(stride=-1), b"rank_stride=-1"),
    (dict(null=("docs",)), b"NULL input"), (dict(null=("hi",)), b"NULL input"),
    (dict(null=("lo",)), b"NULL input"), (dict(null=("od",)), b"NULL output"),
    (dict(null=("oh",)), b"NULL output"), (dict(null=("ol",)), b"NULL output")])
def test_merge_einval_before_any_device_call(kwargs, message):
    from bm25mi._capi import BM25_EINVAL
    rc, msg = _merge_call(**kwargs)
    assert rc == BM25_EINVAL and message in msg and b"merge_sort_keys" in msg, msg
    if b"W=65" in message:
        assert b"merge in stages" in msg
    if b"k=4097" in message:
        assert b"4096" in msg


def test_merge_empty_shapes_are_ok_without_device_work():
    from bm25mi._capi import BM25_OK
    everything = ("docs", "hi", "lo", "od", "oh", "ol")
    assert _merge_call(Q=0, null=everything)[0] == BM25_OK
    assert _merge_call(k=0, null=everything)[0] == BM25_OK
    assert _merge_call(Q=0, k=0, stride=0, W=64)[0] == BM25_OK


def test_null_handle_is_einval_and_outputs_untouched():
    from bm25mi._capi import BM25_EINVAL, lib
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    v = np.arange(5, dtype=np.int32)
    docs = np.arange(5, dtype=np.int32)
    hi, lo, out = (np.full(5, 7, np.uint32), np.full(5, 7, np.uint32), np.full(5, 7, np.int32))
    for call in (lambda: lib.bm25_sort_keys_device(None, p(v), 0, 0, p(docs), 5, p(hi), p(lo), None),
                 lambda: lib.bm25_sort_cursor_device(None, p(v), 0, 0, p(docs), p(hi), p(lo),
                                                     p(docs), 5, p(out), None)):
        assert call() == BM25_EINVAL and b"NULL index" in lib.bm25_last_error()
    assert (hi == 7).all() and (lo == 7).all() and (out == 7).all()


def _fake_index(n_docs):
    """A GpuIndex without a handle: the wrappers' own checks run, and a call
    that passes them reaches C with a NULL index."""
    from bm25mi.index import GpuIndex
    ix = GpuIndex.__new__(GpuIndex)
    ix.n_docs, ix._h = n_docs, None
    return ix


def test_python_wrappers_reject_before_c():
    import torch
    from bm25mi.index import merge_sort_keys_device
    z = torch.zeros((2, 3, 4), dtype=torch.int32)
    o = torch.zeros((3, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match="W=65"):
        merge_sort_keys_device(0, z, z, z, 65, 3, 4, 12, o, o, o)
    with pytest.raises(ValueError, match="rank_stride=5"):
        merge_sort_keys_device(0, z, z, z, 2, 3, 4, 5, o, o, o)
    with pytest.raises(ValueError, match="d_key_hi must be a 32-bit integer tensor"):
        merge_sort_keys_device(0, z, z.view(torch.float32), z, 2, 3, 4, 12, o, o, o)
    with pytest.raises(ValueError, match=r"d_out_docs must be a contiguous 32-bit \[3, 4\]"):
        merge_sort_keys_device(0, z, z, z, 2, 3, 4, 12, o[:2], o, o)
    ix = _fake_index(6)
    v = torch.zeros(6, dtype=torch.int32)
    d = torch.zeros((2, 5), dtype=torch.int32)
    with pytest.raises(ValueError, match="int32, int64 or float32"):
        ix.sort_keys_device(v.to(torch.float64), d, d, d)
    with pytest.raises(ValueError, match=r"contiguous \[6\] tensor"):
        ix.sort_keys_device(v[:5], d, d, d)
    with pytest.raises(ValueError, match="d_docs must be a contiguous int32"):
        ix.sort_keys_device(v, d.to(torch.int64), d, d)
    with pytest.raises(ValueError, match="d_key_lo must be a contiguous 32-bit integer tensor"):
        ix.sort_keys_device(v, d, d, d[:1])
    with pytest.raises(ValueError, match="NULL index"):
        ix.sort_keys_device(v, d, d, d, True)
    a = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError, match=r"d_perm must be a contiguous int32 \[6\]"):
        ix.sort_cursor_device(v, v[:5], a, a, a, a)
    with pytest.raises(ValueError, match=r"d_after_ranks must be a contiguous int32 \[3\]"):
        ix.sort_cursor_device(v, v, a, a, a, a[:2])
    with pytest.raises(ValueError, match=r"d_after_key_hi must be a contiguous 32-bit integer \[3\]"):
        ix.sort_cursor_device(v, v, a.view(torch.float32), a, a, a)
    with pytest.raises(ValueError, match="NULL index"):
        ix.sort_cursor_device(v.to(torch.int64), v, a, a, a, a)


# ------------------------------------------------- model vs the single index
def _mask_rows():
    """Seven rows of the 5000-document fixture: none, 60 % and 30 % masks."""
    allow, qm = position_masks()
    return np.stack([np.ones(5000, bool) if m < 0 else allow[m] for m in qm])


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shards", [2, 3, 5])
def test_merged_shard_lists_are_the_single_index_rows(shards, dtype, descending):
    """The model's shard lists, keyed and merged on (key, doc), equal
    select_want over the whole, for k in {1, 10, 100}, plain and under masks;
    merged by local rank they do not."""
    cuts = CUTS[shards]
    assert (TILE in cuts or shards == 2) and any(c % 64 for c in cuts[1:-1])
    v = seven_valued(dtype)
    assert len(np.unique(key_want(v, descending))) == (6 if dtype == np.float32 else 7)
    ranks, perm = order_want(v, descending)
    keys = key_want(v, descending)
    rank_merge_differs = 0
    for allowed in (None, _mask_rows()):
        for k in (1, 10, 100):
            M = 2 if allowed is None else allowed.shape[0]
            want = select_want(M if allowed is None else allowed, ranks, perm, k)[0]
            lists = shard_sorted_lists(v, cuts, k, descending, allowed, M)
            got = merge_want(lists, k)
            assert np.array_equal(got[0], want), (k, allowed is None)
            assert np.array_equal(got[1], np.where(want >= 0, keys[want], PAD_KEY))
            rank_merge_differs += not np.array_equal(merge_want(lists, k, by=2)[0], want)
    # ranks are per handle: rank 0 of every shard comes first, whatever its value
    assert rank_merge_differs >= 4


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_model_cursors(n):
    """Every (key, doc) pair — keys no document has and docs outside the shard
    on both sides included: the rank cursor of cursor_rank_want, fed to
    select_want, selects exactly the documents strictly after the cursor in the
    collection's order."""
    off = 100
    for dtype in DTYPES:
        for descending in (False, True):
            v = np.array([-3, 0, 0, 5, 9, 5, -3], dtype)[np.arange(n) * 5 % 7]
            probe = np.array([-4, -3, -1, 0, 2, 5, 7, 9, 10], dtype)   # between and beyond
            ak = np.repeat(key_want(probe, descending), n + 6)
            ad = np.tile(np.concatenate([[0, off - 1], off + np.arange(n), [off + n, off + n + 1,
                                                                           2 ** 31 - 1, 5]]),
                         len(probe)).astype(np.int64)
            assert ak.shape == ad.shape
            ar = cursor_rank_want(v, descending, off, ak, ad)
            ranks, perm = order_want(v, descending)
            got = select_want(len(ad), ranks, perm, n, ar, off)[0]
            keys = key_want(v, descending)
            ids = off + np.arange(n)
            for m in range(len(ad)):
                after = (keys > ak[m]) | ((keys == ak[m]) & (ids > ad[m]))
                want = ids[np.lexsort((ids, keys))]
                want = want[after[want - off]]
                assert np.array_equal(got[m][:want.size], want) and (got[m][want.size:] == -1).all()
            # before everything: -2, not -1 (which would end the row); doc -1: -1
            lowest = np.uint64(keys.min())
            assert cursor_rank_want(v, descending, off, [lowest], [off - 1])[0] == -2
            assert cursor_rank_want(v, descending, off, [0], [0])[0] == -2
            assert cursor_rank_want(v, descending, off, [lowest, PAD_KEY], [-1, -1]).tolist() == [-1, -1]
            assert cursor_rank_want(v, descending, off, [PAD_KEY], [-2])[0] == -2
            assert cursor_rank_want(v, descending, off, [PAD_KEY], [2 ** 31 - 1])[0] == n - 1


def test_model_pages_across_shards():
    """Pages of 64 through collection cursors, every shard translating the
    cursor for itself, concatenate to the single-index list; the page after a
    padded page is all padding on every shard."""
    allowed = _mask_rows()
    allowed[2, np.flatnonzero(allowed[2])[150:]] = False   # 150 allowed: the third page is padded
    for dtype in DTYPES:
        v = seven_valued(dtype)
        one = select_after_want(v, True, allowed, 256)
        after, pages = None, []
        for _ in range(4):
            lists = shard_sorted_lists(v, CUTS[3], 64, True, allowed, after=after)
            page = merge_want(lists, 64)
            assert np.array_equal(page[0], select_after_want(v, True, allowed, 64, after)[0])
            pages.append(page)
            after = (page[1][:, -1], page[0][:, -1])
        assert np.array_equal(np.hstack([p[0] for p in pages]), one[0])
        assert np.array_equal(np.hstack([p[1] for p in pages]), one[1])
        assert pages[2][0][2, -1] == -1 and (pages[3][0][2] == -1).all()
        last = shard_sorted_lists(v, CUTS[3], 64, True, allowed, after=(pages[2][1][:, -1],
                                                                        pages[2][0][:, -1]))
        assert all((l[0][2] == -1).all() for l in last)


# ------------------------------------------------------------- the helpers
def _helper_cases():
    nan = np.float32("nan")
    yield np.array([np.iinfo(np.int32).min, np.iinfo(np.int32).max, -1, 0, 1, 7, 7], np.int32)
    yield np.array([np.iinfo(np.int64).min, np.iinfo(np.int64).max, -1, 0, 1, 2 ** 53,
                    2 ** 53 + 1, -2 ** 53 - 1, -2 ** 53], np.int64)   # pairs below float precision
    yield np.array([nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, 3.4e38, -3.4e38,
                    1.0, -1.0, np.float32(np.uint32(0xFFC00001).view(np.float32))], np.float32)
    rng = np.random.default_rng(1)
    yield rng.integers(-2 ** 31, 2 ** 31, 300).astype(np.int32)
    yield rng.integers(-2 ** 63, 2 ** 63 - 1, 300).astype(np.int64)
    yield rng.integers(0, 2 ** 32, 300).astype(np.uint32).view(np.float32)
    for dtype in DTYPES:
        yield np.zeros(0, dtype)


def test_sort_keys_helpers():
    """bm25mi.sort_keys equals key_want bit for bit and orders as order_want;
    sort_key_values(sort_keys(v)) is v except -0.0 -> +0.0 and NaN -> one NaN."""
    import bm25mi
    for v in _helper_cases():
        for descending in (False, True):
            got = bm25mi.sort_keys(v, descending)
            assert got.dtype == np.uint64 and got.shape == v.shape
            assert np.array_equal(got, key_want(v, descending)), (v.dtype, descending)
            perm = np.lexsort((np.arange(len(v)), got))
            assert np.array_equal(perm, order_want(v, descending)[1])
            back = bm25mi.sort_key_values(got, v.dtype, descending)
            assert back.dtype == v.dtype
            if v.dtype == np.float32:
                want = np.where(np.isnan(v), np.float32("nan"), np.where(v == 0, np.float32(0), v))
                assert np.array_equal(back.view(np.uint32), want.astype(np.float32).view(np.uint32))
            else:
                assert np.array_equal(back, v)
    a = np.array([2 ** 53, 2 ** 53 + 1], np.int64)
    assert bm25mi.sort_keys(a)[0] + 1 == bm25mi.sort_keys(a)[1]
    assert bm25mi.sort_keys(np.array([np.iinfo(np.int64).max]))[0] == PAD_KEY  # a real all-ones key
    with pytest.raises(ValueError, match="int32, int64 or float32"):
        bm25mi.sort_keys(np.zeros(3, np.float64))
    with pytest.raises(ValueError, match="int32, int64 or float32"):
        bm25mi.sort_key_values(np.zeros(3, np.uint64), np.int16)


# ------------------------------------- the sharded call's protocol, on gloo
PROTOCOL_CUTS = (0, 37, TILE, 5000)   # a shard of 37 documents, fewer than k
PROTOCOL_K = 100


def _protocol_column():
    return seven_valued(np.float32, seed=9)


def _dense_rows():
    """The fixture's dense score rows with -0.0 folded into +0.0 (the score
    sum's precondition: no addend is -0.0f)."""
    return [np.asarray(r, np.float32) + np.float32(0) for r in after_case(5000)[4]]


class _NumpySortedShard:
    """The GPU calls of a doc shard [lo, hi) on the host, by the model."""

    def __init__(self, values, rows, lo, hi, descending):
        self.v, self.lo, self.n_docs, self.desc = values[lo:hi], lo, hi - lo, descending
        self.rows = [r[lo:hi] for r in rows]
        self.order = order_want(self.v, descending)
        self.calls = []

    def sorted_scratch_bytes(self, M, k):
        assert 0 < k <= self.n_docs
        return 4 * M * (4 + 1 + 256 + min(k + 2048, self.n_docs))

    def sort_cursor_device(self, d_values, d_perm, d_hi, d_lo, d_docs, d_out, descending=False,
                           stream=None):
        import torch
        assert descending == self.desc and np.array_equal(d_perm.numpy(), self.order[1])
        self.calls.append("cursor")
        d_out.copy_(torch.from_numpy(cursor_rank_want(self.v, descending, self.lo,
                                                      join(d_hi.numpy(), d_lo.numpy()),
                                                      d_docs.numpy())))

    def search_sorted_device(self, d_masks, d_ranks, d_perm, k, d_after, d_docs, d_out_ranks,
                             d_scratch, stream=None):
        import torch
        M = d_docs.shape[0]
        assert k <= self.n_docs and tuple(d_docs.shape) == tuple(d_out_ranks.shape) == (M, k)
        assert d_docs.is_contiguous() and d_out_ranks.is_contiguous()
        assert d_scratch.numel() >= self.sorted_scratch_bytes(M, k)
        self.calls.append(("search", k))
        allowed = unpack_rows(d_masks.numpy().view(np.uint32), self.n_docs)
        d, r = select_want(allowed, d_ranks.numpy(), d_perm.numpy(), k,
                           None if d_after is None else d_after.numpy(), self.lo)
        d_docs.copy_(torch.from_numpy(d))
        d_out_ranks.copy_(torch.from_numpy(r))

    def sort_keys_device(self, d_values, d_docs, d_hi, d_lo, descending=False, stream=None):
        import torch
        assert descending == self.desc and d_docs.is_contiguous()
        assert d_hi.data_ptr() == d_docs.data_ptr() + 4 * d_docs.numel()   # the packed planes
        assert d_lo.data_ptr() == d_docs.data_ptr() + 8 * d_docs.numel()
        self.calls.append("keys")
        hi, lo = planes(keys_of_docs(self.v, descending, d_docs.numpy(), self.lo))
        d_hi.copy_(torch.from_numpy(hi.view(np.int32)))
        d_lo.copy_(torch.from_numpy(lo.view(np.int32)))

    def score_docs_device(self, d_queries, d_docs, d_scores, stream=None):
        import torch
        self.calls.append("score")
        docs = d_docs.numpy().astype(np.int64) - self.lo
        mine = (docs >= 0) & (docs < self.n_docs)
        out = np.zeros(docs.shape, np.float32)   # (another shard's document, padding: +0.0f)
        for q, row in enumerate(self.rows):
            out[q][mine[q]] = row[docs[q][mine[q]]]
        d_scores.copy_(torch.from_numpy(out))


def _merge_sort_keys_cpu(device, d_docs, d_hi, d_lo, W, Q, k, rank_stride, out_d, out_h, out_l,
                         stream=None):
    """bm25_merge_sort_keys_device on the host, for the packed gathered buffer."""
    import torch
    assert tuple(d_docs.shape) == (W, 3, Q, k) and d_docs.is_contiguous()
    assert rank_stride == 3 * Q * k
    assert d_hi.data_ptr() == d_docs.data_ptr() + 4 * Q * k
    assert d_lo.data_ptr() == d_docs.data_ptr() + 8 * Q * k
    g = d_docs.numpy()
    docs, keys = merge_want([(g[w, 0], join(g[w, 1], g[w, 2])) for w in range(W)], k)
    hi, lo = planes(keys)
    out_d.copy_(torch.from_numpy(docs))
    out_h.copy_(torch.from_numpy(hi.view(np.int32)))
    out_l.copy_(torch.from_numpy(lo.view(np.int32)))


def _protocol_worker(rank, world, port, out):
    import os
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import bm25mi.index as bi
        from bm25mi.dist import sharded_search_sorted
        bi.merge_sort_keys_device = _merge_sort_keys_cpu  # the host stand-in of the HIP merge
        lo, hi = PROTOCOL_CUTS[rank], PROTOCOL_CUTS[rank + 1]
        v = _protocol_column()
        shard = _NumpySortedShard(v, _dense_rows(), lo, hi, True)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        dm = t(pack_rows(_mask_rows()[:, lo:hi]).view(np.int32))
        order = (t(shard.order[0]), t(shard.order[1]))
        dq = t(after_case(5000)[3])
        p1 = sharded_search_sorted(shard, dm, t(v[lo:hi]), order, PROTOCOL_K, True, d_queries=dq)
        ks = min(PROTOCOL_K, hi - lo)
        assert shard.calls == [("search", ks), "keys", "score"]
        after = (p1[0][:, -1].clone(), p1[1][:, :, -1].clone())
        p2 = sharded_search_sorted(shard, dm, t(v[lo:hi]), order, PROTOCOL_K, True, after)
        assert shard.calls[3:] == ["cursor", ("search", ks), "keys"] and len(p2) == 2
        if rank == 0:
            np.savez(out, d1=p1[0].numpy(), k1=p1[1].numpy(), s1=p1[2].numpy().view(np.int32),
                     d2=p2[0].numpy(), k2=p2[1].numpy())
    finally:
        dist.destroy_process_group()


def test_gloo_sharded_search_sorted_protocol(tmp_path):
    """sharded_search_sorted through a real 3-rank gloo group on the host: each
    rank's list packed as [3, M, k], a 37-document shard padded to k, one
    all-gather, the merge fed rank_stride = 3 M k, the cursor handed over
    across two pages, the scores summed over the ranks — the single index's
    200 first hits, keys and score bits."""
    import socket
    import time
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / "r.npz")
    ctx = mp.spawn(_protocol_worker, args=(3, port, out), nprocs=3, join=False)
    deadline = time.monotonic() + 120
    try:
        while not ctx.join(timeout=5):
            assert time.monotonic() < deadline, "a rank is stuck"
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
    got = np.load(out)
    v, allowed = _protocol_column(), _mask_rows()
    ranks, perm = order_want(v, True)
    want = select_want(allowed, ranks, perm, 2 * PROTOCOL_K)[0]
    keys = key_want(v, True)
    assert np.array_equal(np.hstack([got["d1"], got["d2"]]), want)
    gk = np.concatenate([got["k1"], got["k2"]], axis=2)
    assert np.array_equal(join(gk[0], gk[1]), np.where(want >= 0, keys[want], PAD_KEY))
    rows = _dense_rows()
    bits = np.stack([rows[q][want[q, :PROTOCOL_K]].view(np.uint32) for q in range(len(rows))])
    assert np.array_equal(got["s1"].view(np.uint32), bits)
