"""GPU tests of the sort-by-field search over doc shards
(bm25_sort_keys_device, bm25_sort_cursor_device, bm25_merge_sort_keys_device;
bm25mi_sorted_shards.hip; bm25mi.dist.sharded_search_sorted).

The expected keys, rank cursors and merged rows come from numpy
(tests/sorted_shards_model.py, tests/sorted_model.py); they never go through
the code under test, and every comparison is exact.  Every call runs on a
non-default stream into outputs pre-filled with a marker between guard words.
The constants as built and the shapes that sit next to them:

  64        lanes of a wave; the merge kernel at k <= 128 is one wave: k 63, 64,
            65; n and n_docs 63, 64, 65
  128/1024  the k at which the merge takes its next kernel (KCAP 128 with 64
            threads, 1024 with 256, 4096 with 1024): k 65 and 130; k 4096
  256       threads of a block of the keys and cursor kernels: n 5000, M 70 000
            (a grid past 65535 rows for the merge: Q 70 000)
  64        the largest W"""
import os
import socket
import time

import numpy as np
import pytest
import torch.multiprocessing as mp

from merge_collapse_model import CUTS, shard_csc
from range_model import pack_rows
from sorted_model import order_want, select_want
from sorted_shards_model import (PAD_KEY, cursor_rank_want, join, key_want, keys_of_docs,
                                 merge_want, planes, select_after_want, seven_valued)
from test_gpu_parity import _idx
from test_search_after_host import after_case

pytestmark = pytest.mark.gpu

MARK_I32 = 0xA5A5A5A5 - (1 << 32)
GUARD = 64
DTYPES = (np.int32, np.float32, np.int64)


@pytest.fixture(scope="module")
def make(gpu):
    """index_of(n_docs, doc_offset): a handle over n_docs documents (one term,
    one posting: the calls read the caller's buffers only)."""
    made = {}

    def index_of(n_docs, doc_offset=0):
        if (n_docs, doc_offset) not in made:
            made[n_docs, doc_offset] = _idx(np.array([0, 1], np.int64), np.zeros(1, np.int32),
                                            np.ones(1, np.float32), n_docs, doc_offset=doc_offset)
        return made[n_docs, doc_offset]
    yield index_of
    for ix in made.values():
        ix.close()


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _guarded(n, count=1):
    import torch
    return [torch.full((GUARD + n + GUARD,), MARK_I32, dtype=torch.int32, device="cuda")
            for _ in range(count)]


def _inner(buf, n):
    return buf[GUARD:GUARD + n]


def _read(buf, n):
    a = buf.cpu().numpy()
    assert (a[:GUARD] == MARK_I32).all() and (a[GUARD + n:] == MARK_I32).all(), "guard words written"
    return a[GUARD:GUARD + n].copy()


def run_keys(index, values, descending, docs):
    """sort_keys_device -> uint64 keys of docs' shape."""
    import torch
    docs = np.ascontiguousarray(docs, np.int32)
    n = docs.size
    st = torch.cuda.Stream()
    dv, dd = _dev(values), _dev(docs)
    hi, lo = _guarded(n, 2)
    torch.cuda.synchronize()
    index.sort_keys_device(dv, dd, _inner(hi, n).view(docs.shape), _inner(lo, n).view(docs.shape),
                           descending, st)
    st.synchronize()
    return join(_read(hi, n).view(np.uint32), _read(lo, n).view(np.uint32)).reshape(docs.shape)


def run_cursor(index, values, descending, perm, after_keys, after_docs):
    """sort_cursor_device -> int32 [M]."""
    import torch
    M = len(after_docs)
    st = torch.cuda.Stream()
    hi, lo = planes(after_keys)
    dv, dp, dh, dl = _dev(values), _dev(perm), _dev(hi), _dev(lo)
    dd = _dev(np.asarray(after_docs, np.int32))
    out, = _guarded(M)
    torch.cuda.synchronize()
    index.sort_cursor_device(dv, dp, dh, dl, dd, _inner(out, M), descending, st)
    st.synchronize()
    return _read(out, M)


def run_merge(docs, keys, k, packed):
    """merge_sort_keys_device over docs / keys [W, Q, k] -> (docs, keys uint64)
    [Q, k]; packed: through one [W, 3, Q, k] buffer and rank_stride 3 Q k."""
    import torch
    import bm25mi
    W, Q, _ = docs.shape
    hi, lo = planes(keys)
    st = torch.cuda.Stream()
    if packed:
        g = _dev(np.stack([docs.astype(np.int32), hi.view(np.int32), lo.view(np.int32)], axis=1))
        ins, stride = (g, g[:, 1], g[:, 2]), 3 * Q * k
    else:
        ins, stride = (_dev(docs.astype(np.int32)), _dev(hi), _dev(lo)), Q * k
    outs = _guarded(Q * k, 3)
    torch.cuda.synchronize()
    bm25mi.merge_sort_keys_device(0, *ins, W, Q, k, stride, *[_inner(o, Q * k) for o in outs], st)
    st.synchronize()
    d, h, l = (_read(o, Q * k).reshape(Q, k) for o in outs)
    return d, join(h.view(np.uint32), l.view(np.uint32))


# ------------------------------------------------------------------ 1. keys
@pytest.mark.parametrize("dtype", DTYPES)
def test_keys(make, dtype):
    """Both directions, a handle at doc_offset 0 and one whose last document is
    id 2^31 - 1; d_docs mixes real ids, -1, other negatives and ids just below
    and just above the handle's range: bit-equal to the model, guards intact."""
    n_docs = 5000
    rng = np.random.default_rng(21)
    edge = seven_valued(dtype, n_docs)
    spread = (rng.standard_normal(n_docs) * 1e3).astype(dtype)
    for off in (0, 2 ** 31 - n_docs, 777):
        index = make(n_docs, off)
        lo_id, hi_id = off, off + n_docs - 1
        outside = [-1, -2, -2 ** 31, off - 1 if off else -3,
                   hi_id + 1 if hi_id + 1 < 2 ** 31 else 0, 0 if off else -7]
        for values in (edge, spread):
            for descending in (False, True):
                for n in (1, 63, 64, 65, 5000):
                    docs = rng.integers(lo_id, hi_id + 1, n)
                    if n > 1:
                        bad = rng.random(n) < 0.3
                        docs[bad] = rng.choice(outside, int(bad.sum()))
                        docs[0], docs[1], docs[-1] = lo_id, -1, hi_id
                    got = run_keys(index, values, descending, docs)
                    want = keys_of_docs(values, descending, docs, off)
                    assert np.array_equal(got, want), (off, descending, n)
                    assert n == 1 or ((want == PAD_KEY).any() and (want != PAD_KEY).any())
    # a 2-D page, as the packed buffer holds it
    index = make(n_docs, 777)
    docs = rng.integers(700, 6000, (7, 33))
    assert np.array_equal(run_keys(index, edge, True, docs), keys_of_docs(edge, True, docs, 777))


# --------------------------------------------------------------- 2. cursors
def _cursor_grid(values, descending, off, n, dtype):
    """Every (key, doc): the column's keys, keys between and beyond them, the
    padding key; docs of the shard, on both sides of it, -1 and < -1."""
    probe = np.unique(np.concatenate([values, np.array([-4, -1, 2, 7, 10], dtype)]))
    ks = np.concatenate([key_want(probe, descending), [np.uint64(0), PAD_KEY]])
    ds = np.concatenate([[0, off - 1], off + np.arange(min(n, 70)), [off + n - 1, off + n,
                         2 ** 31 - 1, -1, -2, -9]])
    return np.repeat(ks, len(ds)), np.tile(ds, len(ks))


@pytest.mark.parametrize("n_docs", [1, 64, 65, 5000])
def test_cursors(make, n_docs):
    off = 1000
    index = make(n_docs, off)
    rng = np.random.default_rng(n_docs)
    for dtype in DTYPES:
        base = np.array([-3, 0, 0, 5, 9, 5, -3], dtype) if n_docs < 100 else None
        values = base[np.arange(n_docs) * 5 % 7] if base is not None else seven_valued(dtype, n_docs)
        for descending in (False, True):
            perm = order_want(values, descending)[1]
            if n_docs < 100:
                ak, ad = _cursor_grid(values, descending, off, n_docs, dtype)
            else:  # a sample of the grid, and random documents' own (key, doc)
                ak, ad = _cursor_grid(values, descending, off, n_docs, dtype)
                pick = rng.integers(0, len(ak), 600)
                d = rng.integers(0, n_docs, 600)
                ak = np.concatenate([ak[pick], key_want(values, descending)[d]])
                ad = np.concatenate([ad[pick], off + d])
            got = run_cursor(index, values, descending, perm, ak, ad)
            want = cursor_rank_want(values, descending, off, ak, ad)
            assert np.array_equal(got, want), (n_docs, dtype, descending)
            assert (want == -1).any() and (want == -2).any() and (want >= 0).any()


def test_cursors_more_rows_than_65535(make):
    """70 000 rows at 65 documents: the grid of test_cursors tiled."""
    n_docs, off = 65, 1000
    values = np.array([-3, 0, 0, 5, 9, 5, -3], np.int64)[np.arange(n_docs) * 5 % 7]
    perm = order_want(values, True)[1]
    ak, ad = _cursor_grid(values, True, off, n_docs, np.int64)
    want = cursor_rank_want(values, True, off, ak, ad)
    reps = -(-70_000 // len(ak))
    idx = np.tile(np.arange(len(ak)), reps)[:70_000]
    got = run_cursor(make(n_docs, off), values, True, perm, ak[idx], ad[idx])
    assert np.array_equal(got, want[idx])


def test_cursor_survives_a_bad_perm(make):
    """perm entries outside [0, n_docs): no value outside the column is read
    (nothing faults), and rows whose search meets no such entry are right."""
    n_docs, off = 64, 0
    values = np.arange(n_docs, dtype=np.int32)
    perm = order_want(values, False)[1].copy()
    perm[60] = 10 ** 9
    perm[61] = -5
    ak, ad = key_want(values[[0, 1, 2, 3, 4, 5, 6, 7, 62]], False), np.array([0, 1, 2, 3, 4, 5, 6, 7, 62])
    got = run_cursor(make(n_docs, off), values, False, perm, ak, ad)   # (the last row meets them)
    assert np.array_equal(got[:8], np.arange(8))


# ----------------------------------------------------------------- 3. merge
def _random_lists(rng, W, Q, k, live=None):
    """W strictly ordered lists per row over unique docs, ragged (empty ones
    included), keys from a small set so that entries differ in key_hi only,
    key_lo only or the doc only; behind a list's end: doc < 0 and, after it,
    garbage that looks real."""
    docs = np.full((W, Q, k), -1, np.int32)
    keys = np.zeros((W, Q, k), np.uint64)     # (padding keys are not canonical: 0 sorts first)
    his = np.array([0, 1, 2, 0xFFFFFFFF], np.uint64)
    los = np.array([0, 1, 0x80000000, 0xFFFFFFFF], np.uint64)
    for q in range(Q):
        pool = rng.permutation(4 * W * k + 8)[:rng.integers(0, W * k + 1)]
        owner = rng.integers(0, W, len(pool))
        if live is not None:
            owner[:] = live
        if q == 0:
            pool = pool[:0]                  # a row whose lists are all empty
        kk = (his[rng.integers(0, 4, len(pool))] << np.uint64(32)) | los[rng.integers(0, 4, len(pool))]
        for w in range(W):
            sel = owner[:len(pool)] == w
            d, ky = pool[sel], kk[sel]
            o = np.lexsort((d, ky))[:k]
            docs[w, q, :o.size], keys[w, q, :o.size] = d[o], ky[o]
            if o.size + 1 < k:               # behind the first padding: never read into a result
                docs[w, q, o.size + 1:] = rng.integers(-3, 10 ** 6, k - o.size - 1)
    return docs, keys


def _check_merge(docs, keys, k, what):
    W = docs.shape[0]
    want = merge_want([(docs[w], keys[w]) for w in range(W)], k)
    for packed in (False, True):
        got = run_merge(docs, keys, k, packed)
        assert np.array_equal(got[0], want[0]), (what, packed, "docs")
        assert np.array_equal(got[1], want[1]), (what, packed, "keys")
    return want


@pytest.mark.parametrize("k", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("W", [1, 2, 3, 8, 64])
def test_merge_random_lists(gpu, W, k):
    rng = np.random.default_rng(1000 * W + k)
    docs, keys = _random_lists(rng, W, 6, k)
    want = _check_merge(docs, keys, k, (W, k))
    assert (want[0][0] == -1).all() and (want[0] >= 0).any()
    if W > 1:
        docs, keys = _random_lists(rng, W, 3, k, live=W - 1)   # one live list
        _check_merge(docs, keys, k, (W, k, "one live"))


def test_merge_largest_k(gpu):
    """k = 4096: W = 3, and W = 64 on 4 rows."""
    rng = np.random.default_rng(4096)
    for W, Q in ((3, 2), (64, 4)):
        docs, keys = _random_lists(rng, W, Q, 4096)
        docs[:, 1, :] = -1
        per = 4096 if W == 3 else 200     # row 1: full lists (W = 3), 64 lists of 200
        pool = rng.permutation(10 ** 6)[:W * per].reshape(W, per)
        ky = rng.integers(0, 50, (W, per)).astype(np.uint64) << np.uint64(30)
        for w in range(W):
            o = np.lexsort((pool[w], ky[w]))
            docs[w, 1, :per], keys[w, 1, :per] = pool[w][o], ky[w][o]
        want = _check_merge(docs, keys, 4096, (W, "k 4096"))
        assert (want[0][1] >= 0).all()


def test_merge_more_rows_than_65535(gpu):
    """Q = 70 000 at k = 3: 70 distinct rows, tiled."""
    rng = np.random.default_rng(7)
    docs, keys = _random_lists(rng, 2, 70, 3)
    want = merge_want([(docs[w], keys[w]) for w in range(2)], 3)
    got = run_merge(np.tile(docs, (1, 1000, 1)), np.tile(keys, (1, 1000, 1)), 3, True)
    assert np.array_equal(got[0], np.tile(want[0], (1000, 1)))
    assert np.array_equal(got[1], np.tile(want[1], (1000, 1)))


def test_merge_edges(gpu):
    """Entries that differ only in key_hi, only in key_lo, only in the doc; a
    real entry with the all-ones key ahead of padding; all lists empty; W = 1
    returns its input with padding made canonical."""
    k = 4
    P = int(PAD_KEY)
    rows = [  # (list 0, list 1) of (key, doc)
        ([(1 << 32, 5), (2 << 32, 1)], [(0xFFFFFFFF, 9), (3 << 32, 0)]),          # key_hi
        ([(7, 5), (9, 1)], [(8, 9), (10, 0)]),                                      # key_lo
        ([(7, 5), (7, 11)], [(7, 2), (7, 8)]),                                      # the doc
        ([(5, 3), (P, 4)], [(P, 2)]),                                               # all ones, real
        ([], []),
        ([(P, 2 ** 31 - 1)], [(0, 0)]),
    ]
    docs = np.full((2, len(rows), k), -1, np.int32)
    keys = np.zeros((2, len(rows), k), np.uint64)
    for q, pair in enumerate(rows):
        for w, lst in enumerate(pair):
            for j, (ky, d) in enumerate(lst):
                docs[w, q, j], keys[w, q, j] = d, ky
    want = _check_merge(docs, keys, k, "edges")
    assert want[0].tolist() == [[9, 5, 1, 0], [5, 9, 1, 0], [2, 5, 8, 11], [3, 2, 4, -1],
                                [-1] * 4, [0, 2 ** 31 - 1, -1, -1]]
    assert want[1][3].tolist() == [5, P, P, P] and want[0][3][2] == 4   # a real all-ones entry
    one = run_merge(docs[:1], keys[:1], k, False)
    assert np.array_equal(one[0], docs[0])
    assert np.array_equal(one[1], np.where(docs[0] >= 0, keys[0], PAD_KEY))


# ------------------------------------------------- 4. three handles equal one
def _fixture_masks():
    rng = np.random.default_rng(5)
    n = 5000
    tenant = (np.arange(n) * 7 % 16) == 3
    sparse = np.zeros(n, bool)
    sparse[rng.choice(n, 5, replace=False)] = True          # 0.1 %
    return np.stack([rng.random(n) < 0.9, tenant, sparse])


def _shard_page(handles, cuts, values, descending, orders, allowed, M, k, after):
    """Every shard's search_sorted_device (under its mask slice, from the
    collection cursor) and sort_keys_device -> docs, keys [W, M, k]."""
    import torch
    docs = np.full((len(handles), M, k), -1, np.int32)
    keys = np.full((len(handles), M, k), PAD_KEY, np.uint64)
    for w, (h, lo, hi) in enumerate(zip(handles, cuts[:-1], cuts[1:])):
        ranks, perm = orders[w]
        ar = None
        if after is not None:
            ar = run_cursor(h, values[lo:hi], descending, perm, after[0], after[1])
        ks = min(k, hi - lo)
        st = torch.cuda.Stream()
        dm = None if allowed is None else _dev(pack_rows(allowed[:, lo:hi]))
        dd, dr = _guarded(M * ks, 2)
        scratch = None if allowed is None else torch.empty(h.sorted_scratch_bytes(M, ks),
                                                           dtype=torch.uint8, device="cuda")
        dranks, dperm, dafter = _dev(ranks), _dev(perm), None if ar is None else _dev(ar)
        torch.cuda.synchronize()
        h.search_sorted_device(dm, dranks, dperm, ks, dafter, _inner(dd, M * ks).view(M, ks),
                               _inner(dr, M * ks).view(M, ks), scratch, st)
        st.synchronize()
        docs[w, :, :ks] = _read(dd, M * ks).reshape(M, ks)
        keys[w] = run_keys(h, values[lo:hi], descending, docs[w])
    return docs, keys


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_three_shards_equal_one_handle(make, dtype, descending):
    """The 5000-document column cut at 1111 and 2048 into three handles, each
    with the ranks of its own slice: searched, keyed and merged they give one
    handle's search_sorted over the whole (docs) and the model's keys; pages of
    64 through collection cursors concatenate to the one-handle list."""
    cuts = CUTS[3]
    values = seven_valued(dtype)
    whole = make(5000)
    order = whole.sort_ranks(values, descending)
    assert np.array_equal(order[1], order_want(values, descending)[1])
    handles = [make(hi - lo, lo) for lo, hi in zip(cuts[:-1], cuts[1:])]
    orders = [h.sort_ranks(values[lo:hi], descending)
              for h, lo, hi in zip(handles, cuts[:-1], cuts[1:])]
    allkeys = key_want(values, descending)
    masks = _fixture_masks()
    rank_merge_differs = 0
    for allowed, M in ((None, 2), (masks, 3)):
        for k in (10, 100):
            want = whole.search_sorted(M if allowed is None else allowed, order, k)[0]
            assert np.array_equal(want, select_want(M if allowed is None else allowed, order[0],
                                                    order[1], k)[0])
            docs, keys = _shard_page(handles, cuts, values, descending, orders, allowed, M, k, None)
            got = run_merge(docs, keys, k, True)
            assert np.array_equal(got[0], want), (k, allowed is None)
            assert np.array_equal(got[1], np.where(want >= 0, allkeys[np.maximum(want, 0)], PAD_KEY))
            if allowed is not None:
                assert (want[2, 5:] == -1).all() and (want[2, :5] >= 0).all()
    # pages of 64
    one = whole.search_sorted(masks, order, 256)[0]
    after, pages = None, []
    for _ in range(4):
        docs, keys = _shard_page(handles, cuts, values, descending, orders, masks, 3, 64, after)
        if after is not None and (after[1][2] == -1):   # after a padded page: padding on every shard
            assert (docs[:, 2] == -1).all()
        page = run_merge(docs, keys, 64, True)
        pages.append(page[0])
        after = (page[1][:, -1], page[0][:, -1])
    assert np.array_equal(np.hstack(pages), one)
    assert np.array_equal(one, select_after_want(values, descending, masks, 256)[0])


# ------------------------------- 5. sharded_search_sorted, real process groups
DIST_CUTS = {1: (0, 5000), 2: (0, 37, 5000), 3: (0, 37, 2048, 5000)}  # 37 documents < k
DIST_K = 100


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _dist_masks():
    m = _fixture_masks()
    rng = np.random.default_rng(8)
    return np.vstack([m, rng.random((4, 5000)) < 0.5])     # 7 rows, one per query


def _worker(rank, world, port, data, out):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from bm25mi.dist import sharded_search_sorted
        from bm25mi.index import GpuIndex
        z = np.load(data)
        lo, hi = DIST_CUTS[world][rank], DIST_CUTS[world][rank + 1]
        index = GpuIndex(*shard_csc(z["ip"], z["ix"], z["dt"], lo, hi), hi - lo, device=0,
                         doc_offset=lo)
        dq = torch.from_numpy(z["q"]).cuda()
        dm = torch.from_numpy(np.ascontiguousarray(pack_rows(z["allow"][:, lo:hi])).view(np.int32)).cuda()
        stream = torch.cuda.Stream()   # a non-current stream: the body must order on it
        res = {}
        for name, desc in (("f32", True), ("i64", False)):
            dv = torch.from_numpy(np.ascontiguousarray(z[name][lo:hi])).cuda()
            dr = torch.empty(hi - lo, dtype=torch.int32, device="cuda")
            dp = torch.empty(hi - lo, dtype=torch.int32, device="cuda")
            index.sort_ranks_device(dv, dr, dp, desc)
            torch.cuda.synchronize()
            p1 = sharded_search_sorted(index, dm, dv, (dr, dp), DIST_K, desc, d_queries=dq,
                                       stream=stream)
            torch.cuda.synchronize()
            after = (p1[0][:, -1].contiguous(), p1[1][:, :, -1].contiguous())
            torch.cuda.synchronize()
            p2 = sharded_search_sorted(index, dm, dv, (dr, dp), DIST_K, desc, after, stream=stream)
            p3 = sharded_search_sorted(index, None, dv, (dr, dp), 7, desc, rows=2, stream=stream)
            torch.cuda.synchronize()
            assert len(p2) == 2 and len(p3) == 2
            res[name + "_d"] = np.hstack([p1[0].cpu().numpy(), p2[0].cpu().numpy()])
            res[name + "_k"] = np.concatenate([p1[1].cpu().numpy(), p2[1].cpu().numpy()], axis=2)
            res[name + "_s"] = p1[2].cpu().numpy().view(np.int32)
            res[name + "_all"] = p3[0].cpu().numpy()
        if rank == 0:
            np.savez(out, **res)
        index.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [1, 2, 3])
def test_sharded_search_sorted_real_process_group(gpu, tmp_path, world):
    """1, 2 and 3 gloo ranks sharing cuda:0, each with its doc shard (one of 37
    documents, fewer than k = 100), on a non-current stream: rank 0's two pages
    are the single index's first 200 hits and keys, its scores score_docs'
    bits with 0xFFFFFFFF where the doc is -1."""
    ip, ix, dt, q, rows = after_case(5000)
    allow = _dist_masks()
    cols = {"f32": seven_valued(np.float32, seed=12), "i64": seven_valued(np.int64, seed=13)}
    data, out = str(tmp_path / "in.npz"), str(tmp_path / "r.npz")
    np.savez(data, ip=ip, ix=ix, dt=dt, q=q, allow=allow, **cols)
    ctx = mp.spawn(_worker, args=(world, _free_port(), data, out), nprocs=world, join=False)
    deadline = time.monotonic() + 120
    try:
        while not ctx.join(timeout=5):
            assert time.monotonic() < deadline, "a rank is stuck"
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
    got = np.load(out)
    whole = _idx(ip, ix, dt, 5000)
    try:
        for name, desc in (("f32", True), ("i64", False)):
            v = cols[name]
            ranks, perm = order_want(v, desc)
            want = select_want(allow, ranks, perm, 2 * DIST_K)[0]
            assert (want[2, 5:] == -1).all()     # the 0.1 % row: padded pages
            assert np.array_equal(got[name + "_d"], want), (name, world)
            keys = np.where(want >= 0, key_want(v, desc)[np.maximum(want, 0)], PAD_KEY)
            gk = got[name + "_k"].view(np.uint32)
            assert np.array_equal(join(gk[0], gk[1]), keys), (name, world)
            first = want[:, :DIST_K]
            sc = whole.score_docs(q, np.where(first < 0, 0, first))
            bits = np.where(first < 0, np.uint32(0xFFFFFFFF), sc.view(np.uint32))
            assert np.array_equal(got[name + "_s"].view(np.uint32), bits), (name, world)
            assert np.array_equal(got[name + "_all"], np.stack([perm[:7], perm[:7]]))
    finally:
        whole.close()


# -------------------------------------------------------------- 6. not a search
def test_not_a_search(gpu):
    """After a search, sort_keys_device and sort_cursor_device leave
    last_dispatch(), search_stats() and filtered_stats() as they were."""
    ip, ix, dt, q, rows = after_case(5000)
    index = _idx(ip, ix, dt, 5000)
    try:
        allowed = _dist_masks()
        index.search_filtered(q, 10, pack_rows(allowed), np.arange(7, dtype=np.int32))
        before = (index.last_dispatch(), index.search_stats(), index.filtered_stats())
        v = seven_valued(np.int64)
        perm = order_want(v, False)[1]
        docs = np.arange(-3, 60)
        assert np.array_equal(run_keys(index, v, False, docs), keys_of_docs(v, False, docs))
        ak, ad = key_want(v[:9], False), np.arange(9)
        assert np.array_equal(run_cursor(index, v, False, perm, ak, ad),
                              cursor_rank_want(v, False, 0, ak, ad))
        assert (index.last_dispatch(), index.search_stats(), index.filtered_stats()) == before
    finally:
        index.close()
