"""GPU tests of the doc-shard merge of collapsed lists
(bm25_merge_collapsed_device: merge_collapsed_kernel of
bm25mi_merge_collapse.hip) and of bm25mi.dist.sharded_search_collapsed.

The expected rows come from tests/merge_collapse_model.py (concatenate, order,
walk), which tests/test_merge_collapsed_host.py holds against the single-index
reference on the CPU.  Docs and groups compare exactly, scores on their uint32
views.  Every call runs on a non-default stream into outputs prefilled with a
sentinel and followed by guard words.  The shapes sit next to

  64     entries of a chunk of the walk, and of a list's window at W <= 8
         (k = 63, 64, 65; 130: a third window)
  8      entries of a list's window at W = 64
  4096   the largest k: the LDS group table full
  65535  rows (Q = 70 000: a row per workgroup, past 2^16)"""
import os
import socket
import time

import numpy as np
import pytest
import torch.multiprocessing as mp

from collapse_model import layouts, ref_collapsed
from merge_collapse_model import CUTS, ref_merge_collapsed, same3, shard_csc
from test_gpu_parity import _idx
from test_search_after_host import PAD, after_case, position_masks, score_keys, weighted_case

pytestmark = pytest.mark.gpu

SCORES = np.array([-1.5, -0.0, 0.0, 0.25, 0.25, 1.0, 3.5], np.float32)  # few values: dense ties
GUARD = 64
SENT_D, SENT_S, SENT_G = 123456789, 7.5, 424242


def descending(n):
    """n scores of five values (no -0.0: numpy sorts it beside +0.0), best first."""
    return np.sort(np.array([-1.5, 0.0, 0.25, 1.0, 3.5], np.float32)[np.arange(n) % 5])[::-1]


# ------------------------------------------------------------ constructed lists
def _sort_rows(d, s, g):
    """Each row of [.., n] in (score_keys desc, doc asc) order, padding (doc < 0) last."""
    key = np.where(d >= 0, score_keys(s).astype(np.int64).reshape(d.shape), -1)
    order = np.lexsort((d, -key), axis=-1)
    take = lambda a: np.take_along_axis(a, order, -1)
    return take(d), take(s), take(g)


def random_lists(seed, W, Q, k, groups=(-2, 6)):
    """W best-first lists [Q, k] of random lengths 0 .. k: unique docs per row,
    scores of a few values, groups with heavy repeats (some negative)."""
    rng = np.random.default_rng(seed)
    docs = np.argsort(rng.random((Q, 4 * W * k)), axis=1)[:, :W * k].astype(np.int32)
    docs = docs.reshape(Q, W, k) * 7 + 3
    s = SCORES[rng.integers(0, len(SCORES), (Q, W, k))]
    g = rng.integers(groups[0], groups[1], (Q, W, k)).astype(np.int32)
    n = rng.integers(0, k + 1, (Q, W, 1))
    pad = np.arange(k)[None, None, :] >= n
    docs[pad] = -1
    docs, s, g = _sort_rows(docs, s, g)
    pad = docs < 0
    s = s.copy()
    s.view(np.uint32)[pad] = PAD
    g[pad] = -1
    return [(np.ascontiguousarray(docs[:, w]), np.ascontiguousarray(s[:, w]),
             np.ascontiguousarray(g[:, w])) for w in range(W)]


def deal(scores, groups, owner, W, k, docs=None):
    """One row: merged entries (best first; docs ascending by default, so ties
    keep their order) dealt to the lists by ``owner``."""
    n = len(scores)
    docs = np.arange(n, dtype=np.int32) * 3 + 1 if docs is None else np.asarray(docs, np.int32)
    out = []
    for w in range(W):
        m = np.asarray(owner) == w
        assert m.sum() <= k
        d = np.full((1, k), -1, np.int32)
        s = np.full((1, k), PAD, np.uint32)
        g = np.full((1, k), -1, np.int32)
        d[0, :m.sum()] = docs[m]
        s[0, :m.sum()] = np.asarray(scores, np.float32)[m].view(np.uint32)
        g[0, :m.sum()] = np.asarray(groups, np.int32)[m]
        out.append((d, s.view(np.float32), g))
    return out


def run_merge(lists, k, per_group, packed=False, want_groups=True):
    """bm25_merge_collapsed_device on the lists, as plain [W, Q, k] arrays or
    as the packed [W][docs|scores|groups][Q][k] buffer; outputs prefilled with
    a sentinel, guard words behind them checked."""
    import torch
    from bm25mi.index import merge_collapsed_device
    W, (Q, _) = len(lists), lists[0][0].shape
    d = np.stack([l[0] for l in lists]).astype(np.int32)
    s = np.stack([np.ascontiguousarray(l[1], np.float32).view(np.int32) for l in lists])
    g = np.stack([l[2] for l in lists]).astype(np.int32)
    if packed:
        buf = torch.from_numpy(np.ascontiguousarray(np.stack([d, s, g], 1))).cuda()  # [W, 3, Q, k]
        dd, ds, dg, stride = buf, buf[:, 1], buf[:, 2], 3 * Q * k
    else:
        dd, ds, dg = (torch.from_numpy(a).cuda() for a in (d, s, g))
        stride = Q * k
    n = Q * k
    od = torch.full((n + GUARD,), SENT_D, dtype=torch.int32, device="cuda")
    os_ = torch.full((n + GUARD,), SENT_S, dtype=torch.float32, device="cuda")
    og = torch.full((n + GUARD,), SENT_G, dtype=torch.int32, device="cuda")
    st = torch.cuda.Stream()
    torch.cuda.synchronize()  # (the uploads ran on the current stream)
    merge_collapsed_device(0, dd, ds.view(torch.float32), dg, W, Q, k, stride, per_group, od, os_,
                           og if want_groups else None, st)
    st.synchronize()
    od, os_, og = od.cpu().numpy(), os_.cpu().numpy(), og.cpu().numpy()
    assert (od[n:] == SENT_D).all() and (os_[n:] == SENT_S).all() and (og[n:] == SENT_G).all()
    if not want_groups:
        assert (og == SENT_G).all()
    return od[:n].reshape(Q, k), os_[:n].reshape(Q, k), og[:n].reshape(Q, k)


def check(lists, k, per_group, packed=False, what=""):
    want = ref_merge_collapsed(lists, k, per_group)
    got = run_merge(lists, k, per_group, packed)
    bad = np.nonzero((got[0] != want[0]) | (got[1].view(np.uint32) != want[1].view(np.uint32))
                     | (got[2] != want[2]))
    assert bad[0].size == 0, (what, f"{bad[0].size} mismatches, first at row {bad[0][0]} slot "
                              f"{bad[1][0]}: got {got[0][bad[0][0]][:8]} want {want[0][bad[0][0]][:8]}")
    pad = got[0] < 0  # every slot written: hits, then canonical padding
    assert (got[1].view(np.uint32)[pad] == PAD).all() and (got[2][pad] == -1).all(), what
    return got


# ------------------------------------------------------- 1. kernel vs the model
@pytest.mark.parametrize("k", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("W", [1, 2, 3, 8, 64])
def test_random_lists(gpu, W, k):
    lists = random_lists(1000 * W + k, W, 5, k)
    for i, per_group in enumerate(sorted({1, 2, k})):
        check(lists, k, per_group, packed=(W + i) % 2 == 0, what=(W, k, per_group))


def test_largest_k(gpu):
    """k = 4096: the group table of 8192 slots, up to 4096 groups in it."""
    lists = random_lists(4096, 2, 2, 4096, groups=(-50, 6000))
    check(lists, 4096, 1, what="many groups")
    check(lists, 4096, 4096, packed=True, what="no collapse")
    check(random_lists(4097, 2, 2, 4096), 4096, 2, what="few groups")


def test_many_rows(gpu):
    """Q = 70 000 at W = 2, k = 1: a row's best head, whatever its group."""
    Q = 70_000
    lists = random_lists(7, 2, Q, 1)
    (d0, s0, _), (d1, s1, _) = [tuple(a[:, 0] for a in l) for l in lists]
    k0, k1 = score_keys(s0), score_keys(s1)
    first = (d1 < 0) | ((d0 >= 0) & ((k0 > k1) | ((k0 == k1) & (d0 < d1))))
    want = tuple(np.where(first, lists[0][j][:, 0].view(np.int32), lists[1][j][:, 0].view(np.int32))
                 for j in range(3))
    assert ((d0 < 0) & (d1 >= 0)).any() and ((d0 < 0) & (d1 < 0)).any() and (~first).any()
    got = run_merge(lists, 1, 1)
    assert np.array_equal(got[0][:, 0], want[0])
    assert np.array_equal(got[1][:, 0].view(np.int32), want[1])
    assert np.array_equal(got[2][:, 0], want[2])
    rows = slice(0, 300)   # ... and the model agrees with that shortcut
    assert same3(ref_merge_collapsed([tuple(a[rows] for a in l) for l in lists], 1, 1),
                 tuple(a[rows] for a in got))


# ------------------------------------------------------------ 2. named cases
def test_all_padding_and_single_live_list(gpu):
    k = 65
    for W in (1, 3, 64):
        lists = random_lists(5 + W, W, 4, k)
        empty = [(np.full_like(d, -1), np.full_like(s, np.float32(3.0)), np.full_like(g, 9))
                 for d, s, g in lists]  # (scores and groups of padding are not read)
        got = check(empty, k, 1, what=("all padding", W))
        assert (got[0] == -1).all()
        for live in {0, W - 1}:
            one = [lists[w] if w == live else empty[w] for w in range(W)]
            check(one, k, 1, what=("one live list", W, live))
            got = check(one, k, k, packed=True, what=("one live list", W, live))
            n = (lists[live][0] >= 0).sum(1)
            assert ((got[0] >= 0).sum(1) == n).all()


def test_one_list_ahead_for_more_than_two_windows(gpu):
    """W = 2 (windows of 64): list 0 holds 200 entries that all beat list 1's
    head; W = 64 (windows of 8): 30 of them."""
    for W, ahead, k in ((2, 200, 256), (64, 30, 40)):
        n = ahead + 40
        scores = np.r_[np.full(ahead, 3.5), np.full(40, 1.0)].astype(np.float32)
        owner = np.r_[np.zeros(ahead, int), 1 + np.arange(40) % (W - 1)]
        groups = np.arange(n) % 23
        lists = deal(scores, groups, owner, W, k)
        for per_group in (1, 2, k):
            check(lists, k, per_group, what=(W, per_group))


def test_equal_scores_across_lists_at_a_window_end(gpu):
    """One score everywhere, the lists interleaved by doc id: the order is by
    doc alone, and every window ends inside the tie."""
    for W, k in ((2, 130), (8, 130), (64, 20)):
        n = W * k
        scores = np.full(n, 0.25, np.float32)
        owner = np.arange(n) % W
        for groups, per_group in ((np.arange(n) % 50, 1), (np.arange(n) % 50, 2), (-np.ones(n), 1)):
            check(deal(scores, groups, owner, W, k), k, per_group, packed=True, what=(W, per_group))


def test_group_saturating_at_the_chunk_edge(gpu):
    """Entries 62 .. 66 of the walk share a group, the others have their own:
    the quota fills at entry 63 (per_group 2) or 64 (3) and the next chunk's
    entries of the group are dropped by the table."""
    n, k = 130, 130
    groups = 1000 + np.arange(n)
    groups[62:67] = 5
    scores = descending(n)
    for W in (1, 2, 8):
        lists = deal(scores, groups, np.arange(n) % W, W, k)
        for per_group in (1, 2, 3):
            got = check(lists, k, per_group, what=(W, per_group))
            assert (got[2] == 5).sum() == per_group


def test_one_group_from_several_lists_in_one_chunk(gpu):
    n, k = 64, 64
    scores = np.full(n, 1.0, np.float32)
    for W in (2, 8, 64):
        lists = deal(scores, np.full(n, 3), np.arange(n) % W, W, k)
        for per_group in (1, 2, k):
            got = check(lists, k, per_group, what=(W, per_group))
            assert (got[0] >= 0).sum() == min(per_group, n)
        mixed = np.where(np.arange(n) % 3 == 0, 3, np.arange(n) + 10)
        check(deal(scores, mixed, np.arange(n) % W, W, k), k, 2, what=(W, "mixed"))


def test_extreme_and_negative_groups(gpu):
    top = 2**31 - 1
    n, k, W = 100, 100, 3
    groups = np.array([top, top - 1, -1, -2**31, 0, top, -7, top - 1, 0, top] * 10, np.int64)
    scores = descending(n)
    lists = deal(scores, groups.astype(np.int32), np.arange(n) % W, W, k)
    for per_group in (1, 2, k):
        got = check(lists, k, per_group, what=per_group)
        if per_group < k:  # entries without a group are all kept, as their own negative values
            assert (got[2] == -7).sum() == 10 and (got[2] == -2**31).sum() == 10
            assert (got[2] == top).sum() == per_group


def test_null_out_groups_and_both_strides(gpu):
    lists = random_lists(11, 8, 6, 100)
    want = ref_merge_collapsed(lists, 100, 2)
    for packed in (False, True):
        assert same3(run_merge(lists, 100, 2, packed), want)
        got = run_merge(lists, 100, 2, packed, want_groups=False)
        assert same3(got[:2] + (want[2],), want)
    # W = 1 returns its input (a collapsed list under the same per_group)
    one = [ref_merge_collapsed(lists, 100, 2)]
    assert same3(run_merge(one, 100, 2), one[0])


# ----------------------------------------------- 3. identity with merge_sorted
def test_no_collapse_is_merge_sorted(gpu):
    import torch
    from bm25mi.index import merge_sorted_device
    W, k, Q = 8, 100, 64
    lists = random_lists(21, W, Q, k)
    d = torch.from_numpy(np.stack([l[0] for l in lists])).cuda()
    s = torch.from_numpy(np.stack([l[1] for l in lists])).cuda()
    md = torch.empty((Q, k), dtype=torch.int32, device="cuda")
    ms = torch.empty((Q, k), dtype=torch.float32, device="cuda")
    merge_sorted_device(0, d, s, W, Q, k, Q * k, md, ms)
    torch.cuda.synchronize()
    md, ms = md.cpu().numpy(), ms.cpu().numpy()
    got = run_merge(lists, k, k)
    assert np.array_equal(got[0], md) and np.array_equal(got[1].view(np.uint32), ms.view(np.uint32))
    neg = [(a, b, -1 - (c % 3)) for a, b, c in lists]
    got = run_merge(neg, k, 1, packed=True)
    assert np.array_equal(got[0], md) and np.array_equal(got[1].view(np.uint32), ms.view(np.uint32))
    assert not np.array_equal(run_merge(lists, k, 1)[0], md)  # (the lists do collapse)


# ------------------------------------------------- 4. end to end on one GPU
def _shard_search(handles, cuts, q, k, groups, per_group, w=None, allow=None, qm=None):
    """search_collapsed_device on every shard handle with d_groups_out."""
    import bm25mi
    import torch
    up = lambda a, t: None if a is None else torch.from_numpy(np.array(a, t)).cuda()
    lists = []
    for h, lo, hi in zip(handles, cuts[:-1], cuts[1:]):
        dm = None if allow is None else torch.from_numpy(np.ascontiguousarray(
            bm25mi.pack_mask(allow[:, lo:hi])).view(np.int32)).cuda()
        dd = torch.empty((len(q), k), dtype=torch.int32, device="cuda")
        ds = torch.empty((len(q), k), dtype=torch.float32, device="cuda")
        dg = torch.empty((len(q), k), dtype=torch.int32, device="cuda")
        h.search_collapsed_device(up(q, np.int32), k, up(groups[lo:hi], np.int32), per_group,
                                  up(w, np.float32), dm, up(qm, np.int32), dd, ds, dg)
        torch.cuda.synchronize()
        lists.append((dd.cpu().numpy(), ds.cpu().numpy(), dg.cpu().numpy()))
    return lists


@pytest.mark.parametrize("weighted", [False, True])
def test_three_shards_equal_one_handle(gpu, weighted):
    """The 5000-document fixture as 3 handles cut at 1111 and 2048: each
    shard's collapsed search with its groups, merged, is one handle's
    search_collapsed over the whole, bit for bit — and the reference's."""
    if weighted:
        ip, ix, dt, q, w, rows = weighted_case()
    else:
        ip, ix, dt, q, rows = after_case(5000)
        w = None
    cuts = CUTS[3]
    whole = _idx(ip, ix, dt, 5000)
    handles = [_idx(*shard_csc(ip, ix, dt, lo, hi), hi - lo, doc_offset=lo)
               for lo, hi in zip(cuts[:-1], cuts[1:])]
    lay = layouts(5000)
    tenant_mask = (lay["tenant"] == 3)[None, :]
    plain_differs = 0
    for name, allow in (("uniform", None), ("dominated", None), ("one", None),
                        ("tenant", tenant_mask)):
        packed = None
        if allow is not None:
            import bm25mi
            packed = bm25mi.pack_mask(allow)
        for k in (10, 100):
            for per_group in (1, 2):
                want = whole.search_collapsed(q, k, lay[name], per_group, w, packed,
                                              return_groups=True)
                assert same3(want, ref_collapsed(rows, k, lay[name], per_group, allow, None, 0, True))
                lists = _shard_search(handles, cuts, q, k, lay[name], per_group, w, allow)
                got = run_merge(lists, k, per_group, packed=True)
                assert same3(got, want), (name, k, per_group)
                plain_differs += not same3(ref_merge_collapsed(lists, k, per_group, False), want)
    assert plain_differs >= 8  # (dominated, one and tenant need the second collapse)
    for h in handles + [whole]:
        h.close()


# ------------------------------- 5. sharded_search_collapsed, real process groups
DIST_CUTS = {1: (0, 5000), 2: (0, 37, 5000), 3: (0, 37, 2048, 5000)}  # 37 documents < k
DIST_K = 100
DIST_RUNS = (("uniform", 1, False), ("dominated", 2, True), ("one", 1, False))


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, data, out):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import bm25mi
        from bm25mi.dist import sharded_search_collapsed
        from bm25mi.index import GpuIndex
        z = np.load(data)
        lo, hi = DIST_CUTS[world][rank], DIST_CUTS[world][rank + 1]
        index = GpuIndex(*shard_csc(z["ip"], z["ix"], z["dt"], lo, hi), hi - lo, device=0,
                         doc_offset=lo)
        dq = torch.from_numpy(z["q"]).cuda()
        dm = torch.from_numpy(np.ascontiguousarray(
            bm25mi.pack_mask(z["allow"][:, lo:hi])).view(np.int32)).cuda()
        dqm = torch.from_numpy(z["qm"]).cuda()
        stream = torch.cuda.Stream()   # a non-current stream: the body must order on it
        res = {}
        for name, per_group, masked in DIST_RUNS:
            dg = torch.from_numpy(np.ascontiguousarray(z[name][lo:hi])).cuda()
            torch.cuda.synchronize()
            docs, scores, groups = sharded_search_collapsed(
                index, dq, DIST_K, dg, per_group, None, dm if masked else None,
                dqm if masked else None, stream=stream)
            torch.cuda.synchronize()
            res[name] = np.stack([docs.cpu().numpy(), scores.cpu().numpy().view(np.int32),
                                  groups.cpu().numpy()])
        if rank == 0:
            np.savez(out, **res)
        index.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [1, 2, 3])
def test_sharded_search_collapsed_real_process_group(gpu, tmp_path, world):
    """1, 2 and 3 gloo ranks sharing cuda:0, each with its doc shard (one of 37
    documents, fewer than k = 100): rank 0's rows are the single-index
    collapsed reference, plain and under masks."""
    ip, ix, dt, q, rows = after_case(5000)
    allow, qm = position_masks()
    lay = layouts(5000)
    data, out = str(tmp_path / "in.npz"), str(tmp_path / "r.npz")
    np.savez(data, ip=ip, ix=ix, dt=dt, q=q, allow=allow, qm=qm,
             **{name: lay[name] for name, _, _ in DIST_RUNS})
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
    for name, per_group, masked in DIST_RUNS:
        want = ref_collapsed(rows, DIST_K, lay[name], per_group, allow if masked else None,
                             qm if masked else None, 0, True)
        g = got[name]
        assert same3((g[0], g[1].view(np.float32), g[2]), want), (name, world)
