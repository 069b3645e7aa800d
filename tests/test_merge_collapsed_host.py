"""CPU tests of the doc-shard merge of collapsed lists
(bm25_merge_collapsed_device, bm25mi.index.merge_collapsed_device,
bm25mi.dist.sharded_search_collapsed).

The model (tests/merge_collapse_model.py: concatenate, order, walk) is held
against the single-index reference: the collapsed lists of 2, 3 and 5 doc
shards of the 5000-document fixture, merged and collapsed once more, are the
collapsed rows of the whole — and a plain merge of them is not, which is why
the call exists.  The C call's argument checks precede any device call, so
every BM25_EINVAL and its message are tested here without a GPU; and
sharded_search_collapsed runs its protocol (packing, a short shard's padding,
one all-gather, the merge's stride) through a real 3-rank gloo group with numpy
stand-ins for the two GPU calls."""
import ctypes

import numpy as np
import pytest

from collapse_model import layouts, ref_collapsed
from merge_collapse_model import CUTS, ref_merge_collapsed, same3, shard_lists
from test_gpu_edges import TILE
from test_search_after_host import after_case, position_masks, weighted_case

SYM = "bm25_merge_collapsed_device"


# ------------------------------------------------- model vs the single index
def _per_groups(k):
    return sorted({1, 2, k})


@pytest.mark.parametrize("k", [1, 10, 100])
@pytest.mark.parametrize("shards", [2, 3, 5])
def test_merged_shard_lists_are_the_single_index_rows(shards, k):
    """Every layout, per_group 1, 2 and k: the model over the shards' lists
    equals ref_collapsed over the whole.  Where a layout really collapses
    across shards the plain merge differs — asserted for "dominated" and
    "one", whose groups have members in every shard."""
    rows = after_case(5000)[4]
    cuts = CUTS[shards]
    assert (TILE in cuts or shards == 2) and any(c % 64 for c in cuts[1:-1])
    plain_differs = set()
    for name, g in layouts(5000).items():
        for per_group in _per_groups(k):
            want = ref_collapsed(rows, k, g, per_group, want_groups=True)
            lists = shard_lists(rows, cuts, k, g, per_group)
            assert same3(ref_merge_collapsed(lists, k, per_group), want), (name, per_group)
            if not same3(ref_merge_collapsed(lists, k, per_group, collapse=False), want):
                plain_differs.add((name, per_group))
    if k > 1:
        assert ("dominated", 1) in plain_differs and ("one", 1) in plain_differs
        # ... and where nothing collapses the plain merge is the answer
        assert not {n for n, _ in plain_differs} & {"negative", "distinct"}
        assert not any(p >= k for _, p in plain_differs)


def test_tie_pair_of_one_group_straddles_a_cut():
    """Documents 2047 and 2048: one group, equal scores on row 1, in different
    shards.  per_group = 1 keeps 2047 alone; each shard's own list holds its
    member, so the plain merge keeps both."""
    rows = after_case(5000)[4]
    g = layouts(5000)["uniform"]
    assert g[TILE - 1] == g[TILE] and rows[1][TILE - 1] == rows[1][TILE]
    k = 4096
    lists = shard_lists(rows[1:2], CUTS[3], k, g, 1)
    assert TILE - 1 in lists[1][0][0] and TILE in lists[2][0][0]
    got = ref_merge_collapsed(lists, k, 1)
    assert same3(got, ref_collapsed(rows[1:2], k, g, 1, want_groups=True))
    assert TILE - 1 in got[0][0] and TILE not in got[0][0]
    plain = ref_merge_collapsed(lists, k, 1, collapse=False)
    assert TILE - 1 in plain[0][0] and TILE in plain[0][0]


@pytest.mark.parametrize("shards", [2, 3, 5])
def test_merged_shard_lists_under_masks_and_weights(shards):
    cuts = CUTS[shards]
    rows = after_case(5000)[4]
    allow, qm = position_masks()
    lay = layouts(5000)
    for name in ("uniform", "dominated", "tenant"):
        for per_group, k in ((1, 10), (2, 10), (1, 100)):
            want = ref_collapsed(rows, k, lay[name], per_group, allow, qm, 0, True)
            lists = shard_lists(rows, cuts, k, lay[name], per_group, allow, qm)
            assert same3(ref_merge_collapsed(lists, k, per_group), want), (name, per_group, k)
    # one tenant allowed: one group left, one hit in the collection — and one per shard
    one = (lay["tenant"] == 3)[None, :]
    lists = shard_lists(rows, cuts, 10, lay["tenant"], 1, one)
    want = ref_collapsed(rows, 10, lay["tenant"], 1, one, None, 0, True)
    assert same3(ref_merge_collapsed(lists, 10, 1), want)
    assert (want[0][:, 0] >= 0).all() and (want[0][:, 1:] == -1).all()
    assert not same3(ref_merge_collapsed(lists, 10, 1, collapse=False), want)
    wrows = weighted_case()[5]
    for name in ("uniform", "dominated", "one"):
        for per_group in (1, 2):
            want = ref_collapsed(wrows, 10, lay[name], per_group, want_groups=True)
            lists = shard_lists(wrows, cuts, 10, lay[name], per_group)
            assert same3(ref_merge_collapsed(lists, 10, per_group), want), (name, per_group)


def test_model_identities():
    """W = 1 returns its input; per_group >= k or all groups negative is the
    plain merge."""
    rows = after_case(5000)[4]
    lay = layouts(5000)
    whole = shard_lists(rows, (0, 5000), 10, lay["uniform"], 1)
    assert same3(ref_merge_collapsed(whole, 10, 1), whole[0])
    for name, per_group in (("uniform", 10), ("negative", 1)):
        lists = shard_lists(rows, CUTS[3], 10, lay[name], per_group)
        assert same3(ref_merge_collapsed(lists, 10, per_group),
                     ref_merge_collapsed(lists, 10, per_group, collapse=False))


# ------------------------------------------------------------- the bindings
def test_symbol_exported_bound_and_documented():
    from bm25mi import _capi
    assert SYM in _capi.header_symbols()
    f = getattr(_capi.lib, SYM)
    assert f.restype is ctypes.c_int and SYM in _capi._SIGS and len(f.argtypes) == 13
    text = open(_capi.HEADER).read()
    doc = text[text.index("The merge of collapsed searches over doc shards"):
               text.index("int " + SYM + "(")]
    for phrase in ("rank_stride", "per_group", "bm25_merge_sorted_device", "W > 64", "unspecified",
                   "Replaces no reference call", "3 * Q * k", "0xFFFFFFFF", "d_out_groups may be NULL",
                   "bit for bit", "W = 1 returns its input", "BM25_EINVAL", "k > 4096",
                   "Q may pass 65535", "no host synchronisation", "takes no handle"):
        assert phrase in doc, phrase
    assert "does not do this yet" not in text
    block = text[text.index("Field collapsing"):text.index("int bm25_search_collapsed(")]
    assert SYM in block and "sharded_search_collapsed" in block
    assert _capi.abi_version() == 1  # additive: the ABI version stays
    import bm25mi
    from bm25mi import dist, index
    assert bm25mi.merge_collapsed_device is index.merge_collapsed_device
    assert callable(dist.sharded_search_collapsed)


def _call(W=2, Q=3, k=4, stride=None, per_group=1, null=()):
    from bm25mi._capi import lib
    n = max(1, W, 1) * max(Q, 1) * max(k, 1)
    bufs = {"docs": np.zeros(n, np.int32), "scores": np.zeros(n, np.float32),
            "groups": np.zeros(n, np.int32), "od": np.full(n, 7, np.int32),
            "os": np.full(n, 7.0, np.float32), "og": np.full(n, 7, np.int32)}
    p = lambda name: None if name in null else bufs[name].ctypes.data_as(ctypes.c_void_p)
    rc = lib.bm25_merge_collapsed_device(0, p("docs"), p("scores"), p("groups"), W, Q, k,
                                         Q * k if stride is None else stride, per_group, p("od"),
                                         p("os"), p("og"), None)
    assert (bufs["od"] == 7).all() and (bufs["os"] == 7.0).all() and (bufs["og"] == 7).all()
    return rc, lib.bm25_last_error()


@pytest.mark.parametrize("kwargs,message", [
    (dict(W=0), b"W=0"), (dict(W=-3), b"W=-3"), (dict(W=65), b"W=65"),
    (dict(Q=-1, stride=0), b"Q=-1"), (dict(k=-1, stride=0), b"k=-1"),
    (dict(k=4097), b"k=4097"), (dict(per_group=0), b"per_group=0"),
    (dict(per_group=-2), b"per_group=-2"), (dict(stride=11), b"rank_stride=11"),
    (dict(null=("docs",)), b"NULL input"), (dict(null=("scores",)), b"NULL input"),
    (dict(null=("groups",)), b"NULL input"), (dict(null=("od",)), b"NULL output"),
    (dict(null=("os",)), b"NULL output")])
def test_einval_before_any_device_call(kwargs, message):
    from bm25mi._capi import BM25_EINVAL
    rc, msg = _call(**kwargs)
    assert rc == BM25_EINVAL and message in msg, msg
    if b"k=4097" in message:
        assert b"4096" in msg and b"LDS" in msg


def test_empty_shapes_are_ok_without_device_work():
    """k == 0 or Q == 0: BM25_OK before any pointer or device is looked at."""
    from bm25mi._capi import BM25_OK
    everything = ("docs", "scores", "groups", "od", "os", "og")
    assert _call(Q=0, null=everything)[0] == BM25_OK
    assert _call(k=0, null=everything)[0] == BM25_OK
    assert _call(Q=0, k=0, stride=0, W=64)[0] == BM25_OK


def test_python_wrapper_raises_the_c_message():
    import torch
    from bm25mi.index import merge_collapsed_device
    z = torch.zeros((2, 3, 4), dtype=torch.int32)
    f = z.view(torch.float32)
    o = torch.zeros((3, 4), dtype=torch.int32)
    with pytest.raises(ValueError, match="W=65"):
        merge_collapsed_device(0, z, f, z, 65, 3, 4, 12, 1, o, o.view(torch.float32), o)
    with pytest.raises(ValueError, match="per_group=0"):
        merge_collapsed_device(0, z, f, z, 2, 3, 4, 12, 0, o, o.view(torch.float32))
    with pytest.raises(ValueError, match="rank_stride=5"):
        merge_collapsed_device(0, z, f, z, 2, 3, 4, 5, 1, o, o.view(torch.float32), None)


# ------------------------------------- the sharded call's protocol, on gloo
class _NumpyCollapsedShard:
    """search_collapsed_device of a doc shard [lo, hi) on the host: the
    reference walk over the shard's slice of the fixture's dense rows."""

    def __init__(self, rows, lo, hi):
        self.rows, self.lo, self.n_docs, self.calls = [r[lo:hi] for r in rows], lo, hi - lo, []

    def search_collapsed_device(self, d_queries, k, d_groups, per_group, d_weights, d_masks,
                                d_query_mask, d_docs, d_scores, d_groups_out=None, stream=None):
        import torch
        assert k <= self.n_docs and d_groups.numel() == self.n_docs and d_masks is None
        self.calls.append(k)
        d, s, g = ref_collapsed(self.rows, k, d_groups.numpy(), per_group, None, None, self.lo, True)
        d_docs.copy_(torch.from_numpy(d))
        d_scores.copy_(torch.from_numpy(s))
        d_groups_out.copy_(torch.from_numpy(g))


def _merge_collapsed_cpu(device, d_docs, d_scores, d_groups, W, Q, k, rank_stride, per_group,
                         out_d, out_s, out_g=None, stream=None):
    """bm25_merge_collapsed_device on the host, for the packed gathered buffer."""
    import torch
    assert tuple(d_docs.shape) == (W, 3, Q, k) and d_docs.is_contiguous()
    assert rank_stride == 3 * Q * k
    assert d_scores.data_ptr() == d_docs.data_ptr() + 4 * Q * k
    assert d_groups.data_ptr() == d_docs.data_ptr() + 8 * Q * k
    g = d_docs.numpy()
    lists = [(g[w, 0], g[w, 1].view(np.float32), g[w, 2]) for w in range(W)]
    d, s, gr = ref_merge_collapsed(lists, k, per_group)
    out_d.copy_(torch.from_numpy(d))
    out_s.copy_(torch.from_numpy(s))
    out_g.copy_(torch.from_numpy(gr))


PROTOCOL_CUTS = (0, 37, TILE, 5000)   # a shard of 37 documents, fewer than k
PROTOCOL_K = 100


def _protocol_worker(rank, world, port, out):
    import os
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import bm25mi.index as bi
        from bm25mi.dist import sharded_search_collapsed
        bi.merge_collapsed_device = _merge_collapsed_cpu  # the host stand-in of the HIP merge
        q, rows = after_case(5000)[3:5]
        lo, hi = PROTOCOL_CUTS[rank], PROTOCOL_CUTS[rank + 1]
        shard = _NumpyCollapsedShard(rows, lo, hi)
        g = torch.from_numpy(np.ascontiguousarray(layouts(5000)["dominated"][lo:hi]))
        docs, scores, groups = sharded_search_collapsed(shard, torch.from_numpy(q), PROTOCOL_K, g, 2)
        assert shard.calls == [min(PROTOCOL_K, hi - lo)]
        if rank == 0:
            np.savez(out, docs=docs.numpy(), scores=scores.numpy(), groups=groups.numpy())
    finally:
        dist.destroy_process_group()


def test_gloo_sharded_search_collapsed_protocol(tmp_path):
    """sharded_search_collapsed through a real 3-rank gloo group on the host
    (numpy stand-ins for the shard's search and the HIP merge): each rank's
    list packed as [3, Q, k], a short shard padded to k, one all-gather, the
    merge fed rank_stride = 3 Q k — the single-index rows bit for bit."""
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
    rows = after_case(5000)[4]
    want = ref_collapsed(rows, PROTOCOL_K, layouts(5000)["dominated"], 2, want_groups=True)
    assert same3((got["docs"], got["scores"], got["groups"]), want)
