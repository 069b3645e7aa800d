"""Dead term segments in scored tiles (option seg_skip): the pre-pass marks,
per (query, tile), the term lanes that have no posting in a live sub-block,
and REST drops their segments.  Results are the oracle's bit for bit under
every setting, the count_skips build's four counters are the numpy model's
(tests/seg_model.py on tests/mask_model.py) exactly, and the paths that take
no pre-pass report no seg_skip."""
import itertools

import numpy as np
import pytest

import mask_model as mm
import seg_model as sm
from oracle import oracle
from test_gpu_edges import _csc
from test_gpu_parity import _exact, _idx, _world_bounds_search

pytestmark = pytest.mark.gpu

TILE = mm.TILE
OPTS = ("seg_skip", "tile_mask", "bound_pool", "tile_bound")


def _set(index, **kw):
    for name, v in kw.items():
        index.set_option(name, v)


def _counted(index, run, ref):
    """run() under count_skips: exact, and the four counters."""
    index.set_option("count_skips", 1)
    _exact(run(), ref)
    st = index.search_stats()
    index.set_option("count_skips", 0)
    return (st["bound_skipped_tiles"], st["bound_skipped_postings"],
            st["bound_dropped_segments"], st["bound_dropped_postings"])


def _device_search(index, q, k):
    """search_device: no validation, so an id >= n_terms is padding."""
    import torch
    dq = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    d = torch.empty((len(q), k), dtype=torch.int32, device="cuda")
    s = torch.empty((len(q), k), dtype=torch.float32, device="cuda")
    index.search_device(dq, k, d, s)
    torch.cuda.synchronize()
    return d.cpu().numpy(), s.cpu().numpy()


# ---------------------------------------------------------------- the fixture
A, B, C, D, E, F = range(6)
V_FIX = 6
ANCHORS = (10, 20, 30, 40)
T_DROP, T_CUT, T_BIG, T_LIVE, T_LAST = 50, 51, 52, 53, 79   # 48..55: one 8-tile item
NT_FIX = 80
N_FIX = (NT_FIX - 1) * TILE + 993                            # a partial last tile


def _fixture_csc():
    """k = 4 anchor tiles hold one document with A = 8.0: theta = 8.0 for every
    query with A (f16-exact values, far from every boundary).
    T_DROP: B and C = 5.0 on one document of sub-block 1, D = 2.0 on three
    documents of sub-block 10 (dead: D is dropped).  T_CUT: B alone (cut).
    T_BIG: B and C on one document, E = 1.0 on 300 documents of sub-blocks
    20..24 (a dropped segment of several rows).  T_LIVE: D, B on one document
    (D + D + B reaches theta: a query with D twice keeps both).  T_LAST (993
    documents): B and C on one document, D in sub-block 14."""
    a = [t * TILE + 100 for t in ANCHORS]
    b = [T_DROP * TILE + 70, T_CUT * TILE + 5, T_BIG * TILE + 3, T_LIVE * TILE + 5, T_LAST * TILE + 10]
    c = [T_DROP * TILE + 70, T_BIG * TILE + 3, T_LAST * TILE + 10]
    d = [T_DROP * TILE + x for x in (640, 650, 660)] + [T_LIVE * TILE + 5, T_LAST * TILE + 900]
    e = [T_BIG * TILE + 1280 + i for i in range(300)]
    vals = (8.0, 5.0, 5.0, 2.0, 1.0)
    cols = [(np.array(x, np.int32), np.full(len(x), v, np.float32))
            for x, v in zip((a, b, c, d, e), vals)]
    cols.append((np.zeros(0, np.int32), np.zeros(0, np.float32)))        # F: an empty term
    return _csc(cols, np.float32)


def test_constructed_fixture_drops_segments(gpu):
    ip, ix, dt = _fixture_csc()
    q = np.full((5, 8), -1, np.int32)
    q[0, :4] = [A, B, C, D]                      # D lives in a dead sub-block of T_DROP
    q[1, :4] = [D, B, C, A]                      # ... and is lane 0
    q[2, :4] = [A, B, E, C]                      # E: 300 postings dropped in T_BIG
    q[3, :5] = [D, A, B, D, C]                   # D twice: both dropped (T_DROP), both kept (T_LIVE)
    q[4, :7] = [B, -1, D, 99, C, F, A]           # padding, an id >= V and an empty term between
    k = 4
    # (the oracle refuses an id >= V as the reference does; the device search pads it)
    ref = oracle.search_c(N_FIX, ip, ix, dt, np.where(q >= V_FIX, -1, q), k)
    d_only = {T_DROP * TILE + x for x in (640, 650, 660)} | {T_LAST * TILE + 900}
    assert not d_only & set(ref[0].ravel().tolist())
    assert T_LIVE * TILE + 5 in ref[0][3] and ref[1][3, 0] == 10.0   # D + B + D = 9.0 is listed
    bmax, tmask = mm.tables(ip, ix, dt, N_FIX)
    assert bmax.shape[1] == NT_FIX
    for r, row in enumerate(q):                  # the cases are what the model sees
        cut, L, drop = sm.live_model(bmax, tmask, row, np.float32(8.0))
        lane = {int(t): i for i, t in enumerate(row) if 0 <= t < V_FIX}
        assert cut[T_CUT] and not cut[[T_DROP, T_BIG, T_LAST]].any() and not cut[list(ANCHORS)].any()
        assert L[T_DROP] == 1 << 1 and L[T_LAST] == 1 << 0 and L[T_BIG] == 1 << 0
        if D in lane:
            assert drop[lane[D], T_DROP] and drop[lane[D], T_LAST]
            assert not drop[lane[B], T_DROP] and not drop[lane[C], T_LAST]
        if r == 1:
            assert lane[D] == 0
        if r == 2:
            assert drop[lane[E], T_BIG] and not drop[lane[B], T_BIG]
        if r == 3:
            assert drop[0, T_DROP] and drop[3, T_DROP]
            assert not cut[T_LIVE] and not drop[0, T_LIVE] and not drop[3, T_LIVE]
    index = _idx(ip, ix, dt, N_FIX, segments="dense")
    for flat_bw, seg, tile_mask in itertools.product((8, 0), (1, 0), (1, 0)):
        # (flat_bw = 8: the cut tile and the partly dropped ones share an item)
        _set(index, flat_bw=flat_bw, seg_skip=seg, tile_mask=tile_mask)
        _exact(_device_search(index, q, k), ref)
        d = index.last_dispatch()
        assert d["sample_p"] == 0 and d["tile_skip"] and "flat_rest" in d["kernels"], d
        assert d["seg_skip"] == bool(seg and tile_mask), d
        if flat_bw:
            assert d["band_tiles"]["rest"] == 8, d
        got = _counted(index, lambda: _device_search(index, q, k), ref)
        pool = "bound_pool" in index.last_dispatch()["kernels"]
        for row in q:
            assert mm.theta_bound(bmax, row, k, pool) == 8.0
        want = sm.counts(ip, ix, bmax, tmask, q, k, pool, tile_mask, seg)
        print(f"  flat_bw={flat_bw} seg_skip={seg} tile_mask={tile_mask}: counters {got}, model {want[:4]}")
        assert got == want[:4]
        if seg and tile_mask:
            assert want[2] >= 9 and want[3] >= 300      # D's and E's segments, E's 300 postings
        else:
            assert want[2:4] == (0, 0)
    index.close()


# ------------------------------------------------- every option, the same bits
K = 3  # 98 tiles: the tile-bound threshold (>= 16 k tiles), pooled too (25 groups >= 8 k)


@pytest.fixture(scope="module")
def synth_case():
    from bm25mi import synth
    cfg = synth.Config("seg skip", 200_000, 200_000, 12_800_000, 40, 8, K)
    ip, ix, dt = synth.make_index(cfg, threads=8)
    q = synth.make_queries(cfg).copy()
    q[5, :] = -1                                 # an all-padding row
    q[6, 1:] = q[6, 0]                           # one term eight times
    q[7, 3:] = -1
    ref = oracle.search_c(cfg.n_docs, ip, ix, dt, q, K, threads=8)
    bmax, tmask = mm.tables(ip, ix, dt, cfg.n_docs)
    return cfg.n_docs, ip, ix, dt, q, ref, bmax, tmask


def test_option_sweep_same_bits_and_model_counts(gpu, synth_case):
    N, ip, ix, dt, q, ref, bmax, tmask = synth_case
    index = _idx(ip, ix, dt, N, segments="dense")
    model = {}
    for pooled, tile_mask, seg in itertools.product((False, True), (0, 1), (0, 1)):
        model[pooled, tile_mask, seg] = sm.counts(ip, ix, bmax, tmask, q, K, pooled, tile_mask, seg)
    # the model does drop segments on this data: at least 5 % of those of the scored tiles
    for pooled in (False, True):
        pairs, _, dsegs, _, segs = model[pooled, 1, 1]
        print(f"  model, pooled={pooled}: {pairs} pairs cut, {dsegs} of {segs} segments dropped")
        assert dsegs * 20 >= segs, (dsegs, segs)
    run = lambda: index.search(q, K)
    for seg, tile_mask, pool, tb in itertools.product((1, 0), (1, 0), (1, 0), (1, 0)):
        _set(index, seg_skip=seg, tile_mask=tile_mask, bound_pool=pool, tile_bound=tb)
        _exact(run(), ref)
        d = index.last_dispatch()
        assert d["sample_p"] == 0 and d["tile_skip"] == bool(tb), d
        assert d["seg_skip"] == bool(tb and tile_mask and seg), d
        got = _counted(index, run, ref)
        if not tb:
            assert got == (0, 0, 0, 0), got
            continue
        pooled = "bound_pool" in index.last_dispatch()["kernels"]
        want = model[pooled, tile_mask, seg]
        print(f"  seg_skip={seg} tile_mask={tile_mask} bound_pool={pool}: counters {got}, "
              f"model {want[:4]}")
        assert got == want[:4]
        assert got[:2] == model[pooled, tile_mask, 0][:2]      # the old two do not see seg_skip
        if not (seg and tile_mask):
            assert got[2:] == (0, 0)
    _set(index, **{name: 1 for name in OPTS})
    index.close()


# ------------------------------------------------------------ the other paths
def _both(index, run, ref=None, prepass=None):
    """run() with seg_skip on and off: the same bits (the reference's where
    given), seg_skip reported only where the pre-pass ran."""
    outs = []
    for seg in (1, 0):
        index.set_option("seg_skip", seg)
        outs.append(run())
        d = index.last_dispatch()
        assert d["seg_skip"] == (d["tile_skip"] and bool(seg)), d
        if prepass is not None:
            assert d["tile_skip"] == prepass, d
    index.set_option("seg_skip", 1)
    _exact(outs[0], outs[1])
    if ref is not None:
        _exact(outs[0], ref)
    return outs[0]


def test_other_paths(gpu, synth_case):
    import torch
    N, ip, ix, dt, q, ref, bmax, tmask = synth_case
    index = _idx(ip, ix, dt, N, segments="dense")
    Q = len(q)
    # 16 term lanes: no pre-pass
    q16 = np.concatenate([q, q[::-1]], axis=1)
    _both(index, lambda: index.search(q16, K), oracle.search_c(N, ip, ix, dt, q16, K, threads=8),
          prepass=False)
    # k > 4096: the large-k path, REST without tile bounds
    q4 = q[:4]
    _both(index, lambda: index.search(q4, 4097), oracle.search_c(N, ip, ix, dt, q4, 4097, threads=8),
          prepass=False)
    assert "large_k" in index.last_dispatch()["kernels"]
    # weighted: 1.0 everywhere is the plain search; other weights, seg_skip on and off
    _both(index, lambda: index.search_weighted(q, np.ones(q.shape, np.float32), K), ref)
    w = np.random.default_rng(3).uniform(0.25, 2.0, q.shape).astype(np.float32)
    _both(index, lambda: index.search_weighted(q, w, K))
    # filtered: a mask that allows everything is the plain search; every third document
    _both(index, lambda: index.search_filtered(q, K, np.ones(N, bool)), ref)
    third = np.arange(N) % 3 == 0
    _both(index, lambda: index.search_filtered(q, K, third))
    # search_after: no cursor is the first page; then the page after it
    # (without the all-padding row, which has no last document to continue from)
    qa = np.delete(q, 5, axis=0)
    page = _both(index, lambda: index.search_after(qa, K),
                 tuple(np.delete(x, 5, axis=0) for x in ref))
    after = (np.ascontiguousarray(page[1][:, -1]), np.ascontiguousarray(page[0][:, -1]))
    _both(index, lambda: index.search_after(qa, K, after))
    # a fork on its own stream beside its base
    fork = index.fork()
    dq = torch.from_numpy(q).cuda()
    outs = [(torch.empty((Q, K), dtype=torch.int32, device="cuda"),
             torch.empty((Q, K), dtype=torch.float32, device="cuda")) for _ in range(2)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for h, st, (d, s) in zip((index, fork), streams, outs):
        h.search_device(dq, K, d, s, stream=st)
    torch.cuda.synchronize()
    for h, (d, s) in zip((index, fork), outs):
        _exact((d.cpu().numpy(), s.cpu().numpy()), ref)
        dd = h.last_dispatch()
        assert dd["tile_skip"] and dd["seg_skip"], dd
    fork.close()
    index.close()


def test_two_doc_shards(gpu, synth_case):
    """Two doc shards of one process under the world's tile bounds: each
    shard's pre-pass marks its own tiles' segments under the world threshold."""
    import scipy.sparse as sp
    import torch
    N, ip, ix, dt, q, ref, bmax, tmask = synth_case
    m = sp.csc_matrix((dt, ix, ip), shape=(N, len(ip) - 1))
    cut = 37 * TILE
    shards = []
    for lo, hi in ((0, cut), (cut, N)):
        s = m[lo:hi].tocsc()
        s.sort_indices()
        shards.append(_idx(s.indptr.astype(np.int64), s.indices.astype(np.int32),
                           s.data.astype(np.float32), hi - lo, doc_offset=lo, segments="dense"))
    dq = torch.from_numpy(q).cuda()
    for seg in (1, 0):
        for s in shards:
            s.set_option("seg_skip", seg)
        _exact(_world_bounds_search(shards, dq, K), ref)
        for s in shards:
            d = s.last_dispatch()
            assert d["sample_p"] == 0 and d["tile_skip"] and d["seg_skip"] == bool(seg), d
    for s in shards:
        s.close()


@pytest.mark.parametrize("ntiles", [523, 1030])
def test_long_rows_two_and_four_tiles_per_thread(gpu, ntiles):
    """The pre-pass takes two tiles per thread from 512 tiles and four from
    1024 (80 and 98 tiles above: one): a partial last tile, rows that end
    inside a thread's group and inside a block's chunk.  Exact, and the four
    counters are the model's."""
    from bm25mi import synth
    n_docs = (ntiles - 1) * TILE + 777
    cfg = synth.Config("seg skip rows", n_docs, 4000, 3_000_000, 24, 8, K)
    ip, ix, dt = synth.make_index(cfg, threads=8)
    q = synth.make_queries(cfg).copy()
    q[2, 5:] = -1
    ref = oracle.search_c(n_docs, ip, ix, dt, q, K, threads=8)
    bmax, tmask = mm.tables(ip, ix, dt, n_docs)
    assert bmax.shape[1] == ntiles
    index = _idx(ip, ix, dt, n_docs, segments="dense")
    for seg, tile_mask in itertools.product((1, 0), (1, 0)):
        _set(index, seg_skip=seg, tile_mask=tile_mask)
        _exact(index.search(q, K), ref)
        d = index.last_dispatch()
        assert d["sample_p"] == 0 and d["tile_skip"] and d["seg_skip"] == bool(seg and tile_mask), d
        got = _counted(index, lambda: index.search(q, K), ref)
        pooled = "bound_pool" in index.last_dispatch()["kernels"]
        want = sm.counts(ip, ix, bmax, tmask, q, K, pooled, tile_mask, seg)
        print(f"  {ntiles} tiles seg_skip={seg} tile_mask={tile_mask}: counters {got}, model {want[:4]}")
        assert got == want[:4]
        if seg and tile_mask:
            assert want[0] > 0 and want[2] > 0      # tiles are cut and segments dropped here
    index.close()
