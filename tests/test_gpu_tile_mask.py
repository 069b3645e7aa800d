"""The REST pass's tile bounds on the GPU: the sub-block presence masks
(build_tmask_kernel, bm25_index_masks_export), the pre-pass that turns them
and the per-(term, tile) maxima into one skip bit per (query, tile)
(tile_skip_kernel) and the REST kernel that reads the bits.  Results are the
oracle's bit for bit under every setting of tile_mask, bound_pool and
tile_bound, and the pairs and postings the count_skips build reports are the
numpy model's (tests/mask_model.py) exactly."""
import itertools

import numpy as np
import pytest

import mask_model as mm
from oracle import oracle
from test_gpu_edges import _csc
from test_gpu_parity import _exact, _idx, _world_bounds_search

pytestmark = pytest.mark.gpu

TILE = mm.TILE
COMBOS = list(itertools.product((1, 0), (1, 0), (1, 0)))  # tile_mask, bound_pool, tile_bound


def _export_masks(index):
    import torch
    stride = index.bounds_stride() + 4          # a wider row: zero past the index's own
    out = torch.full((index.n_terms, stride), -1, dtype=torch.int32, device="cuda")
    index.masks_export(out, stride)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)


def test_masks_export_matches_numpy(gpu):
    """A partial last tile (993 documents) and 41 tiles (41 % 8 != 0);
    postings on the edges of the 64-document sub-blocks; an empty term; a
    term in every document."""
    N = 40 * TILE + 993
    rng = np.random.default_rng(11)
    edge = np.array([0, 63, 64, 1983, 2047])
    cols = []
    for tiles in ([0, 7, 8, 39, 40], [40], list(range(41))):
        d = np.concatenate([t * TILE + edge for t in tiles])
        cols.append((np.sort(d[d < N]).astype(np.int32), None))
    cols.append((np.zeros(0, np.int32), None))                      # an empty term
    cols.append((np.arange(N, dtype=np.int32), None))               # every document
    for _ in range(20):
        cols.append((np.sort(rng.choice(N, int(rng.integers(1, 400)), replace=False)).astype(np.int32),
                     None))
    cols = [(d, rng.uniform(0.5, 4.0, len(d)).astype(np.float32)) for d, _ in cols]
    ip, ix, dt = _csc(cols, np.float32)
    index = _idx(ip, ix, dt, N, segments="dense")
    got = _export_masks(index)
    _, want = mm.tables(ip, ix, dt, N)
    nt = want.shape[1]
    assert nt == 41 and got.shape[1] == 48
    assert np.array_equal(got[:, :nt], want)
    assert not got[:, nt:].any()
    assert got[3].sum() == 0 and (got[4, :40] == 0xFFFFFFFF).all() and got[4, 40] == (1 << 16) - 1
    assert got[1, 40] == 3 and got[0, 39] == (1 | 2 | 1 << 30 | 1 << 31)
    fork = index.fork()                          # the table is shared with a fork
    assert np.array_equal(_export_masks(fork), got)
    fork.close()
    with pytest.raises(ValueError, match="stride"):
        import torch
        index.masks_export(torch.empty((len(cols), 8), dtype=torch.int32, device="cuda"), 8)
    index.close()


# ---------------------------------------------------------------- the fixture
A, B, C = 0, 1, 2
ANCHORS = (10, 20, 30, 40)
X, Y, Z, W_ = 50, 51, 52, 53
NT_FIX = 80


def _fixture_csc():
    """k = 4 anchor tiles hold one document with A = 8.0, which sets the
    tile-bound threshold of a query with A to 8.0 (f16-exact values, far from
    every boundary).  Tile X: B = 5.0 and C = 5.0 in different sub-blocks;
    tile Y: in the same sub-block on different documents; tile Z: on the same
    document; tile W: B alone."""
    a = np.array([t * TILE + 100 for t in ANCHORS], np.int32)
    b = np.array([X * TILE + 10, Y * TILE + 70, Z * TILE + 500, W_ * TILE + 5], np.int32)
    c = np.array([X * TILE + 1000, Y * TILE + 100, Z * TILE + 500], np.int32)
    cols = [(a, np.full(len(a), 8.0, np.float32)), (b, np.full(len(b), 5.0, np.float32)),
            (c, np.full(len(c), 5.0, np.float32)), (np.zeros(0, np.int32), np.zeros(0, np.float32))]
    return _csc(cols, np.float32)


def test_constructed_fixture_skips_by_sub_block(gpu):
    N = NT_FIX * TILE
    ip, ix, dt = _fixture_csc()
    q = np.full((3, 8), -1, np.int32)
    q[0, :3] = [A, B, C]
    q[1, :3] = [B, B, A]                         # the duplicate counts twice
    q[2, :4] = [C, -1, A, 3]                     # padding and an empty term between terms
    k = 4
    ref = oracle.search_c(N, ip, ix, dt, q, k)
    assert ref[1][0].tolist() == [10.0, 8.0, 8.0, 8.0] and ref[0][0, 0] == Z * TILE + 500
    assert ref[1][1].tolist() == [10.0] * 4 and W_ * TILE + 5 in ref[0][1]
    index = _idx(ip, ix, dt, N, segments="dense")
    bmax, tmask = mm.tables(ip, ix, dt, N)
    for tile_mask in (1, 0):
        index.set_option("tile_mask", tile_mask)
        index.set_option("count_skips", 0)
        _exact(index.search(q, k), ref)
        d = index.last_dispatch()
        assert d["sample_p"] == 0 and d["tile_skip"] and "flat_rest" in d["kernels"], d
        index.set_option("count_skips", 1)
        _exact(index.search(q, k), ref)
        pool = "bound_pool" in index.last_dispatch()["kernels"]
        pairs = posts = 0
        for r, row in enumerate(q):
            theta = mm.theta_bound(bmax, row, k, pool)
            assert theta == 8.0, (r, theta)
            whole, skipped = mm.skip_model(bmax, tmask, row, theta, use_mask=bool(tile_mask))
            if r == 0:  # X falls to the masks alone; Y and Z are scored; W has B alone
                assert not whole[X] and skipped[X] == bool(tile_mask)
                assert not skipped[Y] and not skipped[Z] and whole[W_]
                assert not skipped[list(ANCHORS)].any()
            if r == 1:  # 2 x 5.0 reaches 8.0 wherever B stands
                assert not skipped[[X, Y, Z, W_]].any()
            pairs += int(skipped.sum())
            posts += mm.skipped_postings(ip, ix, row, skipped)
        st = index.search_stats()
        print(f"  tile_mask={tile_mask}: skipped pairs {st['bound_skipped_tiles']} (model {pairs}), "
              f"postings {st['bound_skipped_postings']} (model {posts})")
        assert st["bound_skipped_tiles"] == pairs and st["bound_skipped_postings"] == posts
    index.close()


# ------------------------------------------------- every option, the same bits
K = 3  # 98 tiles: the tile-bound threshold (>= 16 k tiles), pooled too (25 groups >= 8 k)


@pytest.fixture(scope="module")
def synth_case():
    from bm25mi import synth
    cfg = synth.Config("tile mask", 200_000, 200_000, 12_800_000, 40, 8, K)
    ip, ix, dt = synth.make_index(cfg, threads=8)
    q = synth.make_queries(cfg).copy()
    q[5, :] = -1                                 # an all-padding row
    q[6, 1:] = q[6, 0]                           # one term eight times
    q[7, 3:] = -1
    return cfg.n_docs, ip, ix, dt, q


def _sweep(index, run, ref, model=None, prepass=True):
    """run() under the eight settings: the reference's bits every time;
    prepass: whether a search with the tile bound on launches the pre-pass;
    model(tile_mask, pool) -> the (pairs, postings) count_skips must report
    when the tile bound is on (a search under the tile-bound threshold)."""
    for tile_mask, pool, tb in COMBOS:
        for name, v in (("tile_mask", tile_mask), ("bound_pool", pool), ("tile_bound", tb)):
            index.set_option(name, v)
        _exact(run(), ref)
        d = index.last_dispatch()
        assert d["tile_skip"] == (bool(tb) and prepass), (tile_mask, pool, tb, d)
        if model is None:
            continue
        assert d["sample_p"] == 0, d
        index.set_option("count_skips", 1)
        _exact(run(), ref)
        st = index.search_stats()
        index.set_option("count_skips", 0)
        if not tb:
            assert st["bound_skipped_tiles"] == 0 and st["bound_skipped_postings"] == 0
            continue
        pooled = "bound_pool" in index.last_dispatch()["kernels"]
        want = model(tile_mask, pooled)
        print(f"  tile_mask={tile_mask} bound_pool={pool}: skipped (pairs, postings) "
              f"{(st['bound_skipped_tiles'], st['bound_skipped_postings'])}, model {want}")
        assert (st["bound_skipped_tiles"], st["bound_skipped_postings"]) == want
    for name in ("tile_mask", "bound_pool", "tile_bound"):
        index.set_option(name, 1)


def _counts(ip, ix, bmax, tmask, q, k):
    def model(tile_mask, pooled):
        pairs = posts = 0
        for row in q:
            theta = mm.theta_bound(bmax, row, k, pooled)
            _, skipped = mm.skip_model(bmax, tmask, row, theta, use_mask=bool(tile_mask))
            pairs += int(skipped.sum())
            posts += mm.skipped_postings(ip, ix, row, skipped)
        return pairs, posts
    return model


@pytest.mark.parametrize("case", ["batch", "q1", "t3", "split"])
def test_options_same_bits_and_model_counts(gpu, synth_case, case):
    """98 tiles, k = 3: the tile-bound threshold (P = 0), so the model knows
    theta; a batch with an all-padding row, Q = 1, T = 3, REST over split
    items.  With tile_mask = 0 the skipped pairs are the whole-tile model's,
    with it the masked model's."""
    N, ip, ix, dt, q = synth_case
    k = K
    if case == "q1":
        q = q[3:4]
    if case == "t3":
        q = np.ascontiguousarray(q[:, :3])
    index = _idx(ip, ix, dt, N, segments="dense",
                 options={"rest_split": 1} if case == "split" else None)
    ref = oracle.search_c(N, ip, ix, dt, q, k, threads=8)
    bmax, tmask = mm.tables(ip, ix, dt, N)
    _sweep(index, lambda: index.search(q, k), ref, _counts(ip, ix, bmax, tmask, q, k))
    if case == "split":
        index.search(q, k)
        assert "rest_split" in index.last_dispatch()["kernels"]
    if case == "batch":
        # the masks do cut pairs on this data (config 3's vocabulary and density)
        m = _counts(ip, ix, bmax, tmask, q, k)
        assert m(1, True)[0] > m(0, True)[0]
    index.close()


def test_one_tile_and_sampled_threshold(gpu, synth_case):
    """One tile (the exact pass: no REST, no pre-pass) and k = 20 on 98
    tiles (a sampled threshold, every 8th tile a sample: REST takes the bits
    under the sampled theta)."""
    import scipy.sparse as sp
    N, ip, ix, dt, q = synth_case
    s = sp.csc_matrix((dt, ix, ip), shape=(N, len(ip) - 1))[:TILE].tocsc()
    s.sort_indices()
    ip1, ix1, dt1 = s.indptr.astype(np.int64), s.indices.astype(np.int32), s.data.astype(np.float32)
    one = _idx(ip1, ix1, dt1, TILE, segments="dense")
    ref = oracle.search_c(TILE, ip1, ix1, dt1, q, K)
    _sweep(one, lambda: one.search(q, K), ref, prepass=False)
    assert one.last_dispatch()["sample_p"] == 1
    one.close()
    index = _idx(ip, ix, dt, N, segments="dense")
    ref = oracle.search_c(N, ip, ix, dt, q, 20, threads=8)
    _sweep(index, lambda: index.search(q, 20), ref)
    assert index.last_dispatch()["sample_p"] > 1
    index.close()


def test_shards_under_world_bounds(gpu, synth_case):
    """Two doc shards of one process under the world's tile bounds: each
    shard's pre-pass reads the world threshold and its own tables."""
    import torch
    N, ip, ix, dt, q = synth_case
    import scipy.sparse as sp
    m = sp.csc_matrix((dt, ix, ip), shape=(N, len(ip) - 1))
    cut = 37 * TILE
    shards = []
    for lo, hi in ((0, cut), (cut, N)):
        s = m[lo:hi].tocsc()
        s.sort_indices()
        shards.append(_idx(s.indptr.astype(np.int64), s.indices.astype(np.int32),
                           s.data.astype(np.float32), hi - lo, doc_offset=lo, segments="dense"))
    dq = torch.from_numpy(q).cuda()
    ref = oracle.search_c(N, ip, ix, dt, q, K, threads=8)
    for tile_mask, pool, tb in COMBOS:
        for s in shards:
            for name, v in (("tile_mask", tile_mask), ("bound_pool", pool), ("tile_bound", tb)):
                s.set_option(name, v)
        _exact(_world_bounds_search(shards, dq, K), ref)
        for s in shards:
            d = s.last_dispatch()
            assert d["sample_p"] == 0 and d["tile_skip"] == bool(tb), d
    for s in shards:
        s.close()


def test_large_k_list_path(gpu):
    """k = 4097 on the 1027-tile fixture of tests/test_handle_reuse_host.py:
    the list path's REST (per-tile slots) runs without tile bounds — under
    its low theta they cut too few tiles to pay for the pre-pass — and gives
    the same bits under every setting."""
    from test_handle_reuse_host import N_BIG, pools, reuse_csc
    ip, ix, dt = reuse_csc(big=True)
    q = np.ascontiguousarray(pools()[0][:4, :8])
    index = _idx(ip, ix, dt, N_BIG, segments="dense")
    ref = oracle.search_c(N_BIG, ip, ix, dt, q, 4097, threads=8)
    for tile_mask, pool, tb in COMBOS:
        for name, v in (("tile_mask", tile_mask), ("bound_pool", pool), ("tile_bound", tb)):
            index.set_option(name, v)
        _exact(index.search(q, 4097), ref)
        d = index.last_dispatch()
        assert {"large_k", "flat_rest"} <= d["kernels"] and not d["tile_skip"], d
    # a sampled threshold with sample tiles in groups of 8 and one key each: REST keeps its
    # sample-key skip, and no pre-pass runs
    for name, v in (("tile_mask", 1), ("bound_pool", 1), ("tile_bound", 1), ("theta_bound", 0)):
        index.set_option(name, v)
    _exact(index.search(q, 50), oracle.search_c(N_BIG, ip, ix, dt, q, 50, threads=8))
    d = index.last_dispatch()
    assert d["sample_p"] > 1 and "flat_rest" in d["kernels"] and not d["tile_skip"], d
    index.close()


def test_fork_searches_beside_its_base(gpu, synth_case):
    """Two handles on the shared tables, each with its own skip bitmap: the
    fork searches on one stream while the base does on another."""
    import torch
    N, ip, ix, dt, q = synth_case
    base = _idx(ip, ix, dt, N, segments="dense")
    fork = base.fork()
    assert fork.info()["device_bytes"] == base.info()["device_bytes"]
    qa, qb = q[:20], q[20:]
    refs = [oracle.search_c(N, ip, ix, dt, x, K, threads=8) for x in (qa, qb)]
    dqs = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (qa, qb)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [(torch.empty((len(x), K), dtype=torch.int32, device="cuda"),
             torch.empty((len(x), K), dtype=torch.float32, device="cuda")) for x in (qa, qb)]
    torch.cuda.synchronize()
    for _ in range(3):
        for h, dq, st, (d, s) in zip((base, fork), dqs, streams, outs):
            h.search_device(dq, K, d, s, stream=st)
    torch.cuda.synchronize()
    for h, (d, s), ref in zip((base, fork), outs, refs):
        _exact((d.cpu().numpy(), s.cpu().numpy()), ref)
        assert h.last_dispatch()["tile_skip"]
    fork.close()
    base.close()
