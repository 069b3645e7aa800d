"""Every route of the top-k selection stage under lists of exact length
(tests/select_cases.py): merge_fast_kernel's wave merges by list length and k,
the long-list selection (sampled threshold, digit passes, the give-up on
ties), merge_tail_kernel's block merges, the zero-fill completion, the exact
fallback stage on overflow, a doc shard's unsorted lists and the block merges
of k > 1024 — doc ids and fp32 score bits against the canonical oracle, and
the kernel's own count of block-merged queries against the Python mirror of
its dispatch (select_cases.route)."""
import time

import pytest

import select_cases as sc
from oracle import oracle
from test_gpu_parity import _exact, _idx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world():
    cases = sc.grid()
    return cases, sc.csc_of(cases)


@pytest.fixture(scope="module")
def refs(world):
    """The oracle's top-k of a k batch, computed once per k."""
    cases, (ip, ix, dt) = world
    memo = {}

    def get(k):
        if k not in memo:
            t0 = time.perf_counter()
            q = sc.batch_of(cases, k)[1]
            memo[k] = oracle.search_c(sc.N_DOCS, ip, ix, dt, q, k, threads=16)
            print(f"  oracle k={k}: {time.perf_counter() - t0:.2f} s", flush=True)
        return memo[k]
    return get


@pytest.fixture(scope="module")
def index(gpu, world):
    _, (ip, ix, dt) = world
    index = _idx(ip, ix, dt, sc.N_DOCS, segments="dense", options={"list_cap": sc.LIST_CAP})
    assert index.info()["n_tiles"] == sc.NTILES and index.info()["tile_bounds"]
    yield index
    index.close()


def _routes(k, models, C, unsorted=False):
    """The mirror's route of every row of a batch: the cases, then the
    all-padding row (no positive tile: zero fill with an empty list)."""
    r = [sc.model_route(m, k, unsorted=unsorted, C=C) for m in models]
    return r + [sc.route(0, k, 0, unsorted, C, zero_fill=True)]


@pytest.mark.parametrize("k", sc.KS)
def test_single_index_routes(gpu, world, refs, index, k):
    cases, _ = world
    rows, q = sc.batch_of(cases, k)
    models = [sc.row_model(c.docs, c.vals, k) for c in rows]
    assert [m["cnt"] for m in models] == [c.cnt for c in rows]
    routes = _routes(k, models, sc.LIST_CAP)
    want_block = sum(r in sc.BLOCK_MERGE_ROUTES for r in routes)
    ref = refs(k)
    t0 = time.perf_counter()
    for pool in (1, 0):
        for tb in (1, 0):
            index.set_option("bound_pool", pool)
            index.set_option("tile_bound", tb)
            got = index.search(q, k)
            d, st = index.last_dispatch(), index.search_stats()
            print(f"  k={k} Q={len(q)} bound_pool={pool} tile_bound={tb}: block_merge_queries="
                  f"{st['block_merge_queries']} (mirror {want_block}) fallback_queries="
                  f"{st['fallback_queries']}", flush=True)
            _exact(got, ref)
            assert d["sample_p"] == 0 and "bound_off" not in d["kernels"], d
            # (the pooled bounds serve while they hold 8 k groups of 4 tiles)
            assert ("bound_pool" in d["kernels"]) == (bool(pool) and sc.NTILES // 4 >= 8 * k), d
            assert st["fallback_queries"] == 0, st
            assert st["block_merge_queries"] == want_block, (st, sorted(set(routes)))
    index.set_option("bound_pool", 1)
    index.set_option("tile_bound", 1)
    print(f"  k={k}: 4 searches {time.perf_counter() - t0:.2f} s", flush=True)


def test_list_overflow_takes_the_exact_fallback(gpu):
    """Lists of cap and cap + 1 keys under list_cap = cap: the longer ones,
    and only they, go to the exact fallback stage.  A fresh handle per
    search: the overflow of more than 1/16 of a batch turns the handle's
    tile-bound threshold off for its next searches (bound_off)."""
    cap, k = 1024, 100
    ntiles = 1700  # >= 16 k
    n_docs = ntiles * sc.TILE - 300
    specs = [(k, c, p, None) for c in (cap, cap + 1) for p in sc.PATTERNS] + [(k, 3, "zf", None)]
    cases = sc.make_cases(specs, ntiles, n_docs, seed=77)
    ip, ix, dt = sc.csc_of(cases)
    rows, q = sc.batch_of(cases, k)
    models = [sc.row_model(c.docs, c.vals, k, ntiles) for c in rows]
    assert [m["cnt"] for m in models] == [c.cnt for c in rows]
    routes = _routes(k, models, cap)
    assert routes.count("fallback") == len(sc.PATTERNS)
    ref = oracle.search_c(n_docs, ip, ix, dt, q, k, threads=8)
    for pool, tb in ((1, 1), (0, 0)):
        index = _idx(ip, ix, dt, n_docs, segments="dense",
                     options={"list_cap": cap, "bound_pool": pool, "tile_bound": tb})
        got = index.search(q, k)
        d, st = index.last_dispatch(), index.search_stats()
        print(f"  overflow cap={cap} bound_pool={pool} tile_bound={tb}: fallback_queries="
              f"{st['fallback_queries']} block_merge_queries={st['block_merge_queries']}",
              flush=True)
        _exact(got, ref)
        assert d["sample_p"] == 0 and "bound_off" not in d["kernels"], d
        assert st["fallback_queries"] == routes.count("fallback"), st
        assert st["block_merge_queries"] == sum(r in sc.BLOCK_MERGE_ROUTES for r in routes), st
        # the switch this test keeps away from the others: the next search
        # takes the sampled threshold, exact all the same
        _exact(index.search(q, k), ref)
        assert "bound_off" in index.last_dispatch()["kernels"]
        index.close()


def test_doc_shard_unsorted_lists(gpu, world, refs):
    """The k = 100 and k = 300 batches over two doc shards of the same index
    (37 % / 63 % of the tiles) through the two-half protocol: each shard's
    list goes out unsorted (fast_merge_one's wave_kth_key branch, lists of
    513..1024 keys at k <= 128 included), the W-way merge equals the
    single-index oracle."""
    import torch
    from bm25mi.index import merge_topk_device
    cases, _ = world
    cut = sc.SHARD_CUT_TILE * sc.TILE
    edges = [0, cut, sc.N_DOCS]
    shards = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        ip, ix, dt = sc.slice_docs(cases, lo, hi)
        shards.append(_idx(ip, ix, dt, hi - lo, doc_offset=lo, segments="dense",
                           options={"list_cap": sc.LIST_CAP}))
    W, smax = len(shards), max(hi - lo for lo, hi in zip(edges[:-1], edges[1:]))
    for k in (100, 300):
        rows, q = sc.batch_of(cases, k)
        Q = len(q)
        models = [sc.shard_models(c.docs, c.vals, k, [sc.SHARD_CUT_TILE]) for c in rows]
        dq = torch.from_numpy(q).cuda()
        S = shards[0].sample_width(k, W, smax)
        assert S >= k, S  # every shard reports its share of the k best tile keys
        keys = torch.zeros((W, Q, S), dtype=torch.int64, device="cuda")
        for r, s in enumerate(shards):
            s.search_sample_device(dq, k, W, smax, keys[r])
        d = torch.empty((W, Q, k), dtype=torch.int32, device="cuda")
        sco = torch.empty((W, Q, k), dtype=torch.float32, device="cuda")
        seen = set()
        for r, s in enumerate(shards):
            s.search_finish_device(dq, k, W, smax, keys, d[r], sco[r])
            torch.cuda.synchronize()
            dis, st = s.last_dispatch(), s.search_stats()
            routes = _routes(k, [m[r] for m in models], sc.LIST_CAP, unsorted=True)
            seen |= set(routes)
            want_block = sum(x in sc.BLOCK_MERGE_ROUTES for x in routes)
            print(f"  k={k} shard {r}: block_merge_queries={st['block_merge_queries']} (mirror "
                  f"{want_block}) fallback_queries={st['fallback_queries']}", flush=True)
            assert dis["sample_p"] == 0 and "bound_keys" in dis["kernels"], dis
            assert st["fallback_queries"] == 0, st
            assert st["block_merge_queries"] == want_block, (st, sorted(set(routes)))
        assert {"shard4", "shard8", "shard16"} <= seen and ("shard32" in seen) == (k == 300), seen
        od = torch.empty((Q, k), dtype=torch.int32, device="cuda")
        os_ = torch.empty((Q, k), dtype=torch.float32, device="cuda")
        merge_topk_device(0, d, sco, W, Q, k, od, os_)
        torch.cuda.synchronize()
        _exact((od.cpu().numpy(), os_.cpu().numpy()), refs(k))
    for s in shards:
        s.close()
