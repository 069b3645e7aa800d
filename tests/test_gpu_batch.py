"""The query-batch axis Q at its limits (plans in tests/batch_cases.py, their
edges proved by tests/test_batch_model.py): doc ids and fp32 score bits
against the references the per-entry-point files use.

A  few flat items — fewer items than XCD ranges or claim counters, ranges
   that are no multiple of claim_ch, a grid shrunk by grid_pct — swept on one
   handle per index: score_flat_kernel's claim counters reset themselves at
   the end of a launch, so a miscount shows in the NEXT search of the handle.
B  Q = 65 535, 65 536, 65 537 on every search entry point: the kernels of one
   workgroup per query, the y-grid of the dense rows and its chunk seam.  Row
   i of a batch is row i % 257 of a pool, so a row index cut to 16 bits (65 536
   % 257 = 1) answers another query.
C  the exact fallback stage's own row count: 0, 1, 63, 64, 65, 129 and all of
   130 rows overflow their list (64 rescore / merge blocks serve the stage).
D  Q = 0 on every batch entry point: success, nothing written.

Two limits of Q in the code are not reachable at test size and are not
tested: use_flat needs ntiles * Q < 2^31 - 1, but the workspace alone is 32 B
per (query, tile), 64 GB at that limit; and the Q < 2^20 guard of the split
REST items sits behind ceil(ntiles / 8) * Q < 48 * 19 * CUs, a few hundred
thousand items, so it cannot be the deciding term.

Host time of the references is printed per case (run with -s)."""
import time

import numpy as np
import pytest

import batch_cases as bc
import select_cases as sc
from oracle import oracle
from test_gpu_parity import _doc_slice, _exact, _idx, _want_kernels
from test_gpu_search_filtered import _pack, _want as filtered_want
from test_search_after_host import last_column, ref_after
from test_search_weighted_host import ref_rows

pytestmark = pytest.mark.gpu

BAD_DOC, BAD_SCORE, BAD_WORD = 123456789, 7.5, 0x5A5A5A5A
FLAGS = {"bound_off", "count_skips", "rest_split", "bound_pool"}


def _timed(what, fn):
    t0 = time.perf_counter()
    out = fn()
    print(f"  host reference {what}: {time.perf_counter() - t0:.2f} s", flush=True)
    return out


def _take(ref, rows):
    return ref[0][rows], ref[1][rows]


# ===================================================== A. few items, claims
_A_REFS = {}


def _a_ref(tiles, T, k):
    key = (tiles, T, k)
    if key not in _A_REFS:
        _A_REFS[key] = oracle.search_c(bc.a_docs(tiles), *bc.a_index(tiles), bc.a_queries(T), k,
                                       threads=8)
    return _A_REFS[key]


@pytest.mark.parametrize("name,tiles,segments,bw", bc.A_INDICES, ids=[c[0] for c in bc.A_INDICES])
def test_few_items_on_one_handle(gpu, name, tiles, segments, bw):
    """Every Q of the plan under every (claim_ch, claim_m, grid_pct), T, k and
    threshold route, all on one handle: each search starts from the claim
    counters the one before left.  After an option change a search of 129 rows
    and then one of a single row: a counter left non-zero skips the lone item."""
    ip, ix, dt = bc.a_index(tiles)
    n = bc.a_docs(tiles)
    index = _idx(ip, ix, dt, n, segments=segments, options={"flat_bw": bw})
    info = index.info()
    assert info["n_tiles"] == tiles and info["sparse"] == (segments == "sparse")
    _timed(f"A {name}", lambda: [_a_ref(tiles, T, k) for T in bc.A_TS for k in bc.A_KS])
    searches = 0

    def check(q, k, ref, Q, route, what):
        nonlocal searches
        got = index.search(q[:Q], k)
        searches += 1
        d = index.last_dispatch()
        kernels = d["kernels"]
        if route["sample_p"] == 1:
            P = 1
        elif (route["theta_bound"] and info["tile_bounds"] and tiles >= 16 * k
              and "bound_off" not in kernels):
            P = 0
        else:
            P = 2
        assert d["sample_p"] == P and kernels - FLAGS == _want_kernels(P, True), (what, Q, d)
        phases = {"flat_all": "all", "flat_sample": "sample", "flat_rest": "rest"}
        for kern, ph in phases.items():   # items = bands of min(flat_bw, 8) tiles x queries
            if kern in kernels:
                assert d["band_tiles"][ph] == bw, (what, Q, d)
        try:
            _exact(got, _take(ref, slice(0, Q)))
        except AssertionError as e:
            raise AssertionError(f"{what} Q={Q}: {e}") from None

    t0 = time.perf_counter()
    for T in bc.A_TS:
        q = bc.a_queries(T)
        for k in bc.A_KS:
            ref = _a_ref(tiles, T, k)
            for route in bc.a_routes(tiles):
                for name_, v in route.items():
                    index.set_option(name_, v)
                for ch in bc.A_CLAIM_CH:
                    for cm in bc.A_CLAIM_M:
                        for pct in bc.A_GRID_PCT:
                            index.set_option("claim_ch", ch)
                            index.set_option("claim_m", cm)
                            index.set_option("grid_pct", pct)
                            what = dict(route, T=T, k=k, claim_ch=ch, claim_m=cm, grid_pct=pct)
                            check(q, k, ref, bc.A_ROWS, route, what)
                            check(q, k, ref, 1, route, what)
                            for Q in bc.A_QS:
                                check(q, k, ref, Q, route, what)
    print(f"  A {name}: {searches} searches {time.perf_counter() - t0:.2f} s", flush=True)
    index.close()


# ======================================================== B. Q at 2^16 +- 1
class _World:
    """The 16-tile index of section B (or the 3-tile one), the pool and its
    references, each computed once."""

    def __init__(self, small):
        self.small = small
        self.n = bc.B_SMALL_DOCS if small else bc.B_DOCS
        self.csc = bc.b_index(small)
        self.pool = bc.b_pool()
        self.w = bc.b_weights()
        self.allow = bc.b_masks(self.n)
        self.memo = {}

    def get(self, key, fn):
        if key not in self.memo:
            self.memo[key] = _timed(f"B {'small ' if self.small else ''}{key}", fn)
        return self.memo[key]

    def rows(self):
        return self.get("dense rows", lambda: [oracle.scores_dense_c(self.n, *self.csc, r)
                                               for r in self.pool])

    def plain(self, k):
        return self.get(("plain", k),
                        lambda: oracle.search_c(self.n, *self.csc, self.pool, k, threads=8))

    def filtered(self, k):
        """The 257 x 4 (pool row, mask id 0, 1, 2, -1) reference rows."""
        rows = self.rows()
        return self.get(("filtered", k), lambda: filtered_want(
            [rows[c // 4] for c in range(4 * bc.B_POOL)], k, self.allow,
            [(c % 4 + 1) % 4 - 1 for c in range(4 * bc.B_POOL)]))

    def weighted(self, k):
        return self.get(("weighted", k), lambda: ref_after(
            ref_rows(self.n, *self.csc, self.pool, self.w), k))

    def after(self, k, k_before):
        """(cursors, page): the page of k after a first page of k_before."""
        cur = last_column(self.plain(k_before))
        return cur, self.get(("after", k, k_before), lambda: ref_after(self.rows(), k, cur))


@pytest.fixture(scope="module")
def world(gpu):
    return _World(False)


@pytest.fixture(scope="module")
def small_world(gpu):
    return _World(True)


@pytest.fixture(scope="module")
def big_index(world):
    index = _idx(*world.csc, world.n, segments="dense")
    info = index.info()
    assert info["n_tiles"] == bc.B_TILES and info["tile_bounds"]
    yield index
    index.close()


def _device_search(index, dq, k):
    import torch
    Q = dq.shape[0]
    dd = torch.full((Q, k), BAD_DOC, dtype=torch.int32, device="cuda")
    ds = torch.full((Q, k), BAD_SCORE, dtype=torch.float32, device="cuda")
    index.search_device(dq, k, dd, ds)
    torch.cuda.synchronize()
    return dd.cpu().numpy(), ds.cpu().numpy()


B_ROUTES = (("tile-bound", {"theta_bound": 1, "sample_p": 8}),
            ("sampled", {"theta_bound": 0, "sample_p": 8}),
            ("all", {"theta_bound": 1, "sample_p": 1}))


@pytest.mark.parametrize("Q", bc.B_QS)
def test_large_q_plain_search(world, big_index, Q):
    """search at k = 1 and 10 by each threshold route (the tile-bound keys
    serve k = 1 on 16 tiles), host and device form."""
    import torch
    rows = bc.b_rows(Q)
    q = world.pool[rows]
    dq = torch.from_numpy(q).cuda()
    t0 = time.perf_counter()
    try:
        for k in bc.B_KS:
            want = _take(world.plain(k), rows)
            for name, opts in B_ROUTES:
                for o, v in opts.items():
                    big_index.set_option(o, v)
                _exact(big_index.search(q, k), want)
                d = big_index.last_dispatch()
                P = 1 if name == "all" else 0 if (
                    name == "tile-bound" and k == 1 and "bound_off" not in d["kernels"]) \
                    else bc.sample_geom(bc.B_TILES, k)[0]
                assert d["sample_p"] == P, (name, k, d)
                _exact(_device_search(big_index, dq, k), want)
                assert big_index.search_stats()["fallback_queries"] == 0
    finally:
        big_index.set_option("theta_bound", 1)
        big_index.set_option("sample_p", 8)
    print(f"  B plain Q={Q}: 12 searches {time.perf_counter() - t0:.2f} s", flush=True)


@pytest.mark.parametrize("Q", bc.B_QS)
def test_large_q_filtered_weighted_after(world, big_index, Q):
    """search_filtered (3 masks, mask ids cycling 0, 1, 2, -1), search_weighted
    (signed weights) and search_after (cursors of the page before) at k = 10."""
    rows, k = bc.b_rows(Q), max(bc.B_KS)
    q = world.pool[rows]
    packed = _pack(world.allow)
    want_f, want_w = world.filtered(k), world.weighted(k)
    cur, want_a = world.after(k, k)
    t0 = time.perf_counter()
    _exact(big_index.search_filtered(q, k, packed, bc.b_query_mask(Q)), _take(want_f, bc.b_combo(Q)))
    assert "filtered" in big_index.last_dispatch()["kernels"]
    _exact(big_index.search_weighted(q, world.w[rows], k), _take(want_w, rows))
    assert "weighted" in big_index.last_dispatch()["kernels"]
    page = big_index.search(q, k)
    _exact(page, _take(world.plain(k), rows))
    import bm25mi
    after = bm25mi.page_cursor(*page)
    assert np.array_equal(after[1], cur[1][rows])
    _exact(big_index.search_after(q, k, after), _take(want_a, rows))
    assert "after" in big_index.last_dispatch()["kernels"]
    print(f"  B filtered/weighted/after Q={Q}: {time.perf_counter() - t0:.2f} s", flush=True)


@pytest.mark.parametrize("Q", bc.B_QS)
def test_large_q_boolean_and_score_docs(world, big_index, Q):
    """search_boolean(total_hits=True) with a clause row per query, and
    score_docs with C = 3."""
    from test_gpu_term_masks import _has_of, _want as masks_want
    rows, k = bc.b_rows(Q), max(bc.B_KS)
    q = world.pool[rows]
    mu, an, mn = bc.b_clauses()

    def ref():
        has = _has_of(world.csc[0], world.csc[1], bc.B_V, world.n)
        packed = masks_want(has, mu, an, mn, bc.B_POOL)
        allow = np.unpackbits(packed.view(np.uint8), axis=1, bitorder="little")[:, :world.n] > 0
        return (filtered_want(world.rows(), k, allow, np.arange(bc.B_POOL)),
                allow.sum(axis=1).astype(np.int64))
    want, totals = world.get(("boolean", k), ref)
    assert (totals == world.n).any() and (totals < world.n / 50).sum() > bc.B_POOL / 4
    docs = bc.b_score_docs(world.n)
    dense = np.stack(world.rows())
    want_s = np.where(docs >= 0, np.take_along_axis(dense, np.maximum(docs, 0), axis=1),
                      np.float32(0))
    t0 = time.perf_counter()
    gd, gs, gt = big_index.search_boolean(q, k, mu[rows], an[rows], mn[rows], total_hits=True)
    _exact((gd, gs), _take(want, rows))
    assert np.array_equal(gt, totals[rows])
    got = big_index.score_docs(q, docs[rows])
    assert np.array_equal(got.view(np.uint32), want_s[rows].view(np.uint32))
    print(f"  B boolean/score_docs Q={Q}: {time.perf_counter() - t0:.2f} s", flush=True)


@pytest.fixture(scope="module")
def shards(world):
    cut = bc.B_TILES // 2 * bc.TILE
    edges = [0, cut, world.n]
    out = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        csc = _doc_slice(*world.csc, lo, hi)
        out.append((lo, hi, csc, _idx(*csc, hi - lo, doc_offset=lo, segments="dense")))
    yield out
    for s in out:
        s[3].close()


@pytest.mark.parametrize("Q", bc.B_QS)
def test_large_q_shards_and_merges(world, shards, Q):
    """Two 8-tile shards of the 16-tile index: the two-half protocol
    (search_sample_device / search_finish_device) and merge_topk_device give
    the single-index result; each shard's own search is its oracle's, and
    merge_sorted_device of the two gives the single-index result again."""
    import torch
    from bm25mi.index import merge_sorted_device, merge_topk_device
    rows = bc.b_rows(Q)
    dq = torch.from_numpy(world.pool[rows]).cuda()
    W, smax = len(shards), max(hi - lo for lo, hi, _, _ in shards)
    t0 = time.perf_counter()
    for k in bc.B_KS:
        want = _take(world.plain(k), rows)
        S = shards[0][3].sample_width(k, W, smax)
        assert S > 0
        keys = torch.zeros((W, Q, S), dtype=torch.int64, device="cuda")
        for r, s in enumerate(shards):
            s[3].search_sample_device(dq, k, W, smax, keys[r])
        d = torch.full((W, Q, k), BAD_DOC, dtype=torch.int32, device="cuda")
        sco = torch.full((W, Q, k), BAD_SCORE, dtype=torch.float32, device="cuda")
        for r, s in enumerate(shards):
            s[3].search_finish_device(dq, k, W, smax, keys, d[r], sco[r])
        od = torch.full((Q, k), BAD_DOC, dtype=torch.int32, device="cuda")
        os_ = torch.full((Q, k), BAD_SCORE, dtype=torch.float32, device="cuda")
        merge_topk_device(0, d, sco, W, Q, k, od, os_)
        torch.cuda.synchronize()
        _exact((od.cpu().numpy(), os_.cpu().numpy()), want)
        # sorted lists: each shard's own search
        for r, (lo, hi, csc, index) in enumerate(shards):
            index.search_device(dq, k, d[r], sco[r])
            ref = world.get(("shard", r, k),
                            lambda: oracle.search_c(hi - lo, *csc, world.pool, k, threads=8))
            torch.cuda.synchronize()
            _exact((d[r].cpu().numpy(), sco[r].cpu().numpy()), (ref[0][rows] + lo, ref[1][rows]))
        od.fill_(BAD_DOC)
        os_.fill_(BAD_SCORE)
        merge_sorted_device(0, d, sco, W, Q, k, Q * k, od, os_)
        torch.cuda.synchronize()
        _exact((od.cpu().numpy(), os_.cpu().numpy()), want)
    print(f"  B shards/merges Q={Q}: {time.perf_counter() - t0:.2f} s", flush=True)


def _exact_blocks(got, want, index_of, Q, period):
    """_exact over row blocks of one period of the pool (the expected array
    of a k = 4097 batch is never built whole), then the seam rows by name."""
    for b in range(0, Q, period):
        e = min(Q, b + period)
        idx = index_of[b:e]
        try:
            _exact((got[0][b:e], got[1][b:e]), (want[0][idx], want[1][idx]))
        except AssertionError as err:
            raise AssertionError(f"rows {b}..{e - 1}: {err}") from None
    for r in bc.B_SEAM:
        i = index_of[r]
        assert np.array_equal(got[0][r], want[0][i]), f"row {r}: docs"
        assert np.array_equal(got[1][r].view(np.uint32), want[1][i].view(np.uint32)), f"row {r}"


@pytest.mark.parametrize("case", ["large_lists=0", "large_lists=1", "filtered", "after",
                                  "filtered-dense-k10", "after-dense-k10"])
def test_large_q_dense_rows(small_world, case):
    """Q = 65 537 on the dense-row paths (bm25mi_large.hip), whose chunk of
    queries on gridDim.y is capped at 65 535 rows: rows 65 534..65 536 beside
    the whole result.

    n_docs = 4097 (3 tiles), the smallest index that serves k = 4097.  At k =
    4097 the cap still does not decide the chunk: a row costs its 24 KiB of
    scores, 16 k B of keys and 8 k B + the sort's scratch, more than 120 KiB,
    so the library's scratch budget (at most 4 GiB) gives chunks of fewer than
    35 000 rows whatever n_docs is — the seams these cases cross are the
    budget's.  The 65 535 cap itself decides at small k, where a row costs
    about 27 KiB (150 000 rows would fit): the two k = 10 cases send every
    query down the same dense path (option filter_tiles = 0), in chunks of
    65 535 and 2 rows.

    The filtered and the cursor search build the handle's workspace for k =
    4096 (lists of 65 536 keys a query without the option): list_cap = 64 keeps
    it small; the lists are not used on this path."""
    w = small_world
    Q = bc.B_QS[-1]
    rows = bc.b_rows(Q)
    q = w.pool[rows]
    K = bc.B_BIG_K
    t0 = time.perf_counter()
    if case.startswith("large_lists"):
        index = _idx(*w.csc, w.n, segments="dense", options={"large_lists": int(case[-1])})
        want = w.plain(K)
        got = index.search(q, K)
        assert "large_k" in index.last_dispatch()["kernels"]
        _exact_blocks(got, want, rows, Q, bc.B_POOL)
    else:
        k = K if "k10" not in case else 10
        opts = {"list_cap": bc.B_BIG_LIST_CAP} if k == K else {"filter_tiles": 0}
        index = _idx(*w.csc, w.n, segments="dense", options=opts)
        if case.startswith("filtered"):
            want = w.filtered(k)
            got = index.search_filtered(q, k, _pack(w.allow), bc.b_query_mask(Q))
            _exact_blocks(got, want, bc.b_combo(Q), Q, 4 * bc.B_POOL)
        else:
            cur, want = w.after(k, 10)
            got = index.search_after(q, k, (cur[0][rows], cur[1][rows]))
            _exact_blocks(got, want, rows, Q, bc.B_POOL)
        assert "large_k" in index.last_dispatch()["kernels"]
        assert index.filtered_stats()[0] == Q
    index.close()
    print(f"  B dense rows {case}: {time.perf_counter() - t0:.2f} s", flush=True)


# ============================================ C. the fallback stage's rows
@pytest.fixture(scope="module")
def pools(gpu):
    cases, pools = bc.c_pools()
    return cases, pools, sc.csc_of(cases)


_C_REFS = {}


@pytest.mark.parametrize("segments", ["dense", "sparse"])
def test_fallback_stage_row_counts(pools, segments):
    """F of the Q rows overflow their list of list_cap = 256 keys by one key —
    F = 0, 1, 63, 64, 65, 129, 130 of 130, 1 of 1, 64 of 64 — with theta_bound
    1 and 0 and both score kernels.  The lists are those of the threshold the
    search takes, each with terms of its own (batch_cases.c_pools): the
    tile-bound one (a dense index under theta_bound), else the sampled one —
    under which score_wave_kernel's sample reports a zero-score key for a tile
    without a positive sum, so the all-padding row lists half the index and is
    one of the F.  A fresh handle per search: an overflow of more than 1/16 of
    a batch turns the handle's tile-bound threshold off."""
    cases, term_pools, (ip, ix, dt) = pools
    k, cap = bc.C_K, bc.C_CAP
    t0 = time.perf_counter()
    for Q, F in bc.C_BATCHES:
        for tb in (1, 0):
            for flat in (1, 0):
                bound = segments == "dense" and tb == 1
                zero_keys = not bound and not flat
                key = (bound, zero_keys, Q, F)
                if key not in _C_REFS:
                    q, desc = bc.c_batch(term_pools, "bound" if bound else "sampled", Q, F,
                                         pad_overflows=zero_keys)
                    routes = [sc.model_route(m, k, C=cap)
                              for m in bc.c_models(cases, desc, k, bound, zero_keys)]
                    _C_REFS[key] = (q, oracle.search_c(bc.C_DOCS, ip, ix, dt, q, k, threads=8),
                                    routes)
                q, ref, routes = _C_REFS[key]
                assert routes.count("fallback") == F
                want_block = sum(r in sc.BLOCK_MERGE_ROUTES for r in routes)
                index = _idx(ip, ix, dt, bc.C_DOCS, segments=segments,
                             options={"list_cap": cap, "theta_bound": tb, "flat": flat})
                got = index.search(q, k)
                d, st = index.last_dispatch(), index.search_stats()
                what = (segments, Q, F, tb, flat, d, st)
                print(f"  C {segments} Q={Q} F={F} theta_bound={tb} flat={flat}: "
                      f"fallback_queries={st['fallback_queries']} block_merge_queries="
                      f"{st['block_merge_queries']} (mirror {want_block})", flush=True)
                index.close()
                _exact(got, ref)
                assert d["sample_p"] == (0 if bound else bc.C_SAMPLE_P), what
                assert ("flat_rest" in d["kernels"]) == bool(flat), what
                assert st["fallback_queries"] == F, what
                assert st["block_merge_queries"] == want_block, what
    print(f"  C {segments}: {time.perf_counter() - t0:.2f} s", flush=True)


@pytest.mark.parametrize("segments", ["dense", "sparse"])
def test_filtered_fallback_row_count(gpu, segments):
    """search_filtered under list_cap = 256: 65 of 130 rows receive 257 keys
    (or, the all-padding row, every document) and take the dense path on their
    own; the others' lists fill to the last key."""
    (ip, ix, dt), _ = bc.cf_index()
    q, qm, allow = bc.cf_batch(), bc.cf_query_mask(), bc.cf_masks()
    rows = [oracle.scores_dense_c(bc.CF_DOCS, ip, ix, dt, r) for r in q]
    want = filtered_want(rows, bc.C_K, allow, qm)
    index = _idx(ip, ix, dt, bc.CF_DOCS, segments=segments, options={"list_cap": bc.C_CAP})
    got = index.search_filtered(q, bc.C_K, _pack(allow), qm)
    _exact(got, want)
    assert "filtered" in index.last_dispatch()["kernels"]
    assert index.filtered_stats()[0] == bc.CF_F
    _exact(index.search_filtered(q, bc.C_K, _pack(allow), qm), want)   # the same handle again
    assert index.filtered_stats()[0] == bc.CF_F
    index.close()


# ============================================================== D. Q = 0
def test_empty_batch_on_every_entry_point(small_world):
    """Q = 0 (M = 0 for the mask builders): every host call returns empty
    arrays, every device call leaves its pre-filled outputs alone; the handle
    then searches as before."""
    import torch
    from bm25mi.index import merge_sorted_device, merge_topk_device
    w = small_world
    n, T, k, W = w.n, bc.B_T, 10, (w.n + 31) // 32
    index = _idx(*w.csc, n, segments="dense")
    packed = _pack(w.allow)
    groups = (np.arange(n) % 5).astype(np.int32)
    values = (np.arange(n) % 97).astype(np.int32)
    q0 = np.zeros((0, T), np.int32)
    e1, e2 = np.zeros((0, 1), np.int32), np.zeros((0, 2), np.int32)
    f0, i0 = np.zeros(0, np.float32), np.zeros(0, np.int32)

    def empty(res, *shapes):
        res = res if isinstance(res, tuple) else (res,)
        assert tuple(r.shape for r in res) == shapes, (tuple(r.shape for r in res), shapes)

    empty(index.search(q0, k), (0, k), (0, k))
    empty(index.search(q0, bc.B_BIG_K), (0, bc.B_BIG_K), (0, bc.B_BIG_K))
    empty(index.search_filtered(q0, k, packed, i0), (0, k), (0, k))
    empty(index.search_weighted(q0, np.zeros((0, T), np.float32), k), (0, k), (0, k))
    empty(index.search_after(q0, k, (f0, i0)), (0, k), (0, k))
    empty(index.search_boolean(q0, k, e1, e2, e1, total_hits=True, facets=(groups, 5)),
          (0, k), (0, k), (0,), (0, 5))
    empty(index.score_docs(q0, np.zeros((0, 3), np.int32)), (0, 3))
    empty(index.term_masks(e1, e2, e1), (0, W))
    empty(index.range_masks(values, None, i0, i0), (0, W))
    empty(index.mask_count(np.zeros((0, W), np.uint32)), (0,))
    empty(index.facets(np.zeros((0, W), np.uint32), groups, 5), (0, 5))

    # the device calls: zero-row views of pre-filled buffers
    gd = torch.full((4, k), BAD_DOC, dtype=torch.int32, device="cuda")
    gs = torch.full((4, k), BAD_SCORE, dtype=torch.float32, device="cuda")
    gw = torch.full((4, W), BAD_WORD, dtype=torch.int32, device="cuda")
    gl = torch.full((4, 5), BAD_DOC, dtype=torch.int64, device="cuda")
    gk = torch.full((2, 4, 64), BAD_DOC, dtype=torch.int64, device="cuda")
    g3 = torch.full((4, 3), BAD_SCORE, dtype=torch.float32, device="cuda")
    dq = torch.zeros((4, T), dtype=torch.int32, device="cuda")[:0]
    dw = torch.ones((4, T), dtype=torch.float32, device="cuda")[:0]
    dm = torch.from_numpy(packed.view(np.int32)).cuda()
    dqm = torch.zeros(4, dtype=torch.int32, device="cuda")[:0]
    dc1 = torch.zeros((4, 1), dtype=torch.int32, device="cuda")[:0]
    dgroups = torch.from_numpy(groups).cuda()
    dvalues = torch.from_numpy(values).cuda()
    daf = (torch.zeros(4, dtype=torch.float32, device="cuda")[:0],
           torch.zeros(4, dtype=torch.int32, device="cuda")[:0])
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    index.search_device(dq, k, gd[:0], gs[:0], st)
    index.search_filtered_device(dq, k, dm, dqm, gd[:0], gs[:0], st)
    index.search_weighted_device(dq, dw, k, dm, dqm, gd[:0], gs[:0], st)
    index.search_after_device(dq, k, daf, None, None, None, gd[:0], gs[:0], st)
    index.score_docs_device(dq, torch.zeros((4, 3), dtype=torch.int32, device="cuda")[:0],
                            g3[:0], st)
    index.term_masks_device(dc1, dc1, dc1, None, gw[:0], st)
    index.range_masks_device(dvalues, dc1, dc1, dc1, gw[:0], None, st)
    index.mask_count_device(gw[:0], gl[:0, 0].contiguous(), st)
    index.facets_device(gw[:0], dgroups, 5, gl[:0], st)
    merge_topk_device(0, gd[:0], gs[:0], 2, 0, k, gd[:0], gs[:0], st)
    merge_sorted_device(0, gd[:0], gs[:0], 2, 0, k, 0, gd[:0], gs[:0], st)
    index.search_sample_device(dq, k, 2, n, gk[0, :0], st)
    index.search_finish_device(dq, k, 2, n, gk[:, :0], gd[:0], gs[:0], st)
    st.synchronize()
    torch.cuda.synchronize()
    assert (gd == BAD_DOC).all() and (gs == BAD_SCORE).all() and (g3 == BAD_SCORE).all()
    assert (gw == BAD_WORD).all() and (gl == BAD_DOC).all() and (gk == BAD_DOC).all()

    rows = np.arange(70) % bc.B_POOL
    _exact(index.search(w.pool[rows], k), _take(w.plain(k), rows))
    _exact(index.search_filtered(w.pool[rows], k, packed, bc.b_query_mask(70)),
           _take(w.filtered(k), bc.b_combo(70)))
    index.close()
