"""The case plans of tests/batch_cases.py hit the edges tests/test_gpu_batch.py
is there for (CPU only): the flat kernel's XCD ranges and claims, the memory
cap of the Q >= 2^16 cases, the list lengths of the fallback-stage batches.
A later edit of a plan that moves it off an edge fails here."""
import numpy as np

import batch_cases as bc
import select_cases as sc
from test_search_after_host import ordered


# ------------------------------------------------------------- A. few items
def test_ranges_partition_the_items():
    for n in range(5001):
        r = bc.ranges(n)
        assert len(r) == 8 and sum(r) == n and min(r) >= 0, n
        per = (n + 7) >> 3
        # full ranges, then one shorter, then empty ones
        assert all(x == per for x in r[:n // per if per else 0]), n
        assert sorted(r, reverse=True) == r, n


def _plan_ranges():
    return [(t, Q, n, bc.ranges(n)) for t, Q, n in bc.a_plan()]


def test_plan_has_fewer_items_than_ranges():
    few = [(t, Q, n, r) for t, Q, n, r in _plan_ranges() if n < 8]
    assert few and all(r.count(0) == 8 - n for _, _, n, r in few)
    assert {n for _, _, n, _ in few} == set(range(1, 8))       # 1 tile, Q = 1..7


def test_plan_has_eight_and_nine_items():
    by_n = {}
    for t, Q, n, r in _plan_ranges():
        by_n.setdefault(n, []).append((t, Q, r))
    assert all(r == [1] * 8 for _, _, r in by_n[8])
    assert {(t, Q) for t, Q, _ in by_n[8]} >= {(1, 8), (2, 4)}
    assert {(t, Q) for t, Q, _ in by_n[9]} >= {(1, 9), (9, 1)}
    assert all(r == [2, 2, 2, 2, 1, 0, 0, 0] for _, _, r in by_n[9])  # per = 2: 5..7 empty
    # a range of exactly one item beside longer ones
    assert any(1 in r and max(r) > 1 for _, _, _, r in _plan_ranges())


def test_plan_has_the_claim_edges():
    rs = [r for _, _, _, r in _plan_ranges()]
    for ch in bc.A_CLAIM_CH:
        if ch > 1:
            assert any(0 < x < ch for r in rs for x in r), ch            # shorter than a claim
            assert any(x > ch and x % ch == 1 for r in rs for x in r), ch  # ch * m + 1
        assert any(x % ch == 0 and x >= ch for r in rs for x in r), ch     # whole claims
    cm = max(bc.A_CLAIM_M)
    for ch in bc.A_CLAIM_CH:  # fewer claims than counters: some counter's first claim is past the end
        assert any(0 < bc.claims(x, ch) < cm for r in rs for x in r), ch
    # a range whose length is no multiple of claim_ch, for every claim_ch > 1
    assert all(any(x % ch for r in rs for x in r) for ch in bc.A_CLAIM_CH if ch > 1)
    # 40 tiles x 13 queries: eight ranges of 65 = 64 + 1 items
    assert bc.ranges(bc.a_items(40, 13)) == [65] * 8


def test_plan_sweeps_what_the_issue_lists():
    assert set(bc.A_QS) == set(range(1, 18)) | {31, 32, 33, 63, 64, 65, 127, 128, 129}
    assert max(bc.A_QS) == bc.A_ROWS
    assert set(bc.A_CLAIM_CH) == {1, 3, 64} and set(bc.A_CLAIM_M) >= {1, 8}
    assert set(bc.A_GRID_PCT) == {1, 100} and set(bc.A_TS) == {3, 8} and set(bc.A_KS) == {1, 10}
    assert [t for _, t, _, _ in bc.A_INDICES] == [1, 2, 9, 9, 40, 9]
    assert [bw for *_, bw in bc.A_INDICES] == [1, 1, 1, 1, 1, 8]
    assert {s for _, _, s, _ in bc.A_INDICES} == {"dense", "sparse"}
    # flat_bw = 8 on 9 tiles: two bands, the second of one tile
    assert bc.a_items(9, 5, 8) == 2 * 5
    assert [len(bc.a_routes(t)) for t in (1, 2, 9, 40)] == [1, 1, 3, 3]
    for T in bc.A_TS:
        q = bc.a_queries(T)
        assert q.shape == (bc.A_ROWS, T) and q.max() < bc.A_V
        assert (q[2] == -1).all() and (q[7] == -1).all() and q[0, 0] == q[0, 1] >= 0
        assert q[0, -1] == -1 and len(set(q[5])) == 1
    ip, ix, dt = bc.a_index(9)
    assert len(ip) == bc.A_V + 1 and 200 <= np.diff(ip).min() and np.diff(ip).max() <= 400
    assert np.array_equal(dt * 4, np.round(dt * 4)) and dt.min() > 0     # quarter steps
    assert -(-bc.a_docs(9) // bc.TILE) == 9 and bc.a_docs(9) % bc.TILE


# ------------------------------------------------------------ B. Q past 2^16
def test_pool_rows_expose_a_16_bit_row_index():
    assert bc.B_QS == (65535, 65536, 65537)
    assert 65536 % bc.B_POOL == 1
    pool = bc.b_pool()
    assert pool.shape == (bc.B_POOL, bc.B_T)
    # rows i and i mod 2^16 ask for different queries
    rows = bc.b_rows(65537)
    assert rows[65536] != rows[0] and not np.array_equal(pool[rows[65536]], pool[rows[0]])
    assert len({tuple(r) for r in pool.tolist()}) > 250      # (nearly) all distinct
    assert (pool[2] == -1).all() and pool[0, 0] == pool[0, 1]
    qm = bc.b_query_mask(8)
    assert qm.tolist() == [0, 1, 2, -1, 0, 1, 2, -1]
    combo = bc.b_combo(65537)
    assert len(set(combo.tolist())) == 4 * bc.B_POOL and combo.max() == 4 * bc.B_POOL - 1
    assert np.array_equal(combo % 4 == 3, bc.b_query_mask(65537) == -1)


def test_large_q_cases_stay_under_the_memory_cap():
    plan = bc.b_plan()
    assert {p[0] for p in plan} >= {"search", "shards", "large_lists", "filtered", "after"}
    for what, Q, tiles, k, cap, ws_k in plan:
        b = bc.b_bytes(Q, tiles, k, cap, ws_k)
        assert b < bc.B_MEM_CAP, (what, Q, k, b)
    # the default list of a k <= 32 search: 2048 keys a query, about 1.1 GB at Q = 65 537
    assert bc.list_cap_auto(10) == 2048
    assert 1.0e9 < bc.b_bytes(65537, bc.B_TILES, 10) < 1.2e9
    # the filtered search builds its workspace for k = 4096: without list_cap its lists
    # alone would pass the cap
    assert 8 * bc.list_cap_auto(4096) * 65537 > bc.B_MEM_CAP
    assert bc.B_TILES >= 16 * min(bc.B_KS) and -(-bc.B_DOCS // bc.TILE) == bc.B_TILES
    assert bc.B_SMALL_DOCS >= bc.B_BIG_K > 4096 and -(-bc.B_SMALL_DOCS // bc.TILE) == 3


# --------------------------------------------- C. fallback-stage row counts
_POOLS = None


def _pools():
    global _POOLS
    if _POOLS is None:
        _POOLS = bc.c_pools()
    return _POOLS


def test_fallback_pools_have_lists_of_cap_and_cap_plus_one():
    cases, pools = _pools()
    k, cap = bc.C_K, bc.C_CAP
    assert bc.C_TILES >= 16 * k
    assert bc.sample_geom(bc.C_TILES, k) == (bc.C_SAMPLE_P, 1, 1)
    assert len(pools["bound"]) == len(pools["sampled"]) == bc.C_Q
    for exact, over in pools["bound"]:
        for t, want in ((exact, cap), (over, cap + 1)):
            c = cases[t]
            m = bc.bound_model(c.docs, c.vals, k)
            ref = sc.row_model(c.docs, c.vals, k, bc.C_TILES)
            assert m == {f: ref[f] for f in m} and m["cnt"] == want, (t, m)
            assert sc.row_model(c.docs, c.vals, k, bc.C_TILES, pool=True)["cnt"] == want
            assert not m["zero_fill"]
            # named twice, the scores double and the threshold does not: the noise lists too
            assert bc.bound_model(c.docs, c.vals, k, 2)["cnt"] > cap
    for exact, over in pools["sampled"]:
        for t, want in ((exact, cap), (over, cap + 1)):
            c = cases[t]
            # k positive sample keys: both score kernels sample the same theta
            assert sum(s > 0 for s, _ in bc.sample_keys(c.docs, c.vals, True)) >= k
            for zero_keys in (False, True):
                m = bc.sampled_model(c.docs, c.vals, k, zero_keys)
                assert m["cnt"] == want and not m["zero_fill"], (t, m)
                assert bc.sampled_model(c.docs, 2 * c.vals, k, zero_keys)["cnt"] == want
            tie = c.vals == 2.0    # ties at theta's score on both sides of its document
            assert tie.sum() == 14
    c = cases[pools["bound_dup"]]
    assert k <= bc.bound_model(c.docs, c.vals, k, 2)["cnt"] < cap
    c = cases[pools["sampled_dup"]]
    assert {bc.sampled_model(c.docs, 2 * c.vals, k, z)["cnt"] for z in (False, True)} == {100}
    # an all-padding row: an empty list, but under the wave kernel's zero keys a long one
    none = (np.zeros(0, np.int32), np.zeros(0, np.float32))
    assert bc.bound_model(*none, k)["cnt"] == bc.sampled_model(*none, k)["cnt"] == 0
    assert bc.sampled_model(*none, k, True)["cnt"] == 9 * bc.C_SAMPLE_P * bc.TILE + 1 > cap


def test_fallback_batches_spread_their_overflowing_rows():
    cases, pools = _pools()
    k, cap = bc.C_K, bc.C_CAP
    assert {F for Q, F in bc.C_BATCHES if Q == 130} == {0, 1, 63, 64, 65, 129, 130}
    assert (1, 1) in bc.C_BATCHES and (64, 64) in bc.C_BATCHES
    for Q, F in bc.C_BATCHES:
        over = bc.c_over_rows(Q, F)
        assert len(over) == F
        if 0 < F < Q // 2:  # spread: not at the start, none adjacent
            rows = sorted(over)
            assert rows[0] > 0 and all(b - a > 1 for a, b in zip(rows, rows[1:]))
        for mode, zero_keys in (("bound", False), ("sampled", False), ("sampled", True)):
            q, desc = bc.c_batch(pools, mode, Q, F, pad_overflows=zero_keys)
            assert q.shape == (Q, 4) and len(desc) == Q
            models = bc.c_models(cases, desc, k, mode == "bound", zero_keys)
            got = {r for r, m in enumerate(models) if m["cnt"] > cap}
            assert len(got) == F, (Q, F, mode, zero_keys)
            if not zero_keys:
                assert got == over
            assert ((q >= 0).sum(axis=1) == 2).sum() == 1            # the duplicated-term row
            pads = ((q >= 0).sum(axis=1) == 0).sum()
            assert pads == ((F > 0 and Q > 1) if zero_keys else (F < Q))


def test_filtered_fallback_batch_overflows_65_lists():
    (ip, ix, dt), over = bc.cf_index()
    q, qm, allow = bc.cf_batch(), bc.cf_query_mask(), bc.cf_masks()
    assert set(qm.tolist()) == {-1, 0, 1}
    counts = []
    for r in range(bc.CF_Q):
        row = np.zeros(bc.CF_DOCS, np.float32)
        for t in q[r][q[r] >= 0]:
            row[ix[ip[t]:ip[t + 1]]] += dt[ip[t]:ip[t + 1]]
        o = ordered(row, None if qm[r] < 0 else allow[qm[r]])
        counts.append(bc.filtered_list_count(o, bc.C_K))
    counts = np.array(counts)
    terms = counts[:-1]
    assert set(terms[~over[:-1]].tolist()) == {bc.C_CAP}          # they fit, to the last key
    assert set(terms[over[:-1]].tolist()) == {bc.C_CAP + 1}       # one key too many
    assert counts[-1] > bc.C_CAP                                  # the all-padding row
    assert int((counts > bc.C_CAP).sum()) == bc.CF_F == 65
