"""The case plans of the query-batch tests (tests/test_gpu_batch.py) and the
host arithmetic they rest on — a plain helper module, no fixtures and no
tests.  tests/test_batch_model.py checks on the CPU that the plans hit the
edges they are meant to hit.

A  few flat items: the eight XCD ranges of score_flat_kernel and its claims
B  Q at 65 535, 65 536, 65 537: rows of a 257-row pool, row i = pool[i % 257]
C  the exact fallback stage's own row count: lists of cap / cap + 1 keys
"""
import numpy as np

import select_cases as sc

TILE = 2048


def quarter_index(rng, n_docs, V, df_lo, df_hi, signed=False):
    """A CSC of V terms with df_lo..df_hi postings each (at most n_docs),
    values in quarter steps (0.25 .. 3.0, or -2.0 .. 3.0 without 0): ties at
    every threshold."""
    ip, ix, dt = [0], [], []
    for _ in range(V):
        df = min(n_docs, int(rng.integers(df_lo, df_hi + 1)))
        ix.append(np.sort(rng.choice(n_docs, df, replace=False)).astype(np.int32))
        v = rng.integers(-8 if signed else 1, 13, df)
        v[v == 0] = 1
        dt.append((v / 4).astype(np.float32))
        ip.append(ip[-1] + df)
    return np.array(ip, np.int64), np.concatenate(ix), np.concatenate(dt)


def query_rows(rng, n, T, V):
    """n query rows of T slots: random terms with some padding slots; row 0
    repeats a term and ends in padding, rows 2 and 7 (where they exist) are
    all padding, row 5 repeats one term in every slot."""
    q = rng.integers(0, V, size=(n, T)).astype(np.int32)
    q[rng.random((n, T)) < 0.15] = -1
    q[0, 0] = q[0, 1] = 3
    q[0, T - 1] = -1
    for r in (2, 7):
        if r < n:
            q[r] = -1
    if n > 5:
        q[5] = 11
    return q


# ------------------------------------------------------------- A. few items
def ranges(nitems):
    """The eight ngi of score_flat_kernel: the items of each XCD range."""
    per = (nitems + 7) >> 3
    return [max(0, min(nitems, grp * per + per) - grp * per) for grp in range(8)]


def claims(ngi, claim_ch):
    """Claims that find an item in a range of ngi items."""
    return -(-ngi // claim_ch)


A_V = 200
A_ROWS = 129
A_QS = tuple(range(1, 18)) + (31, 32, 33, 63, 64, 65, 127, 128, 129)
A_CLAIM_CH = (1, 3, 64)
A_CLAIM_M = (1, 3, 8)   # (3 does not divide a full grid's rounds: sharers differ per counter)
A_GRID_PCT = (1, 100)
A_TS = (3, 8)
A_KS = (1, 10)
# (name, tiles, segment table, flat_bw)
A_INDICES = (("t1", 1, "dense", 1), ("t2", 2, "dense", 1), ("t9", 9, "dense", 1),
             ("t9-sparse", 9, "sparse", 1), ("t40", 40, "dense", 1), ("t9-bw8", 9, "dense", 8))


def a_docs(tiles):
    return tiles * TILE - 37  # a partial last tile


def a_index(tiles):
    return quarter_index(np.random.default_rng(900 + tiles), a_docs(tiles), A_V, 200, 400)


def a_queries(T):
    """The fixed 129-row matrix of width T: a batch is its first Q rows."""
    return query_rows(np.random.default_rng(77 + T), A_ROWS, T, A_V)


def a_routes(tiles):
    """The option sets (beside flat_bw) that select each threshold route:
    the exact ALL pass on every index; from 4 tiles on sample_p = 2 samples
    every second tile, with theta_bound 1 (the tile-bound keys where the
    index has 16 k tiles: the 40-tile index at k = 1) and 0."""
    out = [{"sample_p": 1, "theta_bound": 1}]
    if tiles >= 4:
        out += [{"sample_p": 2, "theta_bound": 1}, {"sample_p": 2, "theta_bound": 0}]
    return out


def a_items(tiles, Q, bw=1):
    """Items of the ALL pass: bands of bw tiles x queries."""
    return -(-tiles // bw) * Q


def a_plan():
    """(tiles, Q, nitems) of every planned ALL-pass launch at flat_bw = 1."""
    return [(t, Q, a_items(t, Q)) for _, t, _, bw in A_INDICES if bw == 1 for Q in A_QS]


# ------------------------------------------------------------ B. Q past 2^16
B_POOL = 257
B_QS = (65535, 65536, 65537)
B_T = 4
B_V = 200
B_TILES = 16                       # >= 16 k at k = 1: the tile-bound threshold
B_DOCS = B_TILES * TILE - 5
B_KS = (1, 10)
B_SMALL_DOCS = 4097                # 3 tiles; k = 4097 = n_docs
B_BIG_K = 4097
B_BIG_LIST_CAP = 64                # the k = 4097 filtered / cursor handle (see b_bytes)
B_SEAM = (65534, 65535, 65536)
B_MASKS = 3
B_MEM_CAP = 4 << 30


def b_rows(Q):
    """The pool row of every batch row."""
    return np.arange(Q) % B_POOL


def b_index(small=False):
    n = B_SMALL_DOCS if small else B_DOCS
    return quarter_index(np.random.default_rng(31 if small else 32), n, B_V, 200, 400)


def b_pool():
    return query_rows(np.random.default_rng(5), B_POOL, B_T, B_V)


def b_weights():
    """Signed quarter-step weights of the pool rows (none 0)."""
    w = np.random.default_rng(6).integers(-6, 9, (B_POOL, B_T))
    w[w == 0] = 2
    return (w / 4).astype(np.float32)


def b_masks(n_docs):
    """Three allow-masks: about half, a tenth, and every document but a few."""
    rng = np.random.default_rng(8)
    return np.stack([rng.random(n_docs) < 0.5, rng.random(n_docs) < 0.1,
                     rng.random(n_docs) < 0.98])


def b_query_mask(Q):
    """Mask ids cycling 0, 1, 2, -1 down the batch."""
    return ((np.arange(Q) % 4 + 1) % 4 - 1).astype(np.int32)


def b_combo(Q):
    """(pool row, mask id) of a batch row as one index into the 257 x 4
    reference rows (257 and 4 are coprime: every pair occurs)."""
    return b_rows(Q) * 4 + np.arange(Q) % 4


def b_clauses():
    """Clause rows of the pool for search_boolean: must of 0..1 terms, any of
    0..2, must_not of 0..1; some rows without any clause."""
    rng = np.random.default_rng(9)
    mu = np.where(rng.random((B_POOL, 1)) < 0.4, rng.integers(0, B_V, (B_POOL, 1)), -1)
    an = np.where(rng.random((B_POOL, 2)) < 0.6, rng.integers(0, B_V, (B_POOL, 2)), -1)
    mn = np.where(rng.random((B_POOL, 1)) < 0.5, rng.integers(0, B_V, (B_POOL, 1)), -1)
    return mu.astype(np.int32), an.astype(np.int32), mn.astype(np.int32)


def b_score_docs(n_docs):
    """Candidates [257, 3] for score_docs: random documents, some padding."""
    rng = np.random.default_rng(10)
    d = rng.integers(0, n_docs, (B_POOL, 3)).astype(np.int32)
    d[rng.random(d.shape) < 0.1] = -1
    return d


def list_cap_auto(k):
    """list_cap_for (csrc/bm25mi_capi.cpp) without the list_cap option."""
    return min(65536, max(2048, 64 * k))


def b_bytes(Q, tiles, k, list_cap=0, ws_k=None):
    """Device bytes of a case by the workspace arithmetic: 32 B per (query,
    tile), 8 list_cap B per query (automatic: by the k the workspace was built
    for, ws_k), 8 Q k B of outputs.  The dense rows of the k > 4096 paths come
    on top, bounded by the library's own scratch budget (at most 4 GiB)."""
    cap = list_cap or list_cap_auto(k if ws_k is None else ws_k)
    return 32 * Q * tiles + 8 * cap * Q + 8 * Q * k


def b_plan():
    """(what, Q, tiles, k, list_cap, ws_k) of every case of section B."""
    out = []
    for Q in B_QS:
        for k in B_KS:
            out.append(("search", Q, B_TILES, k, 0, None))
        out.append(("shards", Q, B_TILES // 2, max(B_KS), 0, None))
    Q = B_QS[-1]
    small_tiles = -(-B_SMALL_DOCS // TILE)
    # the plain large-k search builds its workspace with k = 1
    out.append(("large_lists", Q, small_tiles, B_BIG_K, 0, 1))
    # the filtered and cursor searches build theirs with k = 4096: list_cap pinned
    out.append(("filtered", Q, small_tiles, B_BIG_K, B_BIG_LIST_CAP, None))
    out.append(("after", Q, small_tiles, B_BIG_K, B_BIG_LIST_CAP, None))
    out.append(("filtered-dense-k10", Q, small_tiles, 10, 0, None))
    return out


# --------------------------------------------- C. fallback-stage row counts
C_K = 10
C_CAP = 256
C_TILES = 160                      # >= 16 k: the tile-bound threshold serves k = 10
C_DOCS = C_TILES * TILE - 300
C_SAMPLE_P = 8                     # sample_geom(160 tiles, k = 10): P = 8, m = 1, G = 1
C_Q = 130
C_BATCHES = ((130, 0), (130, 1), (130, 63), (130, 64), (130, 65), (130, 129), (130, 130),
             (1, 1), (64, 64))     # (Q, F)


def sample_geom(ntiles, k, pmax=8):
    """sample_geom of csrc/bm25mi_kernels.hip for one index: (P, m, G)."""
    P = 64
    while P >= 2:
        if P <= pmax and ntiles >= 2 * P:
            G = 8 if ntiles >= 4 * 8 * P else 1
            r = ntiles % (G * P)
            nS = (ntiles // (G * P)) * G + min(r, G)
            for m in (1, 2, 4):
                if nS * m >= 2 * k:
                    return P, m, G
        P >>= 1
    return 1, 0, 1


def bound_model(docs, vals, k, mult=1, ntiles=C_TILES):
    """select_cases.row_model for a query that names the term mult times: the
    tile-bound threshold is the k-th largest of the tiles' bounds of the term
    (bound_keys_kernel takes the maximum over the query's slots, not their
    sum), the list holds the documents whose score — mult times the value —
    reaches it (every positive one under the zero-fill threshold)."""
    lb = np.sort(sc.tile_bounds(docs, vals, ntiles))[::-1]
    vk = lb[k - 1] if k <= len(lb) else np.float32(0)
    zf = not vk > 0
    s = np.float32(mult) * vals
    s = np.sort(s[s > 0] if zf else s[s >= vk])[::-1]
    kth = s[k - 1] if len(s) >= k else None
    return {"cnt": len(s), "zero_fill": zf,
            "ties_at_kth": 0 if kth is None else int((s == kth).sum()),
            "above_kth": len(s) if kth is None else int((s > kth).sum())}


def sample_keys(docs, vals, zero_keys, ntiles=C_TILES, P=C_SAMPLE_P, n_docs=C_DOCS):
    """The sample keys of a single-term query, best first, as (score, doc):
    the best document (score descending, doc ascending) of every P-th tile
    that holds a positive score.  zero_keys (score_wave_kernel's select_top):
    a sample tile without one reports its first document, score 0; the flat
    kernel reports no key for it."""
    docs = np.asarray(docs, np.int64)
    keys = []
    for t in range(0, ntiles, P):
        m = (docs // TILE == t) & (vals > 0)
        if m.any():
            best = vals[m].max()
            keys.append((float(best), int(docs[m][vals[m] == best].min())))
        elif zero_keys and t * TILE < n_docs:
            keys.append((0.0, t * TILE))
    return sorted(keys, key=lambda x: (-x[0], x[1]))


def sampled_model(docs, vals, k, zero_keys=False):
    """row_model of select_cases under the sampled threshold of a single-term
    query (theta_wave_kernel): theta is the k-th best sample key, the list
    holds every document at or above it (a key of the same score: up to its
    document); with fewer than k sample keys the zero-fill threshold lists
    every positive document.  A theta of score 0 (zero_keys) lists the
    documents without a posting up to its own as well."""
    docs = np.asarray(docs, np.int64)
    keys = sample_keys(docs, vals, zero_keys)
    pos = vals > 0
    zf = len(keys) < k
    if zf:
        s = vals[pos]
    else:
        ts, td = keys[k - 1]
        if ts == 0.0:   # every positive document, and the zero scores up to document td
            n = int(pos.sum()) + td + 1 - int((docs <= td).sum())
            return {"cnt": n, "zero_fill": False, "ties_at_kth": n, "above_kth": 0}
        s = vals[(vals > ts) | ((vals == ts) & (docs <= td))]
    s = np.sort(s)[::-1]
    kth = s[k - 1] if len(s) >= k else None
    return {"cnt": len(s), "zero_fill": zf,
            "ties_at_kth": 0 if kth is None else int((s == kth).sum()),
            "above_kth": len(s) if kth is None else int((s > kth).sum())}


def sampled_term(rng, n_hi):
    """Postings whose list under the sampled threshold holds n_hi + 12 keys
    whichever score kernel samples: ten sample tiles (of the first 16) hold one
    document of 2.0 each — the ten best sample keys, theta = (2.0, the last of
    them) —, non-sample tiles hold n_hi documents of 3.0, two of 2.0 before
    theta's document (listed) and two after it (the tie rule keeps them out),
    and documents of 1.0 lie in tiles of every kind."""
    st = np.arange(0, C_TILES, C_SAMPLE_P)
    non = np.setdiff1d(np.arange(C_TILES - 1), st)
    two_t = np.sort(rng.choice(st[:16], 10, replace=False))
    two = two_t * TILE + rng.integers(0, TILE, 10)
    hi_t = rng.choice(non, 12, replace=False)
    hi = np.unique(rng.choice(hi_t, n_hi + 40) * TILE + rng.integers(0, TILE, n_hi + 40))
    hi = rng.permutation(hi)[:n_hi]
    assert len(hi) == n_hi
    rest_t = np.setdiff1d(non, hi_t)
    before = rest_t[rest_t < two_t[-1]]
    after = rest_t[rest_t > st[16]]
    ties = np.r_[rng.choice(before, 2, replace=False), rng.choice(after, 2, replace=False)] * TILE \
        + rng.integers(0, TILE, 4)
    low_t = np.r_[rng.choice(np.setdiff1d(rest_t, ties // TILE), 30, replace=False),
                  np.setdiff1d(st, two_t)[:3]]
    low = low_t * TILE + rng.integers(0, TILE, len(low_t))
    docs = np.r_[two, hi, ties, low]
    vals = np.r_[np.full(10, 2.0), np.full(n_hi, 3.0), np.full(4, 2.0), np.full(len(low), 1.0)]
    o = np.argsort(docs)
    assert np.all(np.diff(docs[o]) > 0)
    return docs[o].astype(np.int32), vals[o].astype(np.float32)


def c_pools():
    """Terms per threshold source.  "bound": C_Q pairs (exact, over) of
    select_cases terms whose lists hold C_CAP / C_CAP + 1 keys under the
    tile-bound threshold; "sampled": C_Q pairs of sampled_term postings with
    those lengths under the sampled threshold; "bound_dup" / "sampled_dup":
    one term each whose list stays short when a row names it twice.
    Returns (cases, pools)."""
    cases, pools = [], {"bound": [], "sampled": []}

    def keep(c, postings=None):
        c.term = len(cases)
        c.docs, c.vals = postings if postings else sc.case_postings(c, C_TILES, C_DOCS)
        cases.append(c)
        return c.term

    for i in range(C_Q):
        p = sc.PATTERNS[i % len(sc.PATTERNS)]
        pools["bound"].append(tuple(keep(sc.Case(C_K, cnt, p, None, seed=4000 + 2 * i + j))
                                    for j, cnt in enumerate((C_CAP, C_CAP + 1))))
    pools["bound_dup"] = keep(sc.Case(C_K, 100, "e", None, seed=3999))
    rng = np.random.default_rng(4500)
    for i in range(C_Q):
        pools["sampled"].append(tuple(
            keep(sc.Case(C_K, cnt, "s"), sampled_term(rng, cnt - 12)) for cnt in (C_CAP, C_CAP + 1)))
    pools["sampled_dup"] = keep(sc.Case(C_K, 100, "s"), sampled_term(rng, 88))
    return cases, pools


def c_over_rows(Q, F):
    """The F overflowing rows of a Q-row batch, spread through it."""
    return set() if F == 0 else {(j * Q) // F + (Q - 1) // F // 2 for j in range(F)} \
        if F < Q else set(range(Q))


def c_batch(pools, mode, Q, F, pad_overflows=False, T=4):
    """A batch of Q rows of which F overflow their list.  Row r asks for the
    over term of pair r where it is to overflow, else for the exact term.  One
    row is all padding: its list is empty, so it takes the place of the last
    row that does not overflow (none where F = Q) — or, pad_overflows (the wave
    kernel's sampled threshold lists zero scores for it), of the last row that
    does (none where F = 0).  One row names its term twice: the mode's dup term
    on the first row that is not to overflow, else the over term of row 0.
    Returns (queries, [(term, times) or None per row])."""
    pool = pools[mode]
    over = c_over_rows(Q, F)
    assert len(over) == F and all(0 <= r < Q for r in over)
    fits = [r for r in range(Q) if r not in over]
    pad_row = -1
    if pad_overflows:
        pad_row = max(over) if over and Q > 1 else -1
    elif fits:
        pad_row = fits[-1]
    dup_row = next((r for r in fits if r != pad_row), min(r for r in range(Q) if r != pad_row))
    q = np.full((Q, T), -1, np.int32)
    desc = []
    for r in range(Q):
        if r == pad_row:
            desc.append(None)
            continue
        term = pool[r][1 if r in over else 0]
        if r == dup_row:
            if r not in over:
                term = pools[mode + "_dup"]
            q[r, 2] = term
        q[r, 0] = term
        desc.append((term, 2 if r == dup_row else 1))
    return q, desc


def c_models(cases, desc, k, bound, zero_keys):
    """The list model of every row of a c_batch."""
    empty = (np.zeros(0, np.int32), np.zeros(0, np.float32))
    out = []
    for d in desc:
        docs, vals = empty if d is None else (cases[d[0]].docs, cases[d[0]].vals)
        mult = 1 if d is None else d[1]
        out.append(bound_model(docs, vals, k, mult) if bound
                   else sampled_model(docs, np.float32(mult) * vals, k, zero_keys))
    return out


# the filtered search's own fallback: lists by the filter passes' rule
CF_TILES = 12
CF_DOCS = CF_TILES * TILE - 100
CF_Q, CF_F = 130, 65


def filtered_list_count(order, k):
    """Keys the filtered search's list receives (bm25mi_filter.hip): the
    allowed documents, in result order, down to the k-th of the tiles' best
    four keys — all of them when fewer than k such keys exist."""
    tile = np.asarray(order, np.int64) // TILE
    rank = np.zeros(len(tile), np.int64)
    seen = {}
    for i, t in enumerate(tile.tolist()):
        rank[i] = seen.get(t, 0)
        seen[t] = rank[i] + 1
    cand = np.nonzero(rank < 4)[0]
    return int(cand[k - 1]) + 1 if len(cand) >= k else len(tile)


def cf_index():
    """CF_Q terms: n documents of value 2.0 in tiles 1 and 2 (eight of the
    tiles' best-four keys), then 20 of value 1.0, one per tile and twice over:
    the 9th and 10th such keys are the first two of those, so the list holds
    n + 2 keys — n = C_CAP - 2 (it fits) or C_CAP - 1 (one too many)."""
    rng = np.random.default_rng(12)
    ip, ix, dt, over = [0], [], [], []
    for t in range(CF_Q):
        big = t % 2 == 1
        n = C_CAP - 2 + big
        hi = np.sort(rng.choice(np.arange(TILE, 3 * TILE), n, replace=False))
        assert (hi < 2 * TILE).any() and (hi >= 2 * TILE).any()
        lo_t = np.r_[0, np.arange(3, CF_TILES)]
        lo = np.sort(np.r_[lo_t * TILE + rng.integers(0, TILE - 200, len(lo_t)),
                           lo_t * TILE + TILE - 150 + rng.integers(0, 50, len(lo_t))])
        ix.append(np.r_[lo[lo < TILE], hi, lo[lo >= TILE]].astype(np.int32))
        dt.append(np.where(np.isin(ix[-1], hi), 2.0, 1.0).astype(np.float32))
        assert np.all(np.diff(ix[-1]) > 0)
        ip.append(ip[-1] + len(ix[-1]))
        over.append(big)
    return (np.array(ip, np.int64), np.concatenate(ix), np.concatenate(dt)), np.array(over)


def cf_batch(T=4):
    """Row r asks for term r; row 0 repeats it, the last row (an odd one: its
    term would overflow) is all padding — without a filter every document is a
    zero-score result of it, and its list overflows as well."""
    q = np.full((CF_Q, T), -1, np.int32)
    q[:, 0] = np.arange(CF_Q)
    q[0, 2] = 0
    q[CF_Q - 1] = -1
    return q


def cf_masks():
    """Two masks that leave tiles 0..5 alone (the lists' documents lie in
    0..2): every document, and none past tile 5."""
    m = np.ones((2, CF_DOCS), bool)
    m[1, 6 * TILE:] = False
    return m


def cf_query_mask():
    return (np.arange(CF_Q) % 3 - 1).astype(np.int32)   # -1, 0, 1, ...
