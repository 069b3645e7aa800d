"""Wide indexes with few postings, and a sparse reference for them.

The document axis has limits far beyond what the dense oracle can reach
(oracle.search_c allocates and scans n_docs floats per query): the tile-bound
threshold serves at most 30 720 tiles, an index at most 65 536, a doc id at
most 2^31 - 1.  ``wide_csc`` makes a CSC of about 48 terms and at most about
2 M postings whatever n_docs is, with postings on every position where those
limits bite; ``ref_search`` is the oracle's definition computed over the
touched documents only, with siblings for the term masks, the hit counts and
score_docs.  tests/test_wide_model.py holds them to the C oracle bit for bit
at the widths it reaches; tests/test_gpu_wide.py compares the GPU with them.

A plain helper module: no fixtures, no tests."""
import numpy as np

TILE = 2048
POOL = 4                      # kPool: tiles of a pooled group
BOUND_MAX_TILES = 30_720      # kBoundMaxTiles
MAX_TILES = 65_536
PAD = 0xFFFFFFFF              # score bits of a padding column
AFTER_NONE = -2
INT32_MAX = 2 ** 31 - 1

# the widths of the GPU tests
CAP = BOUND_MAX_TILES * TILE            # last width of the tile-bound threshold
CAP1 = CAP + 1                          # first sampled width: a last tile of one document
C5 = 100_000_000                        # config 5's collection
MAX1 = MAX_TILES * TILE - 1             # the last mask word lacks one bit
MAX = MAX_TILES * TILE                  # tile id 65 535

# the terms of wide_csc
V = 48
N_COMMON = 12                 # terms 0 .. 11: ~150 k postings, values 0.25 .. 1.25
EDGE_LO = 12                  # the edge documents; the first of them score 7.0, the rest 3.0
EDGE_HI = 13                  # the edge documents; the last of them score 7.0, the rest 3.0
RARE0 = 14                    # terms 14 .. 46: 600 .. 1800 postings, values 0.5 .. 9.25
ZFILL = 47                    # 7 postings: fewer than k = 10 (a zero-fill row)
COMMON_DF = 150_000
N_TOP = 4                     # edge documents at the top score of EDGE_LO / EDGE_HI


def n_tiles(n_docs: int) -> int:
    return (n_docs + TILE - 1) // TILE


def edge_docs(n_docs: int) -> np.ndarray:
    """The positions a wide index must carry postings on: document 0 and
    n_docs - 1, the first and last document of tile 0, of tiles 30 719 and
    30 720 (the bound path's cap), of the last two tiles (the last may be
    partial), and of the tiles on both sides of two pooled-group boundaries
    (4g - 1 | 4g) — sorted, unique, those the index has."""
    nt = n_tiles(n_docs)
    g_mid = max(nt // (2 * POOL), 1)
    g_last = max((nt - 1) // POOL, 1)
    tiles = [0, 1, BOUND_MAX_TILES - 1, BOUND_MAX_TILES, nt - 2, nt - 1,
             POOL * g_mid - 1, POOL * g_mid, POOL * g_last - 1, POOL * g_last]
    d = [0, n_docs - 1]
    for t in tiles:
        if 0 <= t < nt:
            d += [t * TILE, min((t + 1) * TILE, n_docs) - 1]
    d = np.unique(np.asarray(d, np.int64))
    return d[(d >= 0) & (d < n_docs)]


def _pick(rng, n_docs: int, df: int) -> np.ndarray:
    """About df distinct documents, sorted."""
    df = min(df, n_docs)
    if n_docs <= 8 * df:
        return np.sort(rng.choice(n_docs, df, replace=False)).astype(np.int64)
    return np.unique(rng.integers(0, n_docs, df))


def _merge(docs, vals, more_docs, more_vals):
    """Column (docs, vals) with (more_docs, more_vals) written over it."""
    keep = ~np.isin(docs, more_docs)
    d = np.concatenate([docs[keep], more_docs])
    v = np.concatenate([vals[keep], more_vals])
    o = np.argsort(d, kind="stable")
    return d[o], v[o]


def wide_csc(n_docs: int, seed: int, signed: bool = False):
    """(indptr int64, indices int32, data float32) of a doc x term CSC with
    V = 48 terms and at most about 2 M postings, in the shape of
    test_gpu_parity._bound_case: N_COMMON common terms of low quarter-step
    values, rare terms of values up to 9.25 (quarter steps: ties).

    Every document of edge_docs holds common term 0 (1.0), EDGE_LO and
    EDGE_HI.  EDGE_LO scores 7.0 on the first N_TOP edge documents (document 0
    among them) and 3.0 on the others; EDGE_HI scores 7.0 on the last N_TOP
    (document n_docs - 1 among them) and 3.0 on the others: a query of either
    term ranks two tie runs by id, one with document 0 and one with document
    n_docs - 1, and the 7.0 run of EDGE_HI ends on the collection's last id.
    ZFILL has 7 postings, document n_docs - 1 among them.

    signed: a third of the values are negative (no tile bounds: the sampled
    path), and term 1 stores some -0.0f."""
    rng = np.random.default_rng(seed)
    edges = edge_docs(n_docs)
    cols = []
    for t in range(V):
        if t < N_COMMON:
            docs = _pick(rng, n_docs, min(COMMON_DF, max(n_docs // 4, 1)))
            vals = (np.round(rng.uniform(0.1, 1.0, len(docs)) * 4) / 4 + 0.25).astype(np.float32)
            if t == 0:
                docs, vals = _merge(docs, vals, edges, np.full(len(edges), 1.0, np.float32))
        elif t in (EDGE_LO, EDGE_HI):
            docs = edges
            vals = np.full(len(edges), 3.0, np.float32)
            top = slice(0, N_TOP) if t == EDGE_LO else slice(max(len(edges) - N_TOP, 0), None)
            vals[top] = 7.0
        elif t == ZFILL:
            docs = _pick(rng, n_docs, 6)
            vals = (np.round(rng.uniform(0.5, 9.0, len(docs)) * 4) / 4 + 0.25).astype(np.float32)
            docs, vals = _merge(docs, vals, np.array([n_docs - 1]), np.array([2.5], np.float32))
            docs, vals = docs[-7:], vals[-7:]
        else:
            docs = _pick(rng, n_docs, int(rng.integers(600, 1801)))
            vals = (np.round(rng.uniform(0.25, 9.0, len(docs)) * 4) / 4 + 0.25).astype(np.float32)
        if signed:
            neg = rng.random(len(docs)) < 1 / 3
            vals = np.where(neg, -vals, vals).astype(np.float32)
            if t == 1:
                vals[::5] = np.float32(-0.0)
        cols.append((docs, vals))
    indptr = np.zeros(V + 1, np.int64)
    np.cumsum([len(d) for d, _ in cols], out=indptr[1:])
    return (indptr, np.concatenate([d for d, _ in cols]).astype(np.int32),
            np.concatenate([v for _, v in cols]).astype(np.float32))


def wide_queries(T: int, Q: int = 8, seed: int = 0) -> np.ndarray:
    """int32 [Q, T] over wide_csc's terms.  Rows 0 .. 5 are fixed: all
    padding; EDGE_LO alone; EDGE_HI alone; ZFILL alone (fewer postings than k
    = 10: zero fill); one rare term in every slot (a duplicate counts each
    time); EDGE_LO, EDGE_HI and a rare term.  The others: T // 2 common terms
    then rare ones, with a padding slot in the middle where T >= 4.  Every row
    with a common term also holds a rare one of >= 600 postings, so that its
    tile-bound threshold stays above the common terms' scores
    (tests/test_wide_model.py checks the list lengths that follow)."""
    rng = np.random.default_rng(1000 * T + seed)
    q = np.full((Q, T), -1, np.int32)
    rare = lambda n: rng.choice(np.arange(RARE0, ZFILL), n, replace=n > ZFILL - RARE0)
    for r in range(Q):
        if r == 0:
            continue
        if r in (1, 2, 3):
            q[r, 0 if r != 2 else T - 1] = (EDGE_LO, EDGE_HI, ZFILL)[r - 1]
        elif r == 4:
            q[r, :] = RARE0 + 3
        elif r == 5:
            q[r, :min(T, 3)] = [EDGE_LO, EDGE_HI, RARE0 + 5][:min(T, 3)]
            if T < 3:
                q[r, T - 1] = RARE0 + 5
        else:
            nc = T // 2
            q[r, :nc] = rng.choice(N_COMMON, nc, replace=nc > N_COMMON)
            q[r, nc:] = rare(T - nc)
            if T >= 4:
                q[r, nc - 1] = -1
    return q


# ------------------------------------------------------------ packed masks
def n_words(n_docs: int) -> int:
    return (n_docs + 31) // 32


def ids_to_words(n_docs: int, ids) -> np.ndarray:
    """Packed uint32 [W] row with the bits of ``ids`` (any order, repeats
    allowed) set: document d at bit d & 31 of word d >> 5."""
    out = np.zeros(n_words(n_docs), np.uint32)
    d = np.unique(np.asarray(ids, np.int64))
    if d.size:
        w = d >> 5
        start = np.flatnonzero(np.r_[True, w[1:] != w[:-1]])
        bit = np.uint32(1) << (d & 31).astype(np.uint32)
        out[w[start]] = np.bitwise_or.reduceat(bit, start)
    return out


def range_words(n_docs: int, lo: int, hi: int) -> np.ndarray:
    """Packed row allowing the documents [lo, hi)."""
    out = np.zeros(n_words(n_docs), np.uint32)
    lo, hi = max(lo, 0), min(hi, n_docs)
    if lo >= hi:
        return out
    w0, w1 = lo >> 5, (hi - 1) >> 5
    out[w0:w1 + 1] = 0xFFFFFFFF
    out[w0] &= np.uint32((0xFFFFFFFF << (lo & 31)) & 0xFFFFFFFF)
    out[w1] &= np.uint32(0xFFFFFFFF >> (31 - ((hi - 1) & 31)))
    return out


def all_ones(n_docs: int, garbage_tail: bool = False) -> np.ndarray:
    """Packed row allowing every document; garbage_tail: the bits of the last
    word past n_docs are set as well (a caller's mask may hold anything there)."""
    out = np.full(n_words(n_docs), 0xFFFFFFFF, np.uint32)
    if not garbage_tail:
        clear_tail(n_docs, out)
    return out


def clear_tail(n_docs: int, words: np.ndarray) -> np.ndarray:
    """Zero the bits at and past n_docs of the last word(s), in place."""
    r = n_docs & 31
    if r and words.shape[-1]:
        words[..., -1] &= np.uint32((1 << r) - 1)
    return words


def bits_of(words: np.ndarray, ids) -> np.ndarray:
    """bool per id: its bit of the packed row."""
    d = np.asarray(ids, np.int64)
    return ((words[d >> 5] >> (d & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)


def _popcount(words: np.ndarray) -> int:
    if hasattr(np, "bitwise_count"):
        return int(np.bitwise_count(words).sum(dtype=np.int64))
    lut = np.array([bin(i).count("1") for i in range(256)], np.uint8)
    return int(lut[np.ascontiguousarray(words).view(np.uint8)].sum(dtype=np.int64))


def ref_mask_count(n_docs: int, masks) -> np.ndarray:
    """int64 [M]: the set bits of every packed row among the documents
    0 .. n_docs - 1 (bits past n_docs are not counted)."""
    m = np.atleast_2d(np.asarray(masks, np.uint32))
    out = np.zeros(len(m), np.int64)
    for i, row in enumerate(m):
        out[i] = _popcount(row[:-1]) if len(row) else 0
        if len(row):
            out[i] += _popcount(clear_tail(n_docs, row[-1:].copy()))
    return out


def _first_set(words: np.ndarray, lo: int, n_docs: int, need: int) -> np.ndarray:
    """The first ``need`` set bits at or after ``lo`` (and below n_docs)."""
    out, have = [], 0
    w, W, step = lo >> 5, n_words(n_docs), 1 << 12
    while w < W and have < need:
        chunk = words[w:w + step]
        # a non-zero word holds a bit; lo's own word may hold none at or after lo: one more
        nz = np.flatnonzero(chunk)[:need - have + 1]
        if nz.size:
            b = np.unpackbits(chunk[nz].astype("<u4").view(np.uint8).reshape(-1, 4), axis=1,
                              bitorder="little")
            wi, bi = np.nonzero(b)
            ids = (w + nz[wi]).astype(np.int64) * 32 + bi
            ids = ids[(ids >= lo) & (ids < n_docs)]
            out.append(ids)
            have += ids.size
        w += len(chunk)
        step = min(step * 4, 1 << 22)
    ids = np.concatenate(out) if out else np.zeros(0, np.int64)
    return ids[:need]


def _first_allowed(allow, lo: int, n_docs: int, need: int, touched: np.ndarray) -> np.ndarray:
    """The ``need`` smallest ids in [lo, n_docs) that ``allow`` lets through
    and that are not in ``touched`` (sorted)."""
    if need <= 0 or lo >= n_docs:
        return np.zeros(0, np.int64)
    a = np.searchsorted(touched, lo)
    if allow is None:
        hi = min(n_docs, lo + need)
        while True:   # widen by the touched ids inside the window
            inside = np.searchsorted(touched, hi) - a
            if hi - lo - inside >= need or hi >= n_docs:
                break
            hi = min(n_docs, lo + need + inside)
        ids = np.arange(lo, hi, dtype=np.int64)
        return ids[~np.isin(ids, touched[a:a + inside], assume_unique=True)][:need]
    if callable(allow):
        out, have, step = [], 0, max(4 * need, 1024)
        while lo < n_docs and have < need:
            ids = np.arange(lo, min(n_docs, lo + step), dtype=np.int64)
            ids = ids[np.asarray(allow(ids), bool)]
            ids = ids[~np.isin(ids, touched, assume_unique=True)]
            out.append(ids)
            have += ids.size
            lo += step
            step = min(step * 4, 1 << 22)
        return np.concatenate(out)[:need] if out else np.zeros(0, np.int64)
    # a packed row: enough set bits that `need` of them survive the touched ids
    want = need
    while True:
        ids = _first_set(allow, lo, n_docs, want)
        free = ids[~np.isin(ids, touched, assume_unique=True)]
        if free.size >= need or ids.size < want:
            return free[:need]
        want = need + 2 * (ids.size - free.size) + 16


# ------------------------------------------------------------ the reference
def score_keys(s) -> np.ndarray:
    """The engine's order of fp32 scores as uint32 (score_key of
    csrc/bm25mi_internal.h): numeric order, -0.0 just below +0.0."""
    u = np.ascontiguousarray(s, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


ZERO_KEY = int(score_keys(np.zeros(1, np.float32))[0])


def touched(indptr, indices, data, row, wrow=None):
    """(ids int64 sorted, scores float32) of the documents one query touches:
    the union of its terms' posting lists, each document's sum in float32 from
    +0.0, one add per term slot in query order — float32(weight * value) when
    weighted, a weight of 0.0 being padding (oracle/).  Ids < 0
    or >= the vocabulary are padding."""
    nv = len(indptr) - 1
    slots = []
    for i, t in enumerate(np.asarray(row).tolist()):
        if t < 0 or t >= nv:
            continue
        w = None if wrow is None else np.float32(wrow[i])
        if w is not None and w == 0:
            continue
        a, b = int(indptr[t]), int(indptr[t + 1])
        if b > a:
            slots.append((np.asarray(indices[a:b], np.int64), np.asarray(data[a:b], np.float32), w))
    if not slots:
        return np.zeros(0, np.int64), np.zeros(0, np.float32)
    ids = np.unique(np.concatenate([d for d, _, _ in slots]))
    acc = np.zeros(len(ids), np.float32)
    for d, v, w in slots:
        pos = np.searchsorted(ids, d)      # a column holds a document once
        acc[pos] = acc[pos] + (v if w is None else (w * v).astype(np.float32))
    return ids, acc


def ref_rows(indptr, indices, data, queries, weights=None):
    """touched() of every query row (ref_search / ref_score_docs take it as
    ``rows`` to share it between calls)."""
    q = np.asarray(queries)
    return [touched(indptr, indices, data, q[r], None if weights is None else weights[r])
            for r in range(len(q))]


def _allow_of(allow, r):
    if allow is None or callable(allow):
        return allow
    if isinstance(allow, np.ndarray) and allow.ndim == 1:
        return allow
    return allow[r]          # one per query: None, a callable or a packed row


def ref_search(n_docs, indptr, indices, data, queries, k, *, weights=None, allow=None,
               after=None, doc_offset=0, rows=None):
    """The oracle's search over the touched documents only -> (docs int32
    [Q, k], scores float32 [Q, k]).  Per query: the touched documents' sums
    (touched()), plus the k smallest untouched ids at score +0.0, without what
    ``allow`` or the cursor excludes, ranked by (score descending, doc
    ascending), the first k; short rows end in doc -1 with score bits
    0xFFFFFFFF.

    allow: None, a callable (int64 ids -> bool), a packed uint32 [W] row (bits
    past n_docs are ignored), or a sequence of those, one per query.
    after: None or (scores float32 [Q], docs int32 [Q]) as search_after takes
    them — global ids, AFTER_NONE: no cursor, -1: exhausted.  Ids in the
    result are global (doc_offset added)."""
    q = np.asarray(queries)
    Q, k = len(q), int(k)
    docs = np.full((Q, k), -1, np.int32)
    bits = np.full((Q, k), PAD, np.uint32)
    for r in range(Q):
        ids, sc = rows[r] if rows is not None else touched(
            indptr, indices, data, q[r], None if weights is None else weights[r])
        al = _allow_of(allow, r)
        cur = None
        if after is not None and int(after[1][r]) != AFTER_NONE:
            c = int(after[1][r])
            if c == -1:
                continue
            cur = (int(score_keys(np.float32(after[0][r]).reshape(1))[0]), c)
        if al is None:
            ok = np.ones(len(ids), bool)
        elif callable(al):
            ok = np.asarray(al(ids), bool)
        else:
            ok = bits_of(al, ids)
        lo, fill = 0, k
        if cur is not None:
            if cur[0] < ZERO_KEY:
                fill = 0                      # every +0.0 comes before the cursor
            elif cur[0] == ZERO_KEY:
                lo = max(cur[1] - doc_offset + 1, 0)
        zeros = _first_allowed(al, lo, n_docs, fill, ids)
        cid = np.concatenate([ids[ok], zeros])
        csc = np.concatenate([sc[ok], np.zeros(len(zeros), np.float32)])
        key = score_keys(csc).astype(np.int64)
        if cur is not None:
            keep = (key < cur[0]) | ((key == cur[0]) & (cid + doc_offset > cur[1]))
            cid, csc, key = cid[keep], csc[keep], key[keep]
        order = np.lexsort((cid, -key))[:k]
        docs[r, :len(order)] = (cid[order] + doc_offset).astype(np.int32)
        bits[r, :len(order)] = csc[order].view(np.uint32)
    return docs, bits.view(np.float32)


def ref_score_docs(n_docs, indptr, indices, data, queries, docs, *, weights=None, doc_offset=0,
                   rows=None) -> np.ndarray:
    """float32 [Q, C]: the sum of query q on document docs[q, c] (global ids),
    +0.0 for padding (negative), for ids outside [doc_offset, doc_offset +
    n_docs) and for documents the query does not touch."""
    q = np.asarray(queries)
    d = np.asarray(docs, np.int64)
    out = np.zeros(d.shape, np.float32)
    for r in range(len(q)):
        ids, sc = rows[r] if rows is not None else touched(
            indptr, indices, data, q[r], None if weights is None else weights[r])
        loc = d[r] - doc_offset
        ok = (d[r] >= 0) & (loc >= 0) & (loc < n_docs)
        pos = np.minimum(np.searchsorted(ids, loc), max(len(ids) - 1, 0))
        hit = ok & (ids[pos] == loc) if len(ids) else np.zeros(len(loc), bool)
        out[r, hit] = sc[pos[hit]]
    return out


def term_words(n_docs, indptr, indices, t) -> np.ndarray:
    """Packed row of the documents that hold term t (none for an id outside
    the vocabulary)."""
    if t < 0 or t >= len(indptr) - 1:
        return np.zeros(n_words(n_docs), np.uint32)
    return ids_to_words(n_docs, indices[int(indptr[t]):int(indptr[t + 1])])


def ref_term_masks(n_docs, indptr, indices, must=None, any=None, must_not=None, base=None,
                   min_match=None) -> np.ndarray:
    """term_masks / min_match on word arrays -> packed uint32 [M, W].  Row m:
    base (1 or M rows) AND every term of must[m] AND NOT any term of
    must_not[m]; the any clause, where it names a term, asks for min_match[m]
    (None: 1) of its slots to hold the document — a repeated id counts each
    time, min_match <= 0 makes the clause optional.  Clause rows are lists of
    ids, negative = padding; the bits past n_docs are 0."""
    clauses = [c for c in (must, any, must_not) if c is not None]
    M = len(clauses[0]) if clauses else len(np.atleast_2d(base))
    row = lambda c, m: [] if c is None else [int(t) for t in c[m] if int(t) >= 0]
    out = np.zeros((M, n_words(n_docs)), np.uint32)
    b = None if base is None else np.atleast_2d(np.asarray(base, np.uint32))
    mm = None if min_match is None else np.broadcast_to(np.asarray(min_match), (M,))
    for m in range(M):
        w = all_ones(n_docs) if b is None else clear_tail(n_docs, b[0 if len(b) == 1 else m].copy())
        for t in row(must, m):
            w &= term_words(n_docs, indptr, indices, t)
        ids = row(any, m)
        need = 1 if mm is None else int(mm[m])
        if ids and need > 0:
            lists = [np.asarray(indices[int(indptr[t]):int(indptr[t + 1])], np.int64)
                     for t in ids if t < len(indptr) - 1]
            d, cnt = np.unique(np.concatenate(lists) if lists else np.zeros(0, np.int64),
                               return_counts=True)
            w &= ids_to_words(n_docs, d[cnt >= need])
        for t in row(must_not, m):
            w &= ~term_words(n_docs, indptr, indices, t)
        out[m] = w
    return out


def doc_slice(indptr, indices, data, lo: int, hi: int):
    """The CSC of documents [lo, hi) with local ids (columns kept)."""
    ip = np.zeros(len(indptr), np.int64)
    ix, dt = [], []
    for t in range(len(indptr) - 1):
        a, b = int(indptr[t]), int(indptr[t + 1])
        col = indices[a:b]
        p0, p1 = np.searchsorted(col, lo), np.searchsorted(col, hi)
        ix.append(np.asarray(col[p0:p1], np.int64) - lo)
        dt.append(data[a + p0:a + p1])
        ip[t + 1] = ip[t] + (p1 - p0)
    return ip, np.concatenate(ix).astype(np.int32), np.concatenate(dt).astype(np.float32)
