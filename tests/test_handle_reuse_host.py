"""CPU side of the handle-reuse tests (tests/test_gpu_handle_reuse.py): one
index handle serving interleaved entry points, shapes, options and streams.

This module holds what the GPU tests import — the fixture index, the pools of
queries, weights, masks and clause rows, the deterministic program of steps
and the builder of every step's expected result — and the tests that guard
them without a GPU: the program is the same on every run and contains every
ordered pair of step kinds, the expected rows of the plain searches are the C
oracle's bit for bit, and the padding of short filtered rows is the documented
one.

The expected rows come from the references the per-entry-point tests use:
oracle.scores_dense_c (unweighted), ref_rows of test_search_weighted_host
(weighted), the (score descending, doc ascending) selection and the doc -1 /
0xFFFFFFFF padding of _want in test_gpu_search_filtered, and a numpy
evaluation of the allowed(m, d) formula of include/bm25mi.h for the boolean
term masks.  The full order of a (row, T, weighted) is computed once; a mask
keeps a subsequence of it and a step takes its first k.

program2 is a second program over the cursor, collapsed, composed boolean and
stateless calls (kinds A, C, G, U) and the old kinds they share handle state
with.  Its expectations are derived from the same cached rows and orders; the
tests at the end hold them, one step per variation, against the models of the
per-entry-point files: ref_after, collapse_model (ref_collapsed and the paged
loop's statistics), min_match_model, range_model, facets_model and
sorted_model."""
import functools

import numpy as np
import pytest

from oracle import oracle
from test_gpu_edges import TILE, _csc
from test_gpu_parity import _sample_p
from test_gpu_search_filtered import PAD, _want
from test_search_weighted_host import ref_rows

N = 300_001                      # 147 tiles of 2048, the last one partial (993 documents)
NT = (N + TILE - 1) // TILE
# a second, sparser fixture: 1027 tiles, the last one holds one document.  The large-k list
# path needs a sample of at least k keys (8 per sample tile at stride 2): k = 4097 fits from
# 1025 tiles on, which the 147 tiles of N never reach
N_BIG = 1026 * TILE + 1
NT_BIG = (N_BIG + TILE - 1) // TILE
V_COMMON, V = 30, 300
T_MAX, POOL = 65, 16
QS = (1, 2, 16, 48)              # 48: the pool three times
TS = (0, 1, 8, 17, 65)
KS_SMALL = (1, 8, 100, 4096)
KS_LARGE = (4097, 20_000, N)
KINDS = "PLFDWBHSM"
SEARCH_KINDS = "PLFDWBH"
MASK_TILE = 73
VARIANTS = {"dense": (False, "dense"), "sparse": (False, "sparse"), "signed": (True, "dense")}
K_MAX = 4096                     # kMaxK: above it the large-k / dense paths
K_LIST_MAX = 131072              # kLargeListMaxK

# one option change before a step: (set, restore) pairs, every one exact
OPTION_PAIRS = [("flat", 0, 1), ("sample_p", 1, 8), ("theta_bound", 0, 1), ("list_cap", 6000, 0),
                ("flat_bw", 2, 0), ("tile_bound", 0, 1), ("bound_pool", 0, 1),
                ("rest_split", 1, 0), ("count_skips", 1, 0), ("grid_pct", 50, 100),
                ("list_cap", 4, 0), ("flat_bw", 1, 0)]
DEFAULTS = {name: dflt for name, _, dflt in OPTION_PAIRS}

# the second program (program2): the ranked and composed calls beside the old kinds they
# share handle state with.  A cursor search, C collapsed search, G composed boolean search,
# U the calls documented as stateless
KINDS2 = "ACGUPLFDH"
NEW_OPTION_PAIRS = [("collapse_page", 8, 0), ("collapse_chunk", 3, 0), ("bool_chunk", 5, 0),
                    ("sorted_bins", 16, 0), ("filter_tiles", 0, 1)]
OPTION_PAIRS2 = NEW_OPTION_PAIRS + OPTION_PAIRS
DEFAULTS2 = {name: dflt for name, _, dflt in OPTION_PAIRS2}
AFTER_NONE = -2
CURSORS = ("none", "page", "deep", "mix")
DEEP = 5000                      # the "deep" cursor: every row's 5000th result
G_MODES = ("min_match", "facets", "all", "sorted", "counts")
U_MODES = ("mask_count", "facets", "range_masks", "sorted", "term_masks")
COLUMNS = ("i32", "i64", "f32")
N_LABELS = 12
TENANTS = 8
# program() as the parent commit computes it: sha256 of repr(program())
PROGRAM_DIGEST = "dbaa5e3aa3db74fbc27bae202f78b52accaa0b5f7fc10d3dbad5b3565b001c9c"


# ------------------------------------------------------------- the fixture
@functools.lru_cache(maxsize=None)
def reuse_csc(signed=False, big=False):
    """300 terms over N documents: 30 common ones (df N/15..N/4, values in
    (0.1, 1]) and 270 rare ones (df 1..300, values up to 9); about half of the
    values are quarter steps (ties at the k-th place), the rest random float32
    (the order of the adds matters).  signed: every third value negated.
    big: the same terms over N_BIG documents, the common ones at df
    N_BIG/60..N_BIG/30 (some 50 postings per term and tile)."""
    rng = np.random.default_rng(9101 if big else 9100)
    n, lo, hi = (N_BIG, 60, 30) if big else (N, 15, 4)
    cols = []
    for t in range(V):
        common = t < V_COMMON
        df = int(rng.integers(n // lo, n // hi + 1)) if common else int(rng.integers(1, 301))
        docs = rng.choice(n, df, replace=False)
        if t in (0, V_COMMON):
            docs[0] = n - 1      # the last document, in the last tile
        docs = np.unique(docs).astype(np.int32)
        v = rng.uniform(0.1, 1.0 if common else 9.0, len(docs))
        quarter = rng.random(len(docs)) < 0.5
        v[quarter] = np.ceil(v[quarter] * 4) / 4
        cols.append((docs, v.astype(np.float32)))
    ip, ix, dt = _csc(cols, np.float32)
    if signed:
        dt = dt.copy()
        dt[2::3] *= -1
    for a in (ip, ix, dt):
        a.setflags(write=False)
    return ip, ix, dt


@functools.lru_cache(maxsize=None)
def pools():
    """(queries int32 [16, 65], weights float32 [16, 65]).  Slots 1 and 4 of
    every row hold common terms; row 3 starts with padding (an all-padding
    query at T = 1), rows 5 and 7 repeat ids, row 9 has a padded tail.  The
    weights are of both signs, NaN on the padding slots."""
    rng = np.random.default_rng(9200)
    q = rng.integers(V_COMMON, V, size=(POOL, T_MAX)).astype(np.int32)
    common = rng.random(q.shape) < 0.3
    q[common] = rng.integers(0, V_COMMON, int(common.sum()))
    q[rng.random(q.shape) < 0.08] = -1
    q[:, 1] = rng.integers(0, V_COMMON, POOL)
    q[:, 4] = rng.integers(0, V_COMMON, POOL)
    q[3, 0] = -1
    q[5, 2] = q[5, 20] = q[5, 1]
    q[7, 10:30] = q[7, 9] = V_COMMON + 7
    q[9, 40:] = -1
    mag = np.exp2(rng.uniform(-3.0, 3.0, q.shape))
    w = (mag * rng.choice([-1.0, 1.0], q.shape)).astype(np.float32)
    exact = rng.random(q.shape) < 0.2
    w[exact] = rng.choice(np.array([-2.0, 0.25, 1.0, 1.5], np.float32), int(exact.sum()))
    w[q < 0] = np.nan
    q.setflags(write=False)
    w.setflags(write=False)
    return q, w


@functools.lru_cache(maxsize=None)
def masks(big=False):
    """bool [3, N] (big: [3, N_BIG]): about half of the documents, about 1 in
    500, tile 73 only."""
    rng = np.random.default_rng(9301 if big else 9300)
    n = N_BIG if big else N
    allow = np.zeros((3, n), bool)
    allow[0] = rng.random(n) < 0.5
    allow[1] = rng.random(n) < 1 / 500
    allow[2, MASK_TILE * TILE:(MASK_TILE + 1) * TILE] = True
    allow.setflags(write=False)
    return allow


@functools.lru_cache(maxsize=None)
def clauses():
    """(must [16, 2], any [16, 5], must_not [16, 3]) int32, -1 = padding: by
    row, at least one of four rare terms / none of three rare terms / one rare
    term (a handful of documents: short rows) / a common term, one of five
    rare ones and not another."""
    rng = np.random.default_rng(9400)
    must = np.full((POOL, 2), -1, np.int32)
    any_ = np.full((POOL, 5), -1, np.int32)
    must_not = np.full((POOL, 3), -1, np.int32)
    rare = lambda n: rng.integers(V_COMMON, V, n)
    for r in range(POOL):
        if r % 4 == 0:
            any_[r, :4] = rare(4)
        elif r % 4 == 1:
            must_not[r] = rare(3)
        elif r % 4 == 2:
            must[r, 1] = rare(1)[0]
        else:
            must[r, 0] = r % V_COMMON
            any_[r] = rare(5)
            any_[r, 2] = any_[r, 0]
            must_not[r, 1] = rare(1)[0]
    for a in (must, any_, must_not):
        a.setflags(write=False)
    return must, any_, must_not


def _has(t):
    ip, ix, _ = reuse_csc()
    h = np.zeros(N, bool)
    h[ix[ip[t]:ip[t + 1]]] = True
    return h


@functools.lru_cache(maxsize=None)
def clause_allow(r, base):
    """allowed(m, d) of include/bm25mi.h for clause row r (bool [N]); base:
    mask 0 of masks() applied to the row, or none.  has(t, d) is the same on
    every variant (a stored negative value counts)."""
    must, any_, must_not = clauses()
    ok = masks()[0].copy() if base else np.ones(N, bool)
    for t in must[r][must[r] >= 0]:
        ok &= _has(t)
    ids = any_[r][any_[r] >= 0]
    if len(ids):
        some = np.zeros(N, bool)
        for t in ids:
            some |= _has(t)
        ok &= some
    for t in must_not[r][must_not[r] >= 0]:
        ok &= ~_has(t)
    ok.setflags(write=False)
    return ok


@functools.lru_cache(maxsize=None)
def clause_allow_mm(r, base, mm):
    """clause_allow with the counting any clause of "Minimum-should-match"
    (include/bm25mi.h): a row that names any-terms needs mm of its slots
    (a repeated id counts each time; mm <= 0: the clause is optional)."""
    must, any_, must_not = clauses()
    ok = masks()[0].copy() if base else np.ones(N, bool)
    for t in must[r][must[r] >= 0]:
        ok &= _has(t)
    ids = any_[r][any_[r] >= 0]
    if len(ids) and mm > 0:
        count = np.zeros(N, np.int32)
        for t in ids:
            count += _has(t)
        ok &= count >= mm
    for t in must_not[r][must_not[r] >= 0]:
        ok &= ~_has(t)
    ok.setflags(write=False)
    return ok


@functools.lru_cache(maxsize=None)
def columns():
    """Document columns of the range, sort and facet calls (read-only): i32
    with heavy ties (16 values), i64 beyond +-2^32 (half of it multiples of
    2^36: ties), f32 quarter steps with NaN, -0.0 and +0.0, and facet labels
    -2 .. 11 (negative: no group)."""
    rng = np.random.default_rng(9600)
    i32 = rng.integers(0, 16, N).astype(np.int32)
    i64 = rng.integers(-(1 << 40), 1 << 40, N)
    tied = rng.random(N) < 0.5
    i64[tied] = (i64[tied] >> 36) << 36
    f32 = (np.round(rng.normal(0.0, 2.0, N) * 4) / 4).astype(np.float32)
    f32[rng.random(N) < 0.03] = np.nan
    f32[rng.random(N) < 0.01] = -0.0
    f32[rng.random(N) < 0.01] = 0.0
    out = {"i32": i32, "i64": i64.astype(np.int64), "f32": f32,
           "labels": rng.integers(-2, N_LABELS, N).astype(np.int32)}
    for a in out.values():
        a.setflags(write=False)
    return out


def range_clauses(name, rows):
    """(fields int32 [M, 2], lo, hi [M, 2] of column ``name``'s dtype) for the
    pool rows ``rows``: a window that moves with the row, an open low end on
    rows 4, 9 and 14, lo > hi (nothing) on row 6, and on rows 1, 5, 9 and 13 a
    second clause on the same field (the window's lower half); the other
    second clauses are padding."""
    dt = columns()[name].dtype
    low = dt.type(-np.inf) if dt.kind == "f" else int(np.iinfo(dt).min)
    M = len(rows)
    fields = np.full((M, 2), -1, np.int32)
    lo, hi = np.zeros((M, 2), dt), np.zeros((M, 2), dt)
    for i, r in enumerate(int(r) for r in rows):
        if name == "i32":
            a, b = r % 8, r % 8 + 5
        elif name == "i64":
            a, b = (r - 8) << 37, ((r - 8) << 37) + (1 << 39)
        else:
            a, b = (r - 8) / 2, (r - 8) / 2 + 2.0
        mid = (a + b) / 2 if dt.kind == "f" else (a + b) // 2
        if r % 5 == 4:
            a = low
        if r == 6:
            a, b = b, a
        fields[i, 0], lo[i, 0], hi[i, 0] = 0, a, b
        if r % 4 == 1:
            fields[i, 1], lo[i, 1], hi[i, 1] = 0, low, mid
    return fields, lo, hi


@functools.lru_cache(maxsize=None)
def collapse_groups(tenant):
    from collapse_model import tenant_groups, uniform_groups
    g = tenant_groups(N, TENANTS) if tenant else uniform_groups(N)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def sort_order(name, descending):
    """(ranks, perm) of a column by the sort model (tests/sorted_model.py)."""
    from sorted_model import order_want
    ranks, perm = order_want(columns()[name], descending)
    ranks.setflags(write=False)
    perm.setflags(write=False)
    return ranks, perm


def rows_of(Q):
    """Pool rows of a step of Q queries (48: the pool three times)."""
    return np.arange(Q) % POOL


def step_min_match(step):
    """min_match of a G or U step's rows: 0 (optional), 1 and 2 by row,
    rotated by the step."""
    return ((rows_of(step["Q"]) + step["i"]) % 3).astype(np.int32)


def step_after_ranks(step):
    """Rank cursors of a sorted G or U step: none (-2), a third of the way
    into the order, and on row 2 the exhausted cursor (-1)."""
    a = np.where(np.arange(step["Q"]) % 2 == 0, AFTER_NONE, N // 3).astype(np.int32)
    a[2:3] = -1
    return a


def collapse_page(step, opts=None):
    """The page of a collapsed search at the step's k: option collapse_page,
    or twice k, at most 4096."""
    page = (step["opts"] if opts is None else opts).get("collapse_page", 0)
    return max(1, min(page or 2 * step["k"], N, K_MAX))


def step_queries(step):
    q, w = pools()
    r = rows_of(step["Q"])
    return np.ascontiguousarray(q[r, :step["T"]]), np.ascontiguousarray(w[r, :step["T"]])


def step_query_mask(step):
    """Mask ids of a filtered step's queries: 0, 1, 2 and -1 (no filter) by
    row, rotated by the step."""
    return ((rows_of(step["Q"]) + step["i"]) % 4 - 1).astype(np.int32)


# ------------------------------------------------------------- the program
def kind_walk(rng, kinds=KINDS):
    """A closed walk over the kinds (nine in both programs) that takes every
    ordered pair, same-kind pairs included, exactly once: an Euler circuit of
    the complete directed graph with loops (81 edges, 82 steps), from P."""
    out = {a: list(rng.permutation(list(kinds))) for a in kinds}
    stack, walk = ["P"], []
    while stack:
        v = stack[-1]
        if out[v]:
            stack.append(out[v].pop(0))
        else:
            walk.append(stack.pop())
    return walk[::-1]


def _spread(rng, values, n, weights=None):
    """n draws that hold every value: the set tiled to n (by weight), shuffled."""
    reps = [1] * len(values) if weights is None else weights
    base = [v for v, c in zip(values, reps) for _ in range(c)]
    out = (base * (n // len(base) + 1))[:max(n, len(base))]
    out = list(rng.permutation(np.array(out, dtype=object)))
    return out[:n] if n >= len(base) else out


@functools.lru_cache(maxsize=None)
def program():
    """The 82 steps (dicts; the same on every run).  Keys: i, kind, Q, T, k,
    form ("host" / "device"), stream (0..2), opt ((name, value) set before the
    step, or None), opts (the non-default options in force at the step), and
    by kind: large_lists (L), dense_by ("option" / "k", D), masked (W: with
    masks), weighted (S), base (B, M: mask 0 as the base).

    One P -> P pair is fixed to (Q 16, T 8, k 100) with list_cap 4 before the
    first and list_cap 0 before the second: the stale-fallback check."""
    rng = np.random.default_rng(9500)
    kinds = kind_walk(rng)
    n = len(kinds)
    Qs = _spread(rng, QS, n, (3, 3, 3, 1))
    forms = _spread(rng, ("host", "device"), n)
    streams = rng.integers(0, 3, n).tolist()
    # a kind's n-th step takes the n-th of the T and of the k values, from a drawn start
    off = {kind: int(rng.integers(0, 12)) for kind in KINDS}
    off_t = {kind: int(rng.integers(0, 5)) for kind in KINDS}
    pp = next(i for i in range(1, n - 1) if kinds[i] == kinds[i + 1] == "P")
    steps, count, opts, pair = [], {}, {}, 0
    for i, kind in enumerate(kinds):
        c = count[kind] = count.get(kind, -1) + 1
        s = {"i": i, "kind": kind, "Q": int(Qs[i]), "T": TS[(c + off_t[kind]) % 5],
             "k": KS_SMALL[(c + off[kind]) % 4], "form": forms[i], "stream": int(streams[i]),
             "opt": None}
        if kind == "L":
            s["k"], s["large_lists"] = KS_LARGE[(c + off[kind]) % 3], 1 - c % 2
        elif kind == "D":
            s["dense_by"] = "option" if c % 2 == 0 else "k"
            if s["dense_by"] == "k":
                s["k"] = KS_LARGE[(c // 2 + off[kind]) % 3]
        elif kind == "W":
            s["masked"] = c % 2 == 0
        elif kind == "S":
            s["weighted"], s["k"] = c % 2 == 1, 0
        elif kind in "BM":
            s["base"] = c % 2 == 1
            if kind == "M":
                s["k"] = 0
        if kind == "B":
            s["form"] = "host"
        if kind == "H":
            s["form"] = "device"
        # the largest outputs stay small batches (k = N: 2.4 MB per query)
        if s["k"] == N:
            s["Q"] = min(s["Q"], 2)
        elif s["k"] > K_MAX:
            s["Q"] = min(s["Q"], 16)
        if i in (pp, pp + 1):
            s.update(Q=16, T=8, k=100)
        # options: set at pp, pp + 4, ... and restored two steps later (the
        # program ends on the defaults); the fixed pair sets list_cap 4 and
        # restores it at once
        if i == pp:
            s["opt"] = ("list_cap", 4)
        elif i == pp + 1:
            s["opt"] = ("list_cap", 0)
        elif (i - pp) % 4 == 0 and i + 2 < n:
            name, val, _ = OPTION_PAIRS[pair % len(OPTION_PAIRS)]
            s["opt"] = (name, val)
        elif (i - pp) % 4 == 2 and opts:
            name, _, dflt = OPTION_PAIRS[pair % len(OPTION_PAIRS)]
            s["opt"] = (name, dflt)
            pair += 1
        if s["opt"]:
            name, val = s["opt"]
            if val == DEFAULTS[name]:
                opts.pop(name, None)
            else:
                opts[name] = val
        s["opts"] = dict(opts)
        steps.append(s)
    return tuple(steps)


def _new_kind_rules(s, kind, c):
    """The variation of a new kind's c-th step (program2)."""
    if kind == "A":
        # (c + c // 4: over nine steps every cursor meets a weighted and a plain search)
        s["cursor"] = CURSORS[(c + c // 4) % 4]
        s["weighted"], s["masked"] = c % 2 == 1, c % 3 == 0
        if c == 6:                   # one step past kMaxK: the dense path under a cursor
            s["k"] = K_MAX + 1
        if s["cursor"] == "mix":     # (the per-row mix needs rows, and scores that differ)
            s["Q"], s["T"] = 16, s["T"] or 8
    elif kind == "C":
        # the layouts alternate; the quota changes every third step, so both layouts meet
        # both quotas; the three switches are the bits of c's Gray code (a bijection of
        # 0..7: all eight combinations, none of them in step with the layout)
        v = (c ^ c >> 1) & 7
        s["weighted"], s["masked"], s["ret_groups"] = bool(v & 1), bool(v & 2), bool(v & 4)
        s["tenant"], s["per_group"] = c % 2 == 1, (1, 3)[c // 3 % 2]
    elif kind == "G":
        s["mode"], s["base"], s["form"] = G_MODES[c % 5], c % 2 == 1, "host"
        s["column"], s["sort_column"], s["descending"] = COLUMNS[c % 3], COLUMNS[(c + 1) % 3], c % 2
        if s["mode"] == "counts":
            s["k"] = 0
    elif kind == "U":
        s["mode"], s["base"] = U_MODES[c % 5], c % 2 == 0
        s["column"], s["descending"] = COLUMNS[c % 3], c // 5 % 2
        s["k"] = min(s["k"], 100)    # (search_sorted's k; the other modes have none)
        # a mode's two steps (c and c + 5) take opposite forms: nine of the ten (mode, form)
        # pairs, the tenth (term_masks on the device) in stateless_steps()
        s["form"] = ("host", "device")[(c % 5 + c // 5) % 2]
        if s["mode"] == "sorted":    # (the rank cursors are by row: none, real, exhausted)
            s["Q"] = 16


@functools.lru_cache(maxsize=None)
def program2():
    """The second program: 82 steps over KINDS2, an Euler circuit like
    program()'s, same keys.  The old kinds keep program()'s step rules; the new
    ones add, by kind: cursor / weighted / masked (A), weighted / masked /
    ret_groups / tenant / per_group (C), mode / base / column / sort_column /
    descending (G, host only) and mode / base / column / descending (U; Q is
    its number of mask rows).

    Options: each pair of NEW_OPTION_PAIRS is set at the first free step of
    the kind it acts on (collapse_page and collapse_chunk at a tenant C step,
    bool_chunk at a searching G step of Q > 5, sorted_bins at a sorted G step,
    filter_tiles at an A step) and restored two steps later; the old pairs fill
    the free steps in between, one at a time.  C steps under collapse_page 8
    keep k <= 100 (a page of 8 at k = 4096 takes hundreds of rounds)."""
    rng = np.random.default_rng(9501)
    kinds = [str(kind) for kind in kind_walk(rng, KINDS2)]
    n = len(kinds)
    Qs = _spread(rng, QS, n, (3, 3, 3, 1))
    forms = _spread(rng, ("host", "device"), n)
    streams = rng.integers(0, 3, n).tolist()
    off = {kind: int(rng.integers(0, 12)) for kind in KINDS2}
    off_t = {kind: int(rng.integers(0, 5)) for kind in KINDS2}
    steps, count = [], {}
    for i, kind in enumerate(kinds):
        c = count[kind] = count.get(kind, -1) + 1
        s = {"i": i, "kind": kind, "Q": int(Qs[i]), "T": TS[(c + off_t[kind]) % 5],
             "k": KS_SMALL[(c + off[kind]) % 4], "form": forms[i], "stream": int(streams[i]),
             "opt": None, "c": c}
        if kind == "L":
            s["k"], s["large_lists"] = KS_LARGE[(c + off[kind]) % 3], 1 - c % 2
        elif kind == "D":
            s["dense_by"] = "option" if c % 2 == 0 else "k"
            if s["dense_by"] == "k":
                s["k"] = KS_LARGE[(c // 2 + off[kind]) % 3]
        elif kind == "H":
            s["form"] = "device"
        else:
            _new_kind_rules(s, kind, c)
        if s["k"] == N:
            s["Q"] = min(s["Q"], 2)
        elif s["k"] > K_MAX or (kind == "C" and s["k"] == K_MAX):
            s["Q"] = min(s["Q"], 16)
        steps.append(s)
    # the option windows: set at j, in force at j and j + 1, restored at j + 2
    targets = {"collapse_page": lambda s: s["kind"] == "C" and s["tenant"],
               "collapse_chunk": lambda s: s["kind"] == "C" and s["tenant"] and s["Q"] > 3,
               "bool_chunk": lambda s: (s["kind"] == "G" and s["Q"] > 5
                                        and s["mode"] in ("min_match", "facets", "all")),
               "sorted_bins": lambda s: s["kind"] == "G" and s["mode"] == "sorted",
               "filter_tiles": lambda s: s["kind"] == "A"}
    free = [True] * n

    def place(j, pair):
        name, val, dflt = pair
        steps[j]["opt"], steps[j + 2]["opt"] = (name, val), (name, dflt)
        free[j] = free[j + 1] = free[j + 2] = False   # (no other window overlaps this one)

    for pair in NEW_OPTION_PAIRS:
        j = next(i for i in range(1, n - 3)
                 if free[i] and free[i + 1] and free[i + 2] and targets[pair[0]](steps[i]))
        place(j, pair)
    old = list(OPTION_PAIRS)
    for j in range(1, n - 3):
        if old and free[j] and free[j + 1] and free[j + 2]:
            place(j, old.pop(0))
    assert not old
    opts = {}
    for s in steps:
        if s["opt"]:
            name, val = s["opt"]
            if val == DEFAULTS2[name]:
                opts.pop(name, None)
            else:
                opts[name] = val
        s["opts"] = dict(opts)
        if s["kind"] == "C" and "collapse_page" in opts:
            s["k"] = min(s["k"], 100)
    return tuple(steps)


def stateless_steps():
    """Ten directed U steps: every mode in both forms (the program holds nine
    of the pairs), for the GPU test that runs them between searches."""
    return tuple({"i": n, "kind": "U", "Q": 16, "T": 0, "k": 8, "form": form, "stream": n % 3,
                  "opt": None, "mode": mode, "base": n % 2 == 0, "column": COLUMNS[n % 3],
                  "descending": n % 2}
                 for n, (mode, form) in enumerate((m, f) for f in ("device", "host")
                                                  for m in U_MODES))


def docs_source(steps, i):
    """The step whose returned documents S step i scores: the nearest earlier
    search step (S and M return none)."""
    for j in range(i - 1, -1, -1):
        if steps[j]["kind"] in SEARCH_KINDS:
            return steps[j]
    raise AssertionError("an S step before any search")


S_COLS = 32  # documents of the previous result an S step scores, plus padding ids


# -------------------------------------------------------- the expectations
class Expect:
    """Expected results over one data set (signed or not; big: the N_BIG
    fixture, which has no clause rows: no B and M steps), cached."""

    def __init__(self, signed, big=False):
        self.signed, self.big = signed, big
        self.n, self.nt = (N_BIG, NT_BIG) if big else (N, NT)
        self.csc = reuse_csc(signed, big)
        self._rows, self._order, self._masked, self._counts = {}, {}, {}, {}  # (_masked: topk)

    def row(self, r, T, weighted):
        """The dense fp32 score row of pool row r's first T slots."""
        key = (r, T, weighted)
        if key not in self._rows:
            q, w = pools()
            ip, ix, dt = self.csc
            if weighted:
                s = ref_rows(self.n, ip, ix, dt, q[r:r + 1, :T], w[r:r + 1, :T])[0]
            else:
                s = oracle.scores_dense_c(self.n, ip, ix, dt, q[r, :T])
            s.setflags(write=False)
            self._rows[key] = s
        return self._rows[key]

    def order(self, r, T, weighted):
        """Every document by (score descending, doc ascending) — _want's rule;
        the zero scores (most documents) keep their id order."""
        key = (r, T, weighted)
        if key not in self._order:
            s = self.row(r, T, weighted)
            parts = []
            for sel in (s > 0, s == 0, s < 0):
                ids = np.nonzero(sel)[0]
                v = s[ids]
                parts.append(ids[np.lexsort((ids, -v.astype(np.float64)))])
            o = np.concatenate(parts).astype(np.int32)
            assert len(o) == self.n  # (no NaN score)
            self._order[key] = o
        return self._order[key]

    def masked(self, r, T, weighted, mask):
        """order() under a mask: None, ("m", id) or ("c", row, base)."""
        o = self.order(r, T, weighted)
        if mask is None:
            return o
        if mask[0] == "m":
            allow = masks(self.big)[mask[1]]
        else:
            assert not self.big
            allow = clause_allow(mask[1], mask[2])
        return o[allow[o]]

    def step_masks(self, step):
        """Per query of a search step: its mask key (None = no filter)."""
        rows = rows_of(step["Q"])
        kind = step["kind"]
        if kind in "FD" or (kind in "WAC" and step["masked"]):
            qm = step_query_mask(step)
            return [None if m < 0 else ("m", int(m)) for m in qm]
        if kind == "B":
            return [("c", int(r), bool(step["base"])) for r in rows]
        return [None] * len(rows)

    def topk(self, step):
        """(docs int32 [Q, k], scores float32 [Q, k]) of a search step."""
        Q, T, k = step["Q"], step["T"], step["k"]
        weighted = step["kind"] == "W"
        key = (step["kind"], Q, T, k, step["i"] % 4, step.get("masked"), step.get("base"))
        if key in self._masked:
            return self._masked[key]
        docs = np.full((Q, k), -1, np.int32)
        bits = np.full((Q, k), PAD, np.uint32)
        done = {}
        for i, (r, m) in enumerate(zip(rows_of(Q).tolist(), self.step_masks(step))):
            if (r, m) in done:
                docs[i], bits[i] = docs[done[(r, m)]], bits[done[(r, m)]]
                continue
            o = self.masked(r, T, weighted, m)[:k]
            docs[i, :len(o)] = o
            bits[i, :len(o)] = self.row(r, T, weighted)[o].view(np.uint32)
            done[(r, m)] = i
        docs.setflags(write=False)
        self._masked[key] = (docs, bits.view(np.float32))
        return self._masked[key]

    def list_counts(self, step):
        """Per query of a tile-pass step (F, B, W): the keys its list receives —
        the allowed documents at or above the k-th best of every tile's best
        four allowed keys (all of them when there are fewer than k such keys).
        A list overflows when this exceeds its capacity.  This restates the
        filter passes' own rule (kTileM = 4 keys per tile): it
        checks a diagnostic, not a result, and changes with that rule."""
        Q, T, k = step["Q"], step["T"], step["k"]
        weighted = step["kind"] == "W"
        out = []
        for r, m in zip(rows_of(Q).tolist(), self.step_masks(step)):
            key = (r, T, weighted, m, k)
            if key not in self._counts:
                self._counts[key] = self._list_count(self.masked(r, T, weighted, m), k,
                                                     self.row(r, T, weighted))
            out.append(self._counts[key])
        return out

    def _list_count(self, o, k, row):
        """The keys a list receives from the order o of a row: those at or
        above theta, which filter_theta_kernel's radix select (block_kth,
        bm25mi_filter.hip) takes from the tiles' best four keys — the k-th
        best of them, with its lower bytes zero where a digit's bucket held
        exactly the keys still needed (the select stops there: the same
        candidates, but more of the other documents reach the list)."""
        from test_search_after_host import score_keys
        if k > 4 * self.nt:      # fewer than k tile-best keys exist
            return len(o)
        n = min(len(o), max(4096, 16 * k))
        while True:              # a prefix of the order holds the k-th tile-best key early
            tile = o[:n] >> 11
            # rank of each document inside its tile, in the order
            idx = np.argsort(tile, kind="stable")
            first = np.r_[0, np.nonzero(np.diff(tile[idx]))[0] + 1]
            rank = np.empty(n, np.int64)
            rank[idx] = np.arange(n) - np.repeat(first, np.diff(np.r_[first, n]))
            cand = np.nonzero(rank < 4)[0]
            whole = n == len(o)
            if len(cand) >= k:
                keys = ((score_keys(row[o[:n]]).astype(np.uint64) << np.uint64(32))
                        | (np.uint64(0xFFFFFFFF) - o[:n].astype(np.uint64)))
                theta = self._block_kth(keys[cand], k, None if whole else int(keys[-1]))
                if theta is not None:
                    return int((keys >= np.uint64(theta)).sum())
            elif whole:
                return len(o)
            n = min(len(o), 4 * n)

    @staticmethod
    def _block_kth(cand, need, low):
        """block_kth on the candidate keys of a prefix of the order (every key
        above ``low``; None: all of them): the select's result, or None where
        it depends on candidates past the prefix."""
        prefix = 0
        for shift in range(56, -1, -8):
            sel = cand if shift == 56 else cand[((cand ^ np.uint64(prefix)) >> np.uint64(shift + 8))
                                                == 0]
            h = np.bincount(((sel >> np.uint64(shift)) & np.uint64(255)).astype(np.int64),
                            minlength=256)
            above = np.cumsum(h[::-1])                      # keys of the digits 255 .. d
            at = int(np.searchsorted(above, need))          # (enough candidates: it exists)
            digit, x = 255 - at, int(h[255 - at])
            left = need - (int(above[at]) - x)
            prefix |= digit << shift
            if x == left and shift and low is not None and low >= prefix:
                return None      # (the bucket may hold candidates the prefix does not)
            need = left
            if x == left or shift == 0:
                return prefix
        return prefix

    def score_docs(self, step, docs):
        """S: the scores of docs [Q, C] (negative ids: +0.0f)."""
        T, weighted = step["T"], step["weighted"]
        out = np.zeros(docs.shape, np.float32)
        for i, r in enumerate(rows_of(len(docs)).tolist()):
            row = self.row(r, T, weighted)
            out[i] = np.where(docs[i] >= 0, row[np.maximum(docs[i], 0)], np.float32(0))
        return out

    def s_docs(self, steps, step):
        """The documents S step scores: the first S_COLS of the previous
        search's expected result (what it returned, once that step passed),
        padding ids and both ends of the collection."""
        src = docs_source(steps, step["i"])
        d = self.topk(src)[0][:, :S_COLS]
        d = d[np.arange(step["Q"]) % len(d)]  # (one row per query of the S step)
        tail = np.tile(np.array([[-1, 0, self.n - 1, -7]], np.int32), (len(d), 1))
        return np.ascontiguousarray(np.concatenate([d, tail], axis=1))

    # ------------------------------------------- the kinds of program2
    def cursors(self, step):
        """A: None (the first page), or (scores float32 [Q], docs int32 [Q])."""
        Q, T, k, how = step["Q"], step["T"], step["k"], step["cursor"]
        if how == "none":
            return None
        a_s, a_d = np.zeros(Q, np.float32), np.full(Q, AFTER_NONE, np.int32)
        for i, (r, m) in enumerate(zip(rows_of(Q).tolist(), self.step_masks(step))):
            o = self.masked(r, T, step["weighted"], m)
            row = self.row(r, T, step["weighted"])
            if how in ("page", "deep"):
                at = (k if how == "page" else DEEP) - 1
                if how == "page" and at >= len(o):
                    a_d[i] = -1          # (page_cursor of a row that ended in padding)
                else:
                    at = min(at, len(o) - 1)
                    a_s[i], a_d[i] = row[o[at]], o[at]
            elif i == 1:
                a_d[i] = -1              # the exhausted row
            elif i % 4:                  # a score between two hits, doc 0: names no hit
                v = row[o[:2048]]
                mid = ((v[:-1].astype(np.float64) + v[1:]) / 2).astype(np.float32)
                ok = np.nonzero((mid < v[:-1]) & (mid > v[1:]))[0]
                ok = ok[ok >= 2]
                a_s[i], a_d[i] = (mid[ok[0]] if len(ok) else np.float32(np.inf)), 0
        return a_s, a_d

    def _after_order(self, step, i, r, m, cur):
        """The masked order of query i strictly after its cursor."""
        from test_search_after_host import score_keys
        o = self.masked(r, step["T"], step["weighted"], m)
        if cur is None or cur[1][i] == AFTER_NONE:
            return o
        if cur[1][i] == -1:
            return o[:0]
        sk = score_keys(self.row(r, step["T"], step["weighted"])[o]).astype(np.int64)
        ck = int(score_keys(np.float32(cur[0][i]).reshape(1))[0])
        after = (sk < ck) | ((sk == ck) & (o > cur[1][i]))
        if not after.any():
            return o[:0]
        at = int(np.argmax(after))
        assert after[at:].all()      # (the order is sorted: what follows a cursor is a tail)
        return o[at:]

    def after(self, step):
        """A: (docs, scores) of the cursor search."""
        key = ("A", step["Q"], step["T"], step["k"], step["i"] % 4, step["cursor"],
               step["weighted"], step["masked"])
        if key not in self._masked:
            Q, k = step["Q"], step["k"]
            docs = np.full((Q, k), -1, np.int32)
            bits = np.full((Q, k), PAD, np.uint32)
            cur = self.cursors(step)
            for i, (r, m) in enumerate(zip(rows_of(Q).tolist(), self.step_masks(step))):
                o = self._after_order(step, i, r, m, cur)[:k]
                docs[i, :len(o)] = o
                bits[i, :len(o)] = self.row(r, step["T"], step["weighted"])[o].view(np.uint32)
            self._masked[key] = (docs, bits.view(np.float32))
        return self._masked[key]

    @staticmethod
    def _collapse_walk(o, groups, per_group, k):
        """The first k documents of the order o kept while their group has room."""
        n = min(len(o), 4 * k + 64)
        while True:
            g = groups[o[:n]]
            idx = np.argsort(g, kind="stable")
            first = np.r_[0, np.nonzero(np.diff(g[idx]))[0] + 1]
            occ = np.empty(n, np.int64)
            occ[idx] = np.arange(n) - np.repeat(first, np.diff(np.r_[first, n]))
            keep = np.nonzero((g < 0) | (occ < per_group))[0]
            if len(keep) >= k or n == len(o):
                return o[keep[:k]]
            n = min(len(o), 4 * n)

    @staticmethod
    def _collapse_rounds(o, groups, per_group, k, p):
        """(rounds, dropped entries) of one row of the engine's loop over pages
        of p (collapse_model.paged_collapsed on the cached order)."""
        seen, n, rounds, dropped, pos = {}, 0, 0, 0, 0
        while True:
            rounds += 1
            at = np.arange(pos, len(o))
            if rounds > 1:
                full = [g for g, c in seen.items() if c >= per_group]
                at = at[~np.isin(groups[o[at]], full)]
            at = at[:p]
            for d in o[at].tolist():
                if n == k:
                    break
                g = int(groups[d])
                if g >= 0:
                    if seen.get(g, 0) >= per_group:
                        dropped += 1
                        continue
                    seen[g] = seen.get(g, 0) + 1
                n += 1
            if n == k or len(at) < p:
                return rounds, dropped
            pos = int(at[-1]) + 1

    def collapsed(self, step, page=None):
        """C: (docs, scores, groups) of the collapsed search, and its
        collapse_stats() at the page in force (None: by the step's opts)."""
        page = collapse_page(step) if page is None else page
        key = ("C", step["Q"], step["T"], step["k"], step["i"] % 4, step["weighted"],
               step["masked"], step["tenant"], step["per_group"], page)
        if key not in self._masked:
            Q, k, pg = step["Q"], step["k"], step["per_group"]
            groups = collapse_groups(step["tenant"])
            docs = np.full((Q, k), -1, np.int32)
            bits = np.full((Q, k), PAD, np.uint32)
            grp = np.full((Q, k), -1, np.int32)
            rounds = []
            for i, (r, m) in enumerate(zip(rows_of(Q).tolist(), self.step_masks(step))):
                o = self.masked(r, step["T"], step["weighted"], m)
                kept = self._collapse_walk(o, groups, pg, k)
                docs[i, :len(kept)] = kept
                bits[i, :len(kept)] = self.row(r, step["T"], step["weighted"])[kept].view(np.uint32)
                grp[i, :len(kept)] = groups[kept]
                rounds.append(self._collapse_rounds(o, groups, pg, k, page))
            stats = {"rounds": max(x for x, _ in rounds),
                     "unfinished_rows": sum(x > 1 for x, _ in rounds),
                     "dropped_entries": sum(d for _, d in rounds),
                     "excluded_rows": sum(x - 1 for x, _ in rounds)}
            self._masked[key] = (docs, bits.view(np.float32), grp, stats)
        return self._masked[key]

    def g_allow(self, step):
        """G: bool [Q, N], the documents each query's composed mask allows —
        clause_allow with min-match, ANDed with the range clauses."""
        from range_model import range_allowed
        rows = rows_of(step["Q"])
        mode = step["mode"]
        mm = step_min_match(step) if mode in ("min_match", "all") else np.ones(len(rows), np.int32)
        allow = np.stack([clause_allow_mm(int(r), bool(step["base"]), int(x))
                          for r, x in zip(rows, mm)])
        if mode in ("all", "sorted"):
            allow &= range_allowed(columns()[step["column"]], *range_clauses(step["column"], rows))
        return allow

    def boolean(self, step):
        """G: a dict of the composed boolean search's outputs — docs, scores,
        ranks (sorted), totals, facets (the modes that ask for them)."""
        from facets_model import facets_want
        from range_model import pack_rows
        from sorted_model import select_want
        key = ("G", step["Q"], step["T"], step["k"], step["i"] % 3, step["mode"], step["base"],
               step["column"], step["sort_column"], step["descending"])
        if key in self._masked:
            return self._masked[key]
        Q, T, k, mode = step["Q"], step["T"], step["k"], step["mode"]
        allow = self.g_allow(step)
        out = {"totals": allow.sum(axis=1).astype(np.int64)}
        if mode in ("facets", "all", "counts"):
            out["facets"] = facets_want(pack_rows(allow), columns()["labels"], N_LABELS)
        docs = np.full((Q, k), -1, np.int32)
        bits = np.full((Q, k), PAD, np.uint32)
        if mode == "sorted":
            ranks, perm = sort_order(step["sort_column"], bool(step["descending"]))
            docs, out["ranks"] = select_want(allow, ranks, perm, k, step_after_ranks(step))
        for i, r in enumerate(rows_of(Q).tolist()):
            row = self.row(r, T, False)
            if mode == "sorted":
                hit = docs[i] >= 0
                bits[i, hit] = row[docs[i, hit]].view(np.uint32)
            else:
                o = self.order(r, T, False)
                o = o[allow[i][o]][:k]
                docs[i, :len(o)] = o
                bits[i, :len(o)] = row[o].view(np.uint32)
        out["docs"], out["scores"] = docs, bits.view(np.float32)
        self._masked[key] = out
        return out

    def stateless(self, step):
        """U: a dict of the stateless call's inputs (host arrays) and outputs."""
        from facets_model import facets_want
        from range_model import pack_rows, range_want
        from sorted_model import select_want
        key = ("U", step["Q"], step["k"], step["i"] % 3, step["mode"], step["base"],
               step["column"], step["descending"])
        if key in self._masked:
            return self._masked[key]
        Q, mode = step["Q"], step["mode"]
        allow = masks()[(np.arange(Q) + step["i"]) % 3]
        out = {"allow": allow, "packed": pack_rows(allow)}
        base = pack_rows(masks()[0:1]) if step["base"] else None   # (mask 0, as term_masks' base)
        if mode == "mask_count":
            out["want"] = allow.sum(axis=1).astype(np.int64)
        elif mode == "facets":
            out["want"] = facets_want(out["packed"], columns()["labels"], N_LABELS)
        elif mode == "range_masks":
            out["clauses"] = range_clauses(step["column"], rows_of(Q))
            out["base"] = base
            out["want"] = range_want(columns()[step["column"]], *out["clauses"], base)
        elif mode == "sorted":
            out["order"] = sort_order(step["column"], bool(step["descending"]))
            out["after"] = step_after_ranks(step)
            out["want"] = select_want(allow, *out["order"], step["k"])
            out["want_after"] = select_want(allow, *out["order"], step["k"], out["after"])
        else:
            out["min_match"] = step_min_match(step)
            out["want"] = pack_rows(np.stack(
                [clause_allow_mm(int(r), bool(step["base"]), int(x))
                 for r, x in zip(rows_of(Q), out["min_match"])]))
        self._masked[key] = out
        return out

    def list_counts2(self, step):
        """list_counts for an A step (the order after each cursor) and for a
        searching G step (the order under each composed mask)."""
        key = ("lists",) + tuple(sorted((n, v) for n, v in step.items()
                                        if n not in ("form", "stream", "opt", "opts", "c")))
        if key in self._counts:
            return self._counts[key]
        out = self._counts[key] = []
        if step["kind"] == "A":
            cur = self.cursors(step)
            for i, (r, m) in enumerate(zip(rows_of(step["Q"]).tolist(), self.step_masks(step))):
                out.append(self._list_count(self._after_order(step, i, r, m, cur), step["k"],
                                            self.row(r, step["T"], step["weighted"])))
        else:
            allow = self.g_allow(step)
            for i, r in enumerate(rows_of(step["Q"]).tolist()):
                o = self.order(r, step["T"], False)
                out.append(self._list_count(o[allow[i][o]], step["k"], self.row(r, step["T"], False)))
        return out

    @staticmethod
    def term_masks(step):
        """M: packed uint32 [Q, W] of the clause rows (base: mask 0, one row)."""
        import bm25mi
        rows = rows_of(step["Q"])
        return bm25mi.pack_mask(np.stack([clause_allow(int(r), bool(step["base"]))
                                          for r in rows]))


@functools.lru_cache(maxsize=None)
def expect(signed, big=False):
    return Expect(signed, big)


# -------------------------------------------------- what a step should launch
def large_lists_apply(step, opts, nonneg, nt=NT):
    """run_search's choice for k > 4096 on an index of nt tiles: the list path
    (large_geom's sample of 8 keys per sample tile must hold 2k keys, or k at
    stride 2) or dense rows."""
    k, T = step["k"], step["T"]
    if not (step.get("large_lists", 1) and k <= K_LIST_MAX and nonneg and opts.get("flat", 1)
            and 1 <= T <= 64):
        return False
    for need in (2, 1):
        for P in (8, 4, 2):
            if nt < 2 * P:
                continue
            G = 8 if nt >= 32 * P else 1
            nS = (nt // (G * P)) * G + min(nt % (G * P), G)
            if nS * 8 >= need * k and (need == 2 or P == 2):
                return True
    return False


def threshold_p(step, opts, tile_bounds, nt=NT):
    """The threshold geometry of a P / H step on nt tiles (search_geom): 0 =
    tile-bound keys, 1 = the exact pass, else the sampling stride."""
    k, T = step["k"], step["T"]
    P = _sample_p(nt, k, 1, opts.get("sample_p", 8))
    if (P > 1 and opts.get("theta_bound", 1) and tile_bounds and 1 <= T <= 16 and nt >= 16 * k):
        return 0
    return P


def uses_flat(step, opts):
    return bool(opts.get("flat", 1)) and 1 <= step["T"] <= 64


# ------------------------------------------------------------------ tests
def test_program_is_deterministic_and_covers_every_pair():
    steps = program()
    program.cache_clear()
    again = program()
    assert steps == again and len(steps) == 82
    kinds = [s["kind"] for s in steps]
    assert kinds[0] == kinds[-1] == "P"
    pairs = set(zip(kinds, kinds[1:]))
    assert pairs == {(a, b) for a in KINDS for b in KINDS} and len(pairs) == 81
    assert {s["Q"] for s in steps} == set(QS)
    assert {s["T"] for s in steps} == set(TS)
    small = {s["k"] for s in steps if s["kind"] in "PFWBH"}
    assert small == set(KS_SMALL)
    for kind in "LD":
        assert {s["k"] for s in steps if s["kind"] == kind and s["k"] > K_MAX} == set(KS_LARGE)
    assert {s["dense_by"] for s in steps if s["kind"] == "D"} == {"option", "k"}
    assert {s["large_lists"] for s in steps if s["kind"] == "L"} == {0, 1}
    assert {s["masked"] for s in steps if s["kind"] == "W"} == {True, False}
    assert {s["weighted"] for s in steps if s["kind"] == "S"} == {True, False}
    for kind in "PLFDWSM":
        assert {s["form"] for s in steps if s["kind"] == kind} == {"host", "device"}, kind
    assert {s["stream"] for s in steps if s["form"] == "device"} == {0, 1, 2}
    seen = {s["opt"] for s in steps if s["opt"]}
    assert {(n, v) for n, v, _ in OPTION_PAIRS} <= seen
    assert steps[-1]["opts"] == {}  # (a second round starts from the same options)
    # consecutive device steps on different streams (order_ws) and on the same
    dev = [(a["stream"], b["stream"]) for a, b in zip(steps, steps[1:])
           if a["form"] == b["form"] == "device" and a["kind"] in SEARCH_KINDS
           and b["kind"] in SEARCH_KINDS]
    assert any(x != y for x, y in dev) and any(x == y for x, y in dev)


def test_program_reaches_the_paths_the_gpu_test_asserts():
    """The shapes and options of the P steps reach, by the geometry rules, the
    tile-bound threshold (a dense non-negative index), a sampled flat search
    and the wave kernel; the fixed P -> P pair has list_cap 4 then 0 at the
    sampled threshold."""
    steps = program()
    P = [s for s in steps if s["kind"] == "P"]
    assert any(threshold_p(s, s["opts"], True) == 0 and uses_flat(s, s["opts"]) for s in P)
    assert any(threshold_p(s, s["opts"], False) > 1 and uses_flat(s, s["opts"]) for s in P)
    assert any(threshold_p(s, s["opts"], False) == 1 and uses_flat(s, s["opts"]) for s in P)
    assert any(s["T"] == 65 for s in P)
    a = next(s for s in P if s["opts"].get("list_cap") == 4)
    b = steps[a["i"] + 1]
    assert b["kind"] == "P" and b["opt"] == ("list_cap", 0) and "list_cap" not in b["opts"]
    for s in (a, b):
        assert (s["Q"], s["T"], s["k"]) == (16, 8, 100) and "sample_p" not in s["opts"]
        assert threshold_p(s, s["opts"], True) > 1
    # at 147 tiles no k > 4096 fits the list path's sample: the program's L steps are
    # served by dense rows; the 1027 tiles of the second fixture serve k = 4097 by lists
    assert not any(large_lists_apply(s, s["opts"], True) for s in steps if s["kind"] == "L")
    assert large_lists_apply({"k": 4097, "T": 8}, {}, True) is False
    assert large_lists_apply({"k": 4097, "T": 8}, {}, True, NT_BIG) is True
    assert large_lists_apply({"k": 4097, "T": 8}, {}, True, 1024) is False
    assert large_lists_apply({"k": 4121, "T": 8}, {}, True, NT_BIG) is False
    for off in ({"flat": 0}, {}):
        step = {"k": 4097, "T": 8 if off else 65, "large_lists": 1}
        assert large_lists_apply(step, off, True, NT_BIG) is False
    assert large_lists_apply({"k": 4097, "T": 8, "large_lists": 0}, {}, True, NT_BIG) is False


def test_fixture_shape():
    ip, ix, dt = reuse_csc()
    assert len(ip) == V + 1 and NT == 147 and N - (NT - 1) * TILE == 993
    df = np.diff(ip)
    assert (df[:V_COMMON] >= N // 15 - 1).all() and (df[:V_COMMON] <= N // 4).all()
    assert (df[V_COMMON:] >= 1).all() and (df[V_COMMON:] <= 300).all()
    assert (dt > 0).all() and dt[:ip[V_COMMON]].max() <= 1.0 and dt.max() <= 9.0
    quarter = (dt * 4 == np.round(dt * 4)).mean()
    assert 0.4 < quarter < 0.6
    assert ix[ip[1] - 1] == N - 1  # the last document has a posting
    sp, sx, sd = reuse_csc(True)
    assert np.array_equal(sp, ip) and np.array_equal(sx, ix)
    assert np.array_equal(np.abs(sd), dt) and (sd[2::3] < 0).all() and (sd[0::3] > 0).all()
    q, w = pools()
    assert q.shape == w.shape == (POOL, T_MAX) and q.max() < V and (q >= -1).all()
    assert (q < 0).any() and np.isnan(w[q < 0]).all() and np.isfinite(w[q >= 0]).all()
    assert (w[q >= 0] < 0).any() and (w[q >= 0] > 0).any()
    assert (q[:, 1] < V_COMMON).all() and (q[:, 4] < V_COMMON).all() and (q[:, 1] >= 0).all()
    allow = masks()
    assert 0.49 < allow[0].mean() < 0.51 and 400 < allow[1].sum() < 800
    assert allow[2].sum() == TILE and allow[2][MASK_TILE * TILE] and not allow[2][MASK_TILE * TILE - 1]
    counts = [int(clause_allow(r, False).sum()) for r in range(POOL)]
    assert min(counts) <= 300 and max(counts) > N // 2 and all(c > 0 for c in counts)


@pytest.mark.parametrize("signed", [False, True])
def test_plain_expectations_are_the_oracle(signed):
    """Every P and L step of the program: the expectation builder's rows are
    oracle.search_c's, docs and score bits."""
    ip, ix, dt = reuse_csc(signed)
    ex = expect(signed)
    seen = set()
    for s in program():
        key = (s["Q"], s["T"], s["k"])
        if s["kind"] not in "PL" or key in seen:
            continue
        seen.add(key)
        docs, scores = ex.topk(s)
        rd, rs = oracle.search_c(N, ip, ix, dt, step_queries(s)[0], s["k"])
        assert np.array_equal(docs, rd), s
        assert np.array_equal(scores.view(np.uint32), rs.view(np.uint32)), s
    assert len(seen) >= 8


def test_short_filtered_rows_are_padded():
    """F and D steps whose k exceeds a mask's allowed documents end in doc
    -1 / score bits 0xFFFFFFFF, as _want (test_gpu_search_filtered) pads them."""
    ex = expect(False)
    allow = masks()
    short = 0
    for s in program():
        if s["kind"] not in "FD":
            continue
        qm = step_query_mask(s)
        n_allowed = np.where(qm < 0, N, allow.sum(axis=1)[np.maximum(qm, 0)])
        if not (n_allowed < s["k"]).any():
            continue
        docs, scores = ex.topk(s)
        for i in np.nonzero(n_allowed < s["k"])[0]:
            assert (docs[i, :n_allowed[i]] >= 0).all() and (docs[i, n_allowed[i]:] == -1).all()
            assert (scores[i, n_allowed[i]:].view(np.uint32) == PAD).all()
        if short < 2:  # the whole step against _want (one lexsort per query: the slow way)
            rows = [ex.row(int(r), s["T"], False) for r in rows_of(s["Q"])]
            wd, ws = _want(rows, s["k"], allow, qm)
            assert np.array_equal(docs, wd)
            assert np.array_equal(scores.view(np.uint32), ws.view(np.uint32))
        short += 1
    assert short >= 2


def test_weighted_and_boolean_expectations_follow_want():
    """A W step with masks and a B step: the cached orders give _want's rows."""
    ex = expect(True)
    steps = program()
    w = next(s for s in steps if s["kind"] == "W" and s["masked"] and s["T"] >= 8 and s["Q"] <= 16)
    q, wt = step_queries(w)
    ip, ix, dt = reuse_csc(True)
    rows = ref_rows(N, ip, ix, dt, q, wt)
    wd, ws = _want(rows, w["k"], masks(), step_query_mask(w))
    docs, scores = ex.topk(w)
    assert np.array_equal(docs, wd) and np.array_equal(scores.view(np.uint32), ws.view(np.uint32))
    b = next(s for s in steps if s["kind"] == "B" and s["Q"] <= 16)
    rows = [ex.row(int(r), b["T"], False) for r in rows_of(b["Q"])]
    allow = np.stack([clause_allow(int(r), bool(b["base"])) for r in rows_of(b["Q"])])
    wd, ws = _want(rows, b["k"], allow, np.arange(b["Q"]))
    docs, scores = ex.topk(b)
    assert np.array_equal(docs, wd) and np.array_equal(scores.view(np.uint32), ws.view(np.uint32))
    # the list model: a list receives at least k keys when k documents are allowed
    for s in (w, b):
        if s["k"] <= K_MAX:
            for c, m, r in zip(ex.list_counts(s), ex.step_masks(s), rows_of(s["Q"]).tolist()):
                n = len(ex.masked(r, s["T"], s["kind"] == "W", m))
                assert min(s["k"], n) <= c <= n


def test_big_fixture_and_its_expectations():
    """The 1027-tile fixture: its last tile holds one document, every tile
    holds postings of the common terms, and the expected rows of a large-k and
    of a small search are oracle.search_c's."""
    ip, ix, dt = reuse_csc(False, True)
    assert NT_BIG == 1027 and N_BIG - (NT_BIG - 1) * TILE == 1 and len(ip) == V + 1
    assert ix[ip[1] - 1] == N_BIG - 1 and (dt > 0).all()
    per_tile = np.bincount(ix[:ip[V_COMMON]] >> 11, minlength=NT_BIG)
    assert per_tile[:-1].min() >= 8 * V_COMMON
    allow = masks(True)
    assert allow.shape == (3, N_BIG) and allow[2].sum() == TILE
    ex = expect(False, True)
    for k in (4097, 100):
        step = {"i": 0, "kind": "L" if k > K_MAX else "P", "Q": 4, "T": 8, "k": k}
        docs, scores = ex.topk(step)
        rd, rs = oracle.search_c(N_BIG, ip, ix, dt, step_queries(step)[0], k)
        assert np.array_equal(docs, rd)
        assert np.array_equal(scores.view(np.uint32), rs.view(np.uint32))
        assert (scores[:, -1] > 0).all()  # (k positive documents: no zero fill)



# ------------------------------------------------- the second program's tests
def _plain(x):
    """A step structure with numpy scalars turned into Python's (their repr
    differs between numpy versions)."""
    if isinstance(x, dict):
        return {str(k): _plain(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return tuple(_plain(v) for v in x)
    return x.item() if isinstance(x, np.generic) else x


def test_first_program_is_unchanged():
    """program() is what it was before program2 existed (the generalised
    kind_walk draws the same numbers)."""
    import hashlib
    assert hashlib.sha256(repr(_plain(program())).encode()).hexdigest() == PROGRAM_DIGEST


def _variation(s):
    kind = s["kind"]
    if kind == "A":
        return kind, s["cursor"], s["weighted"], s["masked"]
    if kind == "C":
        return kind, s["tenant"], s["per_group"], s["weighted"], s["masked"], s["ret_groups"]
    if kind in "GU":
        return kind, s["mode"], s["base"]
    return (kind,)


def test_second_program_is_deterministic_and_covers_every_variation():
    steps = program2()
    program2.cache_clear()
    assert steps == program2() and len(steps) == 82
    kinds = [s["kind"] for s in steps]
    assert kinds[0] == kinds[-1] == "P"
    pairs = set(zip(kinds, kinds[1:]))
    assert pairs == {(a, b) for a in KINDS2 for b in KINDS2} and len(pairs) == 81
    assert {s["Q"] for s in steps} == set(QS) and {s["T"] for s in steps} == set(TS)
    by = lambda kind: [s for s in steps if s["kind"] == kind]
    # A: every cursor, plain and weighted; masked or not; every small k and one k = 4097
    A = by("A")
    assert {(s["cursor"], s["weighted"]) for s in A} == {(c, w) for c in CURSORS for w in (0, 1)}
    assert {s["masked"] for s in A} == {True, False}
    assert {s["k"] for s in A} == set(KS_SMALL) | {K_MAX + 1}
    assert all(s["Q"] <= 16 for s in A if s["k"] > K_MAX)
    assert all(s["Q"] == 16 and s["T"] >= 1 for s in A if s["cursor"] == "mix")
    # C: both layouts with both quotas, every combination of the three switches
    C = by("C")
    assert {(s["tenant"], s["per_group"]) for s in C} == {(t, p) for t in (0, 1) for p in (1, 3)}
    assert [s["tenant"] for s in C] == [c % 2 == 1 for c in range(len(C))]   # they alternate
    assert len({(s["weighted"], s["masked"], s["ret_groups"]) for s in C}) == 8
    assert {s["k"] for s in C} <= set(KS_SMALL) and all(s["Q"] <= 16 for s in C if s["k"] == K_MAX)
    assert any(s["tenant"] and s["k"] > TENANTS * s["per_group"] for s in C)  # second rounds
    # G and U: every mode with and without base (G: host form only)
    G, U = by("G"), by("U")
    assert {s["mode"] for s in G} == set(G_MODES) and {s["mode"] for s in U} == set(U_MODES)
    assert {s["form"] for s in G} == {"host"}
    assert {s["k"] for s in G if s["mode"] == "counts"} == {0}
    assert all(s["k"] > 0 for s in G if s["mode"] != "counts")
    assert {s["column"] for s in G if s["mode"] in ("all", "sorted")} == set(COLUMNS)
    assert {s["base"] for s in U if s["mode"] == "range_masks"} == {True, False}
    assert {s["descending"] for s in U if s["mode"] == "sorted"} == {0, 1}
    # every mode in both forms: nine pairs in the program, all ten with the directed steps
    pairs = {(s["mode"], s["form"]) for s in U}
    assert pairs == {(m, f) for m in U_MODES for f in ("host", "device")} - {("term_masks", "device")}
    assert {(s["mode"], s["form"]) for s in stateless_steps()} == {
        (m, f) for m in U_MODES for f in ("host", "device")}
    # a sorted step (U and G) pages with real cursors: none, a rank, the exhausted one
    for s in [s for s in U + G + list(stateless_steps()) if s["mode"] == "sorted"]:
        a = step_after_ranks(s)
        assert s["kind"] == "G" or {AFTER_NONE, -1} < set(a.tolist()) and (a >= 0).any(), s
        if s["kind"] == "U":
            want = expect(False).stateless(s)
            assert not np.array_equal(want["want"][0], want["want_after"][0])
            assert (want["want_after"][0][2] == -1).all() and (want["want"][0][2] >= 0).any()
    assert any({AFTER_NONE, -1} < set(step_after_ranks(s).tolist()) and s["Q"] >= 16
               for s in G if s["mode"] == "sorted")
    for kind in "ACU":
        assert {s["form"] for s in by(kind)} == {"host", "device"}, kind
    assert {s["stream"] for s in steps if s["form"] == "device"} == {0, 1, 2}
    # the options: every pair, the new ones in force at a step of the kind they act on
    seen = {s["opt"] for s in steps if s["opt"]}
    assert {(n, v) for n, v, _ in OPTION_PAIRS2} <= seen and steps[-1]["opts"] == {}
    assert all(len(s["opts"]) <= 1 for s in steps)
    force = lambda name, ok: any(name in s["opts"] and ok(s) for s in steps)
    assert force("collapse_page", lambda s: s["kind"] == "C" and s["tenant"] and s["k"] == 100)
    assert force("collapse_chunk", lambda s: s["kind"] == "C" and s["tenant"] and s["Q"] > 3)
    assert force("bool_chunk", lambda s: s["kind"] == "G" and s["Q"] > 5 and s["k"] > 0)
    assert force("sorted_bins", lambda s: s["kind"] == "G" and s["mode"] == "sorted")
    assert force("filter_tiles", lambda s: s["kind"] == "A")
    # the old kinds keep program()'s rules
    for kind in "LD":
        assert {s["k"] for s in by(kind) if s["k"] > K_MAX} == set(KS_LARGE)
    assert {s["dense_by"] for s in by("D")} == {"option", "k"}
    assert {s["large_lists"] for s in by("L")} == {0, 1}
    assert {s["form"] for s in by("H")} == {"device"}


def _sample(steps, kind, cost=lambda s: s["Q"] * max(s["k"], 1)):
    """The cheapest step of every variation of a kind."""
    best = {}
    for s in steps:
        if s["kind"] == kind and (_variation(s) not in best or cost(s) < cost(best[_variation(s)])):
            best[_variation(s)] = s
    return list(best.values())


def test_cursor_expectations_are_ref_after():
    """One A step per variation, and the step past kMaxK: Expect.after's rows
    are test_search_after_host.ref_after's on the same score rows, bit for bit."""
    from test_search_after_host import ref_after
    ex = expect(True)
    steps = _sample(program2(), "A") + [s for s in program2() if s["kind"] == "A" and s["k"] > K_MAX]
    assert {s["cursor"] for s in steps} == set(CURSORS)
    for s in steps:
        rows = [ex.row(int(r), s["T"], s["weighted"]) for r in rows_of(s["Q"])]
        qm = step_query_mask(s) if s["masked"] else None
        cur = ex.cursors(s)
        wd, ws = ref_after(rows, s["k"], cur, masks() if s["masked"] else None, qm)
        docs, scores = ex.after(s)
        assert np.array_equal(docs, wd), s
        assert np.array_equal(scores.view(np.uint32), ws.view(np.uint32)), s
        if s["cursor"] == "mix":
            assert cur[1][0] == AFTER_NONE and cur[1][1] == -1 and (docs[1] == -1).all()
            named = np.nonzero(cur[1] == 0)[0]
            assert len(named) >= 8 and np.isfinite(cur[0][named]).sum() >= 4
        if s["cursor"] == "deep":
            assert (cur[1] >= 0).all()


def test_collapsed_expectations_are_ref_collapsed_and_the_paged_loop():
    """One C step per variation: Expect.collapsed's rows and groups are
    collapse_model.ref_collapsed's, and its statistics are those of
    collapse_model.paged_collapsed at the page in force — the figures the GPU
    test holds collapse_stats() against.  A tenant row with k above its 8
    groups' quota takes a second round."""
    from collapse_model import paged_collapsed, ref_collapsed
    ex = expect(False)
    steps = _sample(program2(), "C")
    assert len(steps) >= 8
    two_rounds = 0
    for s in steps:
        rows = [ex.row(int(r), s["T"], s["weighted"]) for r in rows_of(s["Q"])]
        groups = collapse_groups(s["tenant"])
        qm = step_query_mask(s) if s["masked"] else None
        allow = masks() if s["masked"] else None
        want = ref_collapsed(rows, s["k"], groups, s["per_group"], allow, qm, want_groups=True)
        docs, scores, grp, stats = ex.collapsed(s)
        assert np.array_equal(docs, want[0]) and np.array_equal(grp, want[2]), s
        assert np.array_equal(scores.view(np.uint32), want[1].view(np.uint32)), s
        if s["k"] <= 100:        # (the loop's model walks its pages in Python)
            model = {}
            paged = paged_collapsed(rows, s["k"], groups, s["per_group"], collapse_page(s), allow,
                                    qm, want_groups=True, stats=model)
            assert np.array_equal(paged[0], docs) and np.array_equal(paged[2], grp), s
            assert stats == model, (s, stats, model)
            if s["tenant"] and s["k"] > TENANTS * s["per_group"]:
                assert stats["rounds"] >= 2 and stats["unfinished_rows"] > 0, (s, stats)
                two_rounds += 1
    assert two_rounds >= 1
    assert any("collapse_page" in s["opts"] for s in program2() if s["kind"] == "C")


def test_composed_masks_are_the_min_match_and_range_models():
    """One G step per variation: the allowed set behind Expect.boolean is the
    bit-sliced counter of min_match_model on the terms' bitmaps (the any
    clause), the must / must-not / base words, and range_model's rows; totals
    are its popcount.  The sorted rows hold the allowed documents in rank
    order with score_docs' bits and padded tails."""
    from min_match_model import reached_after
    from range_model import pack_rows, range_want
    ex = expect(False)
    must, any_, must_not = clauses()
    word = lambda t: pack_rows(_has(int(t))[None])[0]
    full = pack_rows(np.ones((1, N), bool))[0]
    steps = _sample(program2(), "G")
    assert {s["mode"] for s in steps} == set(G_MODES)
    for s in steps:
        rows = rows_of(s["Q"])
        mm = step_min_match(s) if s["mode"] in ("min_match", "all") else np.ones(len(rows), int)
        want = np.zeros((len(rows), len(full)), np.uint32)
        for i, (r, need) in enumerate(zip(rows.tolist(), mm.tolist())):
            w = pack_rows(masks()[0:1])[0].copy() if s["base"] else full.copy()
            for t in must[r][must[r] >= 0]:
                w &= word(t)
            ids = any_[r][any_[r] >= 0]
            if len(ids) and need > 0:
                w &= (reached_after(need, np.stack([word(t) for t in ids]))
                      if need <= len(ids) else np.uint32(0))
            for t in must_not[r][must_not[r] >= 0]:
                w &= ~word(t)
            want[i] = w
        if s["mode"] in ("all", "sorted"):
            want &= range_want(columns()[s["column"]], *range_clauses(s["column"], rows))
        allow = ex.g_allow(s)
        assert np.array_equal(pack_rows(allow), want), s
        out = ex.boolean(s)
        assert np.array_equal(out["totals"], allow.sum(axis=1))
        assert ("facets" in out) == (s["mode"] in ("facets", "all", "counts"))
        if "facets" in out:
            assert (out["facets"].sum(axis=1) <= out["totals"]).all()
        hit = out["docs"] >= 0
        assert np.take_along_axis(allow, np.maximum(out["docs"], 0), axis=1)[hit].all()
        assert (out["scores"].view(np.uint32)[~hit] == PAD).all()
        if s["mode"] == "sorted":
            r = out["ranks"]
            assert ((np.diff(r, axis=1) > 0) | (r[:, 1:] < 0)).all() and (r[~hit] == -1).all()


def test_document_columns():
    c = columns()
    assert len(np.unique(c["i32"])) == 16 and c["i32"].dtype == np.int32
    assert c["i64"].dtype == np.int64 and c["i64"].max() > 2**32 and c["i64"].min() < -2**32
    assert len(np.unique(c["i64"])) < 0.6 * N
    f = c["f32"]
    assert f.dtype == np.float32 and np.isnan(f).any() and len(np.unique(f[~np.isnan(f)])) < 200
    assert (np.signbit(f) & (f == 0)).any() and (~np.signbit(f) & (f == 0)).any()
    assert (c["labels"] < 0).any() and c["labels"].max() == N_LABELS - 1
    for name in COLUMNS:
        fields, lo, hi = range_clauses(name, np.arange(POOL))
        assert lo.dtype == hi.dtype == c[name].dtype and (fields[:, 0] == 0).all()
        assert (fields[:, 1] == 0).sum() == 4 and (lo[6, 0] > hi[6, 0])
    # min_match 1 is the plain any clause
    for r in range(POOL):
        for base in (False, True):
            assert np.array_equal(clause_allow_mm(r, base, 1), clause_allow(r, base))
