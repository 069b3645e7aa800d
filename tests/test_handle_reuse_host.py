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
keeps a subsequence of it and a step takes its first k."""
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


def rows_of(Q):
    """Pool rows of a step of Q queries (48: the pool three times)."""
    return np.arange(Q) % POOL


def step_queries(step):
    q, w = pools()
    r = rows_of(step["Q"])
    return np.ascontiguousarray(q[r, :step["T"]]), np.ascontiguousarray(w[r, :step["T"]])


def step_query_mask(step):
    """Mask ids of a filtered step's queries: 0, 1, 2 and -1 (no filter) by
    row, rotated by the step."""
    return ((rows_of(step["Q"]) + step["i"]) % 4 - 1).astype(np.int32)


# ------------------------------------------------------------- the program
def kind_walk(rng):
    """A closed walk over the nine kinds that takes every ordered pair, same-
    kind pairs included, exactly once: an Euler circuit of the complete
    directed graph with loops (81 edges, 82 steps), from P."""
    out = {a: list(rng.permutation(list(KINDS))) for a in KINDS}
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
        if kind in "FD" or (kind == "W" and step["masked"]):
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
                self._counts[key] = self._list_count(self.masked(r, T, weighted, m), k)
            out.append(self._counts[key])
        return out

    def _list_count(self, o, k):
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
            if len(cand) >= k:
                return int(cand[k - 1]) + 1
            if n == len(o):
                return len(o)
            n = min(len(o), 4 * n)

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

