"""Candidate lists of exact length for the top-k selection stage
(csrc/bm25mi_kernels.hip: merge_fast_kernel, merge_tail_kernel,
merge_first_kernel) — a plain helper module, no fixtures and no tests.

The lever.  A single-term query on a dense, non-negative index whose values
are f16 numbers runs, under theta_bound, with the tile-bound threshold:
bound_keys_kernel sets theta to (v_k, weakest doc), v_k the k-th largest of
the term's per-tile maxima (build_bmax_kernel: exact for f16 values), and the
REST pass lists every document scoring >= v_k.  merge_fast_kernel reads that
list alone.  So a term whose documents of score >= v_k number ``cnt`` gives
the selection stage a list of exactly ``cnt`` keys:

  * the list documents lie in exactly k "anchor" tiles (k = 1: all of them
    tie, over as many tiles as they need), one of which holds nothing but one
    document of the lowest list score — that tile's maximum is v_k;
  * the anchor tiles lie in distinct groups of 4 tiles, so the pooled bounds
    (pool_bounds_kernel, option bound_pool) give the same v_k;
  * "noise" postings one f16 step below v_k sit in other tiles and inside
    some anchor tiles: one step above theta's edge, they must stay out.

What the model does not fix is the ORDER of the list: the REST pass appends
with atomics.  The selection's provisional thresholds (fast_merge_one<8>,
block_long_merge, long_merge_sampled) sample list positions, so which of
their two outcomes a query takes depends on that order; `route` names the
kernel-level route, which does not.

``list_count`` is the numpy model of cnt, ``route`` mirrors the dispatch of
merge_fast_kernel / select_s, ``grid`` is the case table of the tests.
"""
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from test_bounds_model import TILE, _f16_down

POOL = 4                 # kPool
FAST_MAX_K = 1024        # kFastMaxK: merge_fast_kernel serves k <= this
MERGE_P = 8192           # kMergeP: keys of a block merge's LDS buffer
BLOCK_LONG_MIN = 512     # kBlockLongMin
FAST_KEYS = 2048         # 64 kFastR: the longest list held in registers

NTILES = 16_400                      # >= 16 k at k = 1025 (search_geom), <= 30720
N_DOCS = NTILES * TILE - 1000        # a partial last tile
LIST_CAP = 32_768                    # the tests' list_cap option: no grid list overflows
SHARD_CUT_TILE = 6_000               # the doc-shard test's cut: 37 % / 63 % of the tiles

BASE = 0x2000            # f16 bits of the lowest list score (2^-7); noise is BASE - 1
MID = BASE + 0x800       # pattern d with keys below the k-th score: the tied score

PATTERNS = "abcde"


def f16_bits(bits) -> np.ndarray:
    """f16 bit patterns -> the float32 values (positive f16 order as their bits)."""
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float32)


@dataclass
class Case:
    k: int
    cnt: int                 # intended list length (documents scoring >= v_k)
    pattern: str             # a..e, or "zf" (fewer than k positive tiles: zero fill)
    ge: Optional[int] = None  # pattern d: keys at or above the k-th score (default: all)
    term: int = -1
    seed: int = 0
    docs: np.ndarray = field(default=None, repr=False)
    vals: np.ndarray = field(default=None, repr=False)


def _spread(rng, tiles, tot, n_docs):
    """tot[j] distinct documents in tile tiles[j] (ascending), evenly strided
    from a random start: (docs ascending, index of each doc's tile)."""
    sz = np.minimum(TILE, n_docs - tiles * TILE)
    step = np.maximum((sz - 1) // np.maximum(tot, 1), 1)
    assert np.all((tot - 1) * step < sz)
    r = rng.integers(0, sz - (tot - 1) * step)
    tj = np.repeat(np.arange(len(tiles)), tot)
    first = np.cumsum(tot) - tot
    i = np.arange(int(tot.sum())) - first[tj]
    return tiles[tj] * TILE + r[tj] + i * step[tj], tj, i


def case_postings(c: Case, ntiles=NTILES, n_docs=N_DOCS, noise_tiles=48):
    """The postings (docs ascending int32, values float32) of one term whose
    list at c.k holds exactly c.cnt documents."""
    rng = np.random.default_rng(c.seed)
    k, cnt, groups = c.k, c.cnt, (ntiles + POOL - 1) // POOL
    if c.pattern == "zf":
        # cnt positive documents in fewer than k tiles (k = 1: none at all)
        nt = 0 if cnt == 0 else min(k - 1, 2)
        assert (cnt == 0) == (nt == 0)
        tiles = np.sort(rng.choice(ntiles - 1, nt, replace=False)).astype(np.int64)
        tot = np.full(nt, cnt // max(nt, 1), np.int64)
        tot[:cnt - int(tot.sum())] += 1
        docs, _, _ = _spread(rng, tiles, tot, n_docs)
        return docs.astype(np.int32), f16_bits(BASE + rng.integers(0, 8, len(docs)))
    assert cnt >= k >= 1 and c.pattern in PATTERNS
    if k == 1:  # v_1 is the largest maximum: every list document ties at it
        assert c.pattern == "a"
        na = -(-cnt // 512)
    else:
        na = k
    g = np.sort(rng.choice(np.arange(1, groups - 1), na, replace=False))
    tiles = (g * POOL + rng.integers(0, POOL, na)).astype(np.int64)
    if c.pattern == "b":
        tiles[0] = 0             # the lowest document: the index's first tile
    if c.pattern == "c":
        tiles[-1] = ntiles - 1   # ... its last (partial) tile
    # the designated tile: one list document, the lowest
    jd = {"b": 0, "c": na - 1}.get(c.pattern, int(rng.integers(na)))
    lst = np.zeros(na, np.int64)
    if k == 1:
        lst[:] = cnt // na
        lst[:cnt - int(lst.sum())] += 1
    else:
        others = np.arange(na) != jd
        lst[jd] = 1
        lst[others] = (cnt - 1) // (na - 1)
        lst[np.nonzero(others)[0][:(cnt - 1) % (na - 1)]] += 1
    assert lst.sum() == cnt and lst.min() >= 1
    extra = np.zeros(na, np.int64)   # one noise document inside some anchor tiles
    extra[rng.choice(na, min(na, 3), replace=False)] = 1
    docs, tj, i = _spread(rng, tiles, lst + extra, n_docs)
    noise_slot = rng.integers(0, lst + extra)
    is_noise = (extra[tj] > 0) & (i == noise_slot[tj])
    ld = docs[~is_noise]                       # the list documents, ascending
    pd = int(np.nonzero(tj[~is_noise] == jd)[0][0])  # the designated one's position
    p = np.arange(cnt)
    if c.pattern == "a":
        bits = np.full(cnt, BASE)
    elif c.pattern == "b":
        bits = BASE + p
    elif c.pattern == "c":
        bits = BASE + (cnt - 1 - p)
    elif c.pattern == "d":
        ge = cnt if c.ge is None else c.ge
        assert k - 1 < ge <= cnt
        rest = rng.permutation(np.delete(p, pd))
        tie = BASE if ge == cnt else MID
        bits = np.full(cnt, tie)
        bits[rest[:k - 1]] = MID + 1 + rng.permutation(k - 1)
        if ge < cnt:  # keys below the k-th score: the designated one and cnt - ge - 1 more
            low = rest[k - 1:k - 1 + cnt - ge - 1]
            bits[low] = BASE + rng.integers(0, 0x700, len(low))
            bits[pd] = BASE
    else:
        bits = BASE + rng.integers(0, max(2, cnt // 3), cnt)
        bits[pd] = BASE
    assert bits.min() == BASE and bits[pd] == BASE and bits.max() < 0x7C00
    # noise tiles outside the anchors
    nz = np.setdiff1d(rng.choice(ntiles, noise_tiles, replace=False), tiles)
    nzd = nz * TILE + rng.integers(0, np.minimum(TILE, n_docs - nz * TILE))
    alld = np.concatenate([ld, docs[is_noise], nzd])
    allb = np.concatenate([bits, np.full(len(alld) - cnt, BASE - 1)])
    o = np.argsort(alld, kind="stable")
    assert np.all(np.diff(alld[o]) > 0)
    return alld[o].astype(np.int32), f16_bits(allb[o])


# ---------------------------------------------------------------- the model
def tile_bounds(docs, vals, ntiles=NTILES, pool=False) -> np.ndarray:
    """The term's tile bounds: per-tile maxima rounded down to f16
    (build_bmax_kernel), pooled over groups of 4 tiles (pool_bounds_kernel)."""
    m = np.zeros(ntiles, np.float32)
    np.maximum.at(m, np.asarray(docs, np.int64) // TILE, vals)
    lb = _f16_down(m)
    if pool:
        ng = (ntiles + POOL - 1) // POOL
        lb = np.pad(lb, (0, ng * POOL - ntiles)).reshape(ng, POOL).max(axis=1)
    return lb


def row_model(docs, vals, k, ntiles=NTILES, pool=False) -> dict:
    """What the selection stage sees of a single-term query at k: the length
    of its list, the keys tied at / above the k-th best score, and whether
    the threshold is the zero-fill one (fewer than k positive tiles)."""
    lb = np.sort(tile_bounds(docs, vals, ntiles, pool))[::-1]
    vk = lb[k - 1] if k <= len(lb) else np.float32(0)
    zf = not vk > 0
    lst = vals[vals > 0] if zf else vals[vals >= vk]
    s = np.sort(lst)[::-1]
    kth = s[k - 1] if len(s) >= k else None
    return {"cnt": len(s), "zero_fill": zf, "v_k": float(vk),
            "ties_at_kth": 0 if kth is None else int((s == kth).sum()),
            "above_kth": len(s) if kth is None else int((s > kth).sum())}


def list_count(postings, k, ntiles=NTILES, pool=False) -> int:
    """Tile maxima -> f16 rounded down -> the k-th largest -> the documents
    scoring at least that (every positive one when it is zero)."""
    return row_model(postings[0], postings[1], k, ntiles, pool)["cnt"]


def shard_models(docs, vals, k, cut_tiles, ntiles=NTILES):
    """row_model per doc shard under the two-half protocol (tile-bound keys,
    theta_wave_kernel): theta is the k-th best TILE key of the collection —
    (v_k, the last document L of the k-th tile by (bound desc, tile asc)) —
    so a shard lists its documents scoring > v_k, or v_k with an id <= L."""
    lb = tile_bounds(docs, vals, ntiles)
    order = np.lexsort((np.arange(ntiles), -lb))
    pos = int((lb > 0).sum())
    docs = np.asarray(docs, np.int64)
    edges = [0] + [t * TILE for t in cut_tiles] + [ntiles * TILE]
    out = []
    for lo, hi in zip(edges[:-1], edges[1:]):
        inb = (docs >= lo) & (docs < hi)
        if pos < k:
            keep = inb & (vals > 0)
        else:
            jt = int(order[k - 1])
            vk, L = lb[jt], (jt + 1) * TILE - 1
            keep = inb & ((vals > vk) | ((vals == vk) & (docs <= L)))
        s = np.sort(vals[keep])[::-1]
        kth = s[k - 1] if len(s) >= k else None
        out.append({"cnt": len(s), "zero_fill": pos < k,
                    "ties_at_kth": 0 if kth is None else int((s == kth).sum()),
                    "above_kth": len(s) if kth is None else int((s > kth).sum())})
    return out


# ---------------------------------------------------------------- the mirror
ROUTES = (
    "fallback",             # cnt > C: the exact fallback stage
    "block_long",           # ws.slow -> merge_tail_kernel: block_long_merge, else merge_first_one
    "tail_merge_first",     # ws.slow, more than kMergeP keys: merge_first_one's chunked sort
    "long_sampled",         # long_merge_one: long_merge_sampled serves it (lds_merge_one)
    "long_digits",          # ... the four 8-bit digit passes
    "long_giveup",          # ... more than 1024 keys at or above the k-th score -> ws.slow
    "zero_fill",            # zero-fill theta, cnt < k -> ws.slow (merge_first_one fills)
    "fast4",                # fast_merge_one<4>: the whole list sorted in registers
    "fast8_provisional",    # fast_merge_one<8>, k <= 128: provisional threshold, else wave_kth_key
    "fast8_regs4", "fast8_lds",     # fast_merge_one<8>, k > 128: wave_kth_key + sort_write_any
    "fast16_regs4", "fast16_lds",   # fast_merge_one<16>
    "fast32_regs4", "fast32_lds",   # fast_merge_one<32>
    "fast16_regs2", "fast32_regs2",  # ... at k <= 128: only under the zero-fill threshold
    "shard4", "shard8", "shard16", "shard32",  # a doc shard's list: wave_kth_key, no sort
    "merge_first",          # k > 1024: merge_first_kernel (topk_compact)
    "merge_first_chunked",  # ... more than kMergeP survivors: topk_of's chunked sort
)
# the routes that pass through ws.slow, which search_stats()["block_merge_queries"] counts
BLOCK_MERGE_ROUTES = {"block_long", "tail_merge_first", "long_giveup", "zero_fill"}


def _sampled_serves(cnt, k):
    """long_merge_sampled: every s-th list key sampled (<= 1024), t1 = the
    ceil(2k / s)-th best sample key, served when k..1024 list keys reach t1.
    On a list in ascending or descending order those number (want - 1) s + 1
    .. want s, in random order about want s (a few % either way): decided
    here only with 10 % to spare, else the case is not one a test may use."""
    s = -(-cnt // 1024)
    ns, want = -(-cnt // s), min(-(-2 * k // s), 1024)
    if ns <= want:  # the sample holds no more: t1 = 0, the whole list reaches it
        return False
    lo, hi = (want - 1) * s + 1, want * s
    if lo >= k and hi * 1.1 <= FAST_MAX_K:
        return True
    if lo * 0.9 > FAST_MAX_K:
        return False
    raise ValueError(f"cnt={cnt} k={k}: long_merge_sampled's outcome depends on the list order")


def route(cnt, k, ties_at_kth, unsorted, C, above_kth=None, zero_fill=False):
    """The route of a list of cnt keys through the selection stage at k
    (merge_fast_kernel's dispatch, select_s for k > 1024).  ties_at_kth: the
    keys whose score equals the k-th best score; above_kth: those above it
    (default k - 1: the tie group starts at rank k); unsorted: a doc shard's
    list for the W-way merge; C: the list capacity (list_cap_for)."""
    above = k - 1 if above_kth is None else above_kth
    if cnt > C:
        return "fallback"
    if k > FAST_MAX_K:
        return "merge_first_chunked" if cnt > MERGE_P else "merge_first"
    block_long = ((cnt > 1024 or (cnt > BLOCK_LONG_MIN and not unsorted)) and k <= 128
                  and not zero_fill)
    if block_long:
        return "block_long" if cnt <= MERGE_P else "tail_merge_first"
    if cnt > FAST_KEYS:
        if _sampled_serves(cnt, k):
            return "long_sampled"
        return "long_giveup" if above + ties_at_kth > FAST_MAX_K else "long_digits"
    if zero_fill and cnt < k:
        return "zero_fill"
    nj = (cnt + 63) >> 6
    R = 4 if nj <= 4 else 8 if nj <= 8 else 16 if nj <= 16 else 32
    if unsorted:
        return f"shard{R}"
    if R == 4:
        return "fast4"
    if R == 8 and k <= 128:
        return "fast8_provisional"
    n = min(cnt, k)
    return f"fast{R}_" + ("regs2" if n <= 128 else "regs4" if n <= 256 else "lds")


def model_route(m: dict, k, unsorted=False, C=LIST_CAP):
    return route(m["cnt"], k, m["ties_at_kth"], unsorted, C, above_kth=m["above_kth"],
                 zero_fill=m["zero_fill"])


# ---------------------------------------------------------------- the grid
KS = (1, 64, 100, 128, 129, 256, 300, 600, 1024, 1025)


def grid_specs():
    """(k, cnt, pattern, ge) of every case.  k = 1 has pattern a only: v_1
    is the largest tile maximum, so every list document ties at it.  The
    orders under which fast_merge_one<8>'s first-128-keys threshold keeps
    fewer than k keys (pattern c, k = 128, cnt = 257, the list in doc order:
    96 keys) or more than 256 (pattern b, k = 64, cnt = 512: 409 keys) are in
    the grid; whether a run takes them is the REST pass's append order."""
    out = []
    for k in (1, 64, 100, 128):
        cnts = sorted({c for c in (k, k + 1, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048,
                                   2049, 8192, 8193) if c >= k})
        out += [(k, c, p, None) for c in cnts for p in (PATTERNS if k > 1 else "a")]
        # zero fill: fewer positive documents than k (block merge), and (k > 1:
        # two positive tiles) at least k of them — the wave routes under the
        # zero-fill threshold, which block_long leaves alone
        out.append((k, min(k - 1, 3), "zf", None))
        if k > 1:
            out += [(k, c, "zf", None) for c in (k + 5, 600, 1500, 2500)]
    for k in (129, 256, 300, 600, 1024):
        # (k = 600 is this module's own: 512 < k < 1024, where long_merge_sampled
        # cannot serve a long list and the digit passes always run)
        cnts = (2049, 5000) if k == 600 else \
            sorted({c for c in (k, k + 1, 512, 513, 1024, 1025, 2048, 2049, 5000) if c >= k})
        out += [(k, c, p, None) for c in cnts for p in PATTERNS]
        out.append((k, 3000, "a", None))      # every key ties at the k-th score
        out.append((k, 3000, "d", 1024))      # 1024 keys at or above the k-th score
        out.append((k, 3000, "d", 1025))      # ... 1025: one too many for the wave's slice
        out.append((k, 3, "zf", None))
    for k in (1025,):
        out += [(k, c, p, None) for c in (1025, 1026, 8192, 8193, 20000) for p in PATTERNS]
        out.append((k, 3, "zf", None))
    return out


def make_cases(specs, ntiles=NTILES, n_docs=N_DOCS, seed=2024):
    """Cases with postings, one term each, in spec order."""
    cases = []
    for t, (k, cnt, pattern, ge) in enumerate(specs):
        c = Case(k, cnt, pattern, ge, term=t, seed=seed + t)
        c.docs, c.vals = case_postings(c, ntiles, n_docs)
        cases.append(c)
    return cases


_GRID = None


def grid():
    global _GRID
    if _GRID is None:
        _GRID = make_cases(grid_specs())
    return _GRID


def csc_of(cases):
    """(indptr int64, indices int32, data float32) of the cases' terms."""
    indptr = np.zeros(len(cases) + 1, np.int64)
    np.cumsum([len(c.docs) for c in cases], out=indptr[1:])
    return (indptr, np.concatenate([c.docs for c in cases]).astype(np.int32),
            np.concatenate([c.vals for c in cases]).astype(np.float32))


def batch_of(cases, k, T=4):
    """The query batch of k: one row per case (its term, padded to T with
    -1) and an all-padding row last."""
    rows = [c for c in cases if c.k == k]
    q = np.full((len(rows) + 1, T), -1, np.int32)
    q[:len(rows), 0] = [c.term for c in rows]
    return rows, q


def slice_docs(cases, lo, hi):
    """The CSC of documents [lo, hi) of the cases' terms, local doc ids."""
    parts = [(c.docs[(c.docs >= lo) & (c.docs < hi)] - lo, c.vals[(c.docs >= lo) & (c.docs < hi)])
             for c in cases]
    indptr = np.zeros(len(cases) + 1, np.int64)
    np.cumsum([len(d) for d, _ in parts], out=indptr[1:])
    return (indptr, np.concatenate([d for d, _ in parts]).astype(np.int32),
            np.concatenate([v for _, v in parts]).astype(np.float32))
