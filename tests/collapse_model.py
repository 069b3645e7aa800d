"""The numpy reference of field collapsing (bm25_search_collapsed) and a numpy
restatement of the engine's loop, with the group layouts the tests share.

ref_collapsed is the contract of include/bm25mi.h read literally: the full
result order of a row (tests/test_search_after_host.py: ordered, on the C
oracle's dense rows or the weighted numpy fold) walked from rank 1 with a
counter per group value.  paged_collapsed is how the engine gets there: pages
of p results from ref_after, over-quota entries dropped, the cursor moved, and
from round 2 the documents of saturated groups excluded from the row's mask.
tests/test_search_collapsed_host.py holds the two against each other."""
import functools

import numpy as np

from test_gpu_edges import TILE
from test_search_after_host import AFTER_NONE, PAD, ordered, ref_after, score_keys

MAX_K = 4096


def _allowed(allow, query_mask, r, n_docs):
    m = -1 if allow is None else 0 if query_mask is None else int(query_mask[r])
    return np.ones(n_docs, bool) if m < 0 else np.asarray(allow[m], bool)


def ref_collapsed(rows, k, groups, per_group, allow=None, query_mask=None, doc_offset=0,
                  want_groups=False):
    """rows: the queries' dense score rows; groups int [n_docs] (< 0: no
    group); allow / query_mask / doc_offset as ref_after.  Each row: its full
    order walked with a counter per group, the first k kept, padded with doc
    -1 / score bits 0xFFFFFFFF / group -1."""
    Q = len(rows)
    docs = np.full((Q, k), -1, np.int32)
    bits = np.full((Q, k), PAD, np.uint32)
    grp = np.full((Q, k), -1, np.int32)
    for r, row in enumerate(rows):
        seen, n = {}, 0
        for d in ordered(row, _allowed(allow, query_mask, r, len(row))):
            if n == k:
                break
            g = int(groups[d])
            if g >= 0:
                if seen.get(g, 0) >= per_group:
                    continue
                seen[g] = seen.get(g, 0) + 1
            docs[r, n] = d + doc_offset
            bits[r, n] = row[d:d + 1].view(np.uint32)[0]
            grp[r, n] = g
            n += 1
    out = (docs, bits.view(np.float32))
    return out + (grp,) if want_groups else out


def paged_collapsed(rows, k, groups, per_group, page, allow=None, query_mask=None, doc_offset=0,
                    want_groups=False, stats=None):
    """The loop of bm25_search_collapsed in numpy: per row, pages of ``page``
    results (ref_after), each walked in rank order against the groups' counts;
    the next page starts after the last entry of this one and, from round 2,
    under the row's mask minus the documents of saturated groups.  stats (a
    dict) receives the rounds (the most any row took), the rows unfinished
    after round 1, the dropped entries and the row-rounds under exclusion."""
    Q = len(rows)
    groups = np.asarray(groups)
    docs = np.full((Q, k), -1, np.int32)
    bits = np.full((Q, k), PAD, np.uint32)
    grp = np.full((Q, k), -1, np.int32)
    rounds = [0] * Q
    dropped = 0
    for r, row in enumerate(rows):
        own = _allowed(allow, query_mask, r, len(row))
        p = max(1, min(page, len(row), MAX_K))
        seen, n, after = {}, 0, None
        while k > 0:
            rounds[r] += 1
            ok = own
            if rounds[r] > 1:
                full = [g for g, c in seen.items() if c >= per_group]
                ok = own & ~np.isin(groups, full)
            pd, ps = ref_after([row], p, after, ok[None], None, doc_offset)
            assert rounds[r] <= k + 1, "a row takes at most k + 1 rounds"
            kept = 0
            for d, s in zip(pd[0], ps[0].view(np.uint32)):
                if d < 0 or n == k:
                    break
                g = int(groups[d - doc_offset])
                if g >= 0 and seen.get(g, 0) >= per_group:
                    dropped += 1
                    continue
                if g >= 0:
                    seen[g] = seen.get(g, 0) + 1
                docs[r, n], bits[r, n], grp[r, n] = d, s, g
                n += 1
                kept += 1
            if n == k or pd[0, -1] < 0:
                break
            assert rounds[r] == 1 or kept >= 1
            after = (ps[:, -1].copy(), pd[:, -1].copy())
    if stats is not None:
        stats["rounds"] = max(rounds, default=1) if k > 0 else 0
        stats["unfinished_rows"] = sum(x > 1 for x in rounds)
        stats["dropped_entries"] = dropped
        stats["excluded_rows"] = sum(x - 1 for x in rounds if x > 1)
    out = (docs, bits.view(np.float32))
    return out + (grp,) if want_groups else out


# ---------------------------------------------------------- group layouts
def uniform_groups(n_docs, seed=11):
    """About n_docs / 4 groups, uniform."""
    rng = np.random.default_rng(seed + n_docs)
    return rng.integers(0, max(1, n_docs // 4), n_docs).astype(np.int32)


def tie_row(rows, k=10):
    """The first row whose first run of >= 3 equal scores lies inside its best
    k results (and off the tile edge), with that run."""
    for r, row in enumerate(rows):
        run = first_tie_run(row)
        if run is None or set(run[:3].tolist()) & {TILE - 1, TILE}:
            continue
        if int(np.nonzero(ordered(row) == run[0])[0][0]) + 2 < k:
            return r, run
    return None, None


def tie_groups(rows, n_docs, seed=11):
    """uniform_groups with the tie run of tie_row arranged so that its first
    two documents share a group (1 000 000) and its third is in another
    (1 500 000), and — where they exist — documents 2047 and 2048 (equal scores
    on row 1: after_case) in one group (2 000 000)."""
    g = uniform_groups(n_docs, seed).copy()
    if n_docs > TILE:
        g[TILE - 1] = g[TILE] = 2_000_000
    r, run = tie_row(rows)
    if r is not None:
        g[run[0]] = g[run[1]] = 1_000_000
        g[run[2]] = 1_500_000
    return g


def first_tie_run(row, allowed=None):
    """The documents of the first run of >= 3 equal scores in the row's order
    (None: no such run)."""
    ids = ordered(row, allowed)
    sk = score_keys(row[ids])
    start = 0
    for i in range(1, len(ids) + 1):
        if i == len(ids) or sk[i] != sk[start]:
            if i - start >= 3:
                return ids[start:i]
            start = i
    return None


def dominated_groups(rows, n_docs, depth, seed=11):
    """One group (7) owns the first ``depth`` results of every row; the other
    documents are spread as uniform_groups (shifted past 7)."""
    g = uniform_groups(n_docs, seed) + 8
    for row in rows:
        g[ordered(row)[:depth]] = 7
    return g.astype(np.int32)


def tenant_groups(n_docs, tenants=8):
    """doc % tenants: a mask of one tenant leaves exactly one group."""
    return (np.arange(n_docs) % tenants).astype(np.int32)


def high_groups(n_docs, seed=11):
    """uniform_groups moved up to end at 2^31 - 1."""
    g = uniform_groups(n_docs, seed).astype(np.int64)
    return (g + (2**31 - 1 - g.max())).astype(np.int32)


def distinct_groups(n_docs):
    return np.arange(n_docs, dtype=np.int32)[::-1].copy()


def negative_groups(n_docs):
    return -1 - (np.arange(n_docs, dtype=np.int32) % 3)


@functools.lru_cache(maxsize=None)
def layouts(n_docs, depth=0):
    """name -> groups of the after_case fixture of n_docs documents (read-only)."""
    from test_search_after_host import after_case
    rows = after_case(n_docs)[4]
    out = {"uniform": tie_groups(rows, n_docs),
           "dominated": dominated_groups(rows, n_docs, depth or min(n_docs, 192)),
           "negative": negative_groups(n_docs),
           "distinct": distinct_groups(n_docs),
           "one": np.zeros(n_docs, np.int32),
           "high": high_groups(n_docs),
           "tenant": tenant_groups(n_docs)}
    for a in out.values():
        a.setflags(write=False)
    return out


__all__ = ["AFTER_NONE", "MAX_K", "PAD", "ref_collapsed", "paged_collapsed", "layouts",
           "uniform_groups", "tie_groups", "tie_row", "first_tie_run", "dominated_groups", "tenant_groups",
           "high_groups", "distinct_groups", "negative_groups"]
