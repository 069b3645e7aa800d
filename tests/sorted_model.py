"""The numpy model of the sort-by-field search (include/bm25mi.h, "Sort-by-field
search:"), the expected values of tests/test_search_sorted_host.py and
tests/test_gpu_search_sorted.py.  Never goes through the code under test.

Order of a column: np.lexsort on (doc, mapped key, NaN flag) — integers as
themselves (descending: the complement of the offset-binary value, so the
limits need no negation), float32 in numeric order with -0.0 folded into +0.0
(descending: negated), NaN after every number in both directions, equal values
by doc id ascending.  Selection: the unpacked mask AND rank > after, the first
k in rank order, padded with doc -1 / rank -1."""
import numpy as np

AFTER_NONE = -2


def order_want(values, descending=False):
    """(ranks, perm), int32 [n] each: perm[r] = the document at rank r."""
    v = np.asarray(values)
    n = v.shape[0]
    doc = np.arange(n)
    if v.dtype.kind == "f":
        assert v.dtype == np.float32
        nan = np.isnan(v)
        key = np.where(nan | (v == 0), np.float32(0), v).astype(np.float64)  # (exact: f32 in f64)
        if descending:
            key = -key
        key = key + 0.0   # (-0.0 + 0.0 = +0.0: the zeros are one value)
    else:
        assert v.dtype in (np.int32, np.int64)
        nan = np.zeros(n, bool)
        key = v.astype(np.int64).view(np.uint64) ^ np.uint64(1 << 63)   # offset binary
        if descending:
            key = ~key
    perm = np.lexsort((doc, key, nan)).astype(np.int32)   # (the last key is the primary one)
    ranks = np.empty(n, np.int32)
    ranks[perm] = np.arange(n, dtype=np.int32)
    return ranks, perm


def select_want(allowed, ranks, perm, k, after=None, doc_offset=0):
    """(docs, ranks) int32 [M, k].  allowed: bool [M, n] (or an int M: every
    document allowed for M rows); after: None or int [M] (-2: no cursor, -1:
    an all-padding row)."""
    ranks, perm = np.asarray(ranks), np.asarray(perm)
    n = ranks.shape[0]
    if isinstance(allowed, (int, np.integer)):
        allowed = np.ones((int(allowed), n), bool)
    allowed = np.asarray(allowed, bool)
    M = allowed.shape[0]
    docs = np.full((M, k), -1, np.int32)
    out = np.full((M, k), -1, np.int32)
    for m in range(M):
        a = AFTER_NONE if after is None else int(after[m])
        if a == -1:
            continue
        elig = allowed[m] & (ranks > (a if a >= 0 else -1)) & (ranks >= 0) & (ranks < n)
        r = np.sort(ranks[elig])[:k]
        docs[m, :r.size] = perm[r] + doc_offset
        out[m, :r.size] = r
    return docs, out
