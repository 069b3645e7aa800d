"""The numpy model of the sort-by-field search over doc shards (include/bm25mi.h,
"Sort-by-field search over doc shards"): the expected values of
tests/test_sorted_shards_host.py and tests/test_gpu_sorted_shards.py.  Never
goes through the code under test.

The order key is computed value by value with Python integers from the
header's definition (not with the array arithmetic of bm25mi.sort_keys), the
cursor translation by brute-force counting, the merge by concatenate-and-sort
on (key, doc); the orders and selections of a shard are sorted_model's."""
import numpy as np

from sorted_model import order_want, select_want

PAD_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def key_want(values, descending=False):
    """K(v) of every value: uint64 [n]."""
    v = np.asarray(values)
    out = []
    if v.dtype == np.int32:
        for x in v.tolist():
            u = (x + (1 << 31)) & 0xFFFFFFFF            # (uint32)v ^ 0x80000000
            out.append(0xFFFFFFFF - u if descending else u)
    elif v.dtype == np.int64:
        for x in v.tolist():
            u = (x + (1 << 63)) & 0xFFFFFFFFFFFFFFFF    # (uint64)v ^ (1 << 63)
            out.append(0xFFFFFFFFFFFFFFFF - u if descending else u)
    else:
        assert v.dtype == np.float32
        for bits in np.ascontiguousarray(v).view(np.uint32).tolist():
            if (bits & 0x7FFFFFFF) > 0x7F800000:         # 1. NaN
                out.append(1 << 32)
                continue
            if (bits & 0x7FFFFFFF) == 0:                 # 2. +-0.0
                bits = 0
            u = (~bits) & 0xFFFFFFFF if bits >> 31 else bits | 0x80000000   # 3.
            out.append(0xFFFFFFFF - u if descending else u)                 # 4.
    return np.array(out, np.uint64).reshape(v.shape)


def planes(keys):
    """uint64 keys -> (key_hi, key_lo), uint32 each."""
    k = np.asarray(keys, np.uint64)
    return (k >> np.uint64(32)).astype(np.uint32), (k & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def join(hi, lo):
    return (np.asarray(hi).astype(np.uint32).astype(np.uint64) << np.uint64(32)) \
        | np.asarray(lo).astype(np.uint32).astype(np.uint64)


def keys_of_docs(values, descending, docs, doc_offset=0):
    """What bm25_sort_keys_device writes for global ids ``docs`` on a handle
    over ``values`` at ``doc_offset``: the padding key for ids outside it."""
    docs = np.asarray(docs, np.int64)
    n = len(values)
    local = docs - doc_offset
    ok = (docs >= 0) & (local >= 0) & (local < n)
    out = np.full(docs.shape, PAD_KEY, np.uint64)
    if n:
        out[ok] = key_want(values, descending)[local[ok]]
    return out


def cursor_rank_want(values, descending, doc_offset, after_keys, after_docs):
    """bm25_sort_cursor_device by counting: int32 [M].  after_keys uint64 [M],
    after_docs int [M] (global ids; -1: exhausted; < -1: no cursor)."""
    keys = key_want(values, descending)
    ids = doc_offset + np.arange(len(keys), dtype=np.int64)
    out = np.empty(len(after_docs), np.int32)
    for m, (ak, ad) in enumerate(zip(np.asarray(after_keys, np.uint64).tolist(),
                                     np.asarray(after_docs, np.int64).tolist())):
        if ad < 0:
            out[m] = -1 if ad == -1 else -2
            continue
        c = int(np.count_nonzero((keys < np.uint64(ak)) | ((keys == np.uint64(ak)) & (ids <= ad))))
        out[m] = -2 if c == 0 else c - 1
    return out


def _real_length(docs):
    neg = np.nonzero(np.asarray(docs) < 0)[0]
    return int(neg[0]) if neg.size else len(docs)


def merge_want(lists, k, by=1):
    """lists: W tuples (docs [Q, k'], keys uint64 [Q, k'], ...), padding (doc <
    0) last in every row.  Row q: the real entries concatenated and sorted on
    (tuple[by], doc), the first k, padded with doc -1 / key all ones.  by=1 is
    the contract; by=2 sorts on a third array (the shards' local ranks: the
    merge that does not work)."""
    Q = lists[0][0].shape[0]
    docs = np.full((Q, k), -1, np.int32)
    keys = np.full((Q, k), PAD_KEY, np.uint64)
    for q in range(Q):
        ends = [_real_length(l[0][q]) for l in lists]   # (behind the first doc < 0: never read)
        d = np.concatenate([l[0][q][:n] for l, n in zip(lists, ends)]).astype(np.int64)
        ky = np.concatenate([np.asarray(l[1][q][:n], np.uint64) for l, n in zip(lists, ends)])
        by_ = ky if by == 1 else np.concatenate([l[by][q][:n] for l, n in zip(lists, ends)])
        order = np.lexsort((d, by_))[:k]
        docs[q, :order.size] = d[order]
        keys[q, :order.size] = ky[order]
    return docs, keys


def shard_sorted_lists(values, cuts, k, descending, allowed=None, rows=None, after=None):
    """Every doc shard [cuts[i], cuts[i + 1]) of a column as its own handle:
    the shard's order of its slice, the collection cursor ``after`` = (keys
    uint64 [M], docs [M]) translated to its ranks, the selection at min(k,
    shard documents) under its slice of ``allowed`` (bool [M, n]; None: every
    document, M = rows), padded to k.  Returns W tuples (docs, keys, ranks),
    [M, k] each, docs global."""
    out = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        v = values[lo:hi]
        ranks, perm = order_want(v, descending)
        M = rows if allowed is None else allowed.shape[0]
        ar = None if after is None else cursor_rank_want(v, descending, lo, after[0], after[1])
        ks = min(k, hi - lo)
        d, r = select_want(M if allowed is None else allowed[:, lo:hi], ranks, perm, ks, ar, lo)
        docs = np.full((M, k), -1, np.int32)
        rk = np.full((M, k), -1, np.int32)
        docs[:, :ks], rk[:, :ks] = d, r
        out.append((docs, keys_of_docs(v, descending, docs, lo), rk))
    return out


def select_after_want(values, descending, allowed, k, after=None):
    """The single index: the first k allowed documents strictly after the
    collection cursor (keys uint64 [M], docs [M]) in (K, doc) order — computed
    from the keys alone, without ranks.  Returns (docs, keys) [M, k]."""
    keys = key_want(values, descending)
    n = len(keys)
    ids = np.arange(n, dtype=np.int64)
    order = np.lexsort((ids, keys))
    M = allowed.shape[0]
    docs = np.full((M, k), -1, np.int32)
    out = np.full((M, k), PAD_KEY, np.uint64)
    for m in range(M):
        elig = allowed[m].copy()
        if after is not None:
            ak, ad = np.uint64(after[0][m]), int(after[1][m])
            if ad == -1:
                continue
            if ad >= 0:
                elig &= (keys > ak) | ((keys == ak) & (ids > ad))
        sel = order[elig[order]][:k]
        docs[m, :sel.size] = sel
        out[m, :sel.size] = keys[sel]
    return docs, out


def seven_valued(dtype, n=5000, seed=3):
    """A column of about seven distinct values spread over every document, so
    ties cross every cut; the values sit at the type's edges."""
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.float32:
        vals = np.array([np.nan, -np.inf, -1.5, -0.0, 0.0, 2.25, np.inf], np.float32)
    else:
        info = np.iinfo(dtype)
        vals = np.array([info.min, info.min + 1, -1, 0, 1, info.max - 1, info.max], dtype)
    return vals[rng.integers(0, len(vals), n)]
