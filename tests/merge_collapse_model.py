"""The numpy reference of the doc-shard merge of collapsed lists
(bm25_merge_collapsed_device) and the pieces its CPU and GPU tests share.

ref_merge_collapsed is the contract of include/bm25mi.h read literally: the
real entries of the lists concatenated, ordered by (score_keys descending, doc
ascending) and walked once with a counter per group.  shard_lists cuts a
single-index fixture into doc shards and returns each shard's collapsed list
(ref_collapsed with doc_offset = the cut), which is what the merge is fed by
bm25mi.dist.sharded_search_collapsed; tests/test_merge_collapsed_host.py holds
the merge of those against ref_collapsed on the whole."""
import numpy as np

from test_gpu_edges import TILE
from test_search_after_host import PAD, score_keys

# unaligned cuts of the 5000-document fixture; the sets of 3 and 5 shards hold
# 2048, so the tie pair 2047 / 2048 of one group (collapse_model.tie_groups)
# straddles shards
CUTS = {2: (0, 3001, 5000), 3: (0, 1111, TILE, 5000), 5: (0, 37, 1111, TILE, 3333, 5000)}


def real_length(docs):
    """Entries before the first doc < 0 of one list."""
    neg = np.nonzero(np.asarray(docs) < 0)[0]
    return int(neg[0]) if neg.size else len(docs)


def ref_merge_collapsed(lists, k, per_group, collapse=True):
    """lists: W tuples (docs [Q, k], scores [Q, k] float32, groups [Q, k]),
    each row best-first with padding (doc < 0) last.  Row q: the lists' real
    entries in (score_keys desc, doc asc) order, walked with a counter per
    group (a group < 0: always kept), the first k kept, padded with doc -1 /
    score bits 0xFFFFFFFF / group -1.  collapse=False: the plain merge."""
    Q = lists[0][0].shape[0]
    docs = np.full((Q, k), -1, np.int32)
    bits = np.full((Q, k), PAD, np.uint32)
    grp = np.full((Q, k), -1, np.int32)
    for q in range(Q):
        d, s, g = [], [], []
        for ld, ls, lg in lists:
            n = real_length(ld[q])
            d.append(ld[q, :n])
            s.append(np.ascontiguousarray(ls[q, :n], np.float32).view(np.uint32))
            g.append(lg[q, :n])
        d, s, g = np.concatenate(d), np.concatenate(s), np.concatenate(g)
        order = np.lexsort((d, -score_keys(s.view(np.float32)).astype(np.int64)))
        seen, n = {}, 0
        for i in order:
            if n == k:
                break
            gi = int(g[i])
            if collapse and gi >= 0:
                if seen.get(gi, 0) >= per_group:
                    continue
                seen[gi] = seen.get(gi, 0) + 1
            docs[q, n], bits[q, n], grp[q, n] = d[i], s[i], gi
            n += 1
    return docs, bits.view(np.float32), grp


def shard_lists(rows, cuts, k, groups, per_group, allow=None, query_mask=None):
    """The collapsed list of every doc shard [cuts[i], cuts[i + 1]) of the
    fixture whose dense score rows are ``rows``: ref_collapsed on the shard's
    slice of the rows, groups and masks at min(k, shard documents), padded to
    k, with global doc ids."""
    from collapse_model import ref_collapsed
    out = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        ks = min(k, hi - lo)
        part = ref_collapsed([r[lo:hi] for r in rows], ks, groups[lo:hi], per_group,
                             None if allow is None else allow[:, lo:hi], query_mask, lo, True)
        d = np.full((len(rows), k), -1, np.int32)
        s = np.full((len(rows), k), PAD, np.uint32)
        g = np.full((len(rows), k), -1, np.int32)
        d[:, :ks], s[:, :ks], g[:, :ks] = part[0], part[1].view(np.uint32), part[2]
        out.append((d, s.view(np.float32), g))
    return out


def shard_csc(indptr, indices, data, lo, hi):
    """The CSC index of the documents [lo, hi), ids relative to lo."""
    indptr = np.asarray(indptr, np.int64)
    ip, ix, dt = [0], [], []
    for t in range(len(indptr) - 1):
        a, b = indptr[t], indptr[t + 1]
        sel = (indices[a:b] >= lo) & (indices[a:b] < hi)
        ix.append(indices[a:b][sel] - lo)
        dt.append(data[a:b][sel])
        ip.append(ip[-1] + int(sel.sum()))
    return (np.array(ip, np.int64), np.concatenate(ix).astype(np.int32),
            np.concatenate(dt).astype(np.float32))


def same3(a, b):
    return (np.array_equal(a[0], b[0])
            and np.array_equal(np.ascontiguousarray(a[1]).view(np.uint32),
                               np.ascontiguousarray(b[1]).view(np.uint32))
            and np.array_equal(a[2], b[2]))
