"""The numpy model of the facet counts (include/bm25mi.h, "Facet counts:"), the
expected values of tests/test_facets_host.py and tests/test_gpu_facets.py: per
row, the packed words unpacked to bool over the first n_docs bits, then
np.bincount of the in-range groups of the allowed documents.  Never goes through
the code under test."""
import numpy as np


def unpack_rows(packed, n_docs):
    """Packed uint32 [M, W] -> bool [M, n_docs] (bits at or past n_docs dropped)."""
    packed = np.ascontiguousarray(packed, dtype=np.uint32)
    if packed.shape[1] == 0:
        return np.zeros((packed.shape[0], 0), bool)
    bits = np.unpackbits(packed.view(np.uint8), axis=1, bitorder="little")
    return bits[:, :n_docs].astype(bool)


def facets_want(packed, groups, G):
    """int64 [M, G]: out[m][g] = allowed documents of row m with groups[d] == g."""
    groups = np.asarray(groups).astype(np.int64)
    allowed = unpack_rows(packed, groups.shape[0])
    ok = (groups >= 0) & (groups < G)
    out = np.zeros((allowed.shape[0], G), np.int64)
    for m in range(allowed.shape[0]):
        out[m] = np.bincount(groups[allowed[m] & ok], minlength=G)[:G] if G else 0
    return out
