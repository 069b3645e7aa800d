"""The numpy model of the numeric range filters (include/bm25mi.h, "Numeric
range filters:"), the expected values of tests/test_range_masks_host.py and
tests/test_gpu_range_masks.py: per clause (v >= lo) & (v <= hi) in the column's
own dtype, ANDed over the row's clauses with the unpacked base, packed with the
bits at or past n_docs cleared.  Never goes through the code under test."""
import numpy as np

from facets_model import unpack_rows


def pack_rows(allow):
    """bool [M, n_docs] -> packed uint32 [M, W], bits at or past n_docs 0."""
    allow = np.asarray(allow, bool)
    M, n = allow.shape
    W = (n + 31) // 32
    bits = np.zeros((M, W * 32), np.uint8)
    bits[:, :n] = allow
    return np.ascontiguousarray(np.packbits(bits, axis=1, bitorder="little")).view("<u4").astype(
        np.uint32).reshape(M, W)


def range_allowed(values, fields, lo, hi, base=None):
    """bool [M, n_docs].  values [F, n_docs]; fields int [M, C] (negative:
    padding; >= F: a field that no document has, the clause matches nothing);
    lo, hi [M, C] of the values' dtype; base: packed uint32 [1 or M, W] or None."""
    values = np.asarray(values)
    if values.ndim == 1:
        values = values[None, :]
    F, n = values.shape
    fields = np.asarray(fields)
    lo, hi = np.asarray(lo), np.asarray(hi)
    assert lo.dtype == values.dtype and hi.dtype == values.dtype
    M, C = fields.shape
    allowed = np.ones((M, n), bool)
    if base is not None:
        b = unpack_rows(base, n)
        allowed &= b if b.shape[0] == M else np.broadcast_to(b[:1], (M, n))
    for m in range(M):
        for c in range(C):
            f = int(fields[m, c])
            if f < 0:
                continue
            if f >= F:
                allowed[m] = False
                continue
            v = values[f]
            with np.errstate(invalid="ignore"):
                allowed[m] &= (v >= lo[m, c]) & (v <= hi[m, c])
    return allowed


def edge_case(dtype, n=70):
    """The edge values of one dtype over n documents, two fields -> (values
    [2, n], fields [R, 2], lo, hi): float32 with NaN, +-inf, -0.0 / +0.0 and
    denormals, int64 at +-2^53 + 1 (which no float holds) and at the int64
    limits, int32 at its limits; rows with an exact bound, open ends, lo > hi,
    a repeated field, a padding clause, and no clause at all."""
    dt = np.dtype(dtype)
    rng = np.random.default_rng(70)
    if dt.kind == "f":
        tiny = np.float32(1e-45)
        special = [np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, tiny, -tiny, 1.0, -1.0,
                   np.finfo(np.float32).max, np.finfo(np.float32).min, 16777216.0, 16777218.0]
        low, high = dt.type(-np.inf), dt.type(np.inf)
        near = (dt.type(-0.0), dt.type(0.0))          # -0.0 .. +0.0 holds both zeros
        exact = (dt.type(16777216.0), dt.type(16777217.0))  # (2^24 + 1 rounds to 2^24)
    else:
        ii = np.iinfo(dt)
        big = 2**53 if dt.itemsize == 8 else 2**24
        special = [ii.min, ii.min + 1, ii.max, ii.max - 1, 0, -1, 1, big, big + 1, big + 2,
                   -big, -big - 1, -big - 2]
        low, high = dt.type(ii.min), dt.type(ii.max)
        near = (dt.type(big + 1), dt.type(big + 1))   # one value, between two a float merges
        exact = (dt.type(-big - 1), dt.type(big + 1))
    values = rng.integers(-50, 50, size=(2, n)).astype(dt)
    at = rng.permutation(n)[:len(special)]
    values[0, at] = np.array(special, dt)
    values[1, at[::-1]] = np.array(special, dt)
    rows = [
        ([0, -1], [near[0], 0], [near[1], 0]),
        ([0, 1], [exact[0], low], [exact[1], high]),
        ([1, 0], [low, dt.type(-10)], [dt.type(10), high]),     # open ends on either side
        ([0, 0], [dt.type(-20), dt.type(0)], [dt.type(20), dt.type(30)]),  # a field twice
        ([0, 1], [dt.type(5), low], [dt.type(4), high]),        # lo > hi: the empty clause
        ([-1, -1], [0, 0], [0, 0]),                             # no clause: base alone
        ([1, -5], [low, 0], [high, 0]),                         # everything (but NaN)
        ([0, 1], [low, low], [low, high]),                      # the lowest value alone
        ([0, 1], [high, low], [high, high]),                    # the highest value alone
    ]
    fields = np.array([r[0] for r in rows], np.int32)
    lo = np.array([r[1] for r in rows], dt)
    hi = np.array([r[2] for r in rows], dt)
    return values, fields, lo, hi


def range_want(values, fields, lo, hi, base=None):
    """Packed uint32 [M, W]: the masks bm25_range_masks must give."""
    return pack_rows(range_allowed(values, fields, lo, hi, base))
