"""The numpy / Python model of the field statistics (include/bm25mi.h, "Field
statistics:"), the expected values of tests/test_mask_stats_host.py and
tests/test_gpu_mask_stats.py.  Rows are unpacked as facets_model.unpack_rows
does; count, min and max come from numpy; integer sums are wrapping int64; the
float32 sum is the bins-and-round model written out in Python integers: 32
bins, the carry loop, one rounding.  Never goes through the code under test."""
import struct

import numpy as np

from facets_model import unpack_rows

NBINS = 32


def float_bins(values):
    """finite float32 values -> (32 Python-int bins, +inf count, -inf count);
    NaN is skipped.  A value of biased exponent e is sig * 2^(E - 150) with
    E = max(e, 1); it adds +-(sig << (E & 7)) to bin E >> 3."""
    u = np.ascontiguousarray(values, dtype=np.float32).view(np.uint32).astype(np.int64).ravel()
    e = (u >> 23) & 0xFF
    neg = (u >> 31) != 0
    is_inf = (e == 255) & ((u & 0x7FFFFF) == 0)
    pinf, ninf = int((is_inf & ~neg).sum()), int((is_inf & neg).sum())
    fin = e != 255
    u, e, neg = u[fin], e[fin], neg[fin]
    assert u.size < 2**32   # (so an int64 bin cannot overflow)
    E = np.maximum(e, 1)
    sig = (u & 0x7FFFFF) | np.where(e != 0, 0x800000, 0)
    mag = sig << (E & 7)
    assert mag.size == 0 or int(mag.max()) < 2**31
    acc = np.zeros(NBINS, np.int64)
    np.add.at(acc, E >> 3, np.where(neg, -mag, mag))
    return [int(x) for x in acc], pinf, ninf


def few_bins(values, which):
    """The bins `which` of float_bins(values): what a test looks at."""
    bins = float_bins(values)[0]
    return [bins[b] for b in which]


def carry_digits(bins):
    """The carry loop: 32 digits of 8 bits, low to high, and the last carry
    (signed) — the integer sum(bins[b] << 8 b) as digits + carry << 256."""
    digits, carry = [], 0
    for b in range(NBINS):
        t = bins[b] + carry
        digits.append(t & 0xFF)
        carry = t >> 8  # arithmetic
    return digits, carry


def round_bins(bins, pinf=0, ninf=0):
    """(bins, inf counts) -> the float64 sum: the inf rules, else the signed
    integer of the carry loop, its magnitude's top 53 bits rounded to
    nearest-even on the rest, scaled by 2^-150; an exact zero is +0.0."""
    if pinf and ninf:
        return float("nan")
    if pinf or ninf:
        return float("inf") if pinf else float("-inf")
    digits, carry = carry_digits(bins)
    n = sum(d << (8 * b) for b, d in enumerate(digits)) + (carry << 256)
    assert n == sum(v << (8 * b) for b, v in enumerate(bins))
    neg, n = n < 0, abs(n)
    if n == 0:
        return 0.0
    shift = max(n.bit_length() - 53, 0)
    mant = n >> shift
    if shift:
        rest = n & ((1 << shift) - 1)
        half = 1 << (shift - 1)
        if rest > half or (rest == half and mant & 1):
            mant += 1
    v = float(np.ldexp(np.float64(mant), shift - 150))
    return -v if neg else v


def float_sum(values):
    """The float64 sum of float32 values by the model (NaN skipped)."""
    return round_bins(*float_bins(values))


def bits64(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def _key_f32(v):
    """float32 -> the ascending order key (int64; -0.0 as +0.0)."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.int64)
    u = np.where((u & 0x7FFFFFFF) == 0, 0, u)
    return np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000)


def stats_want(packed, values, groups=None, G=0):
    """-> dict of [M, B] arrays count (int64), min, max (values' dtype), sum
    (int64, or float64 for float32 values); B = G, or 1 when groups is None."""
    values = np.ascontiguousarray(values)
    n = values.shape[0]
    allowed = unpack_rows(packed, n)
    M = allowed.shape[0]
    is_f = values.dtype.kind == "f"
    number = ~np.isnan(values) if is_f else np.ones(n, bool)
    if groups is None:
        B, bucket, ok = 1, np.zeros(n, np.int64), number
    else:
        g = np.asarray(groups).astype(np.int64)
        B, bucket, ok = G, g, number & (g >= 0) & (g < G)
    out = {"count": np.zeros((M, B), np.int64), "min": np.zeros((M, B), values.dtype),
           "max": np.zeros((M, B), values.dtype),
           "sum": np.zeros((M, B), np.float64 if is_f else np.int64)}
    for m in range(M):
        sel = np.flatnonzero(allowed[m] & ok)
        if sel.size == 0:
            continue
        bs = bucket[sel]
        order = np.argsort(bs, kind="stable")
        sel, bs = sel[order], bs[order]
        cuts = np.flatnonzero(np.diff(bs)) + 1
        for part in np.split(sel, cuts):
            b = int(bucket[part[0]])
            v = values[part]
            out["count"][m, b] = part.size
            if is_f:
                k = _key_f32(v)
                lo, hi = v[np.argmin(k)], v[np.argmax(k)]
                out["min"][m, b] = lo if lo != 0 else 0.0   # a zero result is +0.0
                out["max"][m, b] = hi if hi != 0 else 0.0
                out["sum"][m, b] = float_sum(v)
            else:
                out["min"][m, b], out["max"][m, b] = v.min(), v.max()
                with np.errstate(over="ignore"):
                    out["sum"][m, b] = v.astype(np.int64).sum(dtype=np.int64)   # wrapping
    return out


def same_bits(a, b):
    """Bit-for-bit equality of two arrays of one dtype and shape (NaN == NaN,
    -0.0 != +0.0)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
