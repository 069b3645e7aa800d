"""GpuIndex — a device-resident BM25 CSC index on one MI355X.

Host mirror of the reference's index object (bm25_native.BM25v.doc_toks,
bm25_native.py:59-74) backed by libbm25mi.so.  All compute goes through the
C-ABI; this module only validates, converts dtypes and owns the handle.
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np

from . import _capi
from ._capi import check, lib


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _dptr(t):
    """The device pointer of a torch tensor (None: NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(stream) -> int:
    """A torch stream, a raw stream handle or None (the null stream) -> the handle."""
    return getattr(stream, "cuda_stream", stream) or 0


def _topk_out(Q: int, k: int) -> Tuple[np.ndarray, np.ndarray]:
    """The (docs, scores) arrays a host search fills (k < 0: the C call's error)."""
    return np.zeros((Q, max(k, 0)), np.int32), np.zeros((Q, max(k, 0)), np.float32)


def pack_mask(allow) -> np.ndarray:
    """Allow-masks for the filtered search: bool [n_docs] or [M, n_docs] ->
    uint32 [M, W], W = ceil(n_docs / 32), document d at bit d & 31 of word
    d >> 5 (little bit order); the bits past n_docs are 0."""
    a = np.asarray(allow)
    if a.ndim == 1:
        a = a[None, :]
    if a.ndim != 2:
        raise ValueError("allow must be a bool [n_docs] or [M, n_docs] array")
    a = a.astype(bool)
    M, n = a.shape
    W = (n + 31) // 32
    bits = np.zeros((M, W * 32), np.uint8)
    bits[:, :n] = a
    packed = np.packbits(bits, axis=1, bitorder="little")  # [M, 4 W] bytes, low byte first
    return np.ascontiguousarray(packed).view("<u4").astype(np.uint32, copy=False).reshape(M, W)


def pad_clause(rows) -> np.ndarray:
    """Clause rows for the boolean term filters: an int [M, width] array, or
    a ragged list of lists of token ids -> int32 [M, width], short rows padded
    with -1 (padding)."""
    if not isinstance(rows, np.ndarray):
        rows = list(rows)
        if any(not isinstance(r, np.ndarray) and np.ndim(r) == 0 for r in rows):
            raise ValueError("a clause must be a 2-D [M, width] array or a list of lists of "
                             "token ids")
        if len({len(r) for r in rows}) > 1 or not rows:
            width = max((len(r) for r in rows), default=0)
            a = np.full((len(rows), width), -1, np.int32)
            for i, r in enumerate(rows):
                a[i, :len(r)] = np.asarray(r, np.int32)
            return a
        rows = np.asarray(rows)
        if rows.size == 0:
            rows = rows.reshape(len(rows), 0)
    if rows.ndim != 2 or (rows.size and rows.dtype.kind not in "iu"):
        raise ValueError("a clause must be a 2-D [M, width] array or a list of lists of token ids")
    return np.ascontiguousarray(rows, dtype=np.int32)


def min_match_rows(any_rows, spec, what: str = "mask") -> np.ndarray:
    """The min_match argument of the boolean term filters -> int32 [M], one
    entry per row of ``any_rows`` (clause rows as pad_clause takes them).
    ``spec``: an int (every row), an int array [M], or a percentage string
    "NN%" of each row's terms — (n_any(row) * NN) // 100 in integer arithmetic
    (rounded down, as Lucene does), raised to 1 where the row names a term; a
    row without a term gets 0.  Wrong lengths, negative values and
    non-integers raise ValueError."""
    a = pad_clause(any_rows)
    M = a.shape[0]
    if isinstance(spec, str):
        s = spec.strip()
        if not (s.endswith("%") and s[:-1].isdigit() and int(s[:-1]) <= 100):
            raise ValueError(f"min_match {spec!r}: a percentage is written \"NN%\", NN in 0..100")
        n_any = (a >= 0).sum(axis=1).astype(np.int64)
        mm = n_any * int(s[:-1]) // 100
        return np.where(n_any > 0, np.maximum(mm, 1), 0).astype(np.int32)
    mm = np.asarray(spec)
    if mm.dtype.kind not in "iu" or mm.ndim > 1:
        raise ValueError("min_match must be an int, an int [M] array or a string \"NN%\"")
    if mm.ndim == 0:
        mm = np.full(M, mm)
    if mm.shape[0] != M:
        raise ValueError(f"min_match has {mm.shape[0]} entries, expected {M} (one per {what})")
    if mm.size and int(mm.min()) < 0:
        r = int(np.argmax(mm < 0))
        raise ValueError(f"min_match[{r}] = {int(mm[r])} is negative")
    if mm.size and int(mm.max()) > np.iinfo(np.int32).max:
        raise ValueError("min_match entries must fit int32")
    return np.ascontiguousarray(mm, dtype=np.int32)


def facet_codes(labels):
    """Arbitrary per-document labels -> (codes int32 [n], uniques): the group
    ids the facet counts take, with np.unique(..., return_inverse=True)
    semantics — uniques sorted, uniques[codes[d]] == labels[d] — except that a
    None or masked entry has no group: its code is -1 and it is no unique."""
    if isinstance(labels, np.ma.MaskedArray):
        missing = np.ma.getmaskarray(labels).ravel()
        a = np.ma.getdata(labels).ravel()
    else:
        a = np.asarray(labels).ravel()
        missing = np.zeros(a.size, bool)
    if a.dtype == object:
        missing = missing | np.fromiter((x is None for x in a), bool, a.size)
    present = a[~missing]
    if a.dtype == object and present.size:
        present = np.asarray(list(present))  # (strings, ints: numpy's own dtype)
    uniques, inverse = np.unique(present, return_inverse=True)
    if uniques.size > np.iinfo(np.int32).max:
        raise ValueError("more distinct labels than an int32 group id holds")
    codes = np.full(a.size, -1, np.int32)
    codes[~missing] = inverse.ravel()
    return codes, uniques


def _facet_groups(groups, n_groups, n_docs: int):
    """The (groups, n_groups) of the facet calls -> (int32 [n_docs], G);
    shape and dtype errors are raised here, before any C call."""
    if isinstance(n_groups, (bool, np.bool_)) or not isinstance(n_groups, (int, np.integer)):
        raise ValueError("n_groups must be an int")
    G = int(n_groups)
    if G < 0:
        raise ValueError(f"n_groups = {G} is negative")
    if G > np.iinfo(np.int32).max:
        raise ValueError("n_groups must fit int32 (a group id is an int32)")
    g = np.asarray(groups)
    if g.dtype.kind not in "iu":
        raise ValueError("groups must be an integer array (bm25mi.facet_codes makes one of labels)")
    if g.ndim != 1 or g.shape[0] != n_docs:
        raise ValueError(f"groups has shape {g.shape}, expected ({n_docs},) (one per document)")
    if g.size and (int(g.max()) > np.iinfo(np.int32).max or int(g.min()) < np.iinfo(np.int32).min):
        raise ValueError("groups entries must fit int32")
    return np.ascontiguousarray(g, dtype=np.int32), G


# BM25_FIELD_I32 / _F32 / _I64: the dtypes a range filter's columns may have
_FIELD_KINDS = {np.dtype(np.int32): 0, np.dtype(np.float32): 1, np.dtype(np.int64): 2}


def _field_limits(dtype):
    """(lowest, highest) bound of a column dtype: the open ends of a range."""
    dt = np.dtype(dtype)
    if dt not in _FIELD_KINDS:
        raise ValueError(f"dtype {dt} is not a range filter's: int32, int64 or float32")
    if dt.kind == "f":
        return dt.type(-np.inf), dt.type(np.inf)
    return dt.type(np.iinfo(dt).min), dt.type(np.iinfo(dt).max)


def range_rows(rows, columns, dtype):
    """Per-row range dicts -> (fields int32 [M, C], lo, hi [M, C] of ``dtype``),
    the clause rows of the range filters.  ``rows``: one dict per mask row,
    column name -> (lo, hi), both inclusive, None = the open end (the dtype's
    limit, or -inf / +inf), e.g. [{"year": (2019, 2021), "price": (None, 50)},
    {}]; ``columns``: the names of the values' rows, in order.  Rows are
    padded to a common width with field -1 (bounds 0).  An unknown column
    name is a ValueError, as is a bound the dtype cannot hold exactly."""
    dt = np.dtype(dtype)
    low, high = _field_limits(dt)
    names = {name: i for i, name in enumerate(columns)}
    rows = list(rows)
    C = max((len(r) for r in rows), default=0)
    fields = np.full((len(rows), C), -1, np.int32)
    lo = np.zeros((len(rows), C), dt)
    hi = np.zeros((len(rows), C), dt)
    for m, r in enumerate(rows):
        for c, (name, bounds) in enumerate(r.items()):
            if name not in names:
                raise ValueError(f"row {m}: unknown column {name!r} (columns: {list(columns)})")
            if not isinstance(bounds, (tuple, list)) or len(bounds) != 2:
                raise ValueError(f"row {m}, column {name!r}: the bounds are a pair (lo, hi)")
            fields[m, c] = names[name]
            for arr, b, end in ((lo, bounds[0], low), (hi, bounds[1], high)):
                if b is None:
                    arr[m, c] = end
                    continue
                if dt.kind == "i" and (int(b) != b or not int(low) <= int(b) <= int(high)):
                    raise ValueError(f"row {m}, column {name!r}: bound {b!r} is no {dt}")
                arr[m, c] = int(b) if dt.kind == "i" else b
    return fields, lo, hi


def _range_args(values, fields, lo, hi, n_docs: int, rows=None, what: str = "mask"):
    """The (values, fields, lo, hi) of the range calls -> (values [F, n_docs],
    kind, fields int32 [M, C], lo, hi [M, C] of the values' dtype); shape and
    dtype errors are raised here, before any C call."""
    v = np.asarray(values)
    if v.dtype not in _FIELD_KINDS:
        raise ValueError(f"values have dtype {v.dtype}: a range filter takes int32, int64 or "
                         "float32 exactly (nothing is rounded or converted silently)")
    if v.ndim == 1:
        v = v[None, :]
    if v.ndim != 2 or v.shape[1] != n_docs:
        raise ValueError(f"values has shape {np.shape(values)}, expected ({n_docs},) or "
                         f"(F, {n_docs}) (one entry per document)")
    F = v.shape[0]
    bounds = []
    for name, b in (("lo", lo), ("hi", hi)):
        a = np.asarray(b)
        if a.dtype != v.dtype:
            raise ValueError(f"{name} has dtype {a.dtype}, the values have {v.dtype} (bounds are "
                             "of the values' dtype; bm25mi.range_rows makes them)")
        if a.ndim == 1:
            a = a[:, None]
        if a.ndim != 2:
            raise ValueError(f"{name} has shape {np.shape(b)}, expected (M,) or (M, C)")
        bounds.append(np.ascontiguousarray(a))
    lo_a, hi_a = bounds
    if lo_a.shape != hi_a.shape:
        raise ValueError(f"lo has shape {lo_a.shape}, hi has {hi_a.shape}")
    M, C = lo_a.shape
    if rows is not None and M != rows:
        raise ValueError(f"lo and hi have {M} rows, expected {rows} (one per {what})")
    if fields is None:
        if F != 1:
            raise ValueError(f"fields=None needs one field, the values have {F}")
        f = np.zeros((M, C), np.int32)
    else:
        f = np.asarray(fields)
        if f.dtype.kind not in "iu" or f.dtype == np.bool_:
            raise ValueError("fields must be an integer array")
        if f.ndim == 1:
            f = f[:, None]
        if f.shape != (M, C):
            raise ValueError(f"fields has shape {np.shape(fields)}, lo and hi have {(M, C)}")
        if f.size and int(f.max()) >= F:
            m, c = np.argwhere(f >= F)[0]
            raise ValueError(f"fields[{m}][{c}] = {int(f[m, c])} is not below F = {F}")
        # (any negative id is padding: -1 fits int32 whatever the input's width)
        f = np.ascontiguousarray(np.maximum(f.astype(np.int64), -1), dtype=np.int32)
    return np.ascontiguousarray(v), _FIELD_KINDS[v.dtype], f, lo_a, hi_a


def _ranges_arg(ranges):
    """ranges= of search_boolean: (values, fields, lo, hi), or (values, lo, hi)
    for one field -> the quadruple."""
    if not isinstance(ranges, (tuple, list)) or len(ranges) not in (3, 4):
        raise ValueError("ranges must be a quadruple (values, fields, lo, hi) or, for one field, "
                         "a triple (values, lo, hi)")
    return tuple(ranges) if len(ranges) == 4 else (ranges[0], None, ranges[1], ranges[2])


AFTER_NONE = -2  # BM25_AFTER_NONE: an after-docs entry that means "no cursor"


SORTED_MAX_K = 4096  # bm25_search_sorted: hits a row, at most (the LDS sort of a row's list)
_SORT_KINDS = {np.dtype(np.int32): 0, np.dtype(np.float32): 1, np.dtype(np.int64): 2}
STATS_KEYS = ("count", "min", "max", "sum", "mean")  # the dict GpuIndex.stats returns


def _sort_values_arg(values, n_docs: int):
    """A sort column: [n_docs] int32, int64 or float32 exactly -> (contiguous
    array, kind)."""
    v = np.asarray(values)
    if v.dtype not in _SORT_KINDS:
        raise ValueError(f"values have dtype {v.dtype.name}: int32, int64 or float32 (nothing is "
                         "rounded)")
    if v.shape != (n_docs,):
        raise ValueError(f"values has shape {v.shape}, expected ({n_docs},) (one entry per "
                         "document)")
    return np.ascontiguousarray(v), _SORT_KINDS[v.dtype]


def _order_arg(order, n_docs: int):
    """order=(ranks, perm), as GpuIndex.sort_ranks returns them -> two
    contiguous int32 [n_docs] arrays, checked to be inverse permutations (the
    C call's check and message: the first offending index)."""
    if not isinstance(order, (tuple, list)) or len(order) != 2:
        raise ValueError("the order must be a pair (ranks, perm), as sort_ranks returns it")
    out = []
    for name, a in zip(("ranks", "perm"), order):
        a = np.asarray(a)
        if a.dtype.kind not in "iu" or a.shape != (n_docs,):
            raise ValueError(f"{name} must be an integer [{n_docs}] array (one entry per "
                             f"document), got {a.dtype.name} {a.shape}")
        if a.size and (int(a.min()) < np.iinfo(np.int32).min
                       or int(a.max()) > np.iinfo(np.int32).max):
            raise ValueError(f"{name} holds values outside int32")
        out.append(np.ascontiguousarray(a, dtype=np.int32))
    ranks, perm = out
    bad = (ranks < 0) | (ranks >= n_docs)
    ok = ~bad
    back = np.full(n_docs, -1, np.int64)
    back[ok] = perm[ranks[ok]]
    wrong = np.flatnonzero(bad | (back != np.arange(n_docs)))
    if wrong.size:
        d = int(wrong[0])
        r = int(ranks[d])
        if bad[d]:
            raise ValueError(f"ranks[{d}] = {r} is outside [0, {n_docs})")
        raise ValueError(f"ranks[{d}] = {r} but perm[{r}] = {int(perm[r])}: ranks and perm are "
                         "not inverse permutations")
    return ranks, perm


def _after_ranks_arg(after, rows: int, what: str = "mask row"):
    """Cursors of a sorted search: None, or an int [rows] array of ranks, -1 (a
    padding slot's rank: an all-padding row) or -2 (no cursor)."""
    if after is None:
        return None
    a = np.asarray(after)
    if a.dtype.kind not in "iu" or a.shape != (rows,):
        raise ValueError(f"after must hold one rank per {what} ({rows}), got {a.dtype.name} "
                         f"{a.shape}")
    a = np.ascontiguousarray(a, dtype=np.int64)
    low = np.flatnonzero(a < -2)
    if low.size:
        m = int(low[0])
        raise ValueError(f"after_ranks[{m}] = {int(a[m])} is below BM25_AFTER_NONE (-2)")
    return np.ascontiguousarray(np.minimum(a, np.iinfo(np.int32).max), dtype=np.int32)


def sort_keys(values, descending: bool = False) -> np.ndarray:
    """The order keys K(v) of a sort column (include/bm25mi.h, "Sort-by-field
    search over doc shards"), uint64 [n]: what sort_keys_device writes as
    key_hi = K >> 32 and key_lo = K & 0xFFFFFFFF, on the host — for reading a
    page's keys and for making collection cursors without a GPU.  values: int32,
    int64 or float32 exactly.  A column's order is (K ascending, doc id
    ascending)."""
    v = np.ascontiguousarray(values)
    if v.dtype not in _SORT_KINDS:
        raise ValueError(f"values have dtype {v.dtype.name}: int32, int64 or float32 (nothing is "
                         "rounded)")
    if v.dtype == np.int64:
        u = v.view(np.uint64) ^ np.uint64(1 << 63)
        return ~u if descending else u
    if v.dtype == np.int32:
        u = v.view(np.uint32) ^ np.uint32(0x80000000)
        return (~u if descending else u).astype(np.uint64)
    bits = v.view(np.uint32)
    bits = np.where((bits & np.uint32(0x7FFFFFFF)) == 0, np.uint32(0), bits)  # -0.0 as +0.0
    u = np.where((bits >> np.uint32(31)) != 0, ~bits, bits | np.uint32(0x80000000))
    u = (~u if descending else u).astype(np.uint64)
    return np.where(np.isnan(v), np.uint64(1 << 32), u)


def sort_key_values(keys, dtype, descending: bool = False) -> np.ndarray:
    """The values of order keys: the inverse of sort_keys for a column of
    ``dtype`` and direction — the identity on every value except that -0.0
    comes back as +0.0 and every NaN as one NaN."""
    k = np.ascontiguousarray(keys, dtype=np.uint64)
    dt = np.dtype(dtype)
    if dt not in _SORT_KINDS:
        raise ValueError(f"dtype {dt.name}: int32, int64 or float32")
    if dt == np.int64:
        u = ~k if descending else k
        return (u ^ np.uint64(1 << 63)).view(np.int64)
    u = k.astype(np.uint32)  # (the low word; a NaN's key is 1 << 32)
    if descending:
        u = ~u
    if dt == np.int32:
        return (u ^ np.uint32(0x80000000)).view(np.int32)
    bits = np.where((u >> np.uint32(31)) != 0, u & np.uint32(0x7FFFFFFF), ~u)
    out = np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32).copy()
    out[k == np.uint64(1 << 32)] = np.float32("nan")
    return out


def _sorted_k(k, n_docs: int) -> int:
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError("k must be an int")
    k = int(k)
    if k < 0:
        raise ValueError("negative dimensions are not allowed")
    if k > SORTED_MAX_K:
        raise ValueError(f"k = {k}: a sorted search returns at most {SORTED_MAX_K} hits a row")
    if k > n_docs:
        raise ValueError(f"k = {k} is above the index's {n_docs} documents")
    return k


def page_cursor(docs, scores):
    """The cursor after a page of results: its last column as the pair
    (scores [Q] float32, docs [Q] int32) that search_after's ``after`` takes.
    A row that ended in padding gives doc -1, which search_after reads as
    "exhausted" (an all-padding row), so the last column of any page can be
    fed back in.  Works on numpy arrays and on torch tensors (the device
    call's outputs) alike."""
    if docs.ndim != 2 or tuple(docs.shape) != tuple(scores.shape):
        raise ValueError("docs and scores must be 2-D [Q, k] arrays of one shape")
    if docs.shape[1] == 0:
        raise ValueError("a page of k = 0 columns has no cursor")
    if isinstance(docs, np.ndarray):
        return (np.ascontiguousarray(scores[:, -1], dtype=np.float32),
                np.ascontiguousarray(docs[:, -1], dtype=np.int32))
    return scores[:, -1].contiguous(), docs[:, -1].contiguous()


class GpuIndex:
    """A doc x term CSC score matrix resident in HBM.

    Arguments mirror ``scipy.sparse.csc_matrix((data, indices, indptr),
    shape=(n_docs, n_terms))`` — the in-memory form of the bm25s on-disk
    index (indptr/indices/data ``.csc.index.npy``)."""

    def __init__(self, indptr, indices, data, n_docs: int, device: int = 0,
                 doc_offset: int = 0, options: Optional[dict] = None):
        indptr = np.asarray(indptr)
        if indptr.ndim != 1 or indptr.size < 1:
            raise ValueError("indptr must be a 1-D array of n_terms + 1 offsets")
        ip_i64 = indptr.dtype == np.int64 or indptr[-1] > np.iinfo(np.int32).max
        self._indptr = np.ascontiguousarray(indptr, dtype=np.int64 if ip_i64 else np.int32)
        self._indices = np.ascontiguousarray(indices, dtype=np.int32)
        self._data = np.ascontiguousarray(data, dtype=np.float32)
        nnz = int(self._indptr[-1])
        if self._indices.size < nnz or self._data.size < nnz:
            raise ValueError("indices/data shorter than indptr[-1]")
        self.n_docs = int(n_docs)
        self.n_terms = int(self._indptr.size - 1)
        self.nnz = nnz
        self.device = int(device)
        self.doc_offset = int(doc_offset)
        h = ctypes.c_void_p()
        self._h = None
        check(lib.bm25_index_create(self.device, self.n_docs, self.n_terms, nnz,
                                    _ptr(self._indptr), int(ip_i64), _ptr(self._indices),
                                    _ptr(self._data), self.doc_offset, ctypes.byref(h)))
        self._h = h
        # the device holds its own copy
        self._indptr = self._indices = self._data = None
        for name, value in (options or {}).items():
            self.set_option(name, value)

    # ------------------------------------------------------------------
    @classmethod
    def from_csc(cls, m, device: int = 0, doc_offset: int = 0) -> "GpuIndex":
        """From a scipy.sparse CSC matrix (doc x term).  Non-canonical input
        (unsorted indices) is sorted on a copy first; duplicate entries are
        summed (scipy semantics for a CSC with duplicates)."""
        import scipy.sparse as sp
        if not sp.issparse(m):
            raise ValueError("doc_toks must be a scipy.sparse matrix")
        m = m.tocsc()
        if not m.has_canonical_format:
            m = m.copy()
            m.sum_duplicates()
        return cls(m.indptr, m.indices, m.data, m.shape[0], device=device, doc_offset=doc_offset)

    def fork(self) -> "GpuIndex":
        """Another search context on the same device arrays (bm25_index_fork):
        its own workspace, options (copied) and stream, so searches on this
        handle and on the fork may run concurrently on different streams."""
        h = ctypes.c_void_p()
        check(lib.bm25_index_fork(self._h, ctypes.byref(h)))
        g = GpuIndex.__new__(GpuIndex)
        g.__dict__.update({k: v for k, v in self.__dict__.items() if not k.startswith("_")})
        g._indptr = g._indices = g._data = None
        g._h = h
        return g

    # ------------------------------------------------------------------
    def close(self) -> None:
        """Destroy the handle and every fork bm25mi.dist cached on it.  The
        device arrays are shared (bm25_index_fork), so they are released only
        when the last of those handles is gone."""
        for f in self.__dict__.pop("_bm25_forks", []):
            f.close()
        self.__dict__.pop("_bm25_part_streams", None)
        if self._h is not None:
            lib.bm25_index_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self) -> dict:
        vals = [ctypes.c_int64() for _ in range(3)]
        td = ctypes.c_int32()
        nt = ctypes.c_int64()
        db = ctypes.c_int64()
        check(lib.bm25_index_info(self._h, *[ctypes.byref(v) for v in vals], ctypes.byref(td),
                                  ctypes.byref(nt), ctypes.byref(db)))
        sp_ = ctypes.c_int32()
        npairs = ctypes.c_int64()
        check(lib.bm25_index_segments(self._h, ctypes.byref(sp_), ctypes.byref(npairs)))
        hb = ctypes.c_int32()
        bb = ctypes.c_int64()
        check(lib.bm25_index_bounds(self._h, ctypes.byref(hb), ctypes.byref(bb)))
        return {"n_docs": vals[0].value, "n_terms": vals[1].value, "nnz": vals[2].value,
                "tile_docs": td.value, "n_tiles": nt.value, "device_bytes": db.value,
                "sparse": bool(sp_.value), "n_pairs": npairs.value,
                "tile_bounds": bool(hb.value), "tile_bound_bytes": bb.value}

    # ------------------------------------------------------------------
    def search(self, queries: np.ndarray, k: int) -> Tuple[np.ndarray, np.ndarray]:
        """Top-k of every query row (host arrays).  queries: int32 [Q, T]."""
        q = np.ascontiguousarray(queries, dtype=np.int32)
        if q.ndim != 2:
            raise ValueError("queries must be a 2-D [Q, T] int32 array")
        Q, T = q.shape
        k = int(k)
        docs, scores = _topk_out(Q, k)
        check(lib.bm25_search(self._h, _ptr(q), Q, T, k, _ptr(docs), _ptr(scores)))
        return docs, scores

    def max_token_device(self, d_queries, stream=None) -> int:
        """Largest token id of a device batch (bm25_max_token_device; syncs)."""
        Q, T = d_queries.shape
        s = _stream(stream)
        m = ctypes.c_int32()
        check(lib.bm25_max_token_device(self._h, ctypes.c_void_p(d_queries.data_ptr()), Q, T,
                                        ctypes.byref(m), ctypes.c_void_p(s)))
        return m.value

    def search_device(self, d_queries, k: int, d_docs, d_scores, stream=None,
                      validate: bool = False) -> None:
        """Device-resident search: torch int32 [Q, T] in, int32/f32 [Q, k] out,
        enqueued on ``stream`` (a torch.cuda.Stream or raw handle).  Token ids
        >= n_terms count as padding unless ``validate`` (a synchronising
        device check) raises the reference's ValueError (bm25_native.py:91-96)."""
        Q, T = d_queries.shape
        s = _stream(stream)
        if validate:
            m = self.max_token_device(d_queries, stream)
            if m >= self.n_terms:
                raise ValueError(
                    f"The maximum token ID in the query ({m}) is higher than the number "
                    "of tokens in the index.")
        check(lib.bm25_search_device(self._h, ctypes.c_void_p(d_queries.data_ptr()), Q, T,
                                     int(k), ctypes.c_void_p(d_docs.data_ptr()),
                                     ctypes.c_void_p(d_scores.data_ptr()), ctypes.c_void_p(s)))

    # -------------------------------------------- doc-sharded, global theta
    def sample_width(self, k: int, world: int, shard_docs_max: int) -> int:
        w = ctypes.c_int64()
        check(lib.bm25_sample_width(self._h, int(shard_docs_max), int(world), int(k),
                                    ctypes.byref(w)))
        return w.value

    def search_sample_device(self, d_queries, k: int, world: int, shard_docs_max: int, d_keys,
                             stream=None) -> None:
        """This shard's sample keys (torch int64/uint64 [Q, S] on the device)."""
        Q, T = d_queries.shape
        s = _stream(stream)
        check(lib.bm25_search_sample_device(self._h, ctypes.c_void_p(d_queries.data_ptr()), Q, T,
                                            int(k), int(world), int(shard_docs_max),
                                            ctypes.c_void_p(d_keys.data_ptr()),
                                            ctypes.c_void_p(s)))

    def search_finish_device(self, d_queries, k: int, world: int, shard_docs_max: int,
                             d_all_keys, d_docs, d_scores, stream=None) -> None:
        """Global theta from every shard's sample keys ([W, Q, S]), then this
        shard's keys >= theta as a padded [Q, k] list (global doc ids)."""
        Q, T = d_queries.shape
        s = _stream(stream)
        check(lib.bm25_search_finish_device(self._h, ctypes.c_void_p(d_queries.data_ptr()), Q, T,
                                            int(k), int(world), int(shard_docs_max),
                                            ctypes.c_void_p(d_all_keys.data_ptr()),
                                            ctypes.c_void_p(d_docs.data_ptr()),
                                            ctypes.c_void_p(d_scores.data_ptr()),
                                            ctypes.c_void_p(s)))

    def search_finish_streams_device(self, d_queries, k: int, world: int, shard_docs_max: int,
                                     d_all_keys, d_docs, d_scores, stream_theta, stream_rest,
                                     stream_select) -> None:
        """search_finish_device on three streams (bm25_search_finish_streams_
        device): theta, the REST pass and the merges, ordered by events."""
        Q, T = d_queries.shape
        ss = [_stream(x) for x in (stream_theta, stream_rest, stream_select)]
        check(lib.bm25_search_finish_streams_device(
            self._h, ctypes.c_void_p(d_queries.data_ptr()), Q, T, int(k), int(world),
            int(shard_docs_max), ctypes.c_void_p(d_all_keys.data_ptr()),
            ctypes.c_void_p(d_docs.data_ptr()), ctypes.c_void_p(d_scores.data_ptr()),
            *[ctypes.c_void_p(x) for x in ss]))

    # ------------------------------- doc-sharded, one collective (world bounds)
    def bounds_stride(self) -> int:
        """u16 per row of this index's tile bounds (its tiles rounded up to 4)."""
        return (int(self.info()["n_tiles"]) + 3) // 4 * 4

    def bounds_export(self, d_out, stride: int, stream=None) -> None:
        """This index's tile bounds into d_out (a torch int16 [n_terms, stride]
        device tensor; bm25_index_bounds_export)."""
        s = _stream(stream)
        check(lib.bm25_index_bounds_export(self._h, ctypes.c_void_p(d_out.data_ptr()), int(stride),
                                           ctypes.c_void_p(s)))

    def masks_export(self, d_out, stride: int, stream=None) -> None:
        """This index's sub-block presence masks into d_out (a torch int32
        [n_terms, stride] device tensor, stride as bounds_stride();
        bm25_index_masks_export).  Bit s of (term, tile): the term has a
        posting in the tile's s-th sub-block of tile_docs / 32 documents."""
        s = _stream(stream)
        check(lib.bm25_index_masks_export(self._h, ctypes.c_void_p(d_out.data_ptr()), int(stride),
                                          ctypes.c_void_p(s)))

    def set_world_bounds(self, d_world, world: int, stride: int, world_tiles: int) -> None:
        """Every shard's tile bounds ([world, n_terms, stride] int16 on this
        device, kept referenced here) for bm25_search_shard_device; None clears."""
        if d_world is None:
            check(lib.bm25_index_set_world_bounds(self._h, None, 0, 0, 0))
            self.__dict__.pop("_bm25_world_bounds", None)
            return
        check(lib.bm25_index_set_world_bounds(self._h, ctypes.c_void_p(d_world.data_ptr()),
                                              int(world), int(stride), int(world_tiles)))
        self._bm25_world_bounds = d_world
        for f in self.__dict__.get("_bm25_forks", []):
            f.set_world_bounds(d_world, world, stride, world_tiles)

    def search_shard_device(self, d_queries, k: int, d_docs, d_scores, stream=None) -> None:
        """This shard's keys >= the collection's threshold (world bounds) as an
        unsorted padded [Q, k] list for the W-way merge (bm25_search_shard_device)."""
        Q, T = d_queries.shape
        s = _stream(stream)
        check(lib.bm25_search_shard_device(self._h, ctypes.c_void_p(d_queries.data_ptr()), Q, T,
                                           int(k), ctypes.c_void_p(d_docs.data_ptr()),
                                           ctypes.c_void_p(d_scores.data_ptr()),
                                           ctypes.c_void_p(s)))

    def scores_dense(self, query) -> np.ndarray:
        """All n_docs fp32 scores of one query (zero for untouched docs)."""
        q = np.ascontiguousarray(np.asarray(query).ravel(), dtype=np.int32)
        out = np.zeros(self.n_docs, np.float32)
        check(lib.bm25_scores_dense(self._h, _ptr(q), q.size, _ptr(out)))
        return out

    # ------------------------------------------ given (query, document) pairs
    def score_docs(self, queries, docs) -> np.ndarray:
        """Scores of given candidates (bm25_score_docs, host arrays): queries
        int32 [Q, T], docs int32 [Q, C] global doc ids (negative = padding)
        -> float32 [Q, C], out[q, c] bit-equal to
        ``scores_dense(queries[q])[docs[q, c] - doc_offset]``."""
        q = np.ascontiguousarray(queries, dtype=np.int32)
        d = np.ascontiguousarray(docs, dtype=np.int32)
        if q.ndim != 2:
            raise ValueError("queries must be a 2-D [Q, T] int32 array")
        if d.ndim != 2:
            raise ValueError("docs must be a 2-D [Q, C] int32 array")
        if q.shape[0] != d.shape[0]:
            raise ValueError(f"queries has {q.shape[0]} rows, docs has {d.shape[0]}")
        out = np.zeros(d.shape, np.float32)
        check(lib.bm25_score_docs(self._h, _ptr(q), q.shape[0], q.shape[1], _ptr(d), d.shape[1],
                                  _ptr(out)))
        return out

    def score_docs_device(self, d_queries, d_docs, d_scores, stream=None) -> None:
        """Device-resident score_docs (bm25_score_docs_device): torch int32
        [Q, T] and [Q, C] in, float32 [Q, C] out, enqueued on ``stream`` with
        no host synchronisation and no validation — token ids >= n_terms are
        padding, doc ids outside this handle's range score +0.0 (doc shards'
        outputs add up to the single-index output).  Reads the index arrays
        only, so it may overlap a search of the same handle on another stream."""
        if d_queries.dim() != 2 or d_docs.dim() != 2:
            raise ValueError("d_queries and d_docs must be 2-D [Q, T] and [Q, C] tensors")
        Q, T = d_queries.shape
        if d_docs.shape[0] != Q:
            raise ValueError(f"d_queries has {Q} rows, d_docs has {d_docs.shape[0]}")
        C = d_docs.shape[1]
        if d_scores.numel() != Q * C:
            raise ValueError(f"d_scores must hold {Q} x {C} scores")
        s = _stream(stream)
        check(lib.bm25_score_docs_device(self._h, ctypes.c_void_p(d_queries.data_ptr()), Q, T,
                                         ctypes.c_void_p(d_docs.data_ptr()), C,
                                         ctypes.c_void_p(d_scores.data_ptr()), ctypes.c_void_p(s)))

    # ------------------------------------------------------- filtered search
    def _masks_arg(self, masks) -> np.ndarray:
        """bool [n_docs] / [M, n_docs] or packed uint32 [W] / [M, W] -> uint32
        [M, W] for this index (shape errors raised here, before any C call)."""
        m = np.asarray(masks)
        W = (self.n_docs + 31) // 32
        if m.dtype == np.bool_:
            if m.ndim not in (1, 2) or m.shape[-1] != self.n_docs:
                raise ValueError(f"a bool mask must have {self.n_docs} (n_docs) columns, "
                                 f"got shape {m.shape}")
            return pack_mask(m)
        if m.dtype != np.uint32:
            raise ValueError("masks must be bool [M, n_docs] or packed uint32 [M, W] "
                             "(bm25mi.pack_mask)")
        if m.ndim == 1:
            m = m[None, :]
        if m.ndim != 2 or m.shape[1] != W:
            raise ValueError(f"packed masks must have {W} (ceil(n_docs / 32)) words per row, "
                             f"got shape {m.shape}")
        return np.ascontiguousarray(m)

    def _ranked_args(self, queries, weights, masks, query_mask, need_weights=False,
                     need_masks=False):
        """The host arrays of a ranked search -> (q, w, m, M, qm): int32 [Q, T]
        queries, float32 weights or None, packed masks [M, W] or None, int32
        [Q] mask ids in [-1, M) or None (shape errors raised here, before any C
        call).  need_weights: weights are no option (search_weighted);
        need_masks: nor are the masks, and without a mask row the mask ids are
        none either (search_filtered)."""
        q = np.ascontiguousarray(queries, dtype=np.int32)
        if q.ndim != 2:
            raise ValueError("queries must be a 2-D [Q, T] int32 array")
        Q = q.shape[0]
        w = self._weights_arg(q, weights) if need_weights or weights is not None else None
        m = self._masks_arg(masks) if need_masks or masks is not None else None
        M = 0 if m is None else m.shape[0]
        qm = None
        if query_mask is not None:
            qm = np.ascontiguousarray(query_mask, dtype=np.int32)
            if qm.ndim != 1 or qm.size != Q:
                raise ValueError(f"query_mask must hold one mask id per query ({Q}), "
                                 f"got shape {qm.shape}")
            if qm.size and (int(qm.min()) < -1 or int(qm.max()) >= M):
                raise ValueError(f"query_mask entries must be in [-1, {M})")
        elif need_masks and M == 0 and Q > 0:
            raise ValueError("no masks given: query_mask must be -1 for every query")
        return q, w, m, M, qm

    def _ranked_device_args(self, d_queries, d_weights, d_masks, d_query_mask, need_weights=False,
                            need_masks=False) -> Tuple[int, int, int]:
        """The shapes of a device-resident ranked search's tensors -> (Q, T, M);
        need_weights / need_masks as in _ranked_args."""
        if d_queries.dim() != 2:
            raise ValueError("d_queries must be a 2-D [Q, T] tensor")
        Q, T = d_queries.shape
        if (need_weights or d_weights is not None) and (
                tuple(d_weights.shape) != (Q, T) or not d_weights.dtype.is_floating_point
                or d_weights.element_size() != 4):
            raise ValueError(f"d_weights must be a float32 [{Q}, {T}] tensor")
        W = (self.n_docs + 31) // 32
        M = 0
        if need_masks or d_masks is not None:
            if d_masks.dim() != 2 or d_masks.shape[1] != W or d_masks.element_size() != 4:
                raise ValueError(f"d_masks must be a packed [M, {W}] tensor of 32-bit words")
            M = d_masks.shape[0]
        if d_query_mask is not None and d_query_mask.numel() != Q:
            raise ValueError(f"d_query_mask must hold one mask id per query ({Q})")
        if need_masks and d_query_mask is None and M == 0 and Q > 0:
            raise ValueError("no masks given: d_query_mask must be -1 for every query")
        return Q, T, M

    @staticmethod
    def _device_out(d_docs, d_scores, Q: int, k: int) -> None:
        if d_docs.numel() != Q * k or d_scores.numel() != Q * k:
            raise ValueError(f"d_docs and d_scores must hold {Q} x {k} results")

    def search_filtered(self, queries: np.ndarray, k: int, masks,
                        query_mask=None) -> Tuple[np.ndarray, np.ndarray]:
        """Top-k of every query among the documents its mask allows
        (bm25_search_filtered, host arrays).  queries int32 [Q, T]; masks bool
        [M, n_docs] (or [n_docs]) or packed uint32 [M, W] (pack_mask), bits by
        this handle's own documents; query_mask int32 [Q] picks each query's
        mask (-1: no filter; None: mask 0 for every query).  Rows with fewer
        than k allowed documents end in padding (doc -1, score bits ~0)."""
        q, _, m, M, qm = self._ranked_args(queries, None, masks, query_mask, need_masks=True)
        Q, T = q.shape
        k = int(k)
        docs, scores = _topk_out(Q, k)
        check(lib.bm25_search_filtered(self._h, _ptr(q), Q, T, k, _ptr(m) if M else None, M,
                                       _ptr(qm), _ptr(docs), _ptr(scores)))
        return docs, scores

    def search_filtered_device(self, d_queries, k: int, d_masks, d_query_mask, d_docs, d_scores,
                               stream=None) -> None:
        """Device-resident search_filtered (bm25_search_filtered_device): torch
        int32 [Q, T] queries, packed masks [M, W] (int32 or uint32 storage),
        int32 [Q] mask ids (or None: mask 0 for every query) in, int32 / float32
        [Q, k] out, enqueued on ``stream``.  No validation: token ids >=
        n_terms are padding and the mask ids must be in [-1, M).  It may
        synchronise ``stream`` once, to count the queries whose candidate list
        overflowed (they take the dense path)."""
        Q, T, M = self._ranked_device_args(d_queries, None, d_masks, d_query_mask,
                                           need_masks=True)
        k = int(k)
        self._device_out(d_docs, d_scores, Q, k)
        check(lib.bm25_search_filtered_device(
            self._h, _dptr(d_queries), Q, T, k, _dptr(d_masks) if M else None, M,
            _dptr(d_query_mask), _dptr(d_docs), _dptr(d_scores), ctypes.c_void_p(_stream(stream))))

    def filtered_stats(self) -> Tuple[int, int, int]:
        """Counters of the last filtered search (bm25_search_filtered_stats):
        queries served by the dense path, (query, tile) pairs pass A skipped
        on an empty census, pairs pass B re-scored."""
        v = (ctypes.c_int64 * 3)()
        check(lib.bm25_search_filtered_stats(self._h, v, 3))
        return int(v[0]), int(v[1]), int(v[2])

    # ------------------------------------------------- weighted query terms
    @staticmethod
    def _weights_arg(q: np.ndarray, weights) -> np.ndarray:
        """weights -> float32 of the queries' [Q, T] shape (shape errors raised
        here, before any C call)."""
        w = np.ascontiguousarray(weights, dtype=np.float32)
        if w.ndim != 2 or w.shape != q.shape:
            raise ValueError(f"weights must be a float32 array of the queries' shape {q.shape}, "
                             f"got shape {w.shape}")
        return w

    def search_weighted(self, queries: np.ndarray, weights, k: int, masks=None,
                        query_mask=None) -> Tuple[np.ndarray, np.ndarray]:
        """Top-k under weighted query terms (bm25_search_weighted, host
        arrays): queries int32 [Q, T], weights float32 [Q, T], one weight per
        slot.  A document's score is the fp32 sum, in query order from +0.0, of
        float32(weight * value) over the terms it holds — 1.0 everywhere is
        search / search_filtered bit for bit, a weight of 0.0 is the same as
        padding; the weight of a padding slot is ignored, every other must be
        finite.  masks / query_mask as in search_filtered; masks None: no
        filter (query_mask must then be None or all -1)."""
        q, w, m, M, qm = self._ranked_args(queries, weights, masks, query_mask, need_weights=True)
        Q, T = q.shape
        k = int(k)
        docs, scores = _topk_out(Q, k)
        check(lib.bm25_search_weighted(self._h, _ptr(q), _ptr(w), Q, T, k, _ptr(m) if M else None,
                                       M, _ptr(qm), _ptr(docs), _ptr(scores)))
        return docs, scores

    def search_weighted_device(self, d_queries, d_weights, k: int, d_masks, d_query_mask, d_docs,
                               d_scores, stream=None) -> None:
        """Device-resident search_weighted (bm25_search_weighted_device): torch
        int32 [Q, T] queries, float32 [Q, T] weights, packed masks [M, W] (or
        None: no masks) and int32 [Q] mask ids (or None: mask 0 for every
        query; without masks, no filter) in, int32 / float32 [Q, k] out,
        enqueued on ``stream``.  No validation: token ids >= n_terms are
        padding, the weights of non-padding slots must be finite and the mask
        ids in [-1, M).  It may synchronise ``stream`` once, as
        search_filtered_device."""
        Q, T, M = self._ranked_device_args(d_queries, d_weights, d_masks, d_query_mask,
                                           need_weights=True)
        k = int(k)
        self._device_out(d_docs, d_scores, Q, k)
        check(lib.bm25_search_weighted_device(
            self._h, _dptr(d_queries), _dptr(d_weights), Q, T, k, _dptr(d_masks) if M else None,
            M, _dptr(d_query_mask), _dptr(d_docs), _dptr(d_scores),
            ctypes.c_void_p(_stream(stream))))

    # ---------------------------------------------------- cursor pagination
    @staticmethod
    def _after_arg(after, Q: int):
        """The ``after`` of search_after -> (float32 [Q] scores, int32 [Q] docs),
        or (None, None): no cursor."""
        if after is None:
            return None, None
        if not isinstance(after, (tuple, list)) or len(after) != 2:
            raise ValueError("after must be None or a pair (scores [Q], docs [Q])")
        if after[0] is None or after[1] is None:
            raise ValueError("after needs both halves: (scores [Q], docs [Q])")
        a_s, a_d = np.asarray(after[0]), np.asarray(after[1])
        if a_s.dtype != np.float32 or a_d.dtype != np.int32:
            raise ValueError("after must be (float32 scores, int32 docs): page_cursor's pair")
        if a_s.shape != (Q,) or a_d.shape != (Q,):
            raise ValueError(f"after must hold one cursor per query ({Q}), got shapes "
                             f"{a_s.shape} and {a_d.shape}")
        a_s, a_d = np.ascontiguousarray(a_s), np.ascontiguousarray(a_d)
        if a_d.size and int(a_d.min()) < AFTER_NONE:
            raise ValueError(f"after docs must be >= AFTER_NONE ({AFTER_NONE})")
        if bool((np.isnan(a_s) & (a_d >= 0)).any()):
            raise ValueError("after scores must not be NaN where after docs name a document")
        return a_s, a_d

    def search_after(self, queries: np.ndarray, k: int, after=None, weights=None, masks=None,
                     query_mask=None) -> Tuple[np.ndarray, np.ndarray]:
        """The next k results after a cursor (bm25_search_after, host arrays):
        ``after`` is None (no cursor: the first page) or a pair (scores [Q]
        float32, docs [Q] int32) — page_cursor of the previous page — and row
        q holds the first k documents strictly after (after_scores[q],
        after_docs[q]) in the result order (score descending, doc id
        ascending; global ids).  after_docs[q] == AFTER_NONE: no cursor for
        that row; -1: the list is exhausted, the row is all padding.  weights
        (None: plain sums), masks and query_mask as in search_weighted."""
        q, w, m, M, qm = self._ranked_args(queries, weights, masks, query_mask)
        Q, T = q.shape
        a_s, a_d = self._after_arg(after, Q)
        k = int(k)
        docs, scores = _topk_out(Q, k)
        check(lib.bm25_search_after(self._h, _ptr(q), _ptr(w), Q, T, k, _ptr(m) if M else None, M,
                                    _ptr(qm), _ptr(a_s), _ptr(a_d), _ptr(docs), _ptr(scores)))
        return docs, scores

    def search_after_device(self, d_queries, k: int, d_after, d_weights, d_masks, d_query_mask,
                            d_docs, d_scores, stream=None) -> None:
        """Device-resident search_after (bm25_search_after_device): torch int32
        [Q, T] queries, ``d_after`` None or a pair (float32 [Q] scores, int32
        [Q] docs), float32 [Q, T] weights (or None), packed masks [M, W] (or
        None) and int32 [Q] mask ids (or None) in, int32 / float32 [Q, k] out,
        enqueued on ``stream``.  No validation: an after-docs entry < -1 is
        "no cursor", a NaN cursor score leaves its row unspecified.  It may
        synchronise ``stream`` once, as search_filtered_device."""
        Q, T, M = self._ranked_device_args(d_queries, d_weights, d_masks, d_query_mask)
        a_s = a_d = None
        if d_after is not None:
            if not isinstance(d_after, (tuple, list)) or len(d_after) != 2:
                raise ValueError("d_after must be None or a pair (scores [Q], docs [Q])")
            a_s, a_d = d_after
            if a_s is None or a_d is None:
                raise ValueError("d_after needs both halves: (scores [Q], docs [Q])")
            if (tuple(a_s.shape) != (Q,) or tuple(a_d.shape) != (Q,)
                    or not a_s.dtype.is_floating_point or a_s.element_size() != 4
                    or a_d.dtype.is_floating_point or a_d.element_size() != 4
                    or not a_s.is_contiguous() or not a_d.is_contiguous()):
                raise ValueError(f"d_after must be contiguous (float32 [{Q}], int32 [{Q}]) tensors")
        k = int(k)
        self._device_out(d_docs, d_scores, Q, k)
        check(lib.bm25_search_after_device(
            self._h, _dptr(d_queries), _dptr(d_weights), Q, T, k, _dptr(d_masks) if M else None, M,
            _dptr(d_query_mask), _dptr(a_s), _dptr(a_d), _dptr(d_docs), _dptr(d_scores),
            ctypes.c_void_p(_stream(stream))))

    # ------------------------------------------------------ field collapsing
    COLLAPSE_MAX_K = 4096   # the per-row group table lives in LDS

    @classmethod
    def _collapse_args(cls, k, per_group) -> Tuple[int, int]:
        k, per_group = int(k), int(per_group)
        if k > cls.COLLAPSE_MAX_K:
            raise ValueError(f"k={k}: a collapsed search is limited to k <= {cls.COLLAPSE_MAX_K} "
                             "(the per-row group table lives in LDS)")
        if per_group < 1:
            raise ValueError(f"per_group={per_group} must be >= 1")
        return k, per_group

    def search_collapsed(self, queries: np.ndarray, k: int, groups, per_group: int = 1,
                         weights=None, masks=None, query_mask=None, return_groups: bool = False):
        """Top-k with at most ``per_group`` hits of every group
        (bm25_search_collapsed, host arrays): ``groups`` int32 [n_docs] by
        this handle's own documents — any value >= 0 is a group (the codes of
        bm25mi.facet_codes, a hashed host name), a value < 0 means no group.
        Row q is the walk of search_weighted's full order under its mask that
        keeps a document while its group has room, the first k kept, padded
        (doc -1, score bits ~0).  weights (None: plain sums), masks and
        query_mask as in search_after.  k <= 4096.  Returns (docs, scores), and
        the hits' groups (-1 in padding) as a third array with
        ``return_groups``."""
        q, w, m, M, qm = self._ranked_args(queries, weights, masks, query_mask)
        Q, T = q.shape
        g = np.asarray(groups)
        if g.dtype.kind not in "iu" or g.ndim != 1 or g.size != self.n_docs:
            raise ValueError(f"groups must be an integer array of {self.n_docs} (n_docs) entries, "
                             f"got {g.dtype} of shape {g.shape}")
        if g.size and (int(g.max()) > 2**31 - 1 or int(g.min()) < -2**31):
            raise ValueError("groups must fit int32")
        g = np.ascontiguousarray(g, dtype=np.int32)
        k, per_group = self._collapse_args(k, per_group)
        docs, scores = _topk_out(Q, k)
        og = np.zeros((Q, max(k, 0)), np.int32) if return_groups else None
        check(lib.bm25_search_collapsed(self._h, _ptr(q), _ptr(w), Q, T, k,
                                        _ptr(m) if M else None, M, _ptr(qm), _ptr(g), per_group,
                                        _ptr(docs), _ptr(scores), _ptr(og)))
        return (docs, scores, og) if return_groups else (docs, scores)

    def search_collapsed_device(self, d_queries, k: int, d_groups, per_group, d_weights, d_masks,
                                d_query_mask, d_docs, d_scores, d_groups_out=None,
                                stream=None) -> None:
        """Device-resident search_collapsed (bm25_search_collapsed_device):
        torch int32 [Q, T] queries, int32 [n_docs] groups, float32 [Q, T]
        weights (or None), packed masks [M, W] (or None) and int32 [Q] mask ids
        (or None) in; int32 / float32 [Q, k] docs and scores and, optionally,
        int32 [Q, k] groups out, enqueued on ``stream``.  No validation of
        token ids, weights or mask ids.  It synchronises ``stream`` once per
        round (one round where no row's first 2 k results overfill a
        group)."""
        Q, T, M = self._ranked_device_args(d_queries, d_weights, d_masks, d_query_mask)
        if (d_groups.dim() != 1 or d_groups.numel() != self.n_docs or d_groups.element_size() != 4
                or d_groups.dtype.is_floating_point or not d_groups.is_contiguous()):
            raise ValueError(f"d_groups must be a contiguous int32 [{self.n_docs}] (n_docs) tensor")
        k, per_group = self._collapse_args(k, per_group)
        self._device_out(d_docs, d_scores, Q, k)
        if d_groups_out is not None and (d_groups_out.numel() != Q * k
                                         or d_groups_out.element_size() != 4):
            raise ValueError(f"d_groups_out must hold {Q} x {k} int32 groups")
        check(lib.bm25_search_collapsed_device(
            self._h, _dptr(d_queries), _dptr(d_weights), Q, T, k, _dptr(d_masks) if M else None, M,
            _dptr(d_query_mask), _dptr(d_groups), per_group, _dptr(d_docs), _dptr(d_scores),
            _dptr(d_groups_out), ctypes.c_void_p(_stream(stream))))

    def collapse_stats(self) -> dict:
        """Counters of the last collapsed search (bm25_search_collapsed_stats):
        rounds (the most any row took), rows unfinished after round 1, page
        entries dropped as over-quota, rows served under exclusion masks
        (summed over the rounds)."""
        v = (ctypes.c_int64 * 4)()
        check(lib.bm25_search_collapsed_stats(self._h, v, 4))
        return {"rounds": int(v[0]), "unfinished_rows": int(v[1]),
                "dropped_entries": int(v[2]), "excluded_rows": int(v[3])}

    def score_docs_weighted(self, queries, weights, docs) -> np.ndarray:
        """score_docs under weighted query terms (bm25_score_docs_weighted,
        host arrays): out[q, c] is bit for bit the score search_weighted
        reports for docs[q, c] under (queries[q], weights[q])."""
        q = np.ascontiguousarray(queries, dtype=np.int32)
        d = np.ascontiguousarray(docs, dtype=np.int32)
        if q.ndim != 2:
            raise ValueError("queries must be a 2-D [Q, T] int32 array")
        w = self._weights_arg(q, weights)
        if d.ndim != 2:
            raise ValueError("docs must be a 2-D [Q, C] int32 array")
        if q.shape[0] != d.shape[0]:
            raise ValueError(f"queries has {q.shape[0]} rows, docs has {d.shape[0]}")
        out = np.zeros(d.shape, np.float32)
        check(lib.bm25_score_docs_weighted(self._h, _ptr(q), _ptr(w), q.shape[0], q.shape[1],
                                           _ptr(d), d.shape[1], _ptr(out)))
        return out

    def score_docs_weighted_device(self, d_queries, d_weights, d_docs, d_scores,
                                   stream=None) -> None:
        """Device-resident score_docs_weighted (bm25_score_docs_weighted_device):
        as score_docs_device with float32 [Q, T] weights beside the queries —
        no host synchronisation, no validation, the index arrays only; doc ids
        outside this handle's range score +0.0, so doc shards add up."""
        if d_queries.dim() != 2 or d_docs.dim() != 2:
            raise ValueError("d_queries and d_docs must be 2-D [Q, T] and [Q, C] tensors")
        Q, T = d_queries.shape
        if (tuple(d_weights.shape) != (Q, T) or not d_weights.dtype.is_floating_point
                or d_weights.element_size() != 4):
            raise ValueError(f"d_weights must be a float32 [{Q}, {T}] tensor")
        if d_docs.shape[0] != Q:
            raise ValueError(f"d_queries has {Q} rows, d_docs has {d_docs.shape[0]}")
        C = d_docs.shape[1]
        if d_scores.numel() != Q * C:
            raise ValueError(f"d_scores must hold {Q} x {C} scores")
        s = _stream(stream)
        check(lib.bm25_score_docs_weighted_device(
            self._h, ctypes.c_void_p(d_queries.data_ptr()), ctypes.c_void_p(d_weights.data_ptr()),
            Q, T, ctypes.c_void_p(d_docs.data_ptr()), C, ctypes.c_void_p(d_scores.data_ptr()),
            ctypes.c_void_p(s)))

    # -------------------------------------------------- boolean term filters
    def _clauses_arg(self, must, any, must_not, base, rows=None):
        """The clause rows of term_masks / search_boolean: each of must, any,
        must_not an int32 [M, width] array, a ragged list of lists of token
        ids (padded with -1 here) or None (an empty clause); base as
        search_filtered's masks, 1 or M rows, or None.  ``rows``: the row
        count the caller fixes (the queries of search_boolean).  Returns
        (must, any, must_not, M, base, Mb); shape errors are raised here,
        before any C call."""
        out, M = [], rows
        for name, c in (("must", must), ("any", any), ("must_not", must_not)):
            if c is None:
                out.append(None)
                continue
            a = pad_clause(c)
            if M is None:
                M = a.shape[0]
            elif a.shape[0] != M:
                raise ValueError(f"{name} has {a.shape[0]} rows, expected {M} (one per "
                                 f"{'query' if rows is not None else 'mask'})")
            out.append(a)
        b, Mb = None, 0
        if base is not None:
            b = self._masks_arg(base)
            Mb = b.shape[0]
            if M is None:
                M = Mb
            elif Mb not in (1, M):
                raise ValueError(f"base has {Mb} rows, expected 1 or {M}")
        if M is None:
            raise ValueError("no clause and no base given: the number of masks is unknown")
        out = [np.zeros((M, 0), np.int32) if a is None else a for a in out]
        return out[0], out[1], out[2], M, b, Mb

    def term_masks(self, must=None, any=None, must_not=None, base=None, *,
                   min_match=None) -> np.ndarray:
        """Allow-masks of boolean term filters (bm25_term_masks, host arrays)
        -> packed uint32 [M, W], W = ceil(n_docs / 32), the masks
        search_filtered takes: row m allows the documents of this handle that
        hold every term of must[m], at least one of any[m] (when it names
        one), none of must_not[m], and that base allows.  Clauses: int32
        [M, width] arrays or ragged lists of lists (negative ids = padding);
        base: bool [n_docs] / [M, n_docs] or packed uint32 rows, 1 or M.
        min_match (bm25_term_masks_min_match): row m needs min_match[m] of the
        slots of any[m] that hold an id (a repeated id counts each time; 0:
        the clause is optional) — what min_match_rows takes: an int, an int
        [M] array or "NN%"."""
        mu, an, mn, M, b, Mb = self._clauses_arg(must, any, must_not, base)
        mm = None if min_match is None else min_match_rows(an, min_match)
        out = np.zeros((M, (self.n_docs + 31) // 32), np.uint32)
        if mm is None:
            check(lib.bm25_term_masks(self._h, _ptr(mu), mu.shape[1], _ptr(an), an.shape[1],
                                      _ptr(mn), mn.shape[1], M, _ptr(b) if Mb else None, Mb,
                                      _ptr(out)))
        else:
            check(lib.bm25_term_masks_min_match(
                self._h, _ptr(mu), mu.shape[1], _ptr(an), an.shape[1], _ptr(mn), mn.shape[1],
                _ptr(mm), M, _ptr(b) if Mb else None, Mb, _ptr(out)))
        return out

    def term_masks_device(self, d_must, d_any, d_must_not, d_base, d_out, stream=None, *,
                          d_min_match=None) -> None:
        """Device-resident term_masks (bm25_term_masks_device): torch int32
        [M, width] clause tensors (or None: an empty clause), packed base
        masks [1 or M, W] (or None) in, packed masks d_out [M, W] (32-bit
        words) out, enqueued on ``stream`` with no host synchronisation and no
        validation of ids — an id >= n_terms is a term that no document has.
        Reads the index arrays only, so it may overlap a search of the same
        handle on another stream.  d_min_match: int32 [M] on the device
        (bm25_term_masks_min_match_device; entries <= 0: the any clause is
        optional)."""
        W = (self.n_docs + 31) // 32
        if d_out.dim() != 2 or d_out.shape[1] != W or d_out.element_size() != 4:
            raise ValueError(f"d_out must be a packed [M, {W}] tensor of 32-bit words")
        M = d_out.shape[0]
        if d_min_match is not None and (d_min_match.dim() != 1 or d_min_match.shape[0] != M
                                        or d_min_match.element_size() != 4
                                        or d_min_match.is_floating_point()):
            raise ValueError(f"d_min_match must be an int32 [{M}] tensor (one entry per mask)")
        args = []
        for name, c in (("d_must", d_must), ("d_any", d_any), ("d_must_not", d_must_not)):
            if c is None:
                args += [None, 0]
                continue
            if c.dim() != 2 or c.element_size() != 4:
                raise ValueError(f"{name} must be a 2-D [M, width] int32 tensor")
            if c.shape[0] != M:
                raise ValueError(f"{name} has {c.shape[0]} rows, d_out has {M}")
            args += [ctypes.c_void_p(c.data_ptr()) if c.shape[1] else None, c.shape[1]]
        Mb = 0
        if d_base is not None:
            if d_base.dim() != 2 or d_base.shape[1] != W or d_base.element_size() != 4:
                raise ValueError(f"d_base must be a packed [1 or M, {W}] tensor of 32-bit words")
            Mb = d_base.shape[0]
            if Mb not in (1, M):
                raise ValueError(f"d_base has {Mb} rows, expected 1 or {M}")
        s = _stream(stream)
        if d_min_match is None:
            check(lib.bm25_term_masks_device(
                self._h, *args, M, ctypes.c_void_p(d_base.data_ptr()) if Mb else None, Mb,
                ctypes.c_void_p(d_out.data_ptr()), ctypes.c_void_p(s)))
        else:
            check(lib.bm25_term_masks_min_match_device(
                self._h, *args, ctypes.c_void_p(d_min_match.data_ptr()) if M else None, M,
                ctypes.c_void_p(d_base.data_ptr()) if Mb else None, Mb,
                ctypes.c_void_p(d_out.data_ptr()), ctypes.c_void_p(s)))

    def mask_count(self, masks) -> np.ndarray:
        """The number of documents every mask allows (bm25_mask_count, host
        arrays) -> int64 [M]: the set bits of each row among this handle's
        n_docs documents (bits past n_docs of a packed row are ignored).
        masks as search_filtered takes them: bool or packed uint32 rows."""
        m = self._masks_arg(masks)
        out = np.zeros(m.shape[0], np.int64)
        check(lib.bm25_mask_count(self._h, _ptr(m) if m.size else None, m.shape[0], _ptr(out)))
        return out

    def mask_count_device(self, d_masks, d_counts, stream=None) -> None:
        """Device-resident mask_count (bm25_mask_count_device): packed masks
        [M, W] (32-bit words) in, int64 [M] counts out (they need not be
        zeroed), enqueued on ``stream`` with no host synchronisation.  Reads
        the masks only, so it may overlap a search of the same handle."""
        W = (self.n_docs + 31) // 32
        if d_masks.dim() != 2 or d_masks.shape[1] != W or d_masks.element_size() != 4:
            raise ValueError(f"d_masks must be a packed [M, {W}] tensor of 32-bit words")
        M = d_masks.shape[0]
        if (d_counts.dim() != 1 or d_counts.shape[0] != M or d_counts.element_size() != 8
                or d_counts.is_floating_point() or not d_counts.is_contiguous()):
            raise ValueError(f"d_counts must be an int64 [{M}] tensor (one count per mask)")
        if not d_masks.is_contiguous():
            raise ValueError("d_masks must be contiguous")
        s = _stream(stream)
        check(lib.bm25_mask_count_device(
            self._h, ctypes.c_void_p(d_masks.data_ptr()) if M and W else None, M,
            ctypes.c_void_p(d_counts.data_ptr()) if M else None, ctypes.c_void_p(s)))

    def facets(self, masks, groups, n_groups) -> np.ndarray:
        """Facet counts (bm25_mask_facets, host arrays) -> int64 [M, G]:
        out[m][g] = the documents of this handle that mask m allows and whose
        group is g.  masks as mask_count takes them; groups: any integer array
        of n_docs entries (group ids in [0, n_groups); negative: the document
        has no group; bm25mi.facet_codes turns labels into ids), converted to
        contiguous int32.  A group id >= n_groups is a ValueError."""
        m = self._masks_arg(masks)
        g, G = _facet_groups(groups, n_groups, self.n_docs)
        out = np.zeros((m.shape[0], G), np.int64)
        check(lib.bm25_mask_facets(self._h, _ptr(m) if m.size else None, m.shape[0],
                                   _ptr(g) if g.size else None, G, _ptr(out) if out.size else None))
        return out

    def facets_device(self, d_masks, d_groups, n_groups, d_counts, stream=None) -> None:
        """Device-resident facets (bm25_mask_facets_device): packed masks
        [M, W] (32-bit words) and int32 groups [n_docs] in, int64 [M, G]
        counts out (they need not be zeroed), enqueued on ``stream`` with no
        host synchronisation.  A group id outside [0, n_groups) counts nowhere.
        Reads the masks and groups only, so it may overlap a search of the
        same handle."""
        W = (self.n_docs + 31) // 32
        if d_masks.dim() != 2 or d_masks.shape[1] != W or d_masks.element_size() != 4:
            raise ValueError(f"d_masks must be a packed [M, {W}] tensor of 32-bit words")
        M = d_masks.shape[0]
        if isinstance(n_groups, bool) or not isinstance(n_groups, (int, np.integer)):
            raise ValueError("n_groups must be an int")
        G = int(n_groups)
        if G < 0 or G > np.iinfo(np.int32).max:
            raise ValueError(f"n_groups = {G} must be in 0 .. 2^31 - 1")
        if (d_groups.dim() != 1 or d_groups.shape[0] != self.n_docs or d_groups.element_size() != 4
                or d_groups.is_floating_point() or not d_groups.is_contiguous()):
            raise ValueError(f"d_groups must be an int32 [{self.n_docs}] tensor (one group per "
                             "document)")
        if (d_counts.dim() != 2 or tuple(d_counts.shape) != (M, G) or d_counts.element_size() != 8
                or d_counts.is_floating_point() or not d_counts.is_contiguous()):
            raise ValueError(f"d_counts must be an int64 [{M}, {G}] tensor (one row per mask)")
        if not d_masks.is_contiguous():
            raise ValueError("d_masks must be contiguous")
        s = _stream(stream)
        check(lib.bm25_mask_facets_device(
            self._h, ctypes.c_void_p(d_masks.data_ptr()) if M and W else None, M,
            ctypes.c_void_p(d_groups.data_ptr()) if self.n_docs else None, G,
            ctypes.c_void_p(d_counts.data_ptr()) if M and G else None, ctypes.c_void_p(s)))

    def stats(self, masks, values, groups=None, n_groups=0) -> dict:
        """Field statistics (bm25_mask_stats, host arrays) -> a dict of [M, B]
        arrays {count, min, max, sum, mean}: of the documents of this handle
        that mask m allows, whose group is b (groups=None: B = 1, every allowed
        document) and whose value is a number (a float32 NaN is no value),
        count int64, min and max of the values' dtype, sum int64 (integer
        columns; int64 wraps) or float64 (float32 columns: the exact sum of
        the values rounded once — bit-equal to math.fsum, whatever the
        scheduling), and mean = float64 sum / count, NaN where count is 0.
        values: [n_docs] int32, int64 or float32 exactly; masks as mask_count
        takes them; groups and n_groups as facets takes them."""
        m = self._masks_arg(masks)
        v, kind = _sort_values_arg(values, self.n_docs)
        g, G = (None, 0)
        if groups is not None:
            g, G = _facet_groups(groups, n_groups, self.n_docs)
            if G == 0:
                raise ValueError("n_groups = 0 with groups: give the number of groups, or "
                                 "groups=None for one bucket per mask")
        elif n_groups != 0:
            raise ValueError(f"n_groups = {n_groups} without groups")
        M, B = m.shape[0], G or 1
        out = {"count": np.zeros((M, B), np.int64), "min": np.zeros((M, B), v.dtype),
               "max": np.zeros((M, B), v.dtype),
               "sum": np.zeros((M, B), np.float64 if v.dtype.kind == "f" else np.int64)}
        p = lambda a: _ptr(a) if a is not None and a.size else None
        # (grouped with no document: a non-NULL groups pointer still says "grouped")
        pg = None if g is None else _ptr(g if g.size else np.zeros(1, np.int32))
        check(lib.bm25_mask_stats(self._h, p(m), M, p(v), kind, pg, G, p(out["count"]),
                                  p(out["min"]), p(out["max"]), p(out["sum"])))
        with np.errstate(divide="ignore", invalid="ignore"):
            out["mean"] = np.where(out["count"] > 0,
                                   out["sum"].astype(np.float64) / out["count"], np.nan)
        return out

    def stats_scratch_bytes(self, dtype, M: int, n_groups: int = 0) -> int:
        """Bytes of the d_scratch of stats_device for a column dtype (int32,
        int64 or float32), M mask rows and n_groups (0: ungrouped)
        (bm25_mask_stats_scratch)."""
        dt = np.dtype(dtype)
        if dt not in _SORT_KINDS:
            raise ValueError(f"dtype {dt.name}: int32, int64 or float32")
        b = ctypes.c_int64(0)
        check(lib.bm25_mask_stats_scratch(self._h, _SORT_KINDS[dt], int(M), int(n_groups),
                                          ctypes.byref(b)))
        return int(b.value)

    def stats_device(self, d_masks, d_values, d_count, d_min=None, d_max=None, d_sum=None,
                     d_groups=None, n_groups=0, d_scratch=None, stream=None) -> None:
        """Device-resident stats (bm25_mask_stats_device): packed masks [M, W]
        (32-bit words), a column [n_docs] (int32, int64 or float32) and
        optionally int32 groups [n_docs] in; d_count int64 [M, B] and, each
        optional, d_min / d_max [M, B] of the column's dtype and d_sum [M, B]
        (int64, or float64 for a float32 column) out, B = n_groups or 1; they
        need not be cleared.  d_scratch: a contiguous tensor of at least
        stats_scratch_bytes(dtype, M, n_groups) bytes, 8-byte aligned (None:
        allocated here, on the current device).  Enqueued on ``stream`` with no
        host synchronisation.  A group id outside [0, n_groups) is in no
        bucket.  Reads the caller's tensors only, so it may overlap a search of
        the same handle."""
        import torch
        W = (self.n_docs + 31) // 32
        kinds = {torch.int32: 0, torch.float32: 1, torch.int64: 2}
        if d_masks.dim() != 2 or d_masks.shape[1] != W or d_masks.element_size() != 4:
            raise ValueError(f"d_masks must be a packed [M, {W}] tensor of 32-bit words")
        if not d_masks.is_contiguous():
            raise ValueError("d_masks must be contiguous")
        M = d_masks.shape[0]
        if d_values.dtype not in kinds:
            raise ValueError(f"d_values has dtype {d_values.dtype}: int32, int64 or float32")
        if d_values.dim() != 1 or d_values.shape[0] != self.n_docs or not d_values.is_contiguous():
            raise ValueError(f"d_values must be a contiguous [{self.n_docs}] tensor (one entry "
                             "per document)")
        if isinstance(n_groups, bool) or not isinstance(n_groups, (int, np.integer)):
            raise ValueError("n_groups must be an int")
        G = int(n_groups)
        if G < 0 or G > np.iinfo(np.int32).max:
            raise ValueError(f"n_groups = {G} must be in 0 .. 2^31 - 1")
        if (d_groups is None) != (G == 0):
            raise ValueError("d_groups and n_groups come together (d_groups=None with "
                             "n_groups=0: one bucket per mask)")
        if d_groups is not None and (
                d_groups.dim() != 1 or d_groups.shape[0] != self.n_docs
                or d_groups.dtype != torch.int32 or not d_groups.is_contiguous()):
            raise ValueError(f"d_groups must be an int32 [{self.n_docs}] tensor (one group per "
                             "document)")
        B = G or 1
        sum_dtype = torch.float64 if d_values.dtype == torch.float32 else torch.int64
        for name, t, dt, need in (("d_count", d_count, torch.int64, True),
                                  ("d_min", d_min, d_values.dtype, False),
                                  ("d_max", d_max, d_values.dtype, False),
                                  ("d_sum", d_sum, sum_dtype, False)):
            if t is None and not need:
                continue
            if (t is None or t.dim() != 2 or tuple(t.shape) != (M, B) or t.dtype != dt
                    or not t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous {dt} [{M}, {B}] tensor (one row "
                                 "per mask)")
        kind = kinds[d_values.dtype]
        need = 8 * M * B * (36 if kind == 1 else 4)
        s = _stream(stream)
        if d_scratch is None:
            # allocated on the call's stream, so the allocator hands the block
            # on only after the kernels enqueued here
            dev = d_masks.device
            ts = torch.cuda.ExternalStream(s, device=dev) if s else torch.cuda.default_stream(dev)
            with torch.cuda.stream(ts):
                d_scratch = torch.empty(max(need, 8), dtype=torch.uint8, device=dev)
        nbytes = d_scratch.numel() * d_scratch.element_size()
        if not d_scratch.is_contiguous() or nbytes < need or d_scratch.data_ptr() % 8:
            raise ValueError(f"d_scratch must be a contiguous, 8-byte aligned tensor of at least "
                             f"{need} bytes (stats_scratch_bytes)")
        p = lambda t, n: ctypes.c_void_p(t.data_ptr()) if t is not None and n else None
        pg = None if d_groups is None else ctypes.c_void_p(d_groups.data_ptr() or 8)
        check(lib.bm25_mask_stats_device(
            self._h, p(d_masks, M and W), M, p(d_values, self.n_docs), kind, pg, G,
            p(d_count, M), p(d_min, M), p(d_max, M), p(d_sum, M),
            ctypes.c_void_p(d_scratch.data_ptr()), nbytes, ctypes.c_void_p(s)))

    def range_masks(self, values, fields, lo, hi, base=None) -> np.ndarray:
        """Allow-masks of numeric range filters (bm25_range_masks, host arrays)
        -> packed uint32 [M, W], the masks search_filtered takes: row m allows
        the documents of this handle that base allows and with
        lo[m][c] <= values[fields[m][c]][d] <= hi[m][c] for every clause c whose
        field id is not negative (padding).  values: [n_docs] or [F, n_docs],
        int32, int64 or float32 exactly (anything else is a ValueError: nothing
        is rounded); lo, hi: [M, C] (or [M]: one clause a row) of the values'
        dtype, both inclusive, the dtype's limits or +-inf as open ends
        (bm25mi.range_rows makes the three of dicts); fields: int [M, C], or
        None with one field: field 0 for every clause; base as term_masks'."""
        v, kind, f, lo_a, hi_a = _range_args(values, fields, lo, hi, self.n_docs)
        M, C = f.shape
        b, Mb = None, 0
        if base is not None:
            b = self._masks_arg(base)
            Mb = b.shape[0]
            if Mb not in (1, M):
                raise ValueError(f"base has {Mb} rows, expected 1 or {M}")
        out = np.zeros((M, (self.n_docs + 31) // 32), np.uint32)
        check(lib.bm25_range_masks(self._h, _ptr(v) if v.size else None, kind, v.shape[0],
                                   _ptr(f) if f.size else None, _ptr(lo_a) if f.size else None,
                                   _ptr(hi_a) if f.size else None, C, M,
                                   _ptr(b) if Mb and b.size else None, Mb,
                                   _ptr(out) if out.size else None))
        return out

    def range_masks_device(self, d_values, d_fields, d_lo, d_hi, d_out, d_base=None,
                           stream=None) -> None:
        """Device-resident range_masks (bm25_range_masks_device): torch values
        [n_docs] or [F, n_docs] (int32, int64 or float32), int32 fields and
        bounds of the values' dtype [M, C], packed base masks [1 or M, W] (or
        None) in, packed masks d_out [M, W] (32-bit words) out, enqueued on
        ``stream`` with no host synchronisation and no validation of values: a
        field id >= F is a field that no document has, a NaN bound matches
        nothing.  Reads the caller's tensors only, so it may overlap a search
        of the same handle.  d_base and d_out must not overlap."""
        import torch
        W = (self.n_docs + 31) // 32
        kinds = {torch.int32: 0, torch.float32: 1, torch.int64: 2}
        if d_values.dtype not in kinds:
            raise ValueError(f"d_values has dtype {d_values.dtype}: int32, int64 or float32")
        if (d_values.dim() not in (1, 2) or d_values.shape[-1] != self.n_docs
                or not d_values.is_contiguous()):
            raise ValueError(f"d_values must be a contiguous [{self.n_docs}] or "
                             f"[F, {self.n_docs}] tensor (one entry per document)")
        F = 1 if d_values.dim() == 1 else d_values.shape[0]
        if (d_out.dim() != 2 or d_out.shape[1] != W or d_out.element_size() != 4
                or not d_out.is_contiguous()):
            raise ValueError(f"d_out must be a contiguous packed [M, {W}] tensor of 32-bit words")
        M = d_out.shape[0]
        if (d_fields.dim() != 2 or d_fields.shape[0] != M or d_fields.dtype != torch.int32
                or not d_fields.is_contiguous()):
            raise ValueError(f"d_fields must be a contiguous int32 [{M}, C] tensor (one row per "
                             "mask)")
        C = d_fields.shape[1]
        for name, t in (("d_lo", d_lo), ("d_hi", d_hi)):
            if (t.dtype != d_values.dtype or tuple(t.shape) != (M, C) or not t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous {d_values.dtype} [{M}, {C}] tensor "
                                 "(the values' dtype, the shape of d_fields)")
        Mb = 0
        if d_base is not None:
            if (d_base.dim() != 2 or d_base.shape[1] != W or d_base.element_size() != 4
                    or not d_base.is_contiguous()):
                raise ValueError(f"d_base must be a contiguous packed [1 or M, {W}] tensor of "
                                 "32-bit words")
            Mb = d_base.shape[0]
            if Mb not in (1, M):
                raise ValueError(f"d_base has {Mb} rows, expected 1 or {M}")
        s = _stream(stream)
        p = lambda t, n: ctypes.c_void_p(t.data_ptr()) if n else None
        check(lib.bm25_range_masks_device(
            self._h, p(d_values, F and self.n_docs), kinds[d_values.dtype], F, p(d_fields, M * C),
            p(d_lo, M * C), p(d_hi, M * C), C, M, p(d_base, Mb and W), Mb, p(d_out, M and W),
            ctypes.c_void_p(s)))

    # ------------------------------------------------- sort-by-field search
    def sort_ranks(self, values, descending: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """The order of this handle's documents by a column (bm25_sort_ranks,
        host arrays) -> (ranks, perm), int32 [n_docs] each: perm[r] = the
        document at rank r, ranks[d] = the rank of document d.  values: [n_docs]
        int32, int64 or float32 exactly.  Numbers in numeric order (-0.0 equals
        +0.0; int64 never through a float), reversed by ``descending``; NaN
        after every number in both directions; equal values by doc id
        ascending.  Built once per column and direction, the pair is the
        ``order`` of search_sorted and the ``sort`` of search_boolean."""
        v, kind = _sort_values_arg(values, self.n_docs)
        ranks = np.zeros(self.n_docs, np.int32)
        perm = np.zeros(self.n_docs, np.int32)
        check(lib.bm25_sort_ranks(self._h, _ptr(v) if v.size else None, kind,
                                  1 if descending else 0, _ptr(ranks) if v.size else None,
                                  _ptr(perm) if v.size else None))
        return ranks, perm

    def sort_ranks_device(self, d_values, d_ranks, d_perm, descending: bool = False,
                          stream=None) -> None:
        """Device-resident sort_ranks (bm25_sort_ranks_device): a torch
        [n_docs] column (int32, int64 or float32) in, int32 [n_docs] ranks and
        perm out.  A setup call: it allocates the sort's buffers (about 24 bytes
        per document), synchronises ``stream`` and frees them."""
        import torch
        kinds = {torch.int32: 0, torch.float32: 1, torch.int64: 2}
        if d_values.dtype not in kinds:
            raise ValueError(f"d_values has dtype {d_values.dtype}: int32, int64 or float32")
        if tuple(d_values.shape) != (self.n_docs,) or not d_values.is_contiguous():
            raise ValueError(f"d_values must be a contiguous [{self.n_docs}] tensor (one entry per "
                             "document)")
        for name, t in (("d_ranks", d_ranks), ("d_perm", d_perm)):
            if (t.dtype != torch.int32 or tuple(t.shape) != (self.n_docs,)
                    or not t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous int32 [{self.n_docs}] tensor")
        s = _stream(stream)
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if self.n_docs else None
        check(lib.bm25_sort_ranks_device(self._h, p(d_values), kinds[d_values.dtype],
                                         1 if descending else 0, p(d_ranks), p(d_perm),
                                         ctypes.c_void_p(s)))

    def search_sorted(self, masks, order, k: int, after=None) -> Tuple[np.ndarray, np.ndarray]:
        """The first k documents of every mask row in a column's order
        (bm25_search_sorted, host arrays) -> (docs, ranks), int32 [M, k]: row m
        holds the k allowed documents of smallest rank above its cursor, in
        rank order, as global doc ids and their ranks; short rows end in
        padding (doc -1, rank -1).  masks as search_filtered takes them, or an
        int M: that many rows with every document allowed; order=(ranks, perm)
        of sort_ranks; after: None or int [M] cursors — a page's last ranks
        column (-1, a padding slot's rank, gives an all-padding row; -2 is no
        cursor).  0 <= k <= min(n_docs, 4096)."""
        if isinstance(masks, (int, np.integer)) and not isinstance(masks, bool):
            m, M = None, int(masks)
            if M < 0:
                raise ValueError("negative mask shape")
        else:
            m = self._masks_arg(masks)
            M = m.shape[0]
        ranks, perm = _order_arg(order, self.n_docs)
        k = _sorted_k(k, self.n_docs)
        a = _after_ranks_arg(after, M)
        docs = np.zeros((M, k), np.int32)
        out = np.zeros((M, k), np.int32)
        check(lib.bm25_search_sorted(self._h, _ptr(m) if m is not None and m.size else None, M,
                                     _ptr(ranks), _ptr(perm), k, _ptr(a), _ptr(docs), _ptr(out)))
        return docs, out

    def sorted_scratch_bytes(self, M: int, k: int) -> int:
        """Bytes of scratch search_sorted_device needs for M rows at k
        (bm25_search_sorted_scratch)."""
        v = ctypes.c_int64(0)
        check(lib.bm25_search_sorted_scratch(self._h, int(M), int(k), ctypes.byref(v)))
        return int(v.value)

    def search_sorted_device(self, d_masks, d_ranks, d_perm, k: int, d_after, d_docs, d_out_ranks,
                             d_scratch, stream=None) -> None:
        """Device-resident search_sorted (bm25_search_sorted_device): packed
        masks [M, W] (32-bit words; None: every document, M from d_docs), int32
        [n_docs] ranks and perm, int32 [M] cursors (or None) in, int32 [M, k]
        docs and ranks out, d_scratch a contiguous byte tensor of at least
        sorted_scratch_bytes(M, k) (None without masks), enqueued on ``stream``
        with no host synchronisation and no validation of the order arrays.
        Reads the caller's tensors only, so it may overlap a search of the
        same handle."""
        import torch
        W = (self.n_docs + 31) // 32
        k = _sorted_k(k, self.n_docs)
        if d_docs.dim() != 2 or d_docs.shape[1] != k:
            raise ValueError(f"d_docs must be an int32 [M, {k}] tensor")
        M = d_docs.shape[0]
        if d_masks is not None and (d_masks.dim() != 2 or tuple(d_masks.shape) != (M, W)
                                    or d_masks.element_size() != 4
                                    or not d_masks.is_contiguous()):
            raise ValueError(f"d_masks must be a contiguous packed [{M}, {W}] tensor of 32-bit "
                             "words")
        for name, t in (("d_docs", d_docs), ("d_out_ranks", d_out_ranks)):
            if t.dtype != torch.int32 or tuple(t.shape) != (M, k) or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous int32 [{M}, {k}] tensor")
        for name, t in (("d_ranks", d_ranks), ("d_perm", d_perm)):
            if (t.dtype != torch.int32 or tuple(t.shape) != (self.n_docs,)
                    or not t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous int32 [{self.n_docs}] tensor")
        if d_after is not None and (d_after.dtype != torch.int32 or tuple(d_after.shape) != (M,)
                                    or not d_after.is_contiguous()):
            raise ValueError(f"d_after must be a contiguous int32 [{M}] tensor (one cursor per row)")
        nbytes = 0
        if d_scratch is not None:
            if not d_scratch.is_contiguous():
                raise ValueError("d_scratch must be contiguous")
            nbytes = d_scratch.numel() * d_scratch.element_size()
        s = _stream(stream)
        p = lambda t, n=1: ctypes.c_void_p(t.data_ptr()) if t is not None and n else None
        check(lib.bm25_search_sorted_device(
            self._h, p(d_masks, M and W), M, p(d_ranks), p(d_perm), k, p(d_after, M),
            p(d_docs, M * k), p(d_out_ranks, M * k), p(d_scratch, nbytes), nbytes,
            ctypes.c_void_p(s)))

    def _sort_column_arg(self, d_values) -> int:
        """A device sort column of this handle: contiguous [n_docs] int32,
        int64 or float32 -> its kind."""
        import torch
        kinds = {torch.int32: 0, torch.float32: 1, torch.int64: 2}
        if d_values.dtype not in kinds:
            raise ValueError(f"d_values has dtype {d_values.dtype}: int32, int64 or float32")
        if tuple(d_values.shape) != (self.n_docs,) or not d_values.is_contiguous():
            raise ValueError(f"d_values must be a contiguous [{self.n_docs}] tensor (one entry per "
                             "document)")
        return kinds[d_values.dtype]

    def sort_keys_device(self, d_values, d_docs, d_key_hi, d_key_lo, descending: bool = False,
                         stream=None) -> None:
        """The order keys of a page of hits (bm25_sort_keys_device): d_docs, a
        contiguous int32 tensor of global doc ids as search_sorted_device
        writes them, in; d_key_hi and d_key_lo, contiguous 32-bit tensors of
        d_docs' shape, out: the two halves of K(d_values[doc - doc_offset])
        (bm25mi.sort_keys is the host form).  A doc id < 0 or outside this
        handle's documents gets the padding key 0xFFFFFFFF / 0xFFFFFFFF and
        reads no value.  Enqueued on ``stream``; no host synchronisation, no
        scratch; not a search."""
        import torch
        kind = self._sort_column_arg(d_values)
        if d_docs.dtype != torch.int32 or not d_docs.is_contiguous():
            raise ValueError("d_docs must be a contiguous int32 tensor")
        for name, t in (("d_key_hi", d_key_hi), ("d_key_lo", d_key_lo)):
            if (t.element_size() != 4 or t.is_floating_point() or t.shape != d_docs.shape
                    or not t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous 32-bit integer tensor of d_docs' "
                                 f"shape {tuple(d_docs.shape)}")
        n = d_docs.numel()
        s = _stream(stream)
        p = lambda t, c=1: ctypes.c_void_p(t.data_ptr()) if c else None
        check(lib.bm25_sort_keys_device(self._h, p(d_values, self.n_docs), kind,
                                        1 if descending else 0, p(d_docs, n), n, p(d_key_hi, n),
                                        p(d_key_lo, n), ctypes.c_void_p(s)))

    def sort_cursor_device(self, d_values, d_perm, d_after_key_hi, d_after_key_lo, d_after_docs,
                           d_after_ranks, descending: bool = False, stream=None) -> None:
        """A collection cursor per row into this handle's rank cursor
        (bm25_sort_cursor_device): d_after_key_hi, d_after_key_lo (32-bit) and
        d_after_docs (int32), [M] each — the last (key, global doc) column of
        a merged page — in; d_after_ranks int32 [M], the ``d_after`` of
        search_sorted_device, out: -1 for doc -1 (a padding slot: the row is
        exhausted), -2 for a doc < -1 (no cursor), else the rank of the last
        of this handle's documents at or before the cursor (-2 when there is
        none), so exactly the documents strictly after the cursor stay
        eligible.  d_perm is sort_ranks' perm for (d_values, descending).
        Enqueued on ``stream``; no host synchronisation; not a search."""
        import torch
        kind = self._sort_column_arg(d_values)
        if (d_perm.dtype != torch.int32 or tuple(d_perm.shape) != (self.n_docs,)
                or not d_perm.is_contiguous()):
            raise ValueError(f"d_perm must be a contiguous int32 [{self.n_docs}] tensor")
        if d_after_docs.dim() != 1:
            raise ValueError("d_after_docs must be an int32 [M] tensor (one cursor per row)")
        M = d_after_docs.shape[0]
        for name, t, i32 in (("d_after_key_hi", d_after_key_hi, False),
                             ("d_after_key_lo", d_after_key_lo, False),
                             ("d_after_docs", d_after_docs, True),
                             ("d_after_ranks", d_after_ranks, True)):
            if (t.element_size() != 4 or t.is_floating_point() or tuple(t.shape) != (M,)
                    or not t.is_contiguous() or (i32 and t.dtype != torch.int32)):
                raise ValueError(f"{name} must be a contiguous {'int32' if i32 else '32-bit integer'}"
                                 f" [{M}] tensor (one cursor per row)")
        s = _stream(stream)
        p = lambda t, c=1: ctypes.c_void_p(t.data_ptr()) if c else None
        check(lib.bm25_sort_cursor_device(self._h, p(d_values, self.n_docs), kind,
                                          1 if descending else 0, p(d_perm, self.n_docs),
                                          p(d_after_key_hi, M), p(d_after_key_lo, M),
                                          p(d_after_docs, M), M, p(d_after_ranks, M),
                                          ctypes.c_void_p(s)))

    def search_boolean(self, queries: np.ndarray, k: int, must=None, any=None, must_not=None,
                       base=None, *, min_match=None, total_hits: bool = False, facets=None,
                       ranges=None, sort=None, after_ranks=None):
        """Top-k of every query among the documents its clause row lets
        through (bm25_search_boolean, host arrays): search_filtered under
        term_masks(must, any, must_not, base) with one mask per query, the
        masks built on the device and never moved to the host.  Clauses and
        base as term_masks, with one row per query (base: 1 row or Q).
        min_match as term_masks'; total_hits=True returns (docs, scores,
        totals), totals int64 [Q] = the documents each query's mask allows
        (bm25_search_boolean_min_match; k = 0 then gives the totals alone).
        facets=(groups, n_groups), as GpuIndex.facets takes them, appends the
        int64 [Q, n_groups] facet counts of each query's mask as the last
        element of the tuple (bm25_search_boolean_facets).
        ranges=(values, fields, lo, hi), as GpuIndex.range_masks takes them
        with one row per query (or (values, lo, hi) for one field), ANDs each
        query's numeric range clauses into its mask, built on the device
        (bm25_search_boolean_ranges); totals and facets are of that mask.
        sort=(ranks, perm), as sort_ranks returns them, orders every row by
        that column instead of by score (bm25_search_boolean_sorted): the
        first k documents of the query's mask in rank order, their scores
        score_docs' bits, and the int32 [Q, k] ranks returned after scores
        (before totals and facets); after_ranks: None or int [Q] cursors, as
        search_sorted's ``after``.  k <= 4096 then."""
        q = np.ascontiguousarray(queries, dtype=np.int32)
        if q.ndim != 2:
            raise ValueError("queries must be a 2-D [Q, T] int32 array")
        Q, T = q.shape
        if sort is None and after_ranks is not None:
            raise ValueError("after_ranks needs sort=(ranks, perm)")
        if sort is not None:
            return self._search_boolean_sorted(q, k, must, any, must_not, base, min_match,
                                               total_hits, facets, ranges, sort, after_ranks)
        mu, an, mn, _, b, Mb = self._clauses_arg(must, any, must_not, base, rows=Q)
        mm = None if min_match is None else min_match_rows(an, min_match, "query")
        if facets is not None:
            if not isinstance(facets, (tuple, list)) or len(facets) != 2:
                raise ValueError("facets must be a pair (groups, n_groups)")
            fg, G = _facet_groups(facets[0], facets[1], self.n_docs)
        if ranges is not None:
            rv, kind, rf, rlo, rhi = _range_args(*_ranges_arg(ranges), self.n_docs, rows=Q,
                                                 what="query")
        k = int(k)
        docs, scores = _topk_out(Q, k)
        if ranges is not None:
            totals = np.zeros(Q, np.int64) if total_hits else None
            counts = np.zeros((Q, G), np.int64) if facets is not None else None
            give = bool(counts is not None and G and fg.size)
            ranged = bool(rv.size and rf.size)  # (no clause, or no document: no range to test)
            check(lib.bm25_search_boolean_ranges(
                self._h, _ptr(q), Q, T, k, _ptr(mu), mu.shape[1], _ptr(an), an.shape[1], _ptr(mn),
                mn.shape[1], _ptr(mm), _ptr(b) if Mb else None, Mb, _ptr(fg) if give else None,
                G if give else 0, _ptr(rv) if ranged else None, kind, rv.shape[0] if ranged else 0,
                _ptr(rf) if ranged else None, _ptr(rlo) if ranged else None,
                _ptr(rhi) if ranged else None, rf.shape[1] if ranged else 0, _ptr(docs),
                _ptr(scores), _ptr(totals), _ptr(counts) if give else None))
            out = (docs, scores)
            if total_hits:
                out += (totals,)
            if facets is not None:
                out += (counts,)
            return out
        if facets is not None:
            totals = np.zeros(Q, np.int64) if total_hits else None
            counts = np.zeros((Q, G), np.int64)
            give = bool(G and fg.size)  # (G == 0, or no document: all-zero rows, no pointer)
            check(lib.bm25_search_boolean_facets(
                self._h, _ptr(q), Q, T, k, _ptr(mu), mu.shape[1], _ptr(an), an.shape[1], _ptr(mn),
                mn.shape[1], _ptr(mm), _ptr(b) if Mb else None, Mb, _ptr(fg) if give else None,
                G if give else 0, _ptr(docs), _ptr(scores), _ptr(totals),
                _ptr(counts) if give else None))
            return (docs, scores, totals, counts) if total_hits else (docs, scores, counts)
        if mm is None and not total_hits:
            check(lib.bm25_search_boolean(self._h, _ptr(q), Q, T, k, _ptr(mu), mu.shape[1],
                                          _ptr(an), an.shape[1], _ptr(mn), mn.shape[1],
                                          _ptr(b) if Mb else None, Mb, _ptr(docs), _ptr(scores)))
            return docs, scores
        totals = np.zeros(Q, np.int64) if total_hits else None
        check(lib.bm25_search_boolean_min_match(
            self._h, _ptr(q), Q, T, k, _ptr(mu), mu.shape[1], _ptr(an), an.shape[1], _ptr(mn),
            mn.shape[1], _ptr(mm), _ptr(b) if Mb else None, Mb, _ptr(docs), _ptr(scores),
            _ptr(totals)))
        return (docs, scores, totals) if total_hits else (docs, scores)

    def _search_boolean_sorted(self, q, k, must, any, must_not, base, min_match, total_hits,
                               facets, ranges, sort, after_ranks):
        """search_boolean with sort= (bm25_search_boolean_sorted)."""
        Q, T = q.shape
        mu, an, mn, _, b, Mb = self._clauses_arg(must, any, must_not, base, rows=Q)
        mm = None if min_match is None else min_match_rows(an, min_match, "query")
        fg, G, give = None, 0, False
        if facets is not None:
            if not isinstance(facets, (tuple, list)) or len(facets) != 2:
                raise ValueError("facets must be a pair (groups, n_groups)")
            fg, G = _facet_groups(facets[0], facets[1], self.n_docs)
            give = bool(G and fg.size)
        ranged = False
        rv = rf = rlo = rhi = None
        kind = 0
        if ranges is not None:
            rv, kind, rf, rlo, rhi = _range_args(*_ranges_arg(ranges), self.n_docs, rows=Q,
                                                 what="query")
            ranged = bool(rv.size and rf.size)
        ranks, perm = _order_arg(sort, self.n_docs)
        k = _sorted_k(k, self.n_docs)
        a = _after_ranks_arg(after_ranks, Q, "query")
        docs = np.zeros((Q, k), np.int32)
        scores = np.zeros((Q, k), np.float32)
        oranks = np.zeros((Q, k), np.int32)
        totals = np.zeros(Q, np.int64) if total_hits else None
        counts = np.zeros((Q, G), np.int64) if facets is not None else None
        check(lib.bm25_search_boolean_sorted(
            self._h, _ptr(q), Q, T, k, _ptr(mu), mu.shape[1], _ptr(an), an.shape[1], _ptr(mn),
            mn.shape[1], _ptr(mm), _ptr(b) if Mb else None, Mb, _ptr(fg) if give else None,
            G if give else 0, _ptr(rv) if ranged else None, kind, rv.shape[0] if ranged else 0,
            _ptr(rf) if ranged else None, _ptr(rlo) if ranged else None,
            _ptr(rhi) if ranged else None, rf.shape[1] if ranged else 0, _ptr(docs),
            _ptr(scores), _ptr(totals), _ptr(counts) if give else None, _ptr(ranks), _ptr(perm),
            _ptr(a), _ptr(oranks)))
        out = (docs, scores, oranks)
        if total_hits:
            out += (totals,)
        if facets is not None:
            out += (counts,)
        return out

    # ------------------------------------------- bm25.BM25's float64 path
    def set_values_f64(self, data64) -> None:
        """Keep a float64 copy of the values (same CSC order) on the device
        (bm25_index_set_values_f64)."""
        d = np.ascontiguousarray(data64, dtype=np.float64)
        if d.size < self.nnz:
            raise ValueError("data64 shorter than nnz")
        check(lib.bm25_index_set_values_f64(self._h, _ptr(d)))

    def scores_dense_f64(self, query) -> np.ndarray:
        """float64 sums of every document in query order (numpy's
        np.sum(matrix[:, ids], axis=1), bm25.py:143)."""
        q = np.ascontiguousarray(np.asarray(query).ravel(), dtype=np.int32)
        out = np.zeros(self.n_docs, np.float64)
        check(lib.bm25_scores_dense_f64(self._h, _ptr(q), q.size, _ptr(out)))
        return out

    def topn_f64(self, query, n: int) -> Tuple[np.ndarray, np.ndarray]:
        """The n best documents of those float64 sums, (score desc, doc asc)."""
        q = np.ascontiguousarray(np.asarray(query).ravel(), dtype=np.int32)
        docs = np.zeros(max(int(n), 0), np.int32)
        scores = np.zeros(max(int(n), 0), np.float64)
        check(lib.bm25_topn_f64(self._h, _ptr(q), q.size, int(n), _ptr(docs), _ptr(scores)))
        return docs, scores

    # ------------------------------------------------------------------
    def profile_enable(self, on: bool = True) -> None:
        check(lib.bm25_profile_enable(self._h, int(on)))  # (True = 1: score pass events only)

    def profile_read(self) -> dict:
        sm = ctypes.c_double()
        sl = ctypes.c_int64()
        tm = ctypes.c_double()
        ns = ctypes.c_int64()
        rs = ctypes.c_int64()
        check(lib.bm25_profile_read(self._h, ctypes.byref(sm), ctypes.byref(sl), ctypes.byref(tm),
                                    ctypes.byref(ns), ctypes.byref(rs)))
        return {"score_ms": sm.value, "score_launches": sl.value, "total_ms": tm.value,
                "searches": ns.value, "rescored_tiles_last": rs.value}

    # ------------------------------------------------------------------
    def set_option(self, name: str, value: int) -> None:
        """A search option of this handle (bm25_index_set_option: flat,
        flat_bw, items_per_wave, sample_p, list_cap, claim_ch, claim_m,
        tile_bound, theta_bound, filter_tiles, bool_chunk, ...).  In a multi-rank search every rank must
        change an option together (like a collective): the next
        ``bm25mi.dist.sharded_search`` re-checks the sample width they agree on."""
        check(lib.bm25_index_set_option(self._h, name.encode(), int(value)))
        self.__dict__.pop("_bm25_width_ok", None)  # (bm25mi.dist._agree_width's cache)
        for f in self.__dict__.get("_bm25_forks", []):  # (bm25mi.dist's part contexts)
            f.set_option(name, value)

    def get_option(self, name: str) -> int:
        v = ctypes.c_int64()
        check(lib.bm25_index_get_option(self._h, name.encode(), ctypes.byref(v)))
        return v.value

    KERNELS = {1: "flat_sample", 2: "flat_rest", 4: "flat_all", 8: "wave_sample",
               16: "wave_rest", 32: "wave_all", 64: "large_k", 128: "bound_keys",
               256: "bound_off", 512: "count_skips", 1024: "rest_split",
               2048: "bound_pool", 4096: "filtered", 8192: "weighted",
               16384: "after"}  # (flags, not
    # kernels: 256 the tile-bound threshold was off, 512 REST counted the postings it
    # skipped, 1024 REST ran over split items, 2048 the threshold read the pooled bounds,
    # 8192 the search was weighted, 16384 it was called through search_after)

    def last_dispatch(self) -> dict:
        """What the last search launched (bm25_search_dispatch): the score
        kernels by phase, the flat kernel's term lanes and tiles per item
        (ALL, SAMPLE, REST) and the sampling stride."""
        km = ctypes.c_uint32()
        tl = ctypes.c_int32()
        bt = (ctypes.c_int32 * 3)()
        sp_ = ctypes.c_int32()
        check(lib.bm25_search_dispatch(self._h, ctypes.byref(km), ctypes.byref(tl), bt,
                                       ctypes.byref(sp_)))
        return {"kernels": {n for b, n in self.KERNELS.items() if km.value & b},
                # the search came through search_collapsed (bit 262144; the set is its
                # last round's)
                "collapsed": bool(km.value & 262144),
                # tile_skip_kernel ran ahead of REST (bit 32768): reported beside the
                # set, whose exact contents callers compare against the phases taken
                "tile_skip": bool(km.value & 32768),
                # ... and marked the dead term segments of scored tiles (bit 65536)
                "seg_skip": bool(km.value & 65536),
                # ... and the dead rows of the heavy terms' kept segments (bit 131072)
                "row_skip": bool(km.value & 131072),
                "term_lanes": tl.value,
                "band_tiles": {"all": bt[0], "sample": bt[1], "rest": bt[2]},
                "sample_p": sp_.value}

    def search_stats(self) -> dict:
        """Selection statistics of the last search (bm25_search_counters):
        tiles re-scored exactly, queries sent to the exact fallback stage,
        (query, tile) pairs the REST pass skipped by their tile bound and the
        postings of those pairs, queries left to the block merge, the
        non-empty term segments REST dropped in the tiles it scored and their
        postings, the double rows it dropped in the segments it kept and their
        postings (counted like the skipped pairs: count_skips, else -1)."""
        v = (ctypes.c_int64 * 10)()
        check(lib.bm25_search_counters(self._h, v, 10))
        return {"rescored_tiles": v[0], "fallback_queries": v[1],
                "bound_skipped_tiles": v[2], "bound_skipped_postings": v[3],
                "block_merge_queries": v[4], "large_dense_queries": v[5],
                "bound_dropped_segments": v[6], "bound_dropped_postings": v[7],
                "bound_dropped_rows": v[8], "bound_dropped_row_postings": v[9]}


def merge_topk_device(device: int, d_docs, d_scores, W: int, Q: int, k: int, d_out_docs,
                      d_out_scores, stream=None) -> None:
    """Merge W per-shard [Q, k] lists (global doc ids) -> [Q, k] on the GPU."""
    s = _stream(stream)
    check(lib.bm25_merge_topk_device(int(device), ctypes.c_void_p(d_docs.data_ptr()),
                                     ctypes.c_void_p(d_scores.data_ptr()), int(W), int(Q), int(k),
                                     ctypes.c_void_p(d_out_docs.data_ptr()),
                                     ctypes.c_void_p(d_out_scores.data_ptr()),
                                     ctypes.c_void_p(s)))


def merge_sorted_device(device: int, d_docs, d_scores, W: int, Q: int, k: int, rank_stride: int,
                        d_out_docs, d_out_scores, stream=None) -> None:
    """W-way merge of best-first [Q, k] lists (bm25_merge_sorted_device):
    rank w's lists start at element w * rank_stride of d_docs / d_scores."""
    s = _stream(stream)
    check(lib.bm25_merge_sorted_device(int(device), ctypes.c_void_p(d_docs.data_ptr()),
                                       ctypes.c_void_p(d_scores.data_ptr()), int(W), int(Q),
                                       int(k), int(rank_stride),
                                       ctypes.c_void_p(d_out_docs.data_ptr()),
                                       ctypes.c_void_p(d_out_scores.data_ptr()),
                                       ctypes.c_void_p(s)))


def merge_collapsed_device(device: int, d_docs, d_scores, d_groups, W: int, Q: int, k: int,
                           rank_stride: int, per_group: int, d_out_docs, d_out_scores,
                           d_out_groups=None, stream=None) -> None:
    """The doc-shard merge of collapsed lists (bm25_merge_collapsed_device): W
    best-first [Q, k] lists of (doc, score, group) — what search_collapsed_device
    writes with d_groups_out — merged in key order and walked once more under
    per_group.  Rank w's lists start at element w * rank_stride of d_docs /
    d_scores / d_groups; d_out_groups is optional."""
    s = _stream(stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)
    check(lib.bm25_merge_collapsed_device(int(device), ptr(d_docs), ptr(d_scores), ptr(d_groups),
                                          int(W), int(Q), int(k), int(rank_stride), int(per_group),
                                          ptr(d_out_docs), ptr(d_out_scores), ptr(d_out_groups),
                                          ctypes.c_void_p(s)))


def merge_sort_keys_device(device: int, d_docs, d_key_hi, d_key_lo, W: int, Q: int, k: int,
                           rank_stride: int, d_out_docs, d_out_key_hi, d_out_key_lo,
                           stream=None) -> None:
    """The doc-shard merge of sorted-search lists (bm25_merge_sort_keys_device):
    W lists [Q, k] of (doc, key_hi, key_lo), each ascending by (key, doc) with
    padding (doc < 0) last — search_sorted_device's docs with sort_keys_device's
    planes — merged into the first k of their union, padded with doc -1 and
    keys 0xFFFFFFFF.  Rank w's lists start at element w * rank_stride of the
    three inputs (Q * k for plain [W, Q, k] arrays; 3 * Q * k for the packed
    [W, 3, Q, k] buffer of one all-gather, the inputs being its planes).  All
    tensors are contiguous-strided 32-bit integers; the outputs hold Q * k
    elements.  The last column of the outputs is the next page's collection
    cursor."""
    W, Q, k, rank_stride = int(W), int(Q), int(k), int(rank_stride)
    ins = (("d_docs", d_docs), ("d_key_hi", d_key_hi), ("d_key_lo", d_key_lo))
    outs = (("d_out_docs", d_out_docs), ("d_out_key_hi", d_out_key_hi),
            ("d_out_key_lo", d_out_key_lo))
    for name, t in ins + outs:
        if t is not None and (t.element_size() != 4 or t.is_floating_point()):
            raise ValueError(f"{name} must be a 32-bit integer tensor, got {t.dtype}")
    if Q > 0 and k > 0:
        for name, t in outs:
            if t is None or t.numel() != Q * k or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous 32-bit [{Q}, {k}] tensor")
    s = _stream(stream)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)
    check(lib.bm25_merge_sort_keys_device(int(device), ptr(d_docs), ptr(d_key_hi), ptr(d_key_lo),
                                          W, Q, k, rank_stride, ptr(d_out_docs),
                                          ptr(d_out_key_hi), ptr(d_out_key_lo),
                                          ctypes.c_void_p(s)))


class ShardedIndex:
    """A CSC index doc-sharded over several GPUs of this process
    (bm25_sharded_* in include/bm25mi.h): ``search`` has GpuIndex.search's
    contract and returns the single-index result."""

    def __init__(self, indptr, indices, data, n_docs: int, devices):
        devices = [int(d) for d in devices]
        if not devices:
            raise ValueError("need at least one device")
        indptr = np.asarray(indptr)
        ip_i64 = indptr.dtype == np.int64 or indptr[-1] > np.iinfo(np.int32).max
        ip = np.ascontiguousarray(indptr, dtype=np.int64 if ip_i64 else np.int32)
        ix = np.ascontiguousarray(indices, dtype=np.int32)
        dt = np.ascontiguousarray(data, dtype=np.float32)
        devs = np.asarray(devices, np.int32)
        self.n_docs = int(n_docs)
        self.n_terms = int(ip.size - 1)
        self._h = None
        h = ctypes.c_void_p()
        check(lib.bm25_sharded_create(len(devices), _ptr(devs), self.n_docs, self.n_terms,
                                      int(ip[-1]), _ptr(ip), int(ip_i64), _ptr(ix), _ptr(dt),
                                      ctypes.byref(h)))
        self._h = h

    def shards(self):
        n = ctypes.c_int64()
        check(lib.bm25_sharded_info(self._h, ctypes.byref(n), None, None))
        lo = np.zeros(n.value, np.int64)
        hi = np.zeros(n.value, np.int64)
        check(lib.bm25_sharded_info(self._h, ctypes.byref(n), _ptr(lo), _ptr(hi)))
        return list(zip(lo.tolist(), hi.tolist()))

    def search(self, queries: np.ndarray, k: int) -> Tuple[np.ndarray, np.ndarray]:
        q = np.ascontiguousarray(queries, dtype=np.int32)
        if q.ndim != 2:
            raise ValueError("queries must be a 2-D [Q, T] int32 array")
        Q, T = q.shape
        k = int(k)
        docs, scores = _topk_out(Q, k)
        check(lib.bm25_sharded_search(self._h, _ptr(q), Q, T, k, _ptr(docs), _ptr(scores)))
        return docs, scores

    def close(self) -> None:
        if self._h is not None:
            lib.bm25_sharded_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def device_count() -> int:
    return _capi.device_count()
