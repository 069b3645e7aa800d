"""CPU tests of the numeric range filters (bm25_range_masks,
bm25_range_masks_device, bm25_search_boolean_ranges): the symbols are exported,
bound and documented, a NULL handle is rejected without a GPU and leaves the
outputs untouched, the Python layers reject malformed arguments before any C
call, bm25mi.range_rows turns dicts into clause rows, and the numpy model the
GPU tests compare against (tests/range_model.py) agrees with a plain Python
loop on 70 documents."""
import ctypes
import math

import numpy as np
import pytest

from range_model import edge_case, range_allowed, range_want
from test_term_masks_host import _bare_index

SYMS = {"bm25_range_masks": 12, "bm25_range_masks_device": 13, "bm25_search_boolean_ranges": 27}


def test_symbols_exported_bound_and_documented():
    from bm25mi import _capi
    syms = _capi.header_symbols()
    text = open(_capi.HEADER).read()
    for s, n in SYMS.items():
        assert s in syms, s
        f = getattr(_capi.lib, s)
        assert f.argtypes is not None and f.restype is ctypes.c_int, s
        assert s in _capi._SIGS
        assert len(f.argtypes) == n, s
        decl = text[text.rindex(f"int {s}("):]
        decl = decl[:decl.index(");")]
        assert decl.count(",") + 1 == n, s  # the declaration of include/bm25mi.h
    doc = text[text.index("Numeric range filters:"):text.index("int bm25_range_masks(")]
    flat = " ".join(" ".join(line.strip().lstrip("*") for line in doc.splitlines()).split())
    for phrase in ("values [F, n_docs] one dtype per call, rows contiguous: values[f][d] = field f "
                   "of handle-local document d",
                   "kind: BM25_FIELD_I32 (0) int32, BM25_FIELD_F32 (1) float32, BM25_FIELD_I64 "
                   "(2) int64",
                   "fields [M, C] int32 clause c of mask row m tests field fields[m][c]; negative "
                   "= padding",
                   "lo, hi [M, C] of the values' dtype: the clause's bounds, both inclusive",
                   "base [Mb, W] Mb = 0 (NULL), 1 or M",
                   "out [M, W] uint32, W = ceil(n_docs / 32), the layout of bm25_search_filtered",
                   "allowed(m, d) = d < n_docs and base(m, d) and for every c with fields[m][c] "
                   ">= 0: lo[m][c] <= values[fields[m][c]][d] <= hi[m][c]",
                   "int64 is compared as int64, never through a float",
                   "a NaN value fails every clause", "-0.0f equals +0.0f",
                   "lo > hi is an empty clause, and the row is all zeros",
                   "A row with no clause gives base, or every document when there is no base",
                   "several clauses may name the same field",
                   "Every word of every row is written",
                   "Bits at or past n_docs of the last word are written 0 even where base has "
                   "them set",
                   "No word at index >= W of a row is read or written",
                   "No values entry at index >= n_docs of a field row is read",
                   "M may pass 65535", "no global atomics and no scratch",
                   "does not depend on scheduling",
                   "so a shard builds its slice",
                   "leave bm25_search_dispatch, bm25_search_counters and "
                   "bm25_search_filtered_stats alone",
                   "a bad kind", "Mb not in {0, 1, M}",
                   "a fields entry >= F (the message names row, column and value)",
                   "a NaN bound on a non-padding clause",
                   "On any error the outputs are untouched",
                   "M == 0 returns BM25_OK without device work",
                   "never synchronises", "retains no scratch",
                   "no workspace, no index array",
                   "not ordered against the handle's searches",
                   "A field id >= F is a field that no document has: the clause matches nothing "
                   "and nothing out of bounds is read",
                   "A NaN bound matches nothing",
                   "bit for bit", "range(q) AND term clauses(q) AND base",
                   "go up once per call", "the automatic chunk halves",
                   "an explicit bool_chunk keeps its meaning, queries per chunk",
                   "With F == 0, C == 0 or NULL values the call is bm25_search_boolean_facets"):
        assert phrase in flat, phrase
    assert (_capi.lib.bm25_abi_version() == 1)  # additive: the ABI version stays


def test_null_handle_is_einval_and_outputs_untouched():
    from bm25mi._capi import BM25_EINVAL, lib
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    values = np.zeros((1, 70), np.int32)
    fields = np.zeros((2, 1), np.int32)
    lo = np.zeros((2, 1), np.int32)
    hi = np.ones((2, 1), np.int32)
    masks = np.full((2, 3), 0xABABABAB, np.uint32)
    groups = np.zeros(70, np.int32)
    counts = np.full((2, 4), -7, np.int64)
    q = np.zeros((2, 2), np.int32)
    anyc = np.zeros((2, 2), np.int32)
    docs = np.full((2, 3), 7, np.int32)
    scores = np.full((2, 3), 7.0, np.float32)
    totals = np.full(2, -7, np.int64)
    calls = (
        lambda: lib.bm25_range_masks(None, p(values), 0, 1, p(fields), p(lo), p(hi), 1, 2, None, 0,
                                     p(masks)),
        lambda: lib.bm25_range_masks_device(None, p(values), 0, 1, p(fields), p(lo), p(hi), 1, 2,
                                            None, 0, p(masks), None),
        lambda: lib.bm25_search_boolean_ranges(None, p(q), 2, 2, 3, None, 0, p(anyc), 2, None, 0,
                                               None, None, 0, p(groups), 4, p(values), 0, 1,
                                               p(fields), p(lo), p(hi), 1, p(docs), p(scores),
                                               p(totals), p(counts)),
    )
    for call in calls:
        assert call() == BM25_EINVAL
        assert b"NULL index" in lib.bm25_last_error()
    assert (masks == 0xABABABAB).all() and (counts == -7).all() and (totals == -7).all()
    assert (docs == 7).all() and (scores == 7.0).all()


def test_python_layers_reject_ranges_before_c():
    import bm25_native
    g = _bare_index(70)  # no handle: reaching the C call would fail on it
    v = np.zeros((2, 70), np.int32)
    f = np.zeros((2, 1), np.int32)
    lo = np.zeros((2, 1), np.int32)
    hi = np.ones((2, 1), np.int32)
    q = np.zeros((2, 3), np.int32)
    two = [[1, 2], [3]]
    calls = (lambda *a: g.range_masks(*a),
             lambda *a: g.search_boolean(q, 1, any=two, ranges=a),
             lambda *a: g.search_boolean(q, 0, any=two, total_hits=True, ranges=a))
    for call in calls:
        for bad in (np.float64, bool, np.int16, np.uint32):
            with pytest.raises(ValueError, match=f"values have dtype {np.dtype(bad).name}"):
                call(v.astype(bad), f, lo, hi)
        with pytest.raises(ValueError, match=r"values has shape \(2, 69\), expected \(70,\)"):
            call(v[:, :69], f, lo, hi)
        with pytest.raises(ValueError, match=r"values has shape \(1, 2, 70\)"):
            call(v[None], f, lo, hi)
        with pytest.raises(ValueError, match=r"values has shape \(69,\)"):
            call(v[0, :69], f, lo, hi)
        with pytest.raises(ValueError, match=r"fields has shape \(2, 2\), lo and hi have \(2, 1\)"):
            call(v, np.zeros((2, 2), np.int32), lo, hi)
        with pytest.raises(ValueError, match=r"fields has shape \(3,\)"):
            call(v, np.zeros(3, np.int32), lo, hi)
        with pytest.raises(ValueError, match="fields must be an integer array"):
            call(v, f.astype(np.float32), lo, hi)
        with pytest.raises(ValueError, match=r"lo has shape \(2, 1\), hi has \(2, 2\)"):
            call(v, f, lo, np.ones((2, 2), np.int32))
        with pytest.raises(ValueError, match=r"hi has shape \(2, 1, 1\)"):
            call(v, f, lo, hi[:, :, None])
        with pytest.raises(ValueError, match="lo has dtype int64, the values have int32"):
            call(v, f, lo.astype(np.int64), hi)
        with pytest.raises(ValueError, match="hi has dtype float32, the values have int32"):
            call(v, f, lo, hi.astype(np.float32))
        with pytest.raises(ValueError, match="lo has dtype float64, the values have float32"):
            call(v.astype(np.float32), f, lo.astype(np.float64), hi.astype(np.float32))
        with pytest.raises(ValueError, match=r"fields\[1\]\[0\] = 2 is not below F = 2"):
            call(v, np.array([[1], [2]], np.int32), lo, hi)
        with pytest.raises(ValueError, match="fields=None needs one field, the values have 2"):
            call(v, None, lo, hi)
    # rows: one per mask of base, one per query
    with pytest.raises(ValueError, match="base has 3 rows, expected 1 or 2"):
        g.range_masks(v, f, lo, hi, np.ones((3, 70), bool))
    with pytest.raises(ValueError, match=r"lo and hi have 3 rows, expected 2 \(one per query\)"):
        g.search_boolean(q, 1, any=two, ranges=(v, np.zeros((3, 1), np.int32),
                                                np.zeros((3, 1), np.int32),
                                                np.ones((3, 1), np.int32)))
    m = bm25_native.BM25v()
    for bad in (v, (v,), (v, lo), (v, f, lo, hi, hi), 4):
        with pytest.raises(ValueError, match="ranges must be a quadruple"):
            g.search_boolean(q, 1, any=two, ranges=bad)
        with pytest.raises(ValueError, match="ranges must be a quadruple"):
            m.search_boolean(q, 1, any=two, ranges=bad)
    # 1-D values / fields=None / 1-D bounds are accepted: these reach the C
    # call, which the handle-less index fails
    for args in ((v[0], None, lo[:, 0], hi[:, 0]), (v[0], None, lo, hi), (v, f[:, 0], lo, hi)):
        with pytest.raises(ValueError, match="NULL index"):
            g.range_masks(*args)
    with pytest.raises(ValueError, match="NULL index"):
        g.search_boolean(q, 1, any=two, ranges=(v[0], lo, hi))   # the triple: one field
    # the empty batch keeps its shape
    out = m.search_boolean([], 3, must=[], ranges=(v, f, lo, hi))
    assert [a.shape for a in out] == [(0, 0), (0, 0)]
    out = m.search_boolean([], 3, must=[], total_hits=True, facets=(np.zeros(70, np.int64), 4),
                           ranges=(v, f, lo, hi))
    assert [a.shape for a in out] == [(0, 0), (0, 0), (0,), (0, 4)]


def test_device_wrapper_rejects_shapes_before_c():
    import torch
    g = _bare_index(70)
    dv = torch.zeros((2, 70), dtype=torch.int32)
    df = torch.zeros((2, 1), dtype=torch.int32)
    dlo = torch.zeros((2, 1), dtype=torch.int32)
    dhi = torch.ones((2, 1), dtype=torch.int32)
    do = torch.zeros((2, 3), dtype=torch.int32)
    for bad in (dv.to(torch.float64), dv.to(torch.int16), dv.to(torch.bool)):
        with pytest.raises(ValueError, match="d_values has dtype"):
            g.range_masks_device(bad, df, dlo, dhi, do)
    for bad in (dv[:, :69], dv[None], torch.zeros((70, 2), dtype=torch.int32).t(),
                torch.zeros(69, dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"d_values must be a contiguous \[70\] or \[F, 70\]"):
            g.range_masks_device(bad, df, dlo, dhi, do)
    for bad in (do[:, :2], do.to(torch.int64), torch.zeros((3, 2), dtype=torch.int32).t(),
                torch.zeros(6, dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"d_out must be a contiguous packed \[M, 3\]"):
            g.range_masks_device(dv, df, dlo, dhi, bad)
    for bad in (torch.zeros((3, 1), dtype=torch.int32), df.to(torch.int64), df[:, 0],
                df.to(torch.float32)):
        with pytest.raises(ValueError, match=r"d_fields must be a contiguous int32 \[2, C\]"):
            g.range_masks_device(dv, bad, dlo, dhi, do)
    for bad in (dlo.to(torch.int64), dlo.to(torch.float32), torch.zeros((2, 2), dtype=torch.int32),
                dlo[:, 0]):
        with pytest.raises(ValueError, match=r"d_lo must be a contiguous torch.int32 \[2, 1\]"):
            g.range_masks_device(dv, df, bad, dhi, do)
        with pytest.raises(ValueError, match=r"d_hi must be a contiguous torch.int32 \[2, 1\]"):
            g.range_masks_device(dv, df, dlo, bad, do)
    for bad in (torch.zeros((3, 3), dtype=torch.int32), torch.zeros((2, 2), dtype=torch.int32),
                torch.zeros((2, 3), dtype=torch.int64)):
        with pytest.raises(ValueError, match=r"d_base (must be a contiguous packed|has 3 rows)"):
            g.range_masks_device(dv, df, dlo, dhi, do, bad)
    with pytest.raises(ValueError, match="NULL index"):  # well-formed: reaches the C call
        g.range_masks_device(dv, df, dlo, dhi, do, do.clone())


def test_range_rows():
    import bm25mi
    cols = ["year", "price"]
    f, lo, hi = bm25mi.range_rows([{"year": (2019, 2021), "price": (None, 50)}, {}], cols, np.int32)
    assert f.dtype == np.int32 and lo.dtype == np.int32 and hi.dtype == np.int32
    assert f.tolist() == [[0, 1], [-1, -1]]
    assert lo.tolist() == [[2019, -2**31], [0, 0]] and hi.tolist() == [[2021, 50], [0, 0]]
    f, lo, hi = bm25mi.range_rows([{"price": (None, None)}, {"price": (3, None), "year": (1, 2)},
                                   {"year": (-2**63, 2**63 - 1)}], cols, np.int64)
    assert f.tolist() == [[1, -1], [1, 0], [0, -1]] and lo.dtype == np.int64
    assert lo.tolist() == [[-2**63, 0], [3, 1], [-2**63, 0]]
    assert hi.tolist() == [[2**63 - 1, 0], [2**63 - 1, 2], [2**63 - 1, 0]]
    f, lo, hi = bm25mi.range_rows([{"price": (None, 9.5)}, {"price": (0.25, None)}], cols,
                                  np.float32)
    assert lo.dtype == np.float32 and f.tolist() == [[1], [1]]
    assert lo.tolist() == [[-math.inf], [0.25]] and hi.tolist() == [[9.5], [math.inf]]
    f, lo, hi = bm25mi.range_rows([{}, {}], cols, np.int32)        # the empty dict: no clause
    assert f.shape == (2, 0) and lo.shape == (2, 0) and hi.shape == (2, 0)
    f, lo, hi = bm25mi.range_rows([], cols, np.float32)
    assert f.shape == (0, 0) and lo.dtype == np.float32
    with pytest.raises(ValueError, match="row 1: unknown column 'yaer'"):
        bm25mi.range_rows([{}, {"yaer": (1, 2)}], cols, np.int32)
    with pytest.raises(ValueError, match=r"bound 4294967296 is no int32"):
        bm25mi.range_rows([{"year": (2**32, None)}], cols, np.int32)
    with pytest.raises(ValueError, match=r"bound 1.5 is no int64"):
        bm25mi.range_rows([{"year": (1.5, None)}], cols, np.int64)
    with pytest.raises(ValueError, match="the bounds are a pair"):
        bm25mi.range_rows([{"year": 2019}], cols, np.int32)
    with pytest.raises(ValueError, match="dtype float64 is not a range filter's"):
        bm25mi.range_rows([{}], cols, np.float64)
    # what range_rows makes is what the model (and the calls) take
    v = np.array([[2018, 2019, 2020, 2021, 2022], [10, 60, 50, 51, 0]], np.int32)
    f, lo, hi = bm25mi.range_rows([{"year": (2019, 2021), "price": (None, 50)}, {}], cols, np.int32)
    assert range_allowed(v, f, lo, hi).tolist() == [[False, False, True, False, False], [True] * 5]


@pytest.mark.parametrize("dtype", [np.int32, np.float32, np.int64])
def test_numpy_model_against_a_plain_loop(dtype):
    """70 documents, the edge values of range_model.edge_case: NaN values,
    -0.0 against +0.0 bounds, lo > hi, int64 values at +-2^53 + 1 and at the
    int64 limits, garbage tail bits in base, a padding clause, a field id >= F."""
    n = 70
    values, fields, lo, hi = edge_case(dtype, n)
    R = fields.shape[0]
    fields = np.vstack([fields, [[2, -1]], [[0, 2**31 - 1]]]).astype(np.int32)  # ids >= F
    lo = np.vstack([lo, lo[6:7], lo[6:7]])
    hi = np.vstack([hi, hi[6:7], hi[6:7]])
    M = R + 2
    rng = np.random.default_rng(3)
    base_bits = rng.random((M, n)) < 0.7
    base = np.zeros((M, 3), np.uint32)
    for m in range(M):
        for d in range(n):
            if base_bits[m, d]:
                base[m, d >> 5] |= np.uint32(1 << (d & 31))
    base[:, -1] |= np.uint32((0xFFFFFFFF << (n % 32)) & 0xFFFFFFFF)   # garbage tail bits
    py = values.tolist()   # Python ints and floats: exact, IEEE comparisons
    plo, phi = lo.tolist(), hi.tolist()
    for b in (None, base, base[:1]):
        want = np.zeros((M, 3), np.uint32)
        for m in range(M):
            for d in range(n):
                ok = True if b is None else bool(
                    (int(b[m if b.shape[0] > 1 else 0, d >> 5]) >> (d & 31)) & 1)
                for c in range(fields.shape[1]):
                    f = int(fields[m, c])
                    if f < 0:
                        continue
                    ok = ok and f < 2 and plo[m][c] <= py[f][d] <= phi[m][c]
                if ok:
                    want[m, d >> 5] |= np.uint32(1 << (d & 31))
        got = range_want(values, fields, lo, hi, b)
        assert got.dtype == np.uint32 and got.shape == (M, 3) and np.array_equal(got, want)
        assert not got[4].any() and not got[R].any() and not got[R + 1].any()
        assert (got[:, -1] >> np.uint32(n % 32) == 0).all()
    full = range_want(values, fields, lo, hi)
    assert np.array_equal(full[5], np.array([0xFFFFFFFF, 0xFFFFFFFF, 0x3F], np.uint32))
    counts = [int(np.unpackbits(r.view(np.uint8)).sum()) for r in full]
    # the one-value rows find exactly the planted documents
    if np.dtype(dtype).kind == "f":
        zeros = int((values[0] == 0).sum())                # -0.0 and +0.0 both, NaN not
        assert counts[0] == zeros >= 2 and counts[6] == n - 2   # everything but field 1's NaNs
        assert counts[7] == 1 and counts[8] == 1           # -inf alone, +inf alone
    else:
        assert counts[0] == 1 and counts[6] == n and counts[7] == 1 and counts[8] == 1
