"""CPU tests of the boolean term filters (bm25_term_masks,
bm25_term_masks_device, bm25_search_boolean): the symbols are exported, bound
and documented, a NULL handle is rejected without a GPU and leaves the outputs
untouched, the Python layers (GpuIndex.term_masks, GpuIndex.term_masks_device,
GpuIndex.search_boolean, BM25v.search_boolean) reject malformed shapes before
any C call, and ragged clause lists are padded with -1."""
import ctypes

import numpy as np
import pytest

SYMS = ("bm25_term_masks", "bm25_term_masks_device", "bm25_search_boolean")


def test_symbols_exported_bound_and_documented():
    from bm25mi import _capi
    syms = _capi.header_symbols()
    text = open(_capi.HEADER).read()
    for s in SYMS:
        assert s in syms, s
        f = getattr(_capi.lib, s)
        assert f.argtypes is not None and f.restype is ctypes.c_int, s
        assert s in _capi._SIGS
    # the arguments of the three declarations in include/bm25mi.h
    assert len(_capi.lib.bm25_term_masks.argtypes) == 11
    assert len(_capi.lib.bm25_term_masks_device.argtypes) == 12
    assert len(_capi.lib.bm25_search_boolean.argtypes) == 15
    for s in SYMS:  # ... which the bindings match
        decl = text[text.rindex(f"int {s}("):]
        decl = decl[:decl.index(");")]
        assert decl.count(",") + 1 == len(getattr(_capi.lib, s).argtypes), s
    doc = text[text.index("Boolean term filters:"):text.index("int bm25_term_masks(")]
    flat = " ".join(" ".join(line.strip().lstrip("*") for line in doc.splitlines()).split())
    for phrase in ("Replaces no reference call: BM25v.search has no term filter "
                   "(bm25_native.py:76-158)", "d & 31", "d >> 5",
                   "a term that no document has", "bool_chunk", "M * W * 4 bytes",
                   "1.25 MB per mask at 10M documents", "bm25_merge_topk_device",
                   "never synchronises", "not ordered against the handle's searches",
                   "0xFFFFFFFF"):
        assert phrase in flat, phrase
    assert '"bool_chunk"' in text and "BM25_BOOL_CHUNK" in text
    assert _capi.abi_version() == 1  # additive: the ABI version stays


def test_null_handle_is_einval_and_outputs_untouched():
    from bm25mi._capi import BM25_EINVAL, lib
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    must = np.zeros((2, 1), np.int32)
    out = np.full((2, 3), 0xA5A5A5A5, np.uint32)
    assert lib.bm25_term_masks(None, p(must), 1, None, 0, None, 0, 2, None, 0,
                               p(out)) == BM25_EINVAL
    assert b"NULL index" in lib.bm25_last_error()
    assert lib.bm25_term_masks_device(None, p(must), 1, None, 0, None, 0, 2, None, 0, p(out),
                                      None) == BM25_EINVAL
    assert b"NULL index" in lib.bm25_last_error()
    q = np.zeros((2, 2), np.int32)
    docs = np.full((2, 3), 7, np.int32)
    scores = np.full((2, 3), 7.0, np.float32)
    assert lib.bm25_search_boolean(None, p(q), 2, 2, 3, p(must), 1, None, 0, None, 0, None, 0,
                                   p(docs), p(scores)) == BM25_EINVAL
    assert b"NULL index" in lib.bm25_last_error()
    assert (out == 0xA5A5A5A5).all() and (docs == 7).all() and (scores == 7.0).all()


def _bare_index(n_docs=70):
    """A GpuIndex object without a handle: shape validation runs before the
    handle is touched, so it needs no device."""
    from bm25mi.index import GpuIndex
    g = GpuIndex.__new__(GpuIndex)
    g._h = None
    g.n_docs, g.n_terms, g.doc_offset = n_docs, 5, 0
    return g


def test_pad_clause_ragged_lists():
    import bm25mi
    a = bm25mi.pad_clause([[3, 1, 4], [], [2]])
    assert a.dtype == np.int32 and a.flags.c_contiguous
    assert a.tolist() == [[3, 1, 4], [-1, -1, -1], [2, -1, -1]]
    assert bm25mi.pad_clause([[1, 2], [3, 4]]).tolist() == [[1, 2], [3, 4]]
    assert bm25mi.pad_clause([[], []]).shape == (2, 0)
    assert bm25mi.pad_clause([]).shape == (0, 0)
    assert bm25mi.pad_clause([np.array([1, 2]), np.array([5])]).tolist() == [[1, 2], [5, -1]]
    b = np.array([[1, -1], [0, 2]], np.int64)
    got = bm25mi.pad_clause(b)
    assert got.dtype == np.int32 and got.tolist() == b.tolist()
    for bad in ([1, 2, 3], np.zeros(3, np.int32), np.zeros((1, 2, 2), np.int32),
                np.zeros((2, 2), np.float32)):
        with pytest.raises(ValueError, match="2-D .* list of lists"):
            bm25mi.pad_clause(bad)


def test_gpu_index_term_masks_rejects_shapes_before_c():
    g = _bare_index(70)  # W = 3
    with pytest.raises(ValueError, match="must_not has 3 rows, expected 2"):
        g.term_masks(must=[[1], [2]], must_not=[[0], [1], [2]])
    with pytest.raises(ValueError, match="any has 1 rows, expected 2"):
        g.term_masks(must=np.zeros((2, 2), np.int32), any=[[4]])
    with pytest.raises(ValueError, match="base has 3 rows, expected 1 or 2"):
        g.term_masks(must=[[1], [2]], base=np.ones((3, 70), bool))
    with pytest.raises(ValueError, match=r"70 \(n_docs\) columns"):
        g.term_masks(must=[[1], [2]], base=np.ones((2, 69), bool))
    with pytest.raises(ValueError, match="3 .* words per row"):
        g.term_masks(must=[[1]], base=np.zeros((1, 4), np.uint32))
    with pytest.raises(ValueError, match="number of masks is unknown"):
        g.term_masks()
    with pytest.raises(ValueError, match="2-D .* list of lists"):
        g.term_masks(must=[1, 2])
    # the arguments that pass: (must, any, must_not, M, base, Mb)
    mu, an, mn, M, b, Mb = g._clauses_arg([[1, 2], [3]], None, [[], [0]], np.ones(70, bool))
    assert (M, Mb) == (2, 1) and mu.tolist() == [[1, 2], [3, -1]] and an.shape == (2, 0)
    assert mn.tolist() == [[-1], [0]] and b.shape == (1, 3) and b.dtype == np.uint32
    assert g._clauses_arg(None, None, None, np.ones((4, 70), bool))[3:6:2] == (4, 4)


def test_gpu_index_term_masks_device_rejects_shapes_before_c():
    import torch
    g = _bare_index(70)
    c = torch.zeros((2, 3), dtype=torch.int32)
    out = torch.zeros((2, 3), dtype=torch.int32)
    with pytest.raises(ValueError, match=r"d_out must be a packed \[M, 3\]"):
        g.term_masks_device(c, None, None, None, out[:, :2])
    with pytest.raises(ValueError, match=r"d_out must be a packed \[M, 3\]"):
        g.term_masks_device(c, None, None, None, out.to(torch.int64))
    with pytest.raises(ValueError, match=r"d_out must be a packed \[M, 3\]"):
        g.term_masks_device(c, None, None, None, out[0])
    with pytest.raises(ValueError, match="d_any has 3 rows, d_out has 2"):
        g.term_masks_device(c, torch.zeros((3, 1), dtype=torch.int32), None, None, out)
    with pytest.raises(ValueError, match="d_must_not must be a 2-D"):
        g.term_masks_device(c, None, c.to(torch.int64), None, out)
    with pytest.raises(ValueError, match="d_must must be a 2-D"):
        g.term_masks_device(c[0], None, None, None, out)
    with pytest.raises(ValueError, match=r"d_base must be a packed \[1 or M, 3\]"):
        g.term_masks_device(c, None, None, torch.zeros((2, 4), dtype=torch.int32), out)
    with pytest.raises(ValueError, match="d_base has 3 rows, expected 1 or 2"):
        g.term_masks_device(c, None, None, torch.zeros((3, 3), dtype=torch.int32), out)


def test_gpu_index_search_boolean_rejects_shapes_before_c():
    g = _bare_index(70)
    q = np.zeros((2, 3), np.int32)
    with pytest.raises(ValueError, match="queries must be a 2-D"):
        g.search_boolean(np.zeros(3, np.int32), 1, must=[[1]])
    with pytest.raises(ValueError, match=r"must has 3 rows, expected 2 \(one per query\)"):
        g.search_boolean(q, 1, must=[[1], [2], [3]])
    with pytest.raises(ValueError, match="base has 3 rows, expected 1 or 2"):
        g.search_boolean(q, 1, any=[[1], [2]], base=np.ones((3, 70), bool))
    with pytest.raises(ValueError, match=r"70 \(n_docs\) columns"):
        g.search_boolean(q, 1, base=np.ones(71, bool))


def test_bm25v_search_boolean_validation_before_gpu():
    import bm25_native
    m = bm25_native.BM25v()
    docs, scores = m.search_boolean([], 3, must=[])
    assert docs.shape == (0, 0) and scores.shape == (0, 0)
    with pytest.raises(ValueError, match="list of list"):
        m.search_boolean(np.array([1, 2], np.int32), 1, must=[[0]])
    with pytest.raises(ValueError, match="list of list"):
        m.search_boolean(np.array([[1, 2]], np.int64), 1, must=[[0]])
    q = np.array([[0, -1]], np.int32)
    with pytest.raises(ValueError, match=r"must_not must have one row per query \(1\), got 2"):
        m.search_boolean(q, 1, must_not=[[0], [0]])
    with pytest.raises(ValueError, match="one row per query"):
        m.search_boolean(q, 1, must=[[0]], base=np.ones((2, 4), bool))
    with pytest.raises(ValueError, match="negative dimensions"):
        m.search_boolean(q, -1, must=[[0]])
    with pytest.raises(ValueError, match=r"maximum token ID in the query \(5\)"):
        m.search_boolean(q, 1, any=[[5, -1]])
    with pytest.raises(ValueError, match=r"maximum token ID in the query \(6\)"):
        m.search_boolean(np.array([[6, -1]], np.int32), 1, must=[[0]])
