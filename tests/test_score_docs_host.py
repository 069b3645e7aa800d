"""CPU tests of bm25_score_docs / bm25_score_docs_device (scores of given
(query, document) pairs): both symbols are exported, bound and documented,
a NULL handle is rejected without a GPU, and the Python layers
(GpuIndex.score_docs, GpuIndex.score_docs_device, BM25v.score) reject
malformed shapes before any device call."""
import ctypes

import numpy as np
import pytest

SYMS = ("bm25_score_docs", "bm25_score_docs_device")


def test_symbols_exported_bound_and_documented():
    from bm25mi import _capi
    syms = _capi.header_symbols()
    text = open(_capi.HEADER).read()
    for s in SYMS:
        assert s in syms, s
        f = getattr(_capi.lib, s)
        assert f.argtypes is not None and f.restype is ctypes.c_int, s
        assert s in _capi._SIGS
    assert len(_capi.lib.bm25_score_docs.argtypes) == 7
    assert len(_capi.lib.bm25_score_docs_device.argtypes) == 8
    # the contract stands in the header comment, in the other entries' style
    doc = text[text.index("Scores of given (query, document) pairs"):text.index("int bm25_score_docs(")]
    for phrase in ("Replaces no reference call", "GLOBAL doc ids", "query order", "+0.0f",
                   "bm25_scores_dense", "doc_offset", "never synchronises"):
        assert phrase in doc, phrase
    assert _capi.abi_version() == 1  # additive: the ABI version stays


def test_null_handle_is_einval_without_gpu():
    from bm25mi._capi import BM25_EINVAL, lib
    q = np.zeros((1, 2), np.int32)
    d = np.zeros((1, 3), np.int32)
    out = np.full((1, 3), 7.0, np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.bm25_score_docs(None, p(q), 1, 2, p(d), 3, p(out)) == BM25_EINVAL
    assert b"NULL index" in lib.bm25_last_error()
    assert lib.bm25_score_docs_device(None, p(q), 1, 2, p(d), 3, p(out), None) == BM25_EINVAL
    assert b"NULL index" in lib.bm25_last_error()
    assert (out == 7.0).all()


def _bare_index():
    """A GpuIndex object without a handle: shape validation runs before the
    handle is touched, so it needs no device."""
    from bm25mi.index import GpuIndex
    g = GpuIndex.__new__(GpuIndex)
    g._h = None
    g.n_docs, g.n_terms, g.doc_offset = 10, 5, 0
    return g


def test_gpu_index_score_docs_rejects_shapes_before_c():
    g = _bare_index()
    q2 = np.zeros((2, 3), np.int32)
    d2 = np.zeros((2, 4), np.int32)
    with pytest.raises(ValueError, match="queries must be a 2-D"):
        g.score_docs(np.zeros(3, np.int32), d2)
    with pytest.raises(ValueError, match="queries must be a 2-D"):
        g.score_docs(np.zeros((2, 3, 1), np.int32), d2)
    with pytest.raises(ValueError, match="docs must be a 2-D"):
        g.score_docs(q2, np.zeros(4, np.int32))
    with pytest.raises(ValueError, match="docs must be a 2-D"):
        g.score_docs(q2, np.zeros((2, 2, 2), np.int32))
    with pytest.raises(ValueError, match="2 rows, docs has 3"):
        g.score_docs(q2, np.zeros((3, 4), np.int32))


def test_gpu_index_score_docs_device_rejects_shapes_before_c():
    import torch
    g = _bare_index()
    q2 = torch.zeros((2, 3), dtype=torch.int32)
    d2 = torch.zeros((2, 4), dtype=torch.int32)
    s2 = torch.zeros((2, 4), dtype=torch.float32)
    with pytest.raises(ValueError, match="2-D"):
        g.score_docs_device(q2[0], d2, s2)
    with pytest.raises(ValueError, match="2-D"):
        g.score_docs_device(q2, d2[0], s2)
    with pytest.raises(ValueError, match="2 rows, d_docs has 3"):
        g.score_docs_device(q2, torch.zeros((3, 4), dtype=torch.int32), s2)
    with pytest.raises(ValueError, match="2 x 4 scores"):
        g.score_docs_device(q2, d2, s2[:, :3])


def test_bm25v_score_validation_before_gpu():
    import bm25_native
    m = bm25_native.BM25v()
    out = m.score([], [])
    assert out.shape == (0, 0) and out.dtype == np.float32
    d = np.zeros((1, 2), np.int32)
    with pytest.raises(ValueError, match="list of list"):
        m.score(np.array([[1, 2]], np.int64), d)
    with pytest.raises(ValueError, match="list of list"):
        m.score([[1, 2]], d)
    with pytest.raises(ValueError, match="list of list"):
        m.score(np.array([1, 2], np.int32), d)
    q = np.array([[0, -1]], np.int32)
    with pytest.raises(ValueError, match="docs must be a 2-D"):
        m.score(q, np.zeros(2, np.int32))
    with pytest.raises(ValueError, match="docs must be a 2-D"):
        m.score(q, np.zeros((2, 2), np.int32))
    with pytest.raises(ValueError, match=r"maximum token ID in the query \(5\)"):
        m.score(np.array([[5, -1]], np.int32), d)
