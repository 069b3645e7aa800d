"""CPU tests of the filtered search (bm25_search_filtered,
bm25_search_filtered_device, bm25_search_filtered_stats): the symbols are
exported, bound and documented, a NULL handle is rejected without a GPU, the
Python layers (GpuIndex.search_filtered, GpuIndex.search_filtered_device,
BM25v.search_filtered) reject malformed shapes before any C call, and
bm25mi.pack_mask equals a bit-by-bit reference."""
import ctypes

import numpy as np
import pytest

SYMS = ("bm25_search_filtered", "bm25_search_filtered_device", "bm25_search_filtered_stats")


def test_symbols_exported_bound_and_documented():
    from bm25mi import _capi
    syms = _capi.header_symbols()
    text = open(_capi.HEADER).read()
    for s in SYMS:
        assert s in syms, s
        f = getattr(_capi.lib, s)
        assert f.argtypes is not None and f.restype is ctypes.c_int, s
        assert s in _capi._SIGS
    assert len(_capi.lib.bm25_search_filtered.argtypes) == 10
    assert len(_capi.lib.bm25_search_filtered_device.argtypes) == 11
    assert len(_capi.lib.bm25_search_filtered_stats.argtypes) == 3
    doc = text[text.index("Filtered search: the top-k among"):text.index("int bm25_search_filtered(")]
    for phrase in ("Replaces no reference call: BM25v.search has no filter",
                   "(bm25_native.py:76-158)", "ceil(n_docs / 32)", "d & 31", "d >> 5",
                   "-1 = no", "0xFFFFFFFF", "bm25_merge_topk_device", "at most once",
                   "retains scratch", "filter_tiles"):
        assert phrase in doc, phrase
    assert '"filter_tiles"' in text and "4096: the filtered search" in text
    assert _capi.abi_version() == 1  # additive: the ABI version stays


def test_null_handle_is_einval_without_gpu():
    from bm25mi._capi import BM25_EINVAL, lib
    q = np.zeros((1, 2), np.int32)
    m = np.full((1, 1), 0xFFFFFFFF, np.uint32)
    qm = np.zeros(1, np.int32)
    docs = np.full((1, 3), 7, np.int32)
    scores = np.full((1, 3), 7.0, np.float32)
    st = np.full(3, 7, np.int64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.bm25_search_filtered(None, p(q), 1, 2, 3, p(m), 1, p(qm), p(docs),
                                    p(scores)) == BM25_EINVAL
    assert b"NULL index" in lib.bm25_last_error()
    assert lib.bm25_search_filtered_device(None, p(q), 1, 2, 3, p(m), 1, p(qm), p(docs),
                                           p(scores), None) == BM25_EINVAL
    assert b"NULL index" in lib.bm25_last_error()
    assert lib.bm25_search_filtered_stats(None, st.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                          3) == BM25_EINVAL
    assert b"NULL index" in lib.bm25_last_error()
    assert (docs == 7).all() and (scores == 7.0).all() and (st == 7).all()


def _bare_index(n_docs=70):
    """A GpuIndex object without a handle: shape validation runs before the
    handle is touched, so it needs no device."""
    from bm25mi.index import GpuIndex
    g = GpuIndex.__new__(GpuIndex)
    g._h = None
    g.n_docs, g.n_terms, g.doc_offset = n_docs, 5, 0
    return g


def test_gpu_index_search_filtered_rejects_shapes_before_c():
    g = _bare_index(70)  # W = 3
    q = np.zeros((2, 3), np.int32)
    ok = np.ones((2, 70), bool)
    with pytest.raises(ValueError, match="queries must be a 2-D"):
        g.search_filtered(np.zeros(3, np.int32), 1, ok)
    with pytest.raises(ValueError, match=r"70 \(n_docs\) columns"):
        g.search_filtered(q, 1, np.ones((2, 69), bool))
    with pytest.raises(ValueError, match=r"70 \(n_docs\) columns"):
        g.search_filtered(q, 1, np.ones(96, bool))
    with pytest.raises(ValueError, match="3 .* words per row"):
        g.search_filtered(q, 1, np.zeros((2, 2), np.uint32))
    with pytest.raises(ValueError, match="3 .* words per row"):
        g.search_filtered(q, 1, np.zeros((2, 4), np.uint32))
    with pytest.raises(ValueError, match="bool .* or packed uint32"):
        g.search_filtered(q, 1, np.zeros((2, 3), np.int64))
    with pytest.raises(ValueError, match=r"one mask id per query \(2\)"):
        g.search_filtered(q, 1, ok, np.zeros(3, np.int32))
    with pytest.raises(ValueError, match=r"one mask id per query \(2\)"):
        g.search_filtered(q, 1, ok, np.zeros((2, 1), np.int32))
    with pytest.raises(ValueError, match=r"in \[-1, 2\)"):
        g.search_filtered(q, 1, ok, np.array([0, 2], np.int32))
    with pytest.raises(ValueError, match=r"in \[-1, 2\)"):
        g.search_filtered(q, 1, ok, np.array([-2, 1], np.int32))
    with pytest.raises(ValueError, match="no masks given"):
        g.search_filtered(q, 1, np.zeros((0, 3), np.uint32))


def test_gpu_index_search_filtered_device_rejects_shapes_before_c():
    import torch
    g = _bare_index(70)
    q = torch.zeros((2, 3), dtype=torch.int32)
    m = torch.zeros((2, 3), dtype=torch.int32)
    qm = torch.zeros(2, dtype=torch.int32)
    d = torch.zeros((2, 4), dtype=torch.int32)
    s = torch.zeros((2, 4), dtype=torch.float32)
    with pytest.raises(ValueError, match="2-D"):
        g.search_filtered_device(q[0], 4, m, qm, d, s)
    with pytest.raises(ValueError, match=r"packed \[M, 3\]"):
        g.search_filtered_device(q, 4, m[:, :2], qm, d, s)
    with pytest.raises(ValueError, match=r"packed \[M, 3\]"):
        g.search_filtered_device(q, 4, m.to(torch.int64), qm, d, s)
    with pytest.raises(ValueError, match=r"one mask id per query \(2\)"):
        g.search_filtered_device(q, 4, m, torch.zeros(3, dtype=torch.int32), d, s)
    with pytest.raises(ValueError, match="2 x 4 results"):
        g.search_filtered_device(q, 4, m, qm, d[:, :3], s)
    with pytest.raises(ValueError, match="no masks given"):
        g.search_filtered_device(q, 4, m[:0], None, d, s)


def test_bm25v_search_filtered_validation_before_gpu():
    import bm25_native
    m = bm25_native.BM25v()
    docs, scores = m.search_filtered([], 3, np.ones(4, bool))
    assert docs.shape == (0, 0) and scores.shape == (0, 0)
    allow = np.ones(4, bool)
    with pytest.raises(ValueError, match="list of list"):
        m.search_filtered(np.array([1, 2], np.int32), 1, allow)      # a 1-D query array
    with pytest.raises(ValueError, match="list of list"):
        m.search_filtered(np.array([[1, 2]], np.int64), 1, allow)
    q = np.array([[0, -1]], np.int32)
    with pytest.raises(ValueError, match="one row per query"):
        m.search_filtered(q, 1, np.ones((2, 4), bool))
    with pytest.raises(ValueError, match="one row per query"):
        m.search_filtered(q, 1, np.ones((1, 2, 2), bool))
    with pytest.raises(ValueError, match="negative dimensions"):
        m.search_filtered(q, -1, allow)
    with pytest.raises(ValueError, match=r"maximum token ID in the query \(5\)"):
        m.search_filtered(np.array([[5, -1]], np.int32), 1, allow)


@pytest.mark.parametrize("n_docs", [1, 31, 32, 33, 2049])
def test_pack_mask_bit_by_bit(n_docs):
    import bm25mi
    rng = np.random.default_rng(n_docs)
    allow = rng.random((3, n_docs)) < 0.5
    allow[1, :] = True
    allow[2, :] = False
    allow[2, [0, n_docs - 1]] = True
    W = (n_docs + 31) // 32
    want = np.zeros((3, W), np.uint32)
    for m in range(3):
        for d in range(n_docs):
            if allow[m, d]:
                want[m, d >> 5] |= np.uint32(1 << (d & 31))
    got = bm25mi.pack_mask(allow)
    assert got.dtype == np.uint32 and got.shape == (3, W) and got.flags.c_contiguous
    assert np.array_equal(got, want)
    one = bm25mi.pack_mask(allow[0])           # a single mask: one row
    assert one.shape == (1, W) and np.array_equal(one[0], want[0])
    assert np.array_equal(bm25mi.pack_mask(allow.astype(np.uint8)), want)
    with pytest.raises(ValueError, match="allow must be"):
        bm25mi.pack_mask(np.ones((1, 2, 3), bool))
