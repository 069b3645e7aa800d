"""CPU tests of the facet counts (bm25_mask_facets, bm25_mask_facets_device,
bm25_search_boolean_facets): the symbols are exported, bound and documented, a
NULL handle is rejected without a GPU and leaves the outputs untouched, the
Python layers reject malformed arguments before any C call, bm25mi.facet_codes
turns labels into group ids, and the numpy model the GPU tests compare against
(tests/facets_model.py) agrees with a plain Python loop."""
import ctypes

import numpy as np
import pytest

from facets_model import facets_want
from test_term_masks_host import _bare_index

SYMS = {"bm25_mask_facets": 6, "bm25_mask_facets_device": 7, "bm25_search_boolean_facets": 20}


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
    doc = text[text.index("Facet counts:"):text.index("int bm25_mask_facets(")]
    flat = " ".join(" ".join(line.strip().lstrip("*") for line in doc.splitlines()).split())
    for phrase in ("groups [n_docs] int32: groups[d] = the group (category id) of handle-local "
                   "document d, in [0, G); a negative value = the document has no group",
                   "masks [M, W] uint32, W = ceil(n_docs / 32), the layout of bm25_search_filtered",
                   "out [M, G] int64, rows contiguous",
                   "out[m][g] = number of d in [0, n_docs) with bit d of mask row m set and "
                   "groups[d] == g",
                   "Every entry of out is written; the caller need not zero it",
                   "Bits at or past n_docs in the last word are ignored even when set",
                   "No mask word at index >= W of a row is read",
                   "no entry of groups at index >= n_docs is read",
                   "nothing past M * G counts is written", "M may pass 65535",
                   "G == 0 or M == 0 returns BM25_OK without device work",
                   "G lies in [0, 2^31 - 1]", "does not depend on scheduling",
                   "== bm25_mask_count of row m",
                   "the shards' [M, G] outputs add up element-wise to the collection's",
                   "they leave bm25_search_dispatch, bm25_search_counters and "
                   "bm25_search_filtered_stats alone",
                   "the message names d and the value",
                   "On any error the outputs are untouched", "never synchronises",
                   "retains no scratch", "not ordered against the handle's searches",
                   "A groups[d] >= G counts nowhere, exactly like a negative value",
                   "uploaded once per call", "before its mask buffer is reused",
                   "k == 0 with a non-NULL out_facets or out_total_hits builds the masks and "
                   "counts alone",
                   "exactly one of the two with G > 0 is BM25_EINVAL"):
        assert phrase in flat, phrase
    assert _capi.abi_version() == 1  # additive: the ABI version stays


def test_null_handle_is_einval_and_outputs_untouched():
    from bm25mi._capi import BM25_EINVAL, lib
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    masks = np.full((2, 3), 0xFFFFFFFF, np.uint32)
    groups = np.zeros(70, np.int32)
    counts = np.full((2, 4), -7, np.int64)
    q = np.zeros((2, 2), np.int32)
    anyc = np.zeros((2, 2), np.int32)
    docs = np.full((2, 3), 7, np.int32)
    scores = np.full((2, 3), 7.0, np.float32)
    totals = np.full(2, -7, np.int64)
    calls = (
        lambda: lib.bm25_mask_facets(None, p(masks), 2, p(groups), 4, p(counts)),
        lambda: lib.bm25_mask_facets_device(None, p(masks), 2, p(groups), 4, p(counts), None),
        lambda: lib.bm25_search_boolean_facets(None, p(q), 2, 2, 3, None, 0, p(anyc), 2, None, 0,
                                               None, None, 0, p(groups), 4, p(docs), p(scores),
                                               p(totals), p(counts)),
    )
    for call in calls:
        assert call() == BM25_EINVAL
        assert b"NULL index" in lib.bm25_last_error()
    assert (counts == -7).all() and (totals == -7).all()
    assert (docs == 7).all() and (scores == 7.0).all()


def test_python_layers_reject_facets_before_c():
    import bm25_native
    g = _bare_index(70)  # no handle: reaching the C call would fail on it
    masks = np.ones((2, 70), bool)
    groups = np.zeros(70, np.int64)
    q = np.zeros((2, 3), np.int32)
    two = [[1, 2], [3]]
    m = bm25_native.BM25v()
    calls = (lambda gr, G: g.facets(masks, gr, G),
             lambda gr, G: g.search_boolean(q, 1, any=two, facets=(gr, G)),
             lambda gr, G: g.search_boolean(q, 0, any=two, total_hits=True, facets=(gr, G)))
    for call in calls:
        with pytest.raises(ValueError, match=r"groups has shape \(69,\), expected \(70,\)"):
            call(groups[:69], 4)
        with pytest.raises(ValueError, match=r"groups has shape \(2, 35\)"):
            call(groups.reshape(2, 35), 4)
        with pytest.raises(ValueError, match="groups must be an integer array"):
            call(groups.astype(np.float32), 4)
        with pytest.raises(ValueError, match="groups must be an integer array"):
            call(groups.astype(bool), 4)
        with pytest.raises(ValueError, match="n_groups = -1 is negative"):
            call(groups, -1)
        with pytest.raises(ValueError, match="n_groups must be an int"):
            call(groups, 4.0)
        with pytest.raises(ValueError, match="n_groups must fit int32"):
            call(groups, 2**31)
        with pytest.raises(ValueError, match="groups entries must fit int32"):
            call(np.full(70, 2**31, np.int64), 4)
    with pytest.raises(ValueError, match=r"70 \(n_docs\) columns"):
        g.facets(np.ones((2, 69), bool), groups, 4)
    with pytest.raises(ValueError, match="3 .* words per row"):
        g.facets(np.zeros((1, 4), np.uint32), groups, 4)
    for bad in (groups, (groups,), (groups, 4, 4), 4):
        with pytest.raises(ValueError, match=r"facets must be a pair \(groups, n_groups\)"):
            g.search_boolean(q, 1, any=two, facets=bad)
        with pytest.raises(ValueError, match=r"facets must be a pair \(groups, n_groups\)"):
            m.search_boolean(q, 1, any=two, facets=bad)
    # the empty batch keeps its shape with totals and facets
    out = m.search_boolean([], 3, must=[], total_hits=True, facets=(groups, 4))
    assert [a.shape for a in out] == [(0, 0), (0, 0), (0,), (0, 4)] and out[3].dtype == np.int64
    out = m.search_boolean([], 3, must=[], facets=(groups, 4))
    assert [a.shape for a in out] == [(0, 0), (0, 0), (0, 4)]
    assert len(m.search_boolean([], 3, must=[])) == 2  # without facets=: today's shape


def test_device_wrapper_rejects_shapes_before_c():
    import torch
    g = _bare_index(70)
    dm = torch.zeros((2, 3), dtype=torch.int32)
    dg = torch.zeros(70, dtype=torch.int32)
    dc = torch.zeros((2, 4), dtype=torch.int64)
    with pytest.raises(ValueError, match=r"d_masks must be a packed \[M, 3\]"):
        g.facets_device(dm[:, :2], dg, 4, dc)
    with pytest.raises(ValueError, match=r"d_masks must be a packed \[M, 3\]"):
        g.facets_device(dm.to(torch.int64), dg, 4, dc)
    with pytest.raises(ValueError, match="d_masks must be contiguous"):
        g.facets_device(torch.zeros((3, 2), dtype=torch.int32).t(), dg, 4, dc)
    for bad in (torch.zeros(69, dtype=torch.int32), torch.zeros(70, dtype=torch.int64),
                torch.zeros(70, dtype=torch.float32), torch.zeros((70, 1), dtype=torch.int32),
                torch.zeros(140, dtype=torch.int32)[::2]):
        with pytest.raises(ValueError, match=r"d_groups must be an int32 \[70\] tensor"):
            g.facets_device(dm, bad, 4, dc)
    for bad in (torch.zeros((2, 5), dtype=torch.int64), torch.zeros((3, 4), dtype=torch.int64),
                torch.zeros(8, dtype=torch.int64), torch.zeros((2, 4), dtype=torch.int32),
                torch.zeros((2, 4), dtype=torch.float64),
                torch.zeros((4, 2), dtype=torch.int64).t()):
        with pytest.raises(ValueError, match=r"d_counts must be an int64 \[2, 4\] tensor"):
            g.facets_device(dm, dg, 4, bad)
    with pytest.raises(ValueError, match="n_groups = -1 must be in"):
        g.facets_device(dm, dg, -1, dc)
    with pytest.raises(ValueError, match="n_groups must be an int"):
        g.facets_device(dm, dg, 4.0, dc)


def test_facet_codes():
    import bm25mi
    codes, uniq = bm25mi.facet_codes(["en", "de", "en", "fr", "de", "en"])
    assert codes.dtype == np.int32 and codes.tolist() == [1, 0, 1, 2, 0, 1]
    assert uniq.tolist() == ["de", "en", "fr"]
    codes, uniq = bm25mi.facet_codes(np.array([2024, 1999, 2024, 7], np.int64))
    assert codes.dtype == np.int32 and codes.tolist() == [2, 1, 2, 0]
    assert uniq.tolist() == [7, 1999, 2024]
    # None: no group (code -1), and no unique
    labels = ["b", None, "a", None, "b"]
    codes, uniq = bm25mi.facet_codes(labels)
    assert codes.tolist() == [1, -1, 0, -1, 1] and uniq.tolist() == ["a", "b"]
    assert all(labels[d] is None if c < 0 else uniq[c] == labels[d] for d, c in enumerate(codes))
    codes, uniq = bm25mi.facet_codes([None, 5, 3, None, 5])
    assert codes.tolist() == [-1, 1, 0, -1, 1] and uniq.tolist() == [3, 5]
    codes, uniq = bm25mi.facet_codes([None, None])
    assert codes.tolist() == [-1, -1] and len(uniq) == 0
    # masked entries: no group
    ma = np.ma.array([4, 9, 4, 1], mask=[False, True, False, False])
    codes, uniq = bm25mi.facet_codes(ma)
    assert codes.tolist() == [1, -1, 1, 0] and uniq.tolist() == [1, 4]
    codes, uniq = bm25mi.facet_codes([])
    assert codes.dtype == np.int32 and codes.shape == (0,) and len(uniq) == 0
    # np.unique's semantics on a random array
    rng = np.random.default_rng(3)
    a = rng.integers(-50, 50, 500)
    codes, uniq = bm25mi.facet_codes(a)
    u, inv = np.unique(a, return_inverse=True)
    assert np.array_equal(uniq, u) and np.array_equal(codes, inv.ravel())


def test_numpy_model_against_a_plain_loop():
    """70 documents, 3 masks, G = 5: negative groups, groups >= G (G itself and
    2^31 - 1) and garbage bits at or past n_docs in the last word."""
    import bm25mi
    rng = np.random.default_rng(11)
    n, G = 70, 5
    allow = rng.random((3, n)) < 0.6
    allow[1] = True
    groups = rng.integers(0, G, n).astype(np.int32)
    groups[rng.random(n) < 0.2] = -1
    groups[[3, 40]] = -2**31
    groups[[7, 69]] = G
    groups[[8, 33]] = 2**31 - 1
    allow[:, [3, 7, 8, 69]] = True   # the out-of-range documents are allowed ones
    packed = bm25mi.pack_mask(allow)
    packed[:, -1] |= np.uint32(0xFFFFFFFF << (n % 32) & 0xFFFFFFFF)   # garbage tail bits
    want = np.zeros((3, G), np.int64)
    for m in range(3):
        for d in range(n):
            if (int(packed[m, d >> 5]) >> (d & 31)) & 1 and 0 <= groups[d] < G:
                want[m, groups[d]] += 1
    got = facets_want(packed, groups, G)
    assert got.dtype == np.int64 and got.shape == (3, G) and np.array_equal(got, want)
    assert want.sum() > 0 and want[1].sum() == ((groups >= 0) & (groups < G)).sum()
    assert facets_want(packed, groups, 0).shape == (3, 0)
    assert facets_want(packed[:0], groups, G).shape == (0, G)
