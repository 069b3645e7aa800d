"""CPU tests of the sort-by-field search (bm25_sort_ranks(_device),
bm25_search_sorted(_device), bm25_search_sorted_scratch,
bm25_search_boolean_sorted): the symbols are exported, bound and documented,
a NULL handle is rejected without a GPU and leaves the outputs untouched, the
Python layers reject malformed arguments before any C call with the value
named (the C calls' own messages for the same mistakes are checked against a
handle in tests/test_gpu_search_sorted.py), and the numpy model the GPU tests
compare against (tests/sorted_model.py) agrees with hand-written cases.  A
stand-alone program (tests/asan/sorted_check.cpp) drives the host-side
validation of ranks / perm / cursors and the scratch-size arithmetic under
AddressSanitizer and UBSan."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from sorted_model import order_want, select_want
from test_term_masks_host import _bare_index

SYMS = {"bm25_sort_ranks": 6, "bm25_sort_ranks_device": 7, "bm25_search_sorted_scratch": 4,
        "bm25_search_sorted": 9, "bm25_search_sorted_device": 12, "bm25_search_boolean_sorted": 31}


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
    doc = text[text.index("Sort-by-field search:"):text.index("int bm25_sort_ranks(")]
    flat = " ".join(" ".join(line.strip().lstrip("*") for line in doc.splitlines()).split())
    for phrase in ("int64 never goes through a float", "-0.0f == +0.0f",
                   "NaN is \"no value\": it comes after every number in both directions",
                   "descending != 0 reverses the order of the numbers only",
                   "Equal values are ordered by doc id ascending in both directions",
                   "permutations of [0, n_docs) and inverses of each other",
                   "No values entry at index >= n_docs is read",
                   "a setup call, like bm25_index_set_world_bounds",
                   "24 bytes per document", "synchronises `stream`",
                   "ranks[d] > after_ranks[m]", "doc -1 and rank -1",
                   "perm[after + 1 .. after + k]",
                   "no word at index >= W of a row is read",
                   "BM25_AFTER_NONE (-2)", "reads no mask word",
                   "Entries < -2 are \"no cursor\" in the device call and BM25_EINVAL in the host "
                   "call",
                   "0 <= k <= min(n_docs, 4096)", "M may pass 65535",
                   "the message names the first offending index",
                   "On an error the outputs are untouched",
                   "never synchronises and retains nothing",
                   "not ordered against the handle's searches",
                   "A ranks entry outside [0, n_docs) is never eligible",
                   "nothing outside the caller's buffers is touched",
                   "4 M (4 + 1 + 256 + min(k + 2048, n_docs))",
                   "it is bm25_search_boolean_ranges, bit for bit, chunk size included",
                   "bm25_score_docs_device's bits", "score bits 0xFFFFFFFF and rank -1",
                   "go up once per call", "k > 4096 with ranks is BM25_EINVAL",
                   "Out of scope: merging sorted lists of doc shards",
                   "an early-terminating walk of perm for dense masks"):
        assert phrase in flat, phrase
    assert "\"sorted_bins\"" in text and "BM25_SORTED_BINS" in text
    assert _capi.lib.bm25_abi_version() == 1  # additive: the ABI version stays


def test_null_handle_is_einval_and_outputs_untouched():
    from bm25mi._capi import BM25_EINVAL, lib
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    n = 70
    values = np.arange(n, dtype=np.int32)
    ranks = np.full(n, 7, np.int32)
    perm = np.full(n, 7, np.int32)
    masks = np.full((2, 3), 0xFFFFFFFF, np.uint32)
    docs = np.full((2, 3), 7, np.int32)
    oranks = np.full((2, 3), 7, np.int32)
    scores = np.full((2, 3), 7.0, np.float32)
    q = np.zeros((2, 2), np.int32)
    anyc = np.zeros((2, 2), np.int32)
    nbytes = ctypes.c_int64(-7)
    calls = (
        lambda: lib.bm25_sort_ranks(None, p(values), 0, 0, p(ranks), p(perm)),
        lambda: lib.bm25_sort_ranks_device(None, p(values), 0, 0, p(ranks), p(perm), None),
        lambda: lib.bm25_search_sorted_scratch(None, 2, 3, ctypes.byref(nbytes)),
        lambda: lib.bm25_search_sorted(None, p(masks), 2, p(ranks), p(perm), 3, None, p(docs),
                                       p(oranks)),
        lambda: lib.bm25_search_sorted_device(None, p(masks), 2, p(ranks), p(perm), 3, None,
                                              p(docs), p(oranks), None, 0, None),
        lambda: lib.bm25_search_boolean_sorted(None, p(q), 2, 2, 3, None, 0, p(anyc), 2, None, 0,
                                               None, None, 0, None, 0, None, 0, 0, None, None, None,
                                               0, p(docs), p(scores), None, None, p(ranks), p(perm),
                                               None, p(oranks)),
    )
    for call in calls:
        assert call() == BM25_EINVAL
        assert b"NULL index" in lib.bm25_last_error()
    assert (ranks == 7).all() and (perm == 7).all() and (docs == 7).all()
    assert (oranks == 7).all() and (scores == 7.0).all() and nbytes.value == -7


def test_python_layers_reject_before_c():
    import bm25_native
    n = 70
    g = _bare_index(n)  # no handle: reaching the C call would fail on it
    v = np.arange(n, dtype=np.int32)
    ranks, perm = order_want(v)
    masks = np.ones((2, n), bool)
    q = np.zeros((2, 3), np.int32)
    two = [[1, 2], [3]]
    # the column
    for bad in (np.float64, bool, np.int16, np.uint32):
        with pytest.raises(ValueError, match=f"values have dtype {np.dtype(bad).name}"):
            g.sort_ranks(v.astype(bad))
    with pytest.raises(ValueError, match=r"values has shape \(69,\), expected \(70,\)"):
        g.sort_ranks(v[:69])
    with pytest.raises(ValueError, match=r"values has shape \(1, 70\)"):
        g.sort_ranks(v[None])
    # the order, through search_sorted and search_boolean alike
    calls = (lambda order, k=3, after=None: g.search_sorted(masks, order, k, after),
             lambda order, k=3, after=None: g.search_boolean(q, k, any=two, sort=order,
                                                             after_ranks=after))
    for call in calls:
        for bad in (ranks, (ranks,), (ranks, perm, perm), 4):
            with pytest.raises(ValueError, match=r"the order must be a pair \(ranks, perm\)"):
                call(bad)
        with pytest.raises(ValueError, match=r"ranks must be an integer \[70\] array"):
            call((ranks[:69], perm))
        with pytest.raises(ValueError, match=r"perm must be an integer \[70\] array"):
            call((ranks, perm.astype(np.float32)))
        r = ranks.copy()
        r[5], r[9] = 70, -1
        with pytest.raises(ValueError, match=r"ranks\[5\] = 70 is outside \[0, 70\)"):
            call((r, perm))
        r = ranks.copy()
        r[11] = r[40]            # two documents at one rank: 11 is the first offending index
        with pytest.raises(ValueError, match=r"ranks\[11\] = 40 but perm\[40\] = 40: ranks and perm "
                                             "are not inverse permutations"):
            call((r, perm))
        pp = perm.copy()
        pp[3], pp[4] = pp[4], pp[3]
        with pytest.raises(ValueError, match=r"ranks\[3\] = 3 but perm\[3\] = 4"):
            call((ranks, pp))
        # k and the cursors
        with pytest.raises(ValueError, match="k = 4097: a sorted search returns at most 4096"):
            call((ranks, perm), 4097)
        with pytest.raises(ValueError, match="k = 71 is above the index's 70 documents"):
            call((ranks, perm), 71)
        with pytest.raises(ValueError, match="negative dimensions are not allowed"):
            call((ranks, perm), -1)
        with pytest.raises(ValueError, match=r"after_ranks\[1\] = -3 is below BM25_AFTER_NONE"):
            call((ranks, perm), 3, np.array([-2, -3]))
        with pytest.raises(ValueError, match=r"after must hold one rank per (mask row|query) \(2\)"):
            call((ranks, perm), 3, np.array([1, 2, 3]))
        with pytest.raises(ValueError, match="NULL index"):   # well-formed: reaches the C call
            call((ranks, perm), 3, np.array([-2, -1]))
        with pytest.raises(ValueError, match="NULL index"):
            call((ranks.astype(np.int64), perm.tolist()), 0)
    with pytest.raises(ValueError, match=r"after_ranks needs sort=\(ranks, perm\)"):
        g.search_boolean(q, 3, any=two, after_ranks=np.array([1, 2]))
    with pytest.raises(ValueError, match="negative mask shape"):
        g.search_sorted(-1, (ranks, perm), 3)
    with pytest.raises(ValueError, match="NULL index"):
        g.search_sorted(2, (ranks, perm), 3)                  # an int: M rows, no masks
    # bm25_native passes the two keywords through; the empty batch keeps its shape
    m = bm25_native.BM25v()
    out = m.search_boolean([], 3, must=[], sort=(ranks, perm))
    assert [a.shape for a in out] == [(0, 0), (0, 0), (0, 0)] and out[2].dtype == np.int32
    out = m.search_boolean([], 3, must=[], sort=(ranks, perm), total_hits=True)
    assert [a.shape for a in out] == [(0, 0), (0, 0), (0, 0), (0,)]


def test_device_wrappers_reject_shapes_before_c():
    import torch
    n = 70
    g = _bare_index(n)
    dv = torch.zeros(n, dtype=torch.int32)
    dr = torch.zeros(n, dtype=torch.int32)
    dp = torch.zeros(n, dtype=torch.int32)
    for bad in (dv.to(torch.float64), dv.to(torch.int16)):
        with pytest.raises(ValueError, match="d_values has dtype"):
            g.sort_ranks_device(bad, dr, dp)
    with pytest.raises(ValueError, match=r"d_values must be a contiguous \[70\]"):
        g.sort_ranks_device(dv[:69], dr, dp)
    with pytest.raises(ValueError, match=r"d_perm must be a contiguous int32 \[70\]"):
        g.sort_ranks_device(dv, dr, dp.to(torch.int64))
    with pytest.raises(ValueError, match="NULL index"):
        g.sort_ranks_device(dv, dr, dp)
    dm = torch.zeros((2, 3), dtype=torch.int32)
    dd = torch.zeros((2, 5), dtype=torch.int32)
    do = torch.zeros((2, 5), dtype=torch.int32)
    sc = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(ValueError, match=r"d_docs must be an int32 \[M, 4\]"):
        g.search_sorted_device(dm, dr, dp, 4, None, dd, do, sc)
    with pytest.raises(ValueError, match=r"d_masks must be a contiguous packed \[2, 3\]"):
        g.search_sorted_device(dm[:, :2], dr, dp, 5, None, dd, do, sc)
    with pytest.raises(ValueError, match=r"d_out_ranks must be a contiguous int32 \[2, 5\]"):
        g.search_sorted_device(dm, dr, dp, 5, None, dd, do[:1], sc)
    with pytest.raises(ValueError, match=r"d_ranks must be a contiguous int32 \[70\]"):
        g.search_sorted_device(dm, dr[:69], dp, 5, None, dd, do, sc)
    with pytest.raises(ValueError, match=r"d_after must be a contiguous int32 \[2\]"):
        g.search_sorted_device(dm, dr, dp, 5, torch.zeros(3, dtype=torch.int32), dd, do, sc)
    with pytest.raises(ValueError, match="k = 4097"):
        g.search_sorted_device(dm, dr, dp, 4097, None, dd, do, sc)
    with pytest.raises(ValueError, match="NULL index"):
        g.search_sorted_device(dm, dr, dp, 5, None, dd, do, sc)


def test_host_validation_under_sanitizers():
    """check_sort_order / check_after_ranks on exactly sized heap arrays and
    sorted_scratch_bytes at its limits, ASan + UBSan, no device."""
    from bm25mi.build import build_sorted_check
    exe = build_sorted_check()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "sorted_check ok" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------------------ the model
def test_model_ties_by_doc_id():
    v = np.array([5, 3, 5, 3, 9, 3], np.int32)
    ranks, perm = order_want(v)
    assert perm.tolist() == [1, 3, 5, 0, 2, 4] and ranks.tolist() == [3, 0, 4, 1, 5, 2]
    ranks, perm = order_want(v, descending=True)
    assert perm.tolist() == [4, 0, 2, 1, 3, 5]      # 9, then the 5s and the 3s by doc id


def test_model_nan_last_in_both_directions_and_zeros():
    nan, inf = np.float32("nan"), np.float32("inf")
    v = np.array([nan, 1.5, -0.0, -inf, 0.0, nan, inf, -2.0, 0.0], np.float32)
    _, perm = order_want(v)
    assert perm.tolist() == [3, 7, 2, 4, 8, 1, 6, 0, 5]   # +-0 are one value: by doc id
    _, perm = order_want(v, descending=True)
    assert perm.tolist() == [6, 1, 2, 4, 8, 7, 3, 0, 5]   # the NaNs stay last, by doc id
    ranks, perm = order_want(v)
    assert np.array_equal(ranks[perm], np.arange(9))


def test_model_int64_below_float_precision():
    """2^53 and 2^53 + 1 are one float64; INT64 limits are not negated."""
    a = 2 ** 53
    v = np.array([a + 1, a, -a - 1, -a, 2 ** 63 - 1, -2 ** 63, a + 1], np.int64)
    _, perm = order_want(v)
    assert perm.tolist() == [5, 2, 3, 1, 0, 6, 4]
    _, perm = order_want(v, descending=True)
    assert perm.tolist() == [4, 0, 6, 1, 3, 2, 5]
    v32 = np.array([2 ** 31 - 1, -2 ** 31, 0, -1], np.int32)
    assert order_want(v32)[1].tolist() == [1, 3, 2, 0]
    assert order_want(v32, True)[1].tolist() == [0, 2, 3, 1]


def test_model_selection():
    v = np.array([40, 10, 30, 20, 50, 60], np.int32)
    ranks, perm = order_want(v)                     # perm = 1 3 2 0 4 5
    allowed = np.array([[1, 1, 1, 1, 1, 1],
                        [1, 0, 1, 0, 1, 0],         # docs 0 2 4: ranks 3 2 4
                        [0, 0, 0, 0, 0, 0],
                        [0, 0, 0, 0, 0, 1]], bool)
    docs, out = select_want(allowed, ranks, perm, 4, doc_offset=100)
    assert docs.tolist() == [[101, 103, 102, 100], [102, 100, 104, -1], [-1] * 4,
                             [105, -1, -1, -1]]
    assert out.tolist() == [[0, 1, 2, 3], [2, 3, 4, -1], [-1] * 4, [5, -1, -1, -1]]
    # cursors: after rank 2; -2 none; -1 an all-padding row; the last rank: nothing left
    docs, out = select_want(allowed, ranks, perm, 2, after=[2, -2, -1, 5])
    assert docs.tolist() == [[0, 4], [2, 0], [-1, -1], [-1, -1]]
    assert out.tolist() == [[3, 4], [2, 3], [-1, -1], [-1, -1]]
    # no masks: perm[after + 1 .. after + k]
    docs, out = select_want(2, ranks, perm, 3, after=[-2, 3])
    assert docs.tolist() == [[1, 3, 2], [4, 5, -1]] and out.tolist() == [[0, 1, 2], [4, 5, -1]]
