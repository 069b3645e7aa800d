"""CPU tests of minimum-should-match and the hit counts
(bm25_term_masks_min_match, bm25_term_masks_min_match_device, bm25_mask_count,
bm25_mask_count_device, bm25_search_boolean_min_match): the symbols are
exported, bound and documented, a NULL handle is rejected without a GPU and
leaves the outputs untouched, bm25mi.min_match_rows turns an int, an array or
a percentage into int32 rows, the Python layers reject a malformed min_match
before any C call, and the bit-sliced counter of the kernel's counting clause
(tests/min_match_model.py) agrees with a plain integer count."""
import ctypes

import numpy as np
import pytest

from test_term_masks_host import _bare_index

SYMS = {"bm25_term_masks_min_match": 12, "bm25_term_masks_min_match_device": 13,
        "bm25_mask_count": 4, "bm25_mask_count_device": 5, "bm25_search_boolean_min_match": 17}


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
    doc = text[text.index("Minimum-should-match and hit counts:"):
               text.index("int bm25_term_masks_min_match(")]
    flat = " ".join(" ".join(line.strip().lstrip("*") for line in doc.splitlines()).split())
    for phrase in ("n_any(m) = number of slots j of any[m] with any[m][j] >= 0",
                   "count(m, d) >= min_match[m]", "the clause is optional: no constraint",
                   "a repeated id counts each time it occurs",
                   "min_match[m] > n_any(m) allows no document",
                   "bit for bit bm25_term_masks' row", "B > 65535",
                   "the message names row and value", "it counts in n_any and never in count",
                   "Bits at or past n_docs in the last word are ignored even when set",
                   "The caller need not zero the counts", "M may pass 65535",
                   "does not depend on scheduling",
                   "the shards' counts add up to the collection's", "never synchronises",
                   "not ordered against the handle's searches",
                   "leave bm25_search_dispatch, the counters and bm25_search_filtered_stats alone",
                   "before its mask buffer is reused",
                   "k == 0 with a non-NULL out_total_hits still builds and counts the masks"):
        assert phrase in flat, phrase
    assert _capi.abi_version() == 1  # additive: the ABI version stays


def test_null_handle_is_einval_and_outputs_untouched():
    from bm25mi._capi import BM25_EINVAL, lib
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    anyc = np.zeros((2, 2), np.int32)
    mm = np.full(2, 2, np.int32)
    out = np.full((2, 3), 0xA5A5A5A5, np.uint32)
    counts = np.full(2, -7, np.int64)
    q = np.zeros((2, 2), np.int32)
    docs = np.full((2, 3), 7, np.int32)
    scores = np.full((2, 3), 7.0, np.float32)
    totals = np.full(2, -7, np.int64)
    calls = (
        lambda: lib.bm25_term_masks_min_match(None, None, 0, p(anyc), 2, None, 0, p(mm), 2, None, 0,
                                              p(out)),
        lambda: lib.bm25_term_masks_min_match_device(None, None, 0, p(anyc), 2, None, 0, p(mm), 2,
                                                     None, 0, p(out), None),
        lambda: lib.bm25_mask_count(None, p(out), 2, p(counts)),
        lambda: lib.bm25_mask_count_device(None, p(out), 2, p(counts), None),
        lambda: lib.bm25_search_boolean_min_match(None, p(q), 2, 2, 3, None, 0, p(anyc), 2, None, 0,
                                                  p(mm), None, 0, p(docs), p(scores), p(totals)),
    )
    for call in calls:
        assert call() == BM25_EINVAL
        assert b"NULL index" in lib.bm25_last_error()
    assert (out == 0xA5A5A5A5).all() and (counts == -7).all() and (totals == -7).all()
    assert (docs == 7).all() and (scores == 7.0).all()


def test_min_match_rows():
    import bm25mi
    rows = [[1], [1, 2, 3], [1, 2, 3, 4], [1, 2, 3, 4, 5, 6, 7], [1, 2, 3, 4, 5, 6, 7, 8]]
    got = bm25mi.min_match_rows(rows, 2)
    assert got.dtype == np.int32 and got.flags.c_contiguous and got.tolist() == [2] * 5
    assert bm25mi.min_match_rows(rows, np.int64(0)).tolist() == [0] * 5
    assert bm25mi.min_match_rows(rows, [0, 1, 2, 3, 9]).tolist() == [0, 1, 2, 3, 9]
    got = bm25mi.min_match_rows(rows, np.array([5, 4, 3, 2, 1], np.int64))
    assert got.dtype == np.int32 and got.tolist() == [5, 4, 3, 2, 1]
    got = bm25mi.min_match_rows(rows, "75%")
    assert got.dtype == np.int32 and got.tolist() == [1, 2, 3, 5, 6]
    assert bm25mi.min_match_rows(rows, "100%").tolist() == [1, 3, 4, 7, 8]
    assert bm25mi.min_match_rows(rows, "0%").tolist() == [1] * 5   # raised to 1: a term is named
    assert bm25mi.min_match_rows(rows, "50%").tolist() == [1, 1, 2, 3, 4]
    # padding is no term; duplicates are slots of their own; a row without a term gets 0
    padded = np.array([[-1, -1, -1, -1], [4, -1, 4, -1], [3, 3, 3, 3]], np.int32)
    assert bm25mi.min_match_rows(padded, "75%").tolist() == [0, 1, 3]
    assert bm25mi.min_match_rows(padded, "100%").tolist() == [0, 2, 4]
    assert bm25mi.min_match_rows([[], [5]], "75%").tolist() == [0, 1]
    assert bm25mi.min_match_rows(np.zeros((0, 3), np.int32), 3).shape == (0,)
    for bad in ("75", "75 %x", "-5%", "101%", "7.5%", "", 1.5, np.array([1.0, 2.0]), True,
                np.zeros((5, 1), np.int32), None):
        with pytest.raises(ValueError, match="min_match"):
            bm25mi.min_match_rows(rows, bad)
    with pytest.raises(ValueError, match=r"min_match has 3 entries, expected 5 \(one per mask\)"):
        bm25mi.min_match_rows(rows, [1, 2, 3])
    with pytest.raises(ValueError, match=r"min_match\[3\] = -2 is negative"):
        bm25mi.min_match_rows(rows, [1, 2, 3, -2, 0])
    with pytest.raises(ValueError, match=r"min_match\[0\] = -1 is negative"):
        bm25mi.min_match_rows(rows, -1)
    with pytest.raises(ValueError, match="fit int32"):
        bm25mi.min_match_rows(rows, 2**31)


def test_python_layers_reject_min_match_before_c():
    import bm25_native
    g = _bare_index(70)  # no handle: reaching the C call would fail on it
    two = [[1, 2], [3]]
    q = np.zeros((2, 3), np.int32)
    m = bm25_native.BM25v()
    calls = (("mask", lambda mm: g.term_masks(any=two, min_match=mm)),
             ("query", lambda mm: g.search_boolean(q, 1, any=two, min_match=mm)),
             ("query", lambda mm: g.search_boolean(q, 0, any=two, min_match=mm, total_hits=True)),
             ("query", lambda mm: m.search_boolean(q, 1, any=two, min_match=mm)))
    for what, call in calls:
        with pytest.raises(ValueError,
                           match=rf"min_match has 3 entries, expected 2 \(one per {what}\)"):
            call([1, 1, 1])
        with pytest.raises(ValueError, match=r"min_match\[1\] = -1 is negative"):
            call([1, -1])
        with pytest.raises(ValueError, match="min_match must be an int"):
            call(np.array([1.0, 2.0], np.float32))
        with pytest.raises(ValueError, match="min_match must be an int"):
            call(1.0)
        with pytest.raises(ValueError, match="a percentage is written"):
            call("half")
    # BM25v without an any clause: still one entry per query
    with pytest.raises(ValueError, match=r"min_match has 1 entries, expected 2 \(one per query\)"):
        m.search_boolean(q, 1, must=[[0], [0]], min_match=[1])
    # the empty batch keeps its shape with totals
    d, s, t = m.search_boolean([], 3, must=[], total_hits=True)
    assert d.shape == (0, 0) and s.shape == (0, 0) and t.shape == (0,) and t.dtype == np.int64


def test_device_wrappers_reject_shapes_before_c():
    import torch
    g = _bare_index(70)
    c = torch.zeros((2, 3), dtype=torch.int32)
    out = torch.zeros((2, 3), dtype=torch.int32)
    for bad in (torch.zeros(3, dtype=torch.int32), torch.zeros(2, dtype=torch.int64),
                torch.zeros(2, dtype=torch.float32), torch.zeros((2, 1), dtype=torch.int32)):
        with pytest.raises(ValueError, match=r"d_min_match must be an int32 \[2\] tensor"):
            g.term_masks_device(None, c, None, None, out, d_min_match=bad)
    with pytest.raises(ValueError, match=r"d_masks must be a packed \[M, 3\]"):
        g.mask_count_device(out[:, :2], torch.zeros(2, dtype=torch.int64))
    for bad in (torch.zeros(3, dtype=torch.int64), torch.zeros(2, dtype=torch.int32),
                torch.zeros(2, dtype=torch.float64)):
        with pytest.raises(ValueError, match=r"d_counts must be an int64 \[2\] tensor"):
            g.mask_count_device(out, bad)
    with pytest.raises(ValueError, match=r"70 \(n_docs\) columns"):
        g.mask_count(np.ones((2, 69), bool))
    with pytest.raises(ValueError, match="3 .* words per row"):
        g.mask_count(np.zeros((1, 4), np.uint32))


NEEDS = list(range(1, 41)) + [255, 256, 257, 65535]


@pytest.mark.parametrize("need", NEEDS)
def test_bit_sliced_counter_model(need):
    """The counter of the kernel's counting clause against a plain integer
    count: after every one of up to need + 70 additions of random 32-bit words
    (sparse, dense and all-ones words, so that some documents reach ``need``
    exactly at the last step, some early, some never) the sticky word is
    exactly count >= need."""
    import min_match_model as mm
    rng = np.random.default_rng(need)
    words = 6
    assert mm.planes_of(need) == len(bin(need)) - 2 <= mm.PLANES
    cnt, reached = mm.counter_init(need, words)
    assert cnt.shape == (mm.planes_of(need), words) and not reached.any()
    count = np.zeros((words, 32), np.int64)
    for step in range(need + 70):
        w = rng.integers(0, 2**32, size=words, dtype=np.uint64).astype(np.uint32)
        w[0] = 0xFFFFFFFF                       # every step: reaches need at step need exactly
        w[1] &= rng.integers(0, 2**32, dtype=np.uint64).astype(np.uint32)   # sparser
        w[2] = 0xFFFFFFFF if step % 2 else 0     # every other step
        w[3] = 0                                 # never
        mm.counter_add(cnt, reached, w)
        count += (w[:, None] >> np.arange(32, dtype=np.uint32)) & 1
        want = ((count >= need).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1)
        assert np.array_equal(reached, want.astype(np.uint32)), (need, step)
        if step == need - 2:  # one short of need on the word that always counts
            assert reached[0] == 0
    assert reached[0] == 0xFFFFFFFF and reached[3] == 0
    if need <= 257:  # a wrong initial value or a lost carry: off by one either way
        ones = np.full((need, 1), 0xFFFFFFFF, np.uint32)
        assert mm.reached_after(need, ones)[0] == 0xFFFFFFFF
        assert mm.reached_after(need, ones[:-1])[0] == 0
