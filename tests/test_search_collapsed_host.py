"""CPU tests of field collapsing (bm25_search_collapsed,
bm25_search_collapsed_device, bm25_search_collapsed_stats): the symbols are
exported, bound and documented, a NULL handle is rejected without a GPU, and
the Python layers reject malformed shapes, dtypes, groups of the wrong length,
per_group < 1 and k > 4096 before any C call.

The guards of the GPU tests' yardstick (tests/collapse_model.py) run here: the
numpy restatement of the engine's loop gives the literal walk of the contract
for every page size, and the fixtures really hold what the GPU tests lean on —
ties inside one group and across groups, a group on both sides of the tile
edge, a group that owns a row's first 3 p results, a mask that leaves one
group."""
import ctypes

import numpy as np
import pytest

from collapse_model import layouts, paged_collapsed, ref_collapsed, tie_row
from test_gpu_edges import TILE
from test_search_after_host import (_bare_index, _same, after_case, ordered, position_masks,
                                    ref_after, score_keys, weighted_case)

SYMS = {"bm25_search_collapsed": 14, "bm25_search_collapsed_device": 15,
        "bm25_search_collapsed_stats": 3}
K = 10
PAGE = 64   # the page of the GPU tests' round accounting: dominated depth 3 * PAGE


def _same3(a, b):
    return _same(a, b) and np.array_equal(a[2], b[2])


# ------------------------------------------------------------ model guards
@pytest.mark.parametrize("n_docs", [33, 2049, 5000])
@pytest.mark.parametrize("per_group", [1, 2, K])
def test_paged_model_is_the_walk(n_docs, per_group):
    rows = after_case(n_docs)[4]
    for name, g in layouts(n_docs).items():
        want = ref_collapsed(rows, K, g, per_group, want_groups=True)
        for page in (1, 3, K, 2 * K):
            st = {}
            got = paged_collapsed(rows, K, g, per_group, page, want_groups=True, stats=st)
            assert _same3(got, want), (name, page)
            assert 1 <= st["rounds"] <= K + 1, (name, page, st)


def test_paged_model_under_masks_weights_and_offset():
    rows = after_case(5000)[4]
    allow, qm = position_masks()
    lay = layouts(5000)
    for name in ("uniform", "dominated", "tenant"):
        for per_group in (1, 2):
            want = ref_collapsed(rows, K, lay[name], per_group, allow, qm, 10_000, True)
            got = paged_collapsed(rows, K, lay[name], per_group, 2 * K, allow, qm, 10_000, True)
            assert _same3(got, want), name
            assert (want[0][want[0] >= 0] >= 10_000).all()
    wrows = weighted_case()[5]
    want = ref_collapsed(wrows, K, lay["uniform"], 1, want_groups=True)
    assert _same3(paged_collapsed(wrows, K, lay["uniform"], 1, 7, want_groups=True), want)


@pytest.mark.parametrize("n_docs", [33, 2049, 5000])
def test_no_op_layouts_are_the_plain_order(n_docs):
    rows = after_case(n_docs)[4]
    lay = layouts(n_docs)
    plain = ref_after(rows, K)
    assert _same(ref_collapsed(rows, K, lay["negative"], 1), plain)
    assert _same(ref_collapsed(rows, K, lay["distinct"], 1), plain)
    for name in ("uniform", "dominated", "one"):
        assert _same(ref_collapsed(rows, K, lay[name], K), plain), name
    # ... and a layout that is no no-op differs from it
    assert not _same(ref_collapsed(rows, K, lay["one"], 1), plain)
    one = ref_collapsed(rows, K, lay["one"], 1, want_groups=True)
    assert (one[0][:, 0] == plain[0][:, 0]).all() and (one[0][:, 1:] == -1).all()
    assert (one[2][:, 0] == 0).all() and (one[2][:, 1:] == -1).all()


def test_fixtures_hold_what_the_gpu_tests_lean_on():
    rows = after_case(5000)[4]
    lay = layouts(5000)
    g = lay["uniform"]
    # a tie run whose first members share a group, and one of another group
    # behind them: per_group = 1 keeps the first, drops the second, keeps the third
    r, run = tie_row(rows, K)
    assert r is not None and len(run) >= 3
    sk = score_keys(rows[r][run])
    assert (sk == sk[0]).all()
    assert g[run[0]] == g[run[1]] == 1_000_000 and g[run[2]] == 1_500_000
    got = ref_collapsed(rows[r:r + 1], K, g, 1)[0][0]
    assert run[0] in got and run[1] not in got and run[2] in got
    assert run[1] in ref_collapsed(rows[r:r + 1], K, g, 2)[0][0]
    # a group with members on both sides of the tile edge, equal scores on row 1
    assert g[TILE - 1] == g[TILE] and rows[1][TILE - 1] == rows[1][TILE]
    deep = ref_collapsed(rows[1:2], 4096, g, 1)[0][0]
    assert (TILE - 1 in deep) and (TILE not in deep)
    both = ref_collapsed(rows[1:2], 4096, g, 2)[0][0]
    assert (TILE - 1 in both) and (TILE in both)
    # dominated: one group owns every one of each row's first 3 * PAGE results
    d = lay["dominated"]
    for row in rows:
        assert (d[ordered(row)[:3 * PAGE]] == 7).all()
    st = {}
    paged_collapsed(rows, K, d, 1, PAGE, stats=st)
    assert st["rounds"] == 2 and st["unfinished_rows"] == len(rows) and st["excluded_rows"] > 0
    # a mask that leaves exactly one group, with more than a page of documents:
    # two rounds, where the cursor alone would page through all of them
    t = lay["tenant"]
    allow = (t == 3)[None, :]
    assert set(t[allow[0]].tolist()) == {3} and allow.sum() > PAGE
    st = {}
    got = paged_collapsed(rows, K, t, 1, PAGE, allow, None, stats=st)
    assert st["rounds"] == 2 and (got[0][:, 0] >= 0).all() and (got[0][:, 1:] == -1).all()
    assert -(-5000 // PAGE) == 79
    # group values near 2^31 - 1; the uniform layout has about n / 4 groups
    assert lay["high"].max() == 2**31 - 1 and lay["high"].min() > 2**31 - 1 - 5000
    assert 5000 // 8 < len(np.unique(g)) <= 5000 // 4 + 8
    # with the automatic page (2 k) no uniform row needs a second round
    st = {}
    paged_collapsed(rows, K, g, 1, 2 * K, stats=st)
    assert st["rounds"] == 1


# ------------------------------------------------------------- the C-ABI
def test_symbols_exported_bound_and_documented():
    from bm25mi import _capi
    syms = _capi.header_symbols()
    text = open(_capi.HEADER).read()
    for s, nargs in SYMS.items():
        assert s in syms, s
        f = getattr(_capi.lib, s)
        assert f.restype is ctypes.c_int and s in _capi._SIGS, s
        assert len(f.argtypes) == nargs, s
    doc = text[text.index("Field collapsing"):text.index("int bm25_search_collapsed(")]
    for phrase in ("Replaces no reference call: BM25v.search has no grouping",
                   "(bm25_native.py:76-158)", "per_group", "4096", "LDS", "BM25_EINVAL",
                   "262144", "no cursor argument", "out of scope", "out_groups", "-0.0f",
                   "collapse_page", "collapse_chunk", "k + 1", "Doc shards", "bytes per row",
                   "bm25_search_collapsed_stats", "synchronises"):
        assert phrase in doc, phrase
    assert "262144 (a flag)" in text
    for name in ("collapse_page", "collapse_chunk"):
        assert f'"{name}"' in text and f"BM25_{name.upper()}" in text
    assert _capi.abi_version() == 1  # additive: the ABI version stays
    from bm25mi.index import GpuIndex
    for name in ("search_collapsed", "search_collapsed_device", "collapse_stats"):
        assert callable(getattr(GpuIndex, name))
    import bm25_native
    assert callable(bm25_native.BM25v.search_collapsed)


def test_null_handle_is_einval_without_gpu():
    from bm25mi._capi import BM25_EINVAL, lib
    q = np.zeros((1, 2), np.int32)
    g = np.zeros(4, np.int32)
    docs = np.full((1, 3), 7, np.int32)
    scores = np.full((1, 3), 7.0, np.float32)
    og = np.full((1, 3), 7, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.bm25_search_collapsed(None, p(q), None, 1, 2, 3, None, 0, None, p(g), 1, p(docs),
                                     p(scores), p(og)) == BM25_EINVAL
    assert b"NULL index" in lib.bm25_last_error()
    assert lib.bm25_search_collapsed_device(None, p(q), None, 1, 2, 3, None, 0, None, p(g), 1,
                                            p(docs), p(scores), p(og), None) == BM25_EINVAL
    assert b"NULL index" in lib.bm25_last_error()
    out = (ctypes.c_int64 * 4)()
    assert lib.bm25_search_collapsed_stats(None, out, 4) == BM25_EINVAL
    assert b"NULL index" in lib.bm25_last_error()
    assert (docs == 7).all() and (scores == 7.0).all() and (og == 7).all()


# ------------------------------------------------------- the Python layers
def test_gpu_index_collapsed_rejects_before_c():
    g = _bare_index(70)
    q = np.zeros((2, 3), np.int32)
    grp = np.zeros(70, np.int32)
    with pytest.raises(ValueError, match="queries must be a 2-D"):
        g.search_collapsed(np.zeros(3, np.int32), 1, grp)
    with pytest.raises(ValueError, match="weights must be .* shape"):
        g.search_collapsed(q, 1, grp, 1, np.ones((2, 4), np.float32))
    with pytest.raises(ValueError, match=r"70 \(n_docs\) columns"):
        g.search_collapsed(q, 1, grp, 1, None, np.ones((2, 69), bool))
    with pytest.raises(ValueError, match=r"one mask id per query \(2\)"):
        g.search_collapsed(q, 1, grp, 1, None, np.ones((2, 70), bool), np.zeros(3, np.int32))
    with pytest.raises(ValueError, match=r"in \[-1, 0\)"):
        g.search_collapsed(q, 1, grp, 1, None, None, np.array([0, -1], np.int32))
    with pytest.raises(ValueError, match=r"70 \(n_docs\) entries"):
        g.search_collapsed(q, 1, grp[:69])
    with pytest.raises(ValueError, match=r"70 \(n_docs\) entries"):
        g.search_collapsed(q, 1, np.zeros((2, 70), np.int32))
    with pytest.raises(ValueError, match="integer array"):
        g.search_collapsed(q, 1, grp.astype(np.float32))
    with pytest.raises(ValueError, match="fit int32"):
        g.search_collapsed(q, 1, np.full(70, 2**31, np.int64))
    with pytest.raises(ValueError, match="per_group=0 must be >= 1"):
        g.search_collapsed(q, 1, grp, 0)
    with pytest.raises(ValueError, match=r"k=4097: .* limited to k <= 4096 .*LDS"):
        g.search_collapsed(q, 4097, grp)


def test_gpu_index_collapsed_device_rejects_before_c():
    import torch
    g = _bare_index(70)
    q = torch.zeros((2, 3), dtype=torch.int32)
    w = torch.ones((2, 3), dtype=torch.float32)
    m = torch.zeros((2, 3), dtype=torch.int32)
    qm = torch.zeros(2, dtype=torch.int32)
    grp = torch.zeros(70, dtype=torch.int32)
    d = torch.zeros((2, 4), dtype=torch.int32)
    s = torch.zeros((2, 4), dtype=torch.float32)
    with pytest.raises(ValueError, match="2-D"):
        g.search_collapsed_device(q[0], 4, grp, 1, None, None, None, d, s)
    with pytest.raises(ValueError, match="d_weights must be a float32"):
        g.search_collapsed_device(q, 4, grp, 1, w[:, :2], m, qm, d, s)
    with pytest.raises(ValueError, match=r"packed \[M, 3\]"):
        g.search_collapsed_device(q, 4, grp, 1, w, m[:, :2], qm, d, s)
    with pytest.raises(ValueError, match=r"one mask id per query \(2\)"):
        g.search_collapsed_device(q, 4, grp, 1, w, m, torch.zeros(3, dtype=torch.int32), d, s)
    with pytest.raises(ValueError, match=r"int32 \[70\] \(n_docs\)"):
        g.search_collapsed_device(q, 4, grp[:69], 1, None, None, None, d, s)
    with pytest.raises(ValueError, match=r"int32 \[70\] \(n_docs\)"):
        g.search_collapsed_device(q, 4, grp.to(torch.int64), 1, None, None, None, d, s)
    with pytest.raises(ValueError, match=r"int32 \[70\] \(n_docs\)"):
        g.search_collapsed_device(q, 4, grp.to(torch.float32), 1, None, None, None, d, s)
    with pytest.raises(ValueError, match="per_group=-1 must be >= 1"):
        g.search_collapsed_device(q, 4, grp, -1, None, None, None, d, s)
    with pytest.raises(ValueError, match="limited to k <= 4096"):
        g.search_collapsed_device(q, 4097, grp, 1, None, None, None, d, s)
    with pytest.raises(ValueError, match="2 x 4 results"):
        g.search_collapsed_device(q, 4, grp, 1, None, None, None, d[:, :3], s)
    with pytest.raises(ValueError, match="2 x 4 int32 groups"):
        g.search_collapsed_device(q, 4, grp, 1, None, None, None, d, s, d[:, :3])


def test_bm25v_search_collapsed_validation_before_gpu():
    import bm25_native
    m = bm25_native.BM25v()
    docs, scores = m.search_collapsed([], 3, np.zeros(0, np.int32))
    assert docs.shape == (0, 0) and scores.shape == (0, 0)
    q = np.array([[0, -1]], np.int32)
    grp = np.zeros(4, np.int32)
    with pytest.raises(ValueError, match="list of list"):
        m.search_collapsed(np.array([1, 2], np.int32), 1, grp)
    with pytest.raises(ValueError, match="allow must be"):
        m.search_collapsed(q, 1, grp, allow=np.ones((2, 4), bool))
    with pytest.raises(ValueError, match="1-D integer array"):
        m.search_collapsed(q, 1, grp.astype(np.float64))
    with pytest.raises(ValueError, match="per_group=0 must be >= 1"):
        m.search_collapsed(q, 1, grp, 0)
    with pytest.raises(ValueError, match="limited to top_k <= 4096"):
        m.search_collapsed(q, 4097, grp)
    with pytest.raises(ValueError, match="negative dimensions"):
        m.search_collapsed(q, -1, grp)
    with pytest.raises(ValueError, match=r"maximum token ID in the query \(5\)"):
        m.search_collapsed(np.array([[5, -1]], np.int32), 1, grp)
