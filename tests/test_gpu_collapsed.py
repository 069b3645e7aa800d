"""GPU tests of field collapsing (bm25_search_collapsed /
bm25_search_collapsed_device; the kernels of bm25mi_collapse.hip and the loop
run_collapsed of bm25mi_capi.cpp).

The expected rows come from tests/collapse_model.py (ref_collapsed: the literal
walk of the contract over the C oracle's dense rows, the weighted numpy fold
for weighted rows), whose guards run on the CPU
(tests/test_search_collapsed_host.py).  Docs and groups compare exactly and
scores on their uint32 views, by the host call and by the device call (a
non-default stream, outputs pre-filled with garbage).  The shapes sit next to

  64     entries of a chunk of the collapse kernel (k = 64: one chunk; 65: a
         lane past it)
  2048   documents per tile (a group with equal scores on 2047 and 2048)
  4096   the largest k: the LDS group table full"""
import ctypes

import numpy as np
import pytest

from collapse_model import layouts, paged_collapsed, ref_collapsed
from test_gpu_edges import NEG_ZERO32
from test_gpu_parity import _exact, _idx
from test_search_after_host import PAD, after_case, position_masks, weighted_case

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (33, 10), (2049, 64), (2049, 65), (5000, 1), (5000, 100), (5000, 4096)]
# (the sparse segment table changes the score passes alone: every shape but the largest k)
SHAPE_CASES = [(seg, n, k) for seg in ("dense", "sparse") for n, k in SHAPES
               if not (seg == "sparse" and k == 4096)]
PAGE = 64


def _pack(allow):
    import bm25mi
    return None if allow is None else bm25mi.pack_mask(allow)


def _device(index, q, k, groups, per_group, weights=None, packed=None, query_mask=None,
            want_groups=True):
    import torch
    st = torch.cuda.Stream()
    up = lambda a, t: None if a is None else torch.from_numpy(np.array(a, t)).cuda()
    dq = up(q, np.int32)
    dw = up(weights, np.float32)
    dg = up(groups, np.int32)
    dm = None if packed is None else torch.from_numpy(
        np.ascontiguousarray(packed).view(np.int32)).cuda()
    dqm = up(query_mask, np.int32)
    dd = torch.full((len(q), k), 123456789, dtype=torch.int32, device="cuda")
    ds = torch.full((len(q), k), 7.5, dtype=torch.float32, device="cuda")
    dog = torch.full((len(q), k), 424242, dtype=torch.int32, device="cuda") if want_groups else None
    torch.cuda.synchronize()  # (the uploads ran on the current stream)
    index.search_collapsed_device(dq, k, dg, per_group, dw, dm, dqm, dd, ds, dog, st)
    st.synchronize()
    return dd.cpu().numpy(), ds.cpu().numpy(), (dog.cpu().numpy() if want_groups else None)


def _exact3(got, want, what=""):
    _exact(got[:2], want[:2])
    assert np.array_equal(got[2], want[2]), what


def _check(index, q, k, groups, per_group, want, weights=None, packed=None, query_mask=None,
           what=""):
    """The host call and the device call both return ``want`` bit for bit."""
    got = index.search_collapsed(q, k, groups, per_group, weights, packed, query_mask,
                                 return_groups=True)
    assert got[0].dtype == np.int32 and got[1].dtype == np.float32 and got[2].dtype == np.int32
    assert got[0].shape == got[2].shape == (len(q), k), what
    _exact3(got, want, what)
    _exact3(_device(index, q, k, groups, per_group, weights, packed, query_mask), want, what)
    assert not (got[1].view(np.uint32) == NEG_ZERO32).any(), what
    pad = got[0] < 0
    assert (got[1].view(np.uint32)[pad] == PAD).all() and (got[2][pad] == -1).all(), what
    return got


# ------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("segments,n_docs,k", SHAPE_CASES)
def test_shapes_and_layouts(gpu, segments, n_docs, k):
    """Every shape under the uniform, dominated, all-negative, one-group and
    near-2^31 layouts with per_group 1, 2 and k.  At 33 documents the rows run
    through the positive, zero and negative regions into padding; the
    one-group layout with per_group 1 is one hit, then padding."""
    ip, ix, dt, q, rows = after_case(n_docs)
    index = _idx(ip, ix, dt, n_docs, segments=segments)
    lay = layouts(n_docs)
    for name in ("uniform", "dominated", "negative", "one", "high"):
        for per_group in sorted({1, 2, k}):
            want = ref_collapsed(rows, k, lay[name], per_group, want_groups=True)
            got = _check(index, q, k, lay[name], per_group, want, what=(name, per_group))
            if name == "one" and per_group == 1:
                assert (got[0][:, 0] >= 0).all() and (got[0][:, 1:] == -1).all()
    assert index.last_dispatch()["collapsed"]
    index.close()


def test_null_groups_out_is_allowed(gpu):
    ip, ix, dt, q, rows = after_case(2049)
    index = _idx(ip, ix, dt, 2049)
    g = layouts(2049)["dominated"]
    want = ref_collapsed(rows, 65, g, 1)
    _exact(index.search_collapsed(q, 65, g, 1), want)
    _exact(_device(index, q, 65, g, 1, want_groups=False)[:2], want)
    index.close()


# ------------------------------------------- 2. masks, weights, doc_offset
@pytest.fixture(scope="module")
def big(gpu):
    """The 5000-document fixture (3 tiles) with two masks and mask ids mixing
    -1, 0 and 1; one handle at doc_offset 0 and one at 10 000."""
    ip, ix, dt, q, rows = after_case(5000)
    allow, qm = position_masks()
    handles = {off: _idx(ip, ix, dt, 5000, doc_offset=off) for off in (0, 10_000)}
    yield q, rows, allow, qm, _pack(allow), handles
    for h in handles.values():
        h.close()


@pytest.mark.parametrize("doc_offset", [0, 10_000])
def test_masks_and_doc_offset(big, doc_offset):
    q, rows, allow, qm, packed, handles = big
    index = handles[doc_offset]
    lay = layouts(5000)
    for name in ("uniform", "dominated", "tenant", "high"):
        for per_group, k in ((1, 10), (2, 10), (10, 10), (1, 100)):
            want = ref_collapsed(rows, k, lay[name], per_group, allow, qm, doc_offset, True)
            _check(index, q, k, lay[name], per_group, want, None, packed, qm,
                   what=(name, per_group, k))
    # NULL mask ids with masks: mask 0 for every row
    want = ref_collapsed(rows, 10, lay["uniform"], 1, allow, None, doc_offset, True)
    _check(index, q, 10, lay["uniform"], 1, want, None, packed, None)


def test_weights_of_both_signs(gpu):
    ip, ix, dt, q, w, rows = weighted_case()
    allow, qm = position_masks()
    qm = np.resize(qm, len(q)).astype(np.int32)
    index = _idx(ip, ix, dt, 5000)
    lay = layouts(5000)
    for name in ("uniform", "dominated", "one"):
        for per_group in (1, 2):
            want = ref_collapsed(rows, 10, lay[name], per_group, want_groups=True)
            _check(index, q, 10, lay[name], per_group, want, w, what=(name, per_group))
            want = ref_collapsed(rows, 10, lay[name], per_group, allow, qm, 0, True)
            _check(index, q, 10, lay[name], per_group, want, w, _pack(allow), qm)
    index.close()


# --------------------------------------------------------------- 3. identities
def test_no_op_layouts_are_the_plain_searches(big):
    """All groups negative, all distinct, per_group >= k: the rows of
    search_weighted under the same weights and masks, and of search without
    them, bit for bit (k = 4096: the group table holds 4096 keys)."""
    q, rows, allow, qm, packed, handles = big
    index = handles[0]
    lay = layouts(5000)
    ones = np.ones(q.shape, np.float32)
    for k in (10, 4096):
        plain = index.search(q, k)
        masked = index.search_weighted(q, ones, k, packed, qm)
        for name, per_group in (("negative", 1), ("distinct", 1), ("uniform", k), ("one", k)):
            _exact(index.search_collapsed(q, k, lay[name], per_group), plain)
            _exact(index.search_collapsed(q, k, lay[name], per_group, ones), plain)
            _exact(_device(index, q, k, lay[name], per_group)[:2], plain)
            _exact(index.search_collapsed(q, k, lay[name], per_group, None, packed, qm), masked)
    _, _, _, wq, ww, _ = weighted_case()
    wi = _idx(*weighted_case()[:3], 5000)
    _exact(wi.search_collapsed(wq, 10, lay["distinct"], 1, ww), wi.search_weighted(wq, ww, 10))
    # ... and the collapsed prefix of search's order where a layout does collapse
    full = index.search(q, 5000)
    k, g = 10, lay["uniform"]
    got = index.search_collapsed(q, k, g, 1)
    for r in range(len(q)):
        seen, keep = set(), []
        for j, d in enumerate(full[0][r]):
            if g[d] in seen:
                continue
            seen.add(g[d])
            keep.append(j)
            if len(keep) == k:
                break
        _exact((got[0][r:r + 1], got[1][r:r + 1]),
               (full[0][r:r + 1, keep], full[1][r:r + 1, keep]))
    wi.close()


def test_results_do_not_depend_on_the_options(big):
    q, rows, allow, qm, packed, handles = big
    index = handles[0]
    lay = layouts(5000)
    try:
        for name, per_group in (("uniform", 1), ("dominated", 1), ("dominated", 2), ("tenant", 1)):
            want = ref_collapsed(rows, 10, lay[name], per_group, allow, qm, 0, True)
            for page in (1, 7, 64, 0):
                for chunk in (1, 0):
                    index.set_option("collapse_page", page)
                    index.set_option("collapse_chunk", chunk)
                    _check(index, q, 10, lay[name], per_group, want, None, packed, qm,
                           what=(name, per_group, page, chunk))
    finally:
        index.set_option("collapse_page", 0)
        index.set_option("collapse_chunk", 0)
    assert index.get_option("collapse_page") == 0 and index.get_option("collapse_chunk") == 0


# ----------------------------------------------------------- 4. the rounds
def _model_stats(rows, k, groups, per_group, page, allow=None, qm=None):
    st = {}
    paged_collapsed(rows, k, groups, per_group, page, allow, qm, stats=st)
    return st


def test_round_accounting(big):
    """collapse_stats against the numpy restatement of the loop: one round for
    the uniform layout at the automatic page; a dominated row goes on under
    exclusion masks; a mask that leaves one group ends in two rounds where the
    cursor alone would need 79 pages of 64."""
    q, rows, allow, qm, packed, handles = big
    index = handles[0]
    lay = layouts(5000)
    k = 10
    before = index.search(q, k)
    usual = index.last_dispatch()
    assert not usual["collapsed"]
    try:
        index.search_collapsed(q, k, lay["uniform"], 1)
        st = index.collapse_stats()
        assert st == _model_stats(rows, k, lay["uniform"], 1, 2 * k)
        assert st["rounds"] == 1 and st["unfinished_rows"] == 0 and st["excluded_rows"] == 0
        assert index.last_dispatch()["collapsed"]
        assert {"after", "filtered"} <= index.last_dispatch()["kernels"]
        index.set_option("collapse_page", PAGE)
        for chunk in (0, 1):
            index.set_option("collapse_chunk", chunk)
            index.search_collapsed(q, k, lay["dominated"], 1)
            st = index.collapse_stats()
            assert st == _model_stats(rows, k, lay["dominated"], 1, PAGE), chunk
            assert st["rounds"] > 1 and st["excluded_rows"] > 0 and st["dropped_entries"] > 0
            one = (lay["tenant"] == 3)[None, :]
            got = index.search_collapsed(q, k, lay["tenant"], 1, None, _pack(one))
            assert (got[0][:, 0] >= 0).all() and (got[0][:, 1:] == -1).all()
            st = index.collapse_stats()
            assert st["rounds"] == 2, chunk
            assert st == _model_stats(rows, k, lay["tenant"], 1, PAGE, one)
        assert index.last_dispatch()["collapsed"]
    finally:
        index.set_option("collapse_page", 0)
        index.set_option("collapse_chunk", 0)
    # the handle afterwards: a plain search clears the flag and is what it was
    _exact(index.search(q, k), before)
    now = index.last_dispatch()
    assert not now["collapsed"]
    for d in (now, usual):   # (a flag of the handle's threshold history, not of this search)
        d["kernels"] = d["kernels"] - {"bound_off"}
    assert now == usual


# ------------------------------------------------------------- 5. the C-ABI
def test_c_call_rejects_and_leaves_outputs(big):
    from bm25mi._capi import BM25_EINVAL, BM25_OK, lib
    q, rows, allow, qm, packed, handles = big
    index = handles[0]
    g = np.ascontiguousarray(layouts(5000)["uniform"])
    qq = np.ascontiguousarray(q)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    Q, T = qq.shape

    def call(k, groups, per_group, queries=qq, weights=None):
        docs = np.full((Q, max(k, 1)), 7, np.int32)
        scores = np.full((Q, max(k, 1)), 7.0, np.float32)
        og = np.full((Q, max(k, 1)), 7, np.int32)
        rc = lib.bm25_search_collapsed(index._h, p(queries), None if weights is None else p(weights),
                                       Q, T, k, None, 0, None, None if groups is None else p(groups),
                                       per_group, p(docs), p(scores), p(og))
        assert (docs == 7).all() and (scores == 7.0).all() and (og == 7).all()
        return rc, lib.bm25_last_error()

    rc, msg = call(4097, g, 1)
    assert rc == BM25_EINVAL and b"k=4097" in msg and b"4096" in msg and b"LDS" in msg
    rc, msg = call(10, g, 0)
    assert rc == BM25_EINVAL and b"per_group=0" in msg
    rc, msg = call(10, None, 1)
    assert rc == BM25_EINVAL and b"NULL groups" in msg
    bad = qq.copy()
    bad[0, 0] = 40
    rc, msg = call(10, g, 1, bad)
    assert rc == BM25_EINVAL and b"maximum token ID" in msg
    w = np.ones(qq.shape, np.float32)
    w[0, 0] = np.inf
    rc, msg = call(10, g, 1, qq, w)
    assert rc == BM25_EINVAL and b"not finite" in msg
    assert call(0, g, 1)[0] == BM25_OK   # k == 0: no device work, nothing written
    out = (ctypes.c_int64 * 4)()
    assert lib.bm25_search_collapsed_stats(index._h, out, 5) == BM25_EINVAL
    assert lib.bm25_search_collapsed_stats(index._h, out, 1) == BM25_OK


# ------------------------------------------------------ 6. many rows at once
def test_unfinished_rows_scattered_over_a_wide_batch(gpu):
    """2100 rows (past the compaction kernel's 1024 rows a step, and no
    multiple of its waves): every third row sees five documents only and ends
    in round 1, the others are dominated and go on under exclusion masks, in
    sub-batches of 1000, 1 and the automatic size."""
    ip, ix, dt, q, rows = after_case(2049)
    index = _idx(ip, ix, dt, 2049)
    g = layouts(2049)["dominated"]
    allow = np.ones((2, 2049), bool)
    allow[1] = False
    allow[1, [3, 700, 2047, 2048, 9]] = True
    reps = 300
    Q = reps * len(q)
    qq = np.tile(q, (reps, 1))
    qm = (np.arange(Q) % 3 == 0).astype(np.int32)
    k = 10
    # the reference once per (row, mask), spread over the batch
    per = [ref_collapsed(rows, k, g, 1, allow, np.full(len(q), m, np.int32), 0, True)
           for m in (0, 1)]
    want = tuple(np.stack([per[qm[i]][j][i % len(q)] for i in range(Q)]) for j in range(3))
    try:
        index.set_option("collapse_page", PAGE)
        for chunk in (1000, 0):
            index.set_option("collapse_chunk", chunk)
            _check(index, qq, k, g, 1, want, None, _pack(allow), qm, what=chunk)
            st = index.collapse_stats()
            assert st["unfinished_rows"] == int((qm == 0).sum()) and st["rounds"] == 2, st
            assert st["excluded_rows"] == st["unfinished_rows"]
    finally:
        index.set_option("collapse_page", 0)
        index.set_option("collapse_chunk", 0)
    index.close()


# ------------------------------------------------------------ 7. the drop-in
def test_bm25v_search_collapsed_with_facet_codes(gpu):
    """BM25v.search_collapsed over groups made by bm25mi.facet_codes of string
    labels (None: no group), with and without an allow mask."""
    import bm25_native
    import bm25mi
    import scipy.sparse as sp
    ip, ix, dt, q, rows = after_case(2049)
    labels = np.array([None if d % 7 == 0 else f"site{d % 40}" for d in range(2049)], object)
    codes, uniq = bm25mi.facet_codes(labels)
    assert (codes[::7] == -1).all() and len(uniq) == 40
    model = bm25_native.BM25v()
    model.index(sp.csc_matrix((dt, ix, ip), shape=(2049, len(ip) - 1)), np.ones(2049, np.float32))
    _exact(model.search_collapsed(q, 10, codes), ref_collapsed(rows, 10, codes, 1))
    allow = np.arange(2049) % 3 != 0
    _exact(model.search_collapsed(q, 10, codes, 2, allow=allow),
           ref_collapsed(rows, 10, codes, 2, allow[None, :]))
    with pytest.raises(ValueError, match=r"2049 \(n_docs\) entries"):
        model.search_collapsed(q, 10, codes[:100])
