"""CPU tests of the argument rules the ranked searches share
(bm25_search_filtered, _weighted, _after, _collapsed and their _device forms).

The C side: a stand-alone program (tests/asan/ranked_check.cpp) drives the
shared shape and content checks of csrc/bm25mi_host.h under AddressSanitizer
and UBSan on exactly sized heap arrays, with the rule set of each of the four
calls and no device.  (The entry points' use of them is checked against a
handle in tests/test_gpu_ranked_args.py.)

The Python side: one table holds, for each of the ten GpuIndex methods of the
family, every ValueError its wrapper raises before any C call, with the whole
message as a literal, and pairs of mistakes whose order is part of the
behaviour.  A well-formed call reaches the C call, which rejects the missing
handle."""
import os
import subprocess
import types

import numpy as np
import pytest

from test_search_after_host import _bare_index

N = 70   # n_docs of the bare index: W = 3 mask words per row


def test_c_rules_under_sanitizers():
    from bm25mi.build import build_host_program
    exe = build_host_program("ranked_check")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "ranked_check ok" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------- the Python layers
def _host():
    f32, i32 = np.float32, np.int32
    return types.SimpleNamespace(
        q=np.zeros((2, 3), i32), q1=np.zeros(3, i32), w=np.ones((2, 3), f32),
        w4=np.ones((2, 4), f32), bm=np.ones((2, N), bool), bm69=np.ones((2, N - 1), bool),
        fm=np.ones((2, N), f32), pm2=np.zeros((2, 2), np.uint32), pm0=np.zeros((0, 3), np.uint32),
        qm=np.array([0, 1], i32), qm3=np.zeros(3, i32), qm_hi=np.array([0, 2], i32),
        qm_lo=np.array([-2, 0], i32), none=np.array([-1, -1], i32),
        s=np.zeros(2, f32), d=np.zeros(2, i32), g=np.zeros(N, i32),
        nan=np.array([0, np.nan], f32), d_none=np.array([-2, -1], i32),
        docs=np.zeros((2, 4), i32), docs3=np.zeros((3, 4), i32))


def _dev():
    import torch
    f32, i32 = torch.float32, torch.int32
    return types.SimpleNamespace(
        q=torch.zeros((2, 3), dtype=i32), w=torch.ones((2, 3), dtype=f32),
        wi=torch.ones((2, 3), dtype=i32), m=torch.zeros((2, 3), dtype=i32),
        m64=torch.zeros((2, 3), dtype=torch.int64), m0=torch.zeros((0, 3), dtype=i32),
        qm=torch.zeros(2, dtype=i32), qm3=torch.zeros(3, dtype=i32),
        a_s=torch.zeros(2, dtype=f32), a_d=torch.zeros(2, dtype=i32),
        d=torch.zeros((2, 4), dtype=i32), s=torch.zeros((2, 4), dtype=f32),
        g=torch.zeros(N, dtype=i32), gf=torch.zeros(N, dtype=f32),
        og=torch.zeros((2, 4), dtype=i32), c=torch.zeros((2, 4), dtype=i32),
        c3=torch.zeros((3, 4), dtype=i32))


QUERIES = "queries must be a 2-D [Q, T] int32 array"
WEIGHTS = "weights must be a float32 array of the queries' shape (2, 3), got shape (2, 4)"
BOOL_MASK = "a bool mask must have 70 (n_docs) columns, got shape (2, 69)"
MASK_DTYPE = "masks must be bool [M, n_docs] or packed uint32 [M, W] (bm25mi.pack_mask)"
PACKED = "packed masks must have 3 (ceil(n_docs / 32)) words per row, got shape (2, 2)"
QM_SHAPE = "query_mask must hold one mask id per query (2), got shape (3,)"
QM_RANGE2 = "query_mask entries must be in [-1, 2)"
QM_RANGE0 = "query_mask entries must be in [-1, 0)"
NO_MASKS = "no masks given: query_mask must be -1 for every query"
AFTER_PAIR = "after must be None or a pair (scores [Q], docs [Q])"
AFTER_HALVES = "after needs both halves: (scores [Q], docs [Q])"
AFTER_DTYPE = "after must be (float32 scores, int32 docs): page_cursor's pair"
AFTER_SHAPE = "after must hold one cursor per query (2), got shapes (1,) and (2,)"
AFTER_DOCS = "after docs must be >= AFTER_NONE (-2)"
AFTER_NAN = "after scores must not be NaN where after docs name a document"
GROUPS_F = "groups must be an integer array of 70 (n_docs) entries, got float32 of shape (70,)"
GROUPS_N = "groups must be an integer array of 70 (n_docs) entries, got int32 of shape (69,)"
GROUPS_FIT = "groups must fit int32"
K_LDS = "k=4097: a collapsed search is limited to k <= 4096 (the per-row group table lives in LDS)"
PER_GROUP = "per_group=0 must be >= 1"
D_QUERIES = "d_queries must be a 2-D [Q, T] tensor"
D_WEIGHTS = "d_weights must be a float32 [2, 3] tensor"
D_MASKS = "d_masks must be a packed [M, 3] tensor of 32-bit words"
D_QM = "d_query_mask must hold one mask id per query (2)"
D_NO_MASKS = "no masks given: d_query_mask must be -1 for every query"
D_OUT = "d_docs and d_scores must hold 2 x 4 results"
D_AFTER_PAIR = "d_after must be None or a pair (scores [Q], docs [Q])"
D_AFTER_HALVES = "d_after needs both halves: (scores [Q], docs [Q])"
D_AFTER = "d_after must be contiguous (float32 [2], int32 [2]) tensors"
D_GROUPS = "d_groups must be a contiguous int32 [70] (n_docs) tensor"
D_GROUPS_OUT = "d_groups_out must hold 2 x 4 int32 groups"
NULL = "NULL index"   # the C call's own: the wrapper let the arguments through

# (method, message, the call on the bare index g with the arrays a).  Many calls
# make a second mistake further down the wrapper's order, which must lose.
HOST_CASES = [
    ("search_filtered", QUERIES, lambda g, a: g.search_filtered(a.q1, 1, a.bm69, a.qm3)),
    ("search_filtered", BOOL_MASK, lambda g, a: g.search_filtered(a.q, 1, a.bm69, a.qm3)),
    ("search_filtered", MASK_DTYPE, lambda g, a: g.search_filtered(a.q, 1, a.fm)),
    ("search_filtered", PACKED, lambda g, a: g.search_filtered(a.q, 1, a.pm2)),
    ("search_filtered", QM_SHAPE, lambda g, a: g.search_filtered(a.q, 1, a.bm, a.qm3)),
    ("search_filtered", QM_RANGE2, lambda g, a: g.search_filtered(a.q, 1, a.bm, a.qm_hi)),
    ("search_filtered", QM_RANGE2, lambda g, a: g.search_filtered(a.q, 1, a.bm, a.qm_lo)),
    ("search_filtered", QM_RANGE0, lambda g, a: g.search_filtered(a.q, 1, a.pm0, a.qm)),
    ("search_filtered", NO_MASKS, lambda g, a: g.search_filtered(a.q, 1, a.pm0)),
    ("search_filtered", NULL, lambda g, a: g.search_filtered(a.q, 1, a.pm0, a.none)),
    ("search_filtered", NULL, lambda g, a: g.search_filtered(a.q[:0], 1, a.pm0)),
    ("search_filtered", NULL, lambda g, a: g.search_filtered(a.q, -1, a.bm, a.qm)),
    ("search_weighted", QUERIES, lambda g, a: g.search_weighted(a.q1, a.w4, 1)),
    ("search_weighted", WEIGHTS, lambda g, a: g.search_weighted(a.q, a.w4, 1, a.bm69)),
    ("search_weighted", BOOL_MASK, lambda g, a: g.search_weighted(a.q, a.w, 1, a.bm69, a.qm3)),
    ("search_weighted", PACKED, lambda g, a: g.search_weighted(a.q, a.w, 1, a.pm2)),
    ("search_weighted", QM_SHAPE, lambda g, a: g.search_weighted(a.q, a.w, 1, a.bm, a.qm3)),
    ("search_weighted", QM_RANGE2, lambda g, a: g.search_weighted(a.q, a.w, 1, a.bm, a.qm_hi)),
    ("search_weighted", QM_RANGE0, lambda g, a: g.search_weighted(a.q, a.w, 1, None, a.qm)),
    ("search_weighted", NULL, lambda g, a: g.search_weighted(a.q, a.w, 1)),
    ("search_weighted", NULL, lambda g, a: g.search_weighted(a.q, a.w, 1, a.pm0)),
    ("search_weighted", NULL, lambda g, a: g.search_weighted(a.q, a.w, 1, a.bm, a.qm)),
    ("search_after", QUERIES, lambda g, a: g.search_after(a.q1, 1, a.s, a.w4)),
    ("search_after", WEIGHTS, lambda g, a: g.search_after(a.q, 1, a.s, a.w4, a.bm69)),
    ("search_after", BOOL_MASK, lambda g, a: g.search_after(a.q, 1, a.s, a.w, a.bm69, a.qm3)),
    ("search_after", QM_SHAPE, lambda g, a: g.search_after(a.q, 1, a.s, None, a.bm, a.qm3)),
    ("search_after", QM_RANGE2, lambda g, a: g.search_after(a.q, 1, a.s, None, a.bm, a.qm_hi)),
    ("search_after", QM_RANGE0, lambda g, a: g.search_after(a.q, 1, a.s, None, None, a.qm)),
    ("search_after", AFTER_PAIR, lambda g, a: g.search_after(a.q, 1, a.s)),
    ("search_after", AFTER_PAIR, lambda g, a: g.search_after(a.q, 1, (a.s, a.d, a.d))),
    ("search_after", AFTER_HALVES, lambda g, a: g.search_after(a.q, 1, (a.s, None))),
    ("search_after", AFTER_HALVES, lambda g, a: g.search_after(a.q, 1, (None, a.d))),
    ("search_after", AFTER_DTYPE, lambda g, a: g.search_after(a.q, 1, (a.d, a.s))),
    ("search_after", AFTER_DTYPE, lambda g, a: g.search_after(a.q, 1, (a.s.astype("f8"), a.d[:1]))),
    ("search_after", AFTER_SHAPE, lambda g, a: g.search_after(a.q, 1, (a.s[:1], a.d_none - 2))),
    ("search_after", AFTER_DOCS, lambda g, a: g.search_after(a.q, 1, (a.nan, a.d_none - 1))),
    ("search_after", AFTER_NAN, lambda g, a: g.search_after(a.q, 1, (a.nan, a.d))),
    ("search_after", NULL, lambda g, a: g.search_after(a.q, 1, (a.nan, a.d_none))),
    ("search_after", NULL, lambda g, a: g.search_after(a.q, 1)),
    ("search_after", NULL, lambda g, a: g.search_after(a.q, 1, (a.s, a.d), a.w, a.bm, a.qm)),
    ("search_collapsed", QUERIES, lambda g, a: g.search_collapsed(a.q1, 1, a.g[:69], 0, a.w4)),
    ("search_collapsed", WEIGHTS, lambda g, a: g.search_collapsed(a.q, 1, a.g, 1, a.w4, a.bm69)),
    ("search_collapsed", BOOL_MASK,
     lambda g, a: g.search_collapsed(a.q, 1, a.g, 1, None, a.bm69, a.qm3)),
    ("search_collapsed", QM_SHAPE,
     lambda g, a: g.search_collapsed(a.q, 1, a.g[:69], 1, None, a.bm, a.qm3)),
    ("search_collapsed", QM_RANGE2,
     lambda g, a: g.search_collapsed(a.q, 1, a.g[:69], 1, None, a.bm, a.qm_hi)),
    ("search_collapsed", QM_RANGE0,
     lambda g, a: g.search_collapsed(a.q, 1, a.g, 1, None, None, a.qm)),
    ("search_collapsed", GROUPS_F, lambda g, a: g.search_collapsed(a.q, 4097, a.g.astype("f4"), 0)),
    ("search_collapsed", GROUPS_N, lambda g, a: g.search_collapsed(a.q, 4097, a.g[:69], 0)),
    ("search_collapsed", GROUPS_FIT,
     lambda g, a: g.search_collapsed(a.q, 4097, a.g.astype("i8") + 2**31, 0)),
    ("search_collapsed", K_LDS, lambda g, a: g.search_collapsed(a.q, 4097, a.g, 0)),
    ("search_collapsed", PER_GROUP, lambda g, a: g.search_collapsed(a.q, 4096, a.g, 0)),
    ("search_collapsed", NULL, lambda g, a: g.search_collapsed(a.q, 1, a.g)),
    ("search_collapsed", NULL,
     lambda g, a: g.search_collapsed(a.q, 1, a.g.astype("i8"), 2, a.w, a.bm, a.qm, True)),
    ("score_docs_weighted", QUERIES, lambda g, a: g.score_docs_weighted(a.q1, a.w4, a.docs3)),
    ("score_docs_weighted", WEIGHTS, lambda g, a: g.score_docs_weighted(a.q, a.w4, a.docs3[0])),
    ("score_docs_weighted", "docs must be a 2-D [Q, C] int32 array",
     lambda g, a: g.score_docs_weighted(a.q, a.w, a.docs3[0])),
    ("score_docs_weighted", "queries has 2 rows, docs has 3",
     lambda g, a: g.score_docs_weighted(a.q, a.w, a.docs3)),
    ("score_docs_weighted", NULL, lambda g, a: g.score_docs_weighted(a.q, a.w, a.docs)),
]

DEVICE_CASES = [
    ("search_filtered_device", D_QUERIES,
     lambda g, t: g.search_filtered_device(t.q[0], 4, t.m[:, :2], t.qm, t.d, t.s)),
    ("search_filtered_device", D_MASKS,
     lambda g, t: g.search_filtered_device(t.q, 4, t.m[:, :2], t.qm3, t.d, t.s)),
    ("search_filtered_device", D_MASKS,
     lambda g, t: g.search_filtered_device(t.q, 4, t.m64, t.qm, t.d, t.s)),
    ("search_filtered_device", D_MASKS,
     lambda g, t: g.search_filtered_device(t.q, 4, t.m[0], t.qm, t.d, t.s)),
    ("search_filtered_device", D_QM,
     lambda g, t: g.search_filtered_device(t.q, 4, t.m, t.qm3, t.d[:, :3], t.s)),
    ("search_filtered_device", D_NO_MASKS,
     lambda g, t: g.search_filtered_device(t.q, 4, t.m0, None, t.d[:, :3], t.s)),
    ("search_filtered_device", D_OUT,
     lambda g, t: g.search_filtered_device(t.q, 4, t.m, t.qm, t.d[:, :3], t.s)),
    ("search_filtered_device", D_OUT,
     lambda g, t: g.search_filtered_device(t.q, 4, t.m, None, t.d, t.s[:1])),
    ("search_filtered_device", NULL,
     lambda g, t: g.search_filtered_device(t.q, 4, t.m, None, t.d, t.s)),
    ("search_filtered_device", NULL,
     lambda g, t: g.search_filtered_device(t.q, 4, t.m0, t.qm, t.d, t.s)),
    ("search_filtered_device", NULL,
     lambda g, t: g.search_filtered_device(t.q[:0], 4, t.m0, None, t.d[:0], t.s[:0])),
    ("search_weighted_device", D_QUERIES,
     lambda g, t: g.search_weighted_device(t.q[0], t.wi, 4, t.m, t.qm, t.d, t.s)),
    ("search_weighted_device", D_WEIGHTS,
     lambda g, t: g.search_weighted_device(t.q, t.w[:, :2], 4, t.m[:, :2], t.qm, t.d, t.s)),
    ("search_weighted_device", D_WEIGHTS,
     lambda g, t: g.search_weighted_device(t.q, t.wi, 4, t.m, t.qm, t.d, t.s)),
    ("search_weighted_device", D_MASKS,
     lambda g, t: g.search_weighted_device(t.q, t.w, 4, t.m[:, :2], t.qm3, t.d, t.s)),
    ("search_weighted_device", D_QM,
     lambda g, t: g.search_weighted_device(t.q, t.w, 4, None, t.qm3, t.d[:, :3], t.s)),
    ("search_weighted_device", D_OUT,
     lambda g, t: g.search_weighted_device(t.q, t.w, 4, t.m, t.qm, t.d, t.s[:, :3])),
    ("search_weighted_device", NULL,
     lambda g, t: g.search_weighted_device(t.q, t.w, 4, None, None, t.d, t.s)),
    ("search_weighted_device", NULL,
     lambda g, t: g.search_weighted_device(t.q, t.w, 4, t.m0, None, t.d, t.s)),
    ("search_after_device", D_QUERIES,
     lambda g, t: g.search_after_device(t.q[0], 4, t.a_s, t.wi, t.m, t.qm, t.d, t.s)),
    ("search_after_device", D_WEIGHTS,
     lambda g, t: g.search_after_device(t.q, 4, t.a_s, t.wi, t.m[:, :2], t.qm, t.d, t.s)),
    ("search_after_device", D_MASKS,
     lambda g, t: g.search_after_device(t.q, 4, t.a_s, t.w, t.m[:, :2], t.qm3, t.d, t.s)),
    ("search_after_device", D_QM,
     lambda g, t: g.search_after_device(t.q, 4, t.a_s, None, t.m, t.qm3, t.d, t.s)),
    ("search_after_device", D_AFTER_PAIR,
     lambda g, t: g.search_after_device(t.q, 4, t.a_s, None, None, None, t.d[:, :3], t.s)),
    ("search_after_device", D_AFTER_HALVES,
     lambda g, t: g.search_after_device(t.q, 4, (t.a_s, None), None, None, None, t.d, t.s)),
    ("search_after_device", D_AFTER_HALVES,
     lambda g, t: g.search_after_device(t.q, 4, [None, t.a_d], None, None, None, t.d, t.s)),
    ("search_after_device", D_AFTER,
     lambda g, t: g.search_after_device(t.q, 4, (t.a_s[:1], t.a_d), None, None, None, t.d, t.s)),
    ("search_after_device", D_AFTER,
     lambda g, t: g.search_after_device(t.q, 4, (t.a_d, t.a_s), None, None, None, t.d, t.s)),
    ("search_after_device", D_AFTER,
     lambda g, t: g.search_after_device(t.q, 4, (t.s[:, 0], t.a_d), None, None, None, t.d, t.s)),
    ("search_after_device", D_OUT,
     lambda g, t: g.search_after_device(t.q, 4, (t.a_s, t.a_d), None, None, None, t.d[:, :3], t.s)),
    ("search_after_device", NULL,
     lambda g, t: g.search_after_device(t.q, 4, None, None, None, None, t.d, t.s)),
    ("search_after_device", NULL,
     lambda g, t: g.search_after_device(t.q, 4, (t.a_s, t.a_d), t.w, t.m, t.qm, t.d, t.s)),
    ("search_collapsed_device", D_QUERIES,
     lambda g, t: g.search_collapsed_device(t.q[0], 4, t.gf, 0, t.wi, t.m, t.qm, t.d, t.s)),
    ("search_collapsed_device", D_WEIGHTS,
     lambda g, t: g.search_collapsed_device(t.q, 4, t.g, 1, t.wi, t.m[:, :2], t.qm, t.d, t.s)),
    ("search_collapsed_device", D_MASKS,
     lambda g, t: g.search_collapsed_device(t.q, 4, t.g, 1, None, t.m[:, :2], t.qm3, t.d, t.s)),
    ("search_collapsed_device", D_QM,
     lambda g, t: g.search_collapsed_device(t.q, 4, t.gf, 1, None, None, t.qm3, t.d, t.s)),
    ("search_collapsed_device", D_GROUPS,
     lambda g, t: g.search_collapsed_device(t.q, 4097, t.gf, 0, None, None, None, t.d, t.s)),
    ("search_collapsed_device", D_GROUPS,
     lambda g, t: g.search_collapsed_device(t.q, 4, t.g[:69], 1, None, None, None, t.d, t.s)),
    ("search_collapsed_device", K_LDS,
     lambda g, t: g.search_collapsed_device(t.q, 4097, t.g, 0, None, None, None, t.d, t.s)),
    ("search_collapsed_device", PER_GROUP,
     lambda g, t: g.search_collapsed_device(t.q, 4, t.g, 0, None, None, None, t.d[:, :3], t.s)),
    ("search_collapsed_device", D_OUT,
     lambda g, t: g.search_collapsed_device(t.q, 4, t.g, 1, None, None, None, t.d[:, :3], t.s,
                                            t.og[:1])),
    ("search_collapsed_device", D_GROUPS_OUT,
     lambda g, t: g.search_collapsed_device(t.q, 4, t.g, 1, None, None, None, t.d, t.s, t.og[:1])),
    ("search_collapsed_device", NULL,
     lambda g, t: g.search_collapsed_device(t.q, 4, t.g, 1, None, None, None, t.d, t.s)),
    ("search_collapsed_device", NULL,
     lambda g, t: g.search_collapsed_device(t.q, 4, t.g, 2, t.w, t.m, t.qm, t.d, t.s, t.og)),
    ("score_docs_weighted_device", "d_queries and d_docs must be 2-D [Q, T] and [Q, C] tensors",
     lambda g, t: g.score_docs_weighted_device(t.q, t.wi, t.c[0], t.s)),
    ("score_docs_weighted_device", D_WEIGHTS,
     lambda g, t: g.score_docs_weighted_device(t.q, t.wi, t.c3, t.s)),
    ("score_docs_weighted_device", "d_queries has 2 rows, d_docs has 3",
     lambda g, t: g.score_docs_weighted_device(t.q, t.w, t.c3, t.s)),
    ("score_docs_weighted_device", "d_scores must hold 2 x 4 scores",
     lambda g, t: g.score_docs_weighted_device(t.q, t.w, t.c, t.s[:1])),
    ("score_docs_weighted_device", NULL,
     lambda g, t: g.score_docs_weighted_device(t.q, t.w, t.c, t.s)),
]

_ids = lambda cases: [f"{m}-{i}" for i, (m, _, _) in enumerate(cases)]


@pytest.mark.parametrize("method,message,call", HOST_CASES, ids=_ids(HOST_CASES))
def test_host_wrapper_messages(method, message, call):
    with pytest.raises(ValueError) as e:
        call(_bare_index(N), _host())
    assert str(e.value) == message


@pytest.mark.parametrize("method,message,call", DEVICE_CASES, ids=_ids(DEVICE_CASES))
def test_device_wrapper_messages(method, message, call):
    with pytest.raises(ValueError) as e:
        call(_bare_index(N), _dev())
    assert str(e.value) == message


def test_tables_name_all_ten_methods():
    host = {m for m, _, _ in HOST_CASES}
    dev = {m for m, _, _ in DEVICE_CASES}
    assert len(host) == 5 and dev == {m + "_device" for m in host}


def test_filtered_device_needs_a_mask_tensor():
    """search_filtered_device takes no None for d_masks: it asks the tensor
    for its rank first."""
    t = _dev()
    with pytest.raises(AttributeError):
        _bare_index(N).search_filtered_device(t.q, 4, None, None, t.d, t.s)
