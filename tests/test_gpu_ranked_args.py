"""The argument rules of the ranked searches against a handle: the four host
entry points (bm25_search_filtered, _weighted, _after, _collapsed) reject
every single mistake with the code and the whole text the stand-alone check
(tests/asan/ranked_check.cpp) expects of the shared rules — so each entry
point reaches them with its own rule set — the four _device entry points keep
their own, looser rules, and a valid call of each of the eight returns the
bits of the Python method.  No call here passes a NULL pointer to
bm25_search_filtered_device, which checks none."""
import ctypes

import numpy as np
import pytest

from test_gpu_parity import _exact, _idx

pytestmark = pytest.mark.gpu

N_DOCS, N_TERMS, Q, T, K, M = 40, 6, 3, 2, 2, 2
W = (N_DOCS + 31) // 32
CALLS = ("filtered", "weighted", "after", "collapsed")

NEG_K = b"negative dimensions are not allowed (top_k=-1)"
BIG_K = b"kth(=-1) out of bounds (40)"
NEG_SHAPE = b"negative query or mask shape"
TOKEN = b"The maximum token ID in the query (6) is higher than the number of tokens in the index."
NO_MASKS = b"no masks: query_mask must name -1 (no filter) for every query"
ONE_SIDED = b"after_scores and after_docs must both be given or both be NULL"
AFTER_DOCS = (b"after_docs[1] = -3 is below BM25_AFTER_NONE (-2): a cursor names a doc id >= 0, -1 "
              b"(exhausted) or BM25_AFTER_NONE")
AFTER_NAN = b"after_scores[2] = nan is not a score (the cursor of doc 5)"
GROUPS = b"NULL groups (one int32 per document; < 0: no group)"
LDS = b"k=4097: a collapsed search is limited to k <= 4096 (the per-row group table lives in LDS)"
PER_GROUP = b"per_group=0 must be >= 1"
OK = (0, None)


def E(text):
    return (1, text)   # BM25_EINVAL


@pytest.fixture(scope="module")
def index(gpu):
    """40 documents, 6 terms of 10 postings each, quarter-step values (ties)."""
    rng = np.random.default_rng(7)
    ix = np.concatenate([np.sort(rng.choice(N_DOCS, 10, replace=False)) for _ in range(N_TERMS)])
    dt = (rng.integers(1, 9, ix.size) / 4).astype(np.float32)
    g = _idx(np.arange(0, 61, 10, dtype=np.int64), ix.astype(np.int32), dt, N_DOCS)
    yield g
    g.close()


def _args(**over):
    """The valid arguments of every call of the family; ``over`` replaces some
    (None: a NULL pointer)."""
    rng = np.random.default_rng(11)
    a = dict(queries=np.array([[0, 5], [3, -1], [2, 4]], np.int32),
             weights=np.array([[1, 2], [0.5, 9], [-1, 0.25]], np.float32),
             Q=Q, T=T, k=K, M=M,
             masks=np.packbits(rng.random((M, W * 32)) < 0.7, axis=1,
                               bitorder="little").view(np.uint32),
             query_mask=np.array([0, 1, -1], np.int32),
             after_scores=np.array([1.5, 0, 0], np.float32),
             after_docs=np.array([7, -1, -2], np.int32),
             groups=(np.arange(N_DOCS) % 3).astype(np.int32), per_group=1,
             docs=np.full((Q, K), 7, np.int32), scores=np.full((Q, K), 7.0, np.float32),
             og=np.full((Q, K), 7, np.int32))
    a["masks"][:, W - 1] &= np.uint32((1 << (N_DOCS - 32 * (W - 1))) - 1)   # no bit past n_docs
    a.update(over)
    return a


def _changed(name, at, v):
    a = _args()[name]
    a[at] = v
    return a


def _host_call(h, call, a):
    from bm25mi._capi import lib
    p = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)
    shape = (a["Q"], a["T"], a["k"], p(a["masks"]), a["M"], p(a["query_mask"]))
    out = (p(a["docs"]), p(a["scores"]))
    if call == "filtered":
        rc = lib.bm25_search_filtered(h, p(a["queries"]), *shape, *out)
    elif call == "weighted":
        rc = lib.bm25_search_weighted(h, p(a["queries"]), p(a["weights"]), *shape, *out)
    elif call == "after":
        rc = lib.bm25_search_after(h, p(a["queries"]), p(a["weights"]), *shape,
                                   p(a["after_scores"]), p(a["after_docs"]), *out)
    else:
        rc = lib.bm25_search_collapsed(h, p(a["queries"]), p(a["weights"]), *shape, p(a["groups"]),
                                       a["per_group"], *out, p(a["og"]))
    return rc, (lib.bm25_last_error() if rc else None)


NAN, INF = np.float32("nan"), np.float32("inf")
# (what, the calls it goes to, the changed arguments, the result)
HOST_CASES = [
    ("valid", CALLS, {}, OK),
    ("k = 0, every pointer NULL", CALLS,
     dict(k=0, queries=None, weights=None, masks=None, query_mask=None, after_scores=None,
          after_docs=None, groups=None, docs=None, scores=None, og=None), OK),
    ("Q = 0, every pointer NULL", CALLS,
     dict(Q=0, queries=None, weights=None, masks=None, query_mask=None, after_scores=None,
          after_docs=None, groups=None, docs=None, scores=None, og=None), OK),
    ("k = -1", CALLS, dict(k=-1), E(NEG_K)),
    ("k = 41", CALLS, dict(k=41), E(BIG_K)),
    ("M = -1", CALLS, dict(M=-1), E(NEG_SHAPE)),
    ("NULL queries", CALLS, dict(queries=None), E(b"NULL queries")),
    ("NULL masks", CALLS, dict(masks=None), E(b"NULL masks")),
    ("NULL docs", CALLS, dict(docs=None), E(b"NULL output")),
    ("NULL scores", CALLS, dict(scores=None), E(b"NULL output")),
    ("token id 6", CALLS, dict(queries=_changed("queries", (1, 1), 6)), E(TOKEN)),
    ("mask id -2", CALLS, dict(query_mask=_changed("query_mask", 1, -2)),
     E(b"query_mask[1] = -2 is outside [-1, 2)")),
    ("mask id M", CALLS, dict(query_mask=_changed("query_mask", 1, 2)),
     E(b"query_mask[1] = 2 is outside [-1, 2)")),
    ("T = 0, NULL queries and weights", CALLS, dict(T=0, queries=None, weights=None), OK),
    ("NULL weights", ("weighted",), dict(weights=None), E(b"NULL weights")),
    ("NULL weights", ("after", "collapsed"), dict(weights=None), OK),
    ("NaN weight", CALLS[1:], dict(weights=_changed("weights", (1, 0), NAN)),
     E(b"weights[1][0] = nan is not finite")),
    ("Inf weight", CALLS[1:], dict(weights=_changed("weights", (1, 0), INF)),
     E(b"weights[1][0] = inf is not finite")),
    ("NaN weight of a padding slot", CALLS[1:], dict(weights=_changed("weights", (1, 1), NAN)), OK),
    ("no masks, no mask ids", ("filtered",), dict(M=0, masks=None, query_mask=None), E(NO_MASKS)),
    ("no masks, no mask ids", CALLS[1:], dict(M=0, masks=None, query_mask=None), OK),
    ("cursor scores alone", ("after",), dict(after_docs=None), E(ONE_SIDED)),
    ("cursor docs alone, k = 0", ("after",), dict(after_scores=None, k=0), E(ONE_SIDED)),
    ("cursor doc -3", ("after",), dict(after_docs=_changed("after_docs", 1, -3)),
     E(AFTER_DOCS)),
    ("NaN cursor of doc 5", ("after",),
     dict(after_docs=_changed("after_docs", 2, 5),
          after_scores=_changed("after_scores", 2, NAN)), E(AFTER_NAN)),
    ("NaN cursors of no document", ("after",),
     dict(after_scores=np.array([1.5, NAN, NAN], np.float32)), OK),
    ("k = 4097", ("collapsed",), dict(k=4097), E(LDS)),
    ("per_group = 0", ("collapsed",), dict(per_group=0), E(PER_GROUP)),
    ("NULL groups", ("collapsed",), dict(groups=None), E(GROUPS)),
    # two mistakes: the first named wins
    ("k = -1 and NULL queries", CALLS, dict(k=-1, queries=None), E(NEG_K)),
    ("NULL masks and NULL output", CALLS, dict(masks=None, docs=None), E(b"NULL masks")),
    ("token id 6 and a NaN weight", CALLS[1:],
     dict(queries=_changed("queries", (1, 1), 6), weights=_changed("weights", (1, 0), NAN)),
     E(TOKEN)),
    ("a NaN weight and mask id M", CALLS[1:],
     dict(weights=_changed("weights", (1, 0), NAN), query_mask=_changed("query_mask", 0, 2)),
     E(b"weights[1][0] = nan is not finite")),
    ("mask id M and cursor doc -3", ("after",),
     dict(query_mask=_changed("query_mask", 2, 2),
          after_docs=_changed("after_docs", 0, -3)),
     E(b"query_mask[2] = 2 is outside [-1, 2)")),
]


def test_host_entry_points_apply_the_shared_rules(index):
    for what, calls, over, want in HOST_CASES:
        for call in calls:
            a = _args(**over)
            got = _host_call(index._h, call, a)
            assert got == want, (what, call, got)
            if want != OK:   # a rejected call wrote nothing
                for name, fill in (("docs", 7), ("scores", 7.0), ("og", 7)):
                    assert a[name] is None or (a[name] == fill).all(), (what, call, name)


def _python(index, call, a):
    if call == "filtered":
        return index.search_filtered(a["queries"], K, a["masks"], a["query_mask"])
    if call == "weighted":
        return index.search_weighted(a["queries"], a["weights"], K, a["masks"], a["query_mask"])
    if call == "after":
        return index.search_after(a["queries"], K, (a["after_scores"], a["after_docs"]),
                                  a["weights"], a["masks"], a["query_mask"])
    return index.search_collapsed(a["queries"], K, a["groups"], a["per_group"], a["weights"],
                                  a["masks"], a["query_mask"], return_groups=True)


def test_valid_host_calls_are_the_python_methods(index):
    for call in CALLS:
        a = _args()
        assert _host_call(index._h, call, a) == OK
        want = _python(index, call, a)
        _exact((a["docs"], a["scores"]), want[:2])
        assert (a["docs"] >= -1).all() and (a["docs"] != 7).any(), call
        if call == "collapsed":
            assert np.array_equal(a["og"], want[2])


def test_no_terms_need_no_queries_and_no_weights(index):
    """T = 0 with NULL queries and NULL weights: every score is +0.0, so a row
    is its first k allowed documents; the weighted call still runs as a
    weighted search, and both are the Python method's bits."""
    a = _args()
    allow = np.unpackbits(a["masks"].view(np.uint8), axis=1, bitorder="little")[:, :N_DOCS] > 0
    rows = [np.nonzero(allow[m] if m >= 0 else np.ones(N_DOCS, bool))[0][:K]
            for m in a["query_mask"]]
    assert all(len(r) == K for r in rows)
    none = np.zeros((Q, 0), np.int32)
    for call in ("filtered", "weighted"):
        a = _args(T=0, queries=None, weights=None)
        assert _host_call(index._h, call, a) == OK
        assert ("weighted" in index.last_dispatch()["kernels"]) == (call == "weighted")
        assert np.array_equal(a["docs"], np.array(rows, np.int32)), call
        assert (a["scores"].view(np.uint32) == 0).all(), call
        want = _python(index, call, dict(a, queries=none, weights=none.astype(np.float32)))
        _exact((a["docs"], a["scores"]), want)


# ------------------------------------------------------ the device entry points
def _device_call(h, call, a, stream=None):
    """a: torch tensors (or None: a NULL pointer) where _args has arrays."""
    from bm25mi._capi import lib
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    shape = (a["Q"], a["T"], a["k"], p(a["masks"]), a["M"], p(a["query_mask"]))
    out = (p(a["docs"]), p(a["scores"]))
    s = ctypes.c_void_p(stream.cuda_stream if stream is not None else 0)
    if call == "filtered":
        rc = lib.bm25_search_filtered_device(h, p(a["queries"]), *shape, *out, s)
    elif call == "weighted":
        rc = lib.bm25_search_weighted_device(h, p(a["queries"]), p(a["weights"]), *shape, *out, s)
    elif call == "after":
        rc = lib.bm25_search_after_device(h, p(a["queries"]), p(a["weights"]), *shape,
                                          p(a["after_scores"]), p(a["after_docs"]), *out, s)
    else:
        rc = lib.bm25_search_collapsed_device(h, p(a["queries"]), p(a["weights"]), *shape,
                                              p(a["groups"]), a["per_group"], *out, p(a["og"]), s)
    return rc, (lib.bm25_last_error() if rc else None)


def _device_args(**over):
    import torch
    a = _args()
    a["masks"] = a["masks"].view(np.int32)
    a = {n: torch.from_numpy(v).cuda() if isinstance(v, np.ndarray) else v for n, v in a.items()}
    a.update(over)
    return a


DEVICE_CASES = [
    ("k = -1", CALLS, dict(k=-1), E(NEG_K)),
    ("k = 41", CALLS, dict(k=41), E(BIG_K)),
    ("M = -1", CALLS, dict(M=-1), E(NEG_SHAPE)),
    ("Q = -1", CALLS, dict(Q=-1), E(NEG_SHAPE)),
    ("k = 0", CALLS, dict(k=0), OK),
    ("cursor scores alone", ("after",), dict(after_docs=None), E(ONE_SIDED)),
    ("cursor docs alone, k = 0", ("after",), dict(after_scores=None, k=0), E(ONE_SIDED)),
    ("NULL queries", ("weighted",), dict(queries=None), E(b"NULL queries or weights")),
    ("NULL weights", ("weighted",), dict(weights=None), E(b"NULL queries or weights")),
    ("NULL queries", ("after", "collapsed"), dict(queries=None), E(b"NULL queries")),
    ("NULL masks", CALLS[1:], dict(masks=None), E(b"NULL masks")),
    ("NULL docs", CALLS[1:], dict(docs=None), E(b"NULL output")),
    ("NULL scores", CALLS[1:], dict(scores=None), E(b"NULL output")),
    ("NULL groups", ("collapsed",), dict(groups=None), E(GROUPS)),
    ("k = 4097", ("collapsed",), dict(k=4097), E(LDS)),
    ("per_group = 0", ("collapsed",), dict(per_group=0), E(PER_GROUP)),
    ("NULL masks and NULL output", CALLS[1:], dict(masks=None, docs=None), E(b"NULL masks")),
    ("NULL groups and NULL output", ("collapsed",), dict(groups=None, scores=None), E(GROUPS)),
    ("k = 41 and NULL queries", CALLS[1:], dict(k=41, queries=None), E(BIG_K)),
]


def test_device_entry_points_keep_their_rules(index):
    import torch
    for what, calls, over, want in DEVICE_CASES:
        for call in calls:
            a = _device_args(**over)
            got = _device_call(index._h, call, a)
            assert got == want, (what, call, got)
            torch.cuda.synchronize()
            for name, fill in (("docs", 7), ("scores", 7.0), ("og", 7)):   # nothing ran
                assert a[name] is None or bool((a[name] == fill).all()), (what, call, name)


def test_valid_device_calls_are_the_python_methods(index):
    import torch
    st = torch.cuda.Stream()
    for call in CALLS:
        a = _device_args()
        torch.cuda.synchronize()   # (the uploads ran on the current stream)
        assert _device_call(index._h, call, a, st) == OK
        st.synchronize()
        want = _python(index, call, _args())
        _exact((a["docs"].cpu().numpy(), a["scores"].cpu().numpy()), want[:2])
        if call == "collapsed":
            assert np.array_equal(a["og"].cpu().numpy(), want[2])
