"""GPU tests of what one index handle keeps between calls (bm25mi_capi.cpp):
the grow-only workspace, the shared large-k / filtered arena, the host calls'
staging buffers, the "last search" dispatch and counters, the two-half
protocol's flags, the threshold source and the stream ordering of the
workspace.  The per-entry-point files drive one entry point through a fresh
handle; here one handle serves plain, large-k, filtered, dense-filtered,
weighted, boolean and two-half searches, score_docs and term_masks, of
changing Q, T and k, by host and device calls on three streams, with exact
option changes in between (the program of tests/test_handle_reuse_host.py:
every ordered pair of the nine kinds).

Every comparison is exact: docs equal and scores equal on their uint32 views,
against the expectations of tests/test_handle_reuse_host.py.  Device calls
write into buffers pre-filled with garbage, and a step's outputs are read only
after its own stream was synchronised; between device steps nothing
synchronises the device, so steps on different streams rely on the handle's
own ordering (order_ws).

bm25_search_boolean is bm25_search_filtered under device-built masks: its
dispatch carries the filtered flag like an F step's."""
import numpy as np
import pytest

from test_gpu_parity import _exact, _idx, _want_kernels
from test_handle_reuse_host import (DEFAULTS, K_MAX, N, N_BIG, SEARCH_KINDS, VARIANTS, clauses,
                                    expect, large_lists_apply, masks, pools, program, reuse_csc,
                                    rows_of, step_queries, step_query_mask, threshold_p, uses_flat)

pytestmark = pytest.mark.gpu

BAD_DOC, BAD_SCORE, BAD_WORD = 123456789, 7.5, 0x5A5A5A5A
FLAGS = {"bound_off", "count_skips", "rest_split", "bound_pool"}
WAVE = {"wave_sample", "wave_rest", "wave_all"}


@pytest.fixture(scope="module")
def dev(gpu):
    """The pools on the device (uploaded once, before any step) and four
    streams (the program's steps use the first three)."""
    import torch
    import bm25mi
    q, w = pools()
    must, any_, must_not = clauses()
    up = lambda a: torch.from_numpy(np.array(a)).cuda()
    packed = bm25mi.pack_mask(masks())
    d = {"q": up(q), "w": up(w), "masks": up(packed.view(np.int32)), "packed": packed,
         "must": up(must), "any": up(any_), "must_not": up(must_not),
         "streams": [torch.cuda.Stream() for _ in range(4)]}
    torch.cuda.synchronize()
    return d


@pytest.fixture(scope="module")
def dev_big(dev):
    """dev with the masks of the 1027-tile fixture."""
    import torch
    import bm25mi
    packed = bm25mi.pack_mask(masks(True))
    d = dict(dev, masks=torch.from_numpy(packed.view(np.int32)).cuda(), packed=packed)
    torch.cuda.synchronize()
    return d


def _open(variant, big=False):
    signed, segments = VARIANTS[variant]
    index = _idx(*reuse_csc(signed, big), N_BIG if big else N, segments=segments)
    info = index.info()
    assert info["sparse"] == (segments == "sparse") and info["n_tiles"] == (1027 if big else 147)
    assert info["tile_bounds"] == (variant == "dense")
    return index


def _step(kind, Q, T, k, i=0, form="host", stream=0, **kw):
    return dict({"i": i, "kind": kind, "Q": Q, "T": T, "k": k, "form": form, "stream": stream,
                 "opt": None}, **kw)


class Runner:
    """One handle, the options in force on it, its steps in flight."""

    def __init__(self, index, variant, dev, steps=None, big=False):
        self.ix, self.dev, self.variant = index, dev, variant
        self.ex = expect(VARIANTS[variant][0], big)
        self.n, self.nt = self.ex.n, self.ex.nt
        self.steps = program() if steps is None else steps
        self.opts = {}
        self.pending = []
        self.seen = set()
        self.last = None        # the dispatch after the last search step
        self.armed = False      # the last P step ran with list_cap 4 and overflowed
        self.list_searches = 0  # L steps the large-k list path served

    # ------------------------------------------------------------ options
    def set_option(self, name, value):
        self.ix.set_option(name, value)
        assert self.ix.get_option(name) == value
        if name in DEFAULTS:
            if value == DEFAULTS[name]:
                self.opts.pop(name, None)
            else:
                self.opts[name] = value

    # -------------------------------------------------------------- a step
    def run(self, step, counters=True, options=True):
        """Run one step; host forms are checked at once, device forms when
        flush() has synchronised their stream.  counters: also read the
        counters of the last search (that waits for its stream)."""
        if options and step["opt"]:
            self.set_option(*step["opt"])
        kind = step["kind"]
        if kind == "L":
            self.ix.set_option("large_lists", step["large_lists"])
        dense_opt = kind == "D" and step["dense_by"] == "option"
        if dense_opt:
            self.ix.set_option("filter_tiles", 0)
        try:
            if step["form"] == "host":
                self._host(step)
            else:
                self._device(step)
        finally:
            if dense_opt:
                self.ix.set_option("filter_tiles", 1)
        self._diagnostics(step, counters or step["form"] == "host")
        if len(self.pending) >= 3:
            self.flush()

    def _want(self, step):
        kind = step["kind"]
        if kind == "S":
            docs = self.ex.s_docs(self.steps, step)
            return docs, self.ex.score_docs(step, docs)
        if kind == "M":
            return self.ex.term_masks(step)
        return self.ex.topk(step)

    def _host(self, step):
        ix, kind, k = self.ix, step["kind"], step["k"]
        q, w = step_queries(step)
        want = self._want(step)
        what = (self.variant, step)
        if kind in "PL":
            _exact(ix.search(q, k), want)
        elif kind in "FD":
            _exact(ix.search_filtered(q, k, self.dev["packed"], step_query_mask(step)), want)
        elif kind == "W":
            if step["masked"]:
                _exact(ix.search_weighted(q, w, k, self.dev["packed"], step_query_mask(step)),
                       want)
            else:
                _exact(ix.search_weighted(q, w, k), want)
        elif kind == "B":
            must, any_, must_not = (c[rows_of(step["Q"])] for c in clauses())
            base = self.dev["packed"][0:1] if step["base"] else None
            _exact(ix.search_boolean(q, k, must, any_, must_not, base), want)
        elif kind == "S":
            docs, scores = want
            got = ix.score_docs_weighted(q, w, docs) if step["weighted"] else ix.score_docs(q, docs)
            assert np.array_equal(got.view(np.uint32), scores.view(np.uint32)), what
        elif kind == "M":
            must, any_, must_not = (c[rows_of(step["Q"])] for c in clauses())
            base = self.dev["packed"][0:1] if step["base"] else None
            assert np.array_equal(ix.term_masks(must, any_, must_not, base), want), what
        else:
            raise AssertionError(kind)

    def _device(self, step):
        import torch
        ix, kind, k, Q, T = self.ix, step["kind"], step["k"], step["Q"], step["T"]
        dev = self.dev
        st = dev["streams"][step["stream"]]
        want = self._want(step)
        with torch.cuda.stream(st):  # the step's inputs and garbage outputs: on its own stream
            rows = torch.from_numpy(rows_of(Q)).cuda()
            dq = dev["q"][rows][:, :T].contiguous()
            dw = dev["w"][rows][:, :T].contiguous()
            if kind in SEARCH_KINDS:
                dd = torch.full((Q, k), BAD_DOC, dtype=torch.int32, device="cuda")
                ds = torch.full((Q, k), BAD_SCORE, dtype=torch.float32, device="cuda")
                out = (dd, ds)
            keep = [dq, dw, rows]
            if kind in "PL":
                ix.search_device(dq, k, dd, ds, st)
            elif kind in "FD" or (kind == "W" and step["masked"]):
                dqm = torch.from_numpy(step_query_mask(step)).cuda()
                keep.append(dqm)
                if kind == "W":
                    ix.search_weighted_device(dq, dw, k, dev["masks"], dqm, dd, ds, st)
                else:
                    ix.search_filtered_device(dq, k, dev["masks"], dqm, dd, ds, st)
            elif kind == "W":
                ix.search_weighted_device(dq, dw, k, None, None, dd, ds, st)
            elif kind == "H":
                S = ix.sample_width(k, 1, self.n)
                keys = torch.full((Q, max(S, 1)), 7, dtype=torch.int64, device="cuda")
                keep.append(keys)
                if S > 0:
                    ix.search_sample_device(dq, k, 1, self.n, keys, st)
                ix.search_finish_device(dq, k, 1, self.n, keys.unsqueeze(0), dd, ds, st)
            elif kind == "S":
                ddocs = torch.from_numpy(want[0]).cuda()
                out = torch.full(want[0].shape, BAD_SCORE, dtype=torch.float32, device="cuda")
                keep.append(ddocs)
                if step["weighted"]:
                    ix.score_docs_weighted_device(dq, dw, ddocs, out, st)
                else:
                    ix.score_docs_device(dq, ddocs, out, st)
                want = want[1]
            elif kind == "M":
                cl = [dev[name][rows].contiguous() for name in ("must", "any", "must_not")]
                base = dev["masks"][0:1] if step["base"] else None
                out = torch.full(want.shape, BAD_WORD, dtype=torch.int32, device="cuda")
                keep += cl
                ix.term_masks_device(cl[0], cl[1], cl[2], base, out, st)
            else:
                raise AssertionError(kind)
        self.pending.append((st, step, out, want, keep))

    def flush(self):
        """Synchronise each pending step's own stream, then compare its outputs."""
        for st, step, out, want, _ in self.pending:
            st.synchronize()
            what = (self.variant, step)
            if step["kind"] in SEARCH_KINDS:
                _exact((out[0].cpu().numpy(), out[1].cpu().numpy()), want)
            elif step["kind"] == "S":
                assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)), what
            else:
                assert np.array_equal(out.cpu().numpy().view(np.uint32), want), what
        self.pending = []

    # ------------------------------------------- the "last search" reports
    def _diagnostics(self, step, counters):
        ix, kind, k, Q = self.ix, step["kind"], step["k"], step["Q"]
        d = ix.last_dispatch()
        what = (self.variant, step, d)
        if kind not in SEARCH_KINDS:
            # score_docs and term_masks are no searches: the reports stay
            assert self.last is None or d == self.last, what
            return
        self.last = d
        kernels = d["kernels"]
        self.seen |= kernels
        tile_passes = k <= K_MAX and (kind in "FB" or kind == "W")
        assert ("weighted" in kernels) == (kind == "W"), what
        assert ("filtered" in kernels) == tile_passes, what
        if kind in "LD" or (kind == "W" and k > K_MAX):
            assert "large_k" in kernels, what
        if kind in "PH":
            assert "large_k" not in kernels, what
        if kind == "P":
            # (whether the handle has turned the tile-bound threshold off for a while is
            # its own report, "bound_off": taken from the dispatch, not predicted — the
            # results are checked against the oracle either way)
            flat = uses_flat(step, self.opts)
            P = threshold_p(step, dict(self.opts, theta_bound=self.opts.get("theta_bound", 1)
                                       and "bound_off" not in kernels),
                            self.variant == "dense", self.nt)
            assert kernels - FLAGS == _want_kernels(P, flat) and d["sample_p"] == P, (what, P)
        if not counters:
            return
        stats = ix.search_stats()
        if k <= K_MAX:
            assert stats["large_dense_queries"] == 0, (what, stats)
        elif kind == "L":
            lists = large_lists_apply(step, self.opts, self.variant != "signed", self.nt)
            assert (stats["large_dense_queries"] >= 0) == lists, (what, stats)
            assert lists or stats["large_dense_queries"] == -1, (what, stats)
            if lists:  # the list path: a sampled threshold at stride 2, at most Q handed on
                assert stats["large_dense_queries"] <= Q, (what, stats)
                assert {"flat_sample", "flat_rest"} <= kernels and d["sample_p"] == 2, what
                self.list_searches += 1
            if not lists:  # dense rows select without the counters: they read zero,
                # not what the previous search left
                assert (stats["rescored_tiles"], stats["fallback_queries"],
                        stats["block_merge_queries"]) == (0, 0, 0), (what, stats)
        if kind == "D":
            assert ix.filtered_stats()[0] == Q, what
        elif tile_passes:
            # the lists that overflowed (list_counts: the keys each receives, a
            # restatement of the filter passes' rule — a check of this counter only).
            # An automatic capacity is that of the largest k since the workspace
            # was built: between this k's and 4096's
            n_dense = ix.filtered_stats()[0]
            counts = self.ex.list_counts(step)
            cap = self.opts.get("list_cap", 0)
            lo_cap = cap or min(65536, max(2048, 64 * k))
            hi_cap = cap or 65536
            lo, hi = sum(c > hi_cap for c in counts), sum(c > lo_cap for c in counts)
            assert lo <= n_dense <= hi, (what, n_dense, lo, hi)
            if cap == 4 and kind == "F":
                assert n_dense == (Q if k > 4 else 0), what
            assert ("large_k" in kernels) == (n_dense > 0), what
        if kind == "P":
            if (self.opts.get("list_cap") == 4 and "sample_p" not in self.opts
                    and step["T"] >= 8 and k == 100):
                assert stats["fallback_queries"] > 0, (what, stats)
                self.armed = True
            elif self.armed and "list_cap" not in self.opts and step["T"] >= 8 and k == 100:
                assert stats["fallback_queries"] == 0, (what, stats)  # (not the last search's)
                self.armed = False


# ------------------------------------------------------------ 1. the program
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_program_on_one_handle(dev, variant):
    """The 82 steps on one handle, twice: the second round starts from grown
    buffers.  Reading the counters waits for the search's stream: the first
    round reads them after host steps and after every second device step, so
    that device steps still follow each other unsynchronised; the second round
    reads them after every step."""
    index = _open(variant)
    run = Runner(index, variant, dev)
    for rnd in (0, 1):
        n_dev = 0
        for step in run.steps:
            n_dev += step["form"] == "device"
            run.run(step, counters=rnd == 1 or n_dev % 2 == 0)
        run.flush()
        assert run.opts == {}
    want = {"flat_sample", "flat_rest", "flat_all", "large_k", "filtered", "weighted"}
    if variant == "dense":
        want.add("bound_keys")  # 147 tiles serve k <= 9
    assert want <= run.seen and WAVE & run.seen, (want - run.seen, run.seen)
    index.close()


# ------------------------------------------------------ 2. the shared arena
def test_arena_partial_fit(dev):
    """A small arena (a dense filtered search of two queries), then at once a
    large-k search that needs more: some of its buffers come from the arena,
    the rest are stream-ordered; the same search again with the arena regrown;
    then the arena's other users."""
    index = _open("dense")
    run = Runner(index, "dense", dev, steps=())
    run.run(_step("D", 2, 8, 100, dense_by="option"))
    big = _step("L", 48, 8, N, large_lists=0, form="device", stream=1)
    run.run(big)
    run.flush()
    run.run(big)
    run.flush()
    run.run(_step("F", 48, 8, 100, i=1))
    run.run(_step("W", 16, 8, K_MAX + 1, i=2, masked=True, form="device", stream=2))
    run.run(_step("L", 16, 8, K_MAX + 1, large_lists=1, form="device", stream=0))
    run.flush()
    run.run(_step("F", 48, 17, K_MAX, i=3, form="device", stream=1))
    run.flush()
    index.close()


# --------------------------------------------------------- 3. the workspace
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_workspace_shrinks_and_grows(dev, variant):
    """The workspace keeps the largest Q and k seen; list_cap frees it."""
    index = _open(variant)
    run = Runner(index, variant, dev, steps=())
    for n, (Q, k) in enumerate([(1, 1), (48, 100), (2, 4096), (48, 1), (1, 100)]):
        run.run(_step("P", Q, 8, k, form=("host", "device")[n % 2], stream=n % 3))
    run.flush()
    run.set_option("list_cap", 4)
    run.run(_step("F", 16, 8, 10, i=1))
    run.run(_step("P", 48, 8, 100, form="device", stream=1))
    run.run(_step("L", 16, 8, K_MAX + 1, large_lists=1, form="device", stream=2))
    run.run(_step("H", 2, 8, 8, form="device", stream=0))
    run.flush()
    run.set_option("list_cap", 0)
    run.run(_step("P", 48, 8, 100))
    if variant == "sparse":
        # only the query width changes: the segment table alone grows
        run.run(_step("P", 48, 65, 100, form="device", stream=1))
        run.run(_step("P", 48, 8, 100, form="device", stream=2))
        run.flush()
    index.close()


# ------------------------------------------------- 4. the two-half protocol
def _two_half_inputs(dev, run, st, Q, T, k):
    import torch
    with torch.cuda.stream(st):
        rows = torch.from_numpy(rows_of(Q)).cuda()
        dq = dev["q"][rows][:, :T].contiguous()
        S = run.ix.sample_width(k, 1, N)
        keys = torch.full((Q, max(S, 1)), 7, dtype=torch.int64, device="cuda")
        dd = torch.full((Q, k), BAD_DOC, dtype=torch.int32, device="cuda")
        ds = torch.full((Q, k), BAD_SCORE, dtype=torch.float32, device="cuda")
    return dq, S, keys, dd, ds


@pytest.mark.parametrize("variant", ["dense", "signed"])
def test_two_half_with_workspace_free_calls_between(dev, variant):
    """score_docs_device and term_masks_device between the sample half and the
    finish half, on another stream: they read the index arrays only, so the
    search's result is the plain search's and theirs are their references'.
    Then the finish half on three streams, followed at once by a plain search
    on a fourth."""
    index = _open(variant)
    run = Runner(index, variant, dev, steps=(_step("P", 16, 8, 8),))
    A, B, C, D = dev["streams"]
    Q, T, k = 16, 8, 8
    want = run.ex.topk(_step("P", Q, T, k))
    for three in (False, True):
        dq, S, keys, dd, ds = _two_half_inputs(dev, run, A, Q, T, k)
        assert S > 0
        index.search_sample_device(dq, k, 1, N, keys, A)
        run.run(_step("S", Q, 17, 0, i=1, weighted=three, form="device", stream=1))
        run.run(_step("M", Q, 0, 0, base=not three, form="device", stream=1))
        if three:
            B.wait_stream(A)  # (the keys: the caller's all-gather would sit here)
            index.search_finish_streams_device(dq, k, 1, N, keys.unsqueeze(0), dd, ds, B, C, A)
            last = A
            # a plain search on a fourth stream, right behind the finish half (its
            # counters are not read here: that would wait for the stream)
            run.run(_step("P", 48, 17, 100, form="device", stream=3), counters=False)
        else:
            index.search_finish_device(dq, k, 1, N, keys.unsqueeze(0), dd, ds, A)
            last = A
        last.synchronize()
        _exact((dd.cpu().numpy(), ds.cpu().numpy()), want)
        D.synchronize()
        run.flush()
        assert index.search_stats()["large_dense_queries"] == 0
    index.close()


# ------------------------------------------------------- 5. a base and a fork
def test_base_and_fork_interleaved(dev):
    """A base on stream A and its fork on stream B run the program's first 20
    steps alternately, one synchronisation per pair of steps.  The program's
    option changes go to the base only, after the fork was made: the fork
    keeps the options it copied."""
    import torch
    base = _open("dense")
    fork = base.fork()
    A, B = dev["streams"][0], dev["streams"][1]
    rb = Runner(base, "dense", dict(dev, streams=[A, A, A]))
    rf = Runner(fork, "dense", dict(dev, streams=[B, B, B]))
    base.set_option("grid_pct", 50)   # both may run at once: half the slots each
    fork.set_option("grid_pct", 50)
    changed = set()
    for step in rb.steps[:20]:
        rb.run(step, counters=False)
        rf.run(step, counters=False, options=False)
        torch.cuda.synchronize()
        rb.flush()
        rf.flush()
        if step["opt"]:
            changed.add(step["opt"][0])
        for name in changed:
            assert base.get_option(name) == rb.opts.get(name, DEFAULTS[name]), (step, name)
            assert fork.get_option(name) == DEFAULTS[name], (step, name)
    assert {"flat", "sample_p", "theta_bound", "list_cap"} <= changed
    fork.close()
    base.close()


# ------------------------------------------- 6. the large-k list path (1027 tiles)
def _list_step(**kw):
    return _step("L", kw.pop("Q", 4), 8, K_MAX + 1, large_lists=1, **kw)


def test_list_path_between_other_searches(dev_big):
    """On the 1027-tile fixture k = 4097 takes the large-k list path, which
    asks for the workspace with k = 1: first on a fresh handle, then between
    plain, filtered and two-half searches that need longer lists, after
    list_cap freed the workspace, and beside the dense rows (large_lists 0).
    Counter [5] is >= 0 after every list search, -1 after dense rows and 0
    after the next small search (asserted by the runner after each step)."""
    index = _open("dense", big=True)
    run = Runner(index, "dense", dev_big, steps=(), big=True)
    run.run(_list_step(form="device", stream=0))
    run.run(_step("P", 4, 8, 100, form="device", stream=1))
    run.run(_list_step())
    run.run(_step("F", 4, 8, K_MAX, i=1, form="device", stream=2))
    run.run(_list_step(form="device", stream=0))
    run.run(_step("H", 4, 8, 8, form="device", stream=1))
    run.run(_list_step(Q=8, form="device", stream=1))
    run.flush()
    run.set_option("list_cap", 4)   # frees the workspace; the list path's capacity too
    run.run(_list_step(form="device", stream=2))
    run.run(_step("P", 4, 8, 100))
    run.run(_list_step())
    run.set_option("list_cap", 0)
    run.run(_list_step(form="device", stream=0))
    run.run(_step("P", 4, 8, 100, form="device", stream=1))
    run.run(_step("L", 4, 8, K_MAX + 1, large_lists=0))
    run.run(_step("W", 4, 8, 100, i=2, masked=True, form="device", stream=2))
    run.run(_list_step(form="device", stream=2))
    run.flush()
    assert run.list_searches == 8 and not run.armed
    index.close()


def test_arena_partial_fit_list_path(dev_big):
    """The arena of test_arena_partial_fit with the list path among its users:
    sized by a small dense filtered search, outgrown by dense large-k rows,
    then used by the list path, the filtered and the weighted search."""
    index = _open("dense", big=True)
    run = Runner(index, "dense", dev_big, steps=(), big=True)
    run.run(_step("D", 2, 8, 100, dense_by="option"))
    run.run(_list_step(Q=8, form="device", stream=0))      # needs more than the arena holds
    run.run(_list_step(Q=8, form="device", stream=1))      # regrown
    rows = _step("L", 8, 8, 20_000, large_lists=0, form="device", stream=1)
    run.run(rows)
    run.flush()
    run.run(rows)
    run.run(_list_step(Q=8, form="device", stream=2))
    run.run(_step("F", 8, 8, 100, i=1))
    run.run(_step("W", 4, 8, K_MAX + 1, i=2, masked=True, form="device", stream=2))
    run.run(_list_step(form="device", stream=0))
    run.flush()
    assert run.list_searches == 4
    index.close()

