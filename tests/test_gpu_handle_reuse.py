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
dispatch carries the filtered flag like an F step's.

A second program (program2, test_ranked_program_on_one_handle) and the tests
of section 7 do the same for the calls that share one argument path and more
handle state: the cursor search (A), the collapsed search and its kept state
(C), the composed boolean searches with min_match, facets, ranges, sort= and
k = 0 (G) and the calls documented as stateless (U).  After every step the
runner holds the handle's reports to what the step should leave: the cursor
and collapsed flags on exactly the calls that set them, collapse_stats() equal
to the paged loop's model for the last C step and unchanged by everything
else, the dense-path count of a chunked boolean search the sum over its
chunks, and every report untouched by a call that runs no search."""
import numpy as np
import pytest

from test_gpu_parity import _exact, _idx, _want_kernels
from test_handle_reuse_host import (DEFAULTS, DEFAULTS2, K_MAX, N, N_BIG, N_LABELS, SEARCH_KINDS,
                                    VARIANTS, clauses, collapse_groups, collapse_page, columns,
                                    expect, large_lists_apply, masks, pools, program, program2,
                                    range_clauses, reuse_csc, rows_of, sort_order,
                                    stateless_steps, step_after_ranks, step_min_match,
                                    step_queries, step_query_mask, threshold_p, uses_flat)

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
         "groups": {t: up(collapse_groups(t)) for t in (False, True)},
         "columns": {name: up(col) for name, col in columns().items()},
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
        # collapse_stats() as the last C step left them (a fresh handle: zeros)
        self.cstats = dict.fromkeys(("rounds", "unfinished_rows", "dropped_entries",
                                     "excluded_rows"), 0)

    # ------------------------------------------------------------ options
    def set_option(self, name, value):
        self.ix.set_option(name, value)
        assert self.ix.get_option(name) == value
        if name in DEFAULTS2:
            if value == DEFAULTS2[name]:
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
        counters = counters or step["form"] == "host"
        # (S and M steps overlap a search in flight: their check reads no counters)
        wait = counters and kind in "GU"
        before = None if self._searches(step) else self._reports(wait)
        try:
            if step["form"] == "host":
                self._host(step)
            else:
                self._device(step)
        finally:
            if dense_opt:
                self.ix.set_option("filter_tiles", self.opts.get("filter_tiles", 1))
        if before is not None:
            # no search ran (score_docs, the mask calls, a boolean call that only selects
            # by rank or only counts): every report of the handle is what it was
            assert self._reports(wait) == before, (self.variant, step)
        self._diagnostics(step, counters)
        if len(self.pending) >= 3:
            self.flush()

    @staticmethod
    def _searches(step):
        """Does the step run a search of the handle (one that writes its reports)?"""
        kind = step["kind"]
        return kind in SEARCH_KINDS or kind in "AC" or (
            kind == "G" and step["mode"] not in ("sorted", "counts"))

    def _reports(self, counters):
        """The handle's reports; the counters (which wait for the last
        search's stream) only where the caller reads them anyway."""
        ix = self.ix
        out = (ix.last_dispatch(), ix.collapse_stats())
        return out + (ix.search_stats(), ix.filtered_stats()) if counters else out

    def _weighted(self, step):
        return step["kind"] == "W" or (step["kind"] in "AC" and step["weighted"])

    def _want(self, step):
        kind = step["kind"]
        if kind == "A":
            return self.ex.after(step)
        if kind == "C":
            return self.ex.collapsed(step, collapse_page(step, self.opts))
        if kind == "G":
            return self.ex.boolean(step)
        if kind == "U":
            return self.ex.stateless(step)
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
        elif kind == "A":
            w = w if step["weighted"] else None
            m, qm = (self.dev["packed"], step_query_mask(step)) if step["masked"] else (None, None)
            _exact(ix.search_after(q, k, self.ex.cursors(step), w, m, qm), want)
        elif kind == "C":
            w = w if step["weighted"] else None
            m, qm = (self.dev["packed"], step_query_mask(step)) if step["masked"] else (None, None)
            got = ix.search_collapsed(q, k, collapse_groups(step["tenant"]), step["per_group"], w,
                                      m, qm, return_groups=step["ret_groups"])
            _exact(got[:2], want[:2])
            if step["ret_groups"]:
                assert np.array_equal(got[2], want[2]), what
        elif kind == "G":
            self._host_boolean(step, q, want)
        elif kind == "U":
            self._host_stateless(step, want)
        else:
            raise AssertionError(kind)

    def _host_boolean(self, step, q, want):
        ix, mode, what = self.ix, step["mode"], (self.variant, step)
        rows = rows_of(step["Q"])
        must, any_, must_not = (c[rows] for c in clauses())
        base = self.dev["packed"][0:1] if step["base"] else None
        kw = {"total_hits": True}
        if mode in ("min_match", "all"):
            kw["min_match"] = step_min_match(step)
        if mode in ("facets", "all", "counts"):
            kw["facets"] = (columns()["labels"], N_LABELS)
        if mode in ("all", "sorted"):
            kw["ranges"] = (columns()[step["column"]],) + range_clauses(step["column"], rows)
        if mode == "sorted":
            kw["sort"] = sort_order(step["sort_column"], bool(step["descending"]))
            kw["after_ranks"] = step_after_ranks(step)
        got = list(ix.search_boolean(q, step["k"], must, any_, must_not, base, **kw))
        _exact((got.pop(0), got.pop(0)), (want["docs"], want["scores"]))
        for name in ("ranks", "totals", "facets"):
            if name in want or name == "totals":
                assert np.array_equal(got.pop(0), want[name]), (what, name)
        assert not got, what

    def _host_stateless(self, step, want):
        ix, mode, what = self.ix, step["mode"], (self.variant, step)
        if mode == "mask_count":
            got = ix.mask_count(want["packed"])
        elif mode == "facets":
            got = ix.facets(want["packed"], columns()["labels"], N_LABELS)
        elif mode == "range_masks":
            got = ix.range_masks(columns()[step["column"]], *want["clauses"], want["base"])
        elif mode == "term_masks":
            must, any_, must_not = (c[rows_of(step["Q"])] for c in clauses())
            base = self.dev["packed"][0:1] if step["base"] else None
            got = ix.term_masks(must, any_, must_not, base, min_match=want["min_match"])
        else:
            order = ix.sort_ranks(columns()[step["column"]], bool(step["descending"]))
            for a, b in zip(order, want["order"]):
                assert np.array_equal(a, b), what
            got = ix.search_sorted(want["packed"], order, step["k"])
            paged = ix.search_sorted(want["packed"], order, step["k"], want["after"])
            for a, b in zip(paged, want["want_after"]):
                assert np.array_equal(a, b), what
            for a, b in zip(got, want["want"]):
                assert np.array_equal(a, b), what
            return
        assert got.dtype == want["want"].dtype and np.array_equal(got, want["want"]), what

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
            elif kind in "AC":
                up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
                dd = torch.full((Q, k), BAD_DOC, dtype=torch.int32, device="cuda")
                ds = torch.full((Q, k), BAD_SCORE, dtype=torch.float32, device="cuda")
                dwt = dw if step["weighted"] else None
                dm, dqm = (dev["masks"], up(step_query_mask(step))) if step["masked"] else (None, None)
                keep.append(dqm)
                if kind == "A":
                    cur = self.ex.cursors(step)
                    d_after = None if cur is None else (up(cur[0]), up(cur[1]))
                    keep.append(d_after)
                    ix.search_after_device(dq, k, d_after, dwt, dm, dqm, dd, ds, st)
                    out = (dd, ds)
                else:
                    dg = (torch.full((Q, k), BAD_DOC, dtype=torch.int32, device="cuda")
                          if step["ret_groups"] else None)
                    ix.search_collapsed_device(dq, k, dev["groups"][step["tenant"]],
                                               step["per_group"], dwt, dm, dqm, dd, ds, dg, st)
                    out = (dd, ds, dg)
            elif kind == "U":
                out, want = self._device_stateless(step, want, st, keep)
            else:
                raise AssertionError(kind)
        self.pending.append((st, step, out, want, keep))

    def _device_stateless(self, step, want, st, keep):
        """A U step's device form (inside the step's stream context): the
        output tensors, garbage-filled, and the arrays they must equal."""
        import torch
        ix, dev, mode, Q, k = self.ix, self.dev, step["mode"], step["Q"], step["k"]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        bad = lambda shape, dtype, v=BAD_DOC: torch.full(shape, v, dtype=dtype, device="cuda")
        dm = up(want["packed"].view(np.int32))
        keep.append(dm)
        if mode == "mask_count":
            out = bad((Q,), torch.int64)
            ix.mask_count_device(dm, out, st)
        elif mode == "facets":
            out = bad((Q, N_LABELS), torch.int64)
            ix.facets_device(dm, dev["columns"]["labels"], N_LABELS, out, st)
        elif mode == "range_masks":
            cl = [up(a) for a in want["clauses"]]
            base = dev["masks"][0:1] if step["base"] else None
            out = bad(want["want"].shape, torch.int32)
            keep += cl
            ix.range_masks_device(dev["columns"][step["column"]], cl[0], cl[1], cl[2], out, base, st)
        elif mode == "term_masks":
            rows = up(rows_of(Q))
            cl = [dev[name][rows].contiguous() for name in ("must", "any", "must_not")]
            mm = up(want["min_match"])
            base = dev["masks"][0:1] if step["base"] else None
            out = bad(want["want"].shape, torch.int32)
            keep += cl + [mm]
            ix.term_masks_device(cl[0], cl[1], cl[2], base, out, st, d_min_match=mm)
        else:
            ranks, perm = bad((N,), torch.int32), bad((N,), torch.int32)
            ix.sort_ranks_device(dev["columns"][step["column"]], ranks, perm,
                                 bool(step["descending"]), st)
            scratch = torch.empty(max(ix.sorted_scratch_bytes(Q, k), 1), dtype=torch.uint8,
                                  device="cuda")
            after = up(want["after"])
            outs = [bad((Q, k), torch.int32) for _ in range(4)]
            keep += [scratch, after]
            ix.search_sorted_device(dm, ranks, perm, k, None, outs[0], outs[1], scratch, st)
            ix.search_sorted_device(dm, ranks, perm, k, after, outs[2], outs[3], scratch, st)
            return ([ranks, perm] + outs,
                    list(want["order"]) + list(want["want"]) + list(want["want_after"]))
        return [out], [want["want"]]

    def flush(self):
        """Synchronise each pending step's own stream, then compare its outputs."""
        for st, step, out, want, _ in self.pending:
            st.synchronize()
            what = (self.variant, step)
            if step["kind"] in SEARCH_KINDS or step["kind"] == "A":
                _exact((out[0].cpu().numpy(), out[1].cpu().numpy()), want)
            elif step["kind"] == "C":
                _exact((out[0].cpu().numpy(), out[1].cpu().numpy()), want[:2])
                if out[2] is not None:
                    assert np.array_equal(out[2].cpu().numpy(), want[2]), what
            elif step["kind"] == "U":
                for n, (t, w) in enumerate(zip(out, want)):
                    got = t.cpu().numpy()
                    assert got.shape == w.shape and got.itemsize == w.itemsize, (what, n)
                    assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(w).view(np.uint8)), (what, n)
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
        # the collapsed search's statistics are the last C step's, whatever ran since
        if kind == "C":
            self.cstats = self._want(step)[3]
        assert ix.collapse_stats() == self.cstats, (what, ix.collapse_stats(), self.cstats)
        if not self._searches(step):
            # no search: the reports stay (run() compared all of them around the step)
            assert self.last is None or d == self.last, what
            return
        self.last = d
        kernels = d["kernels"]
        self.seen |= kernels | ({"collapsed"} if d["collapsed"] else set())
        # the flags of one call do not outlive it: a collapsed search's pages are cursor
        # searches (its dispatch is its last round's), no other kind carries either flag
        assert d["collapsed"] == (kind == "C"), what
        assert ("after" in kernels) == (kind in "AC"), what
        ranked = kind in "FBWACG"        # run_filtered's callers
        tiles_on = self.opts.get("filter_tiles", 1)
        tile_passes = ranked and tiles_on and k <= K_MAX
        # optional weights of no slot (A and C at T = 0): the host call stages the empty
        # array and passes a pointer, the flag is set; an empty tensor has no pointer
        given = step["T"] > 0 or kind == "W" or step["form"] == "host"
        assert ("weighted" in kernels) == (self._weighted(step) and given), what
        assert ("filtered" in kernels) == bool(tile_passes), what
        if kind in "LD" or (ranked and not tile_passes):
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
        if kind == "D" or (ranked and not tile_passes and kind != "C"):
            # every query by the dense path; a chunked boolean search sums its chunks
            assert ix.filtered_stats()[0] == Q, what
        elif tile_passes and kind != "C":   # (a collapsed search: its last round's sub-batch)
            # the lists that overflowed (list_counts: the keys each receives, a
            # restatement of the filter passes' rule — a check of this counter only).
            # An automatic capacity is that of the largest k since the workspace
            # was built: between this k's and 4096's
            n_dense = ix.filtered_stats()[0]
            counts = self.ex.list_counts2(step) if kind in "AG" else self.ex.list_counts(step)
            cap = self.opts.get("list_cap", 0)
            lo_cap = cap or min(65536, max(2048, 64 * k))
            hi_cap = cap or 65536
            lo, hi = sum(c > hi_cap for c in counts), sum(c > lo_cap for c in counts)
            assert lo <= n_dense <= hi, (what, n_dense, lo, hi)
            if cap == 4 and kind == "F":
                assert n_dense == (Q if k > 4 else 0), what
            if not (kind == "G" and self.opts.get("bool_chunk")):   # (the last chunk's set)
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


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_ranked_program_on_one_handle(dev, variant):
    """program2's 82 steps on one handle, twice, with the counters read as in
    test_program_on_one_handle: cursor, collapsed, composed boolean and the
    stateless calls between the plain, large-k, filtered and two-half searches
    they share the workspace, the arena, the staging buffers and the reports
    with."""
    index = _open(variant)
    run = Runner(index, variant, dev, steps=program2())
    for rnd in (0, 1):
        n_dev = 0
        for step in run.steps:
            n_dev += step["form"] == "device"
            run.run(step, counters=rnd == 1 or n_dev % 2 == 0)
            assert run.opts == step["opts"]
        run.flush()
        assert run.opts == {}
    want = {"after", "filtered", "weighted", "large_k", "collapsed"}
    assert want <= run.seen, (want - run.seen, run.seen)
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


# ------------------------------------- 7. the cursor, collapsed and composed calls
def _a_step(Q, T, k, cursor="none", weighted=False, masked=False, **kw):
    return _step("A", Q, T, k, cursor=cursor, weighted=weighted, masked=masked, **kw)


def _c_step(Q, T, k, tenant=False, per_group=1, weighted=False, masked=False, ret_groups=False,
            **kw):
    return _step("C", Q, T, k, tenant=tenant, per_group=per_group, weighted=weighted,
                 masked=masked, ret_groups=ret_groups, **kw)


def _g_step(Q, T, k, mode, base=False, column="i32", sort_column="i64", descending=0, **kw):
    return _step("G", Q, T, 0 if mode == "counts" else k, mode=mode, base=base, column=column,
                 sort_column=sort_column, descending=descending, **kw)


def test_collapse_state_shrinks_and_grows(dev):
    """The collapsed search's kept state (cstate) grows only, and its carving
    depends on Q, on the page and on whether the groups go to the caller: the
    smallest layout, the largest (48 rows, pages of 4096, the rows' groups kept
    in the state), a small one again inside the large buffer, and the large
    one once more, with a plain, a cursor and a k = N search in between.  The
    third and the last collapsed search are held to one expectation."""
    index = _open("dense")
    run = Runner(index, "dense", dev, steps=())
    big = _c_step(48, 8, 100, tenant=True, per_group=3, form="device", stream=1)
    run.run(_c_step(1, 8, 1, ret_groups=True, form="device", stream=0))
    run.run(_step("P", 16, 8, 100))
    run.set_option("collapse_page", 4096)
    run.run(big)
    run.run(_a_step(16, 8, 100, "page", i=1, form="device", stream=2))
    run.flush()
    assert run.cstats["rounds"] == 2 and run.cstats["unfinished_rows"] == 48
    run.set_option("collapse_page", 8)
    run.run(_c_step(2, 8, 8, weighted=True, ret_groups=True, form="device", stream=0))
    run.set_option("collapse_page", 4096)
    run.run(_step("L", 2, 8, N, large_lists=0, form="device", stream=2))
    run.run(big)
    run.flush()
    run.set_option("collapse_page", 0)
    index.close()


@pytest.mark.parametrize("weighted,masked", [(True, True), (False, False)])
def test_pages_chain_across_other_calls(dev, weighted, masked):
    """Three pages of k = 100 by device calls on two streams, each cursor
    page_cursor of the page before (tensors of the device, never read by the
    host), with a collapsed, a large-k and a rank-sorted boolean call of the
    same handle between them: the pages concatenated are the first 300 of
    every row's order under its mask."""
    import torch
    import bm25mi
    index = _open("signed")
    run = Runner(index, "signed", dev, steps=())
    Q, T, k = 16, 8, 100
    first = _a_step(Q, T, k, weighted=weighted, masked=masked)
    s1, s2 = dev["streams"][1], dev["streams"][2]
    with torch.cuda.stream(s1):
        rows = torch.from_numpy(rows_of(Q)).cuda()
        dq = dev["q"][rows][:, :T].contiguous()
        dw = dev["w"][rows][:, :T].contiguous() if weighted else None
        dm = dev["masks"] if masked else None
        dqm = torch.from_numpy(step_query_mask(first)).cuda() if masked else None
        pages = [(torch.full((Q, k), BAD_DOC, dtype=torch.int32, device="cuda"),
                  torch.full((Q, k), BAD_SCORE, dtype=torch.float32, device="cuda"))
                 for _ in range(3)]
    s1.synchronize()  # (the inputs: read on both streams below)
    between = [_c_step(16, 8, 8, tenant=True, weighted=weighted, form="device", stream=2),
               _step("L", 2, 8, N, large_lists=0, form="device", stream=1),
               _g_step(16, 8, 100, "sorted", base=True)]
    cursor = None
    for n, (dd, ds) in enumerate(pages):
        st = (s1, s2)[n % 2]
        if n:
            st.wait_stream((s1, s2)[(n - 1) % 2])  # (the page before: the caller's own order)
            with torch.cuda.stream(st):
                cursor = bm25mi.page_cursor(*pages[n - 1])
        index.search_after_device(dq, k, cursor, dw, dm, dqm, dd, ds, st)
        assert "after" in index.last_dispatch()["kernels"]
        if n < 2:
            run.run(between[n], counters=False)
            if n == 1:
                run.run(between[2])
    s1.synchronize()
    s2.synchronize()
    run.flush()
    docs = np.concatenate([p[0].cpu().numpy() for p in pages], axis=1)
    bits = np.concatenate([p[1].cpu().numpy() for p in pages], axis=1).view(np.uint32)
    ex = run.ex
    for i, (r, m) in enumerate(zip(rows_of(Q).tolist(), ex.step_masks(first))):
        o = ex.masked(r, T, weighted, m)[:3 * k]
        want_d = np.full(3 * k, -1, np.int32)
        want_b = np.full(3 * k, 0xFFFFFFFF, np.uint32)
        want_d[:len(o)] = o
        want_b[:len(o)] = ex.row(r, T, weighted)[o].view(np.uint32)
        assert np.array_equal(docs[i], want_d) and np.array_equal(bits[i], want_b), (i, r, m)
    index.close()


def test_collapsed_and_cursor_on_base_and_fork(dev):
    """The base runs a device collapsed search on stream 1 while its fork runs
    a device cursor search on stream 2 and a collapsed search on stream 0, with
    no device-wide synchronisation; then the base searches plainly.  Each
    handle has its own state, flags and collapse_stats()."""
    base = _open("dense")
    fork = base.fork()
    rb = Runner(base, "dense", dev, steps=())
    rf = Runner(fork, "dense", dev, steps=())
    for r in (rb, rf):
        r.set_option("grid_pct", 50)   # both may run at once: half the slots each
    rb.run(_c_step(16, 8, 100, tenant=True, ret_groups=True, form="device", stream=1),
           counters=False)
    assert fork.collapse_stats() == rf.cstats and not fork.last_dispatch()["collapsed"]
    rf.run(_a_step(16, 8, 100, "deep", masked=True, i=1, form="device", stream=2),
           counters=False)
    rf.run(_c_step(48, 17, 8, per_group=3, weighted=True, form="device", stream=0),
           counters=False)
    rb.run(_step("P", 16, 8, 100, form="device", stream=1), counters=False)
    assert rb.cstats["rounds"] == 2 and rf.cstats["rounds"] == 1
    assert base.collapse_stats() == rb.cstats and fork.collapse_stats() == rf.cstats
    assert fork.last_dispatch()["collapsed"] and not base.last_dispatch()["collapsed"]
    rf.flush()
    rb.flush()
    fork.close()
    base.close()


def test_boolean_chunks_share_staging(dev):
    """The composed boolean calls stage their queries and rows in the buffers
    every host search uses, one chunk of bool_chunk queries at a time: a
    chunked search with ranges, facets and totals, a plain search of a larger
    Q x T, the rank-sorted form (it writes the staging rows and runs no
    search), a filtered search, and the counts alone.  With list_cap 4 every
    list that receives more than four keys overflows: the chunked search
    reports the sum over its ten chunks, not its last chunk's three queries
    (the runner holds every report against its model after each step)."""
    index = _open("dense")
    run = Runner(index, "dense", dev, steps=())
    run.set_option("bool_chunk", 5)
    run.set_option("list_cap", 4)
    chunked = _g_step(48, 8, 100, "all", base=True, column="i32")
    run.run(chunked)
    counts = run.ex.list_counts2(chunked)
    n_dense = index.filtered_stats()[0]
    assert n_dense == sum(c > 4 for c in counts) and n_dense > 48 % 5, (n_dense, counts)
    run.set_option("list_cap", 0)
    run.run(_step("P", 48, 65, 100))
    run.run(_g_step(48, 8, 100, "sorted", column="f32", sort_column="i64", descending=1, i=1))
    run.run(_step("F", 48, 17, 100, i=2))
    run.run(_g_step(48, 8, 0, "counts", base=True, i=3))
    run.set_option("bool_chunk", 0)
    run.run(_g_step(48, 8, 100, "facets", i=4))
    index.close()


def test_stateless_calls_between_searches(dev):
    """Every stateless call in both forms (stateless_steps: mask_count, facets,
    range_masks, sort_ranks with search_sorted, term_masks with min_match, on
    the device and on the host), each right behind a search of another kind
    on another stream: the results are the models', and every report of the
    handle reads the same before and after the call."""
    index = _open("dense")
    run = Runner(index, "dense", dev, steps=())
    searches = [_c_step(16, 8, 100, tenant=True, form="device", stream=1),
                _a_step(16, 8, 100, "deep", weighted=True, form="device", stream=2),
                _step("P", 48, 8, 100, form="device", stream=0),
                _g_step(16, 8, 100, "all", base=True),
                _step("L", 2, 8, K_MAX + 1, large_lists=0, form="device", stream=1)]
    for n, step in enumerate(stateless_steps()):
        run.run(dict(searches[n % 5], i=n), counters=False)
        # (a device form reads no counters around it: nothing waits for the search)
        run.run(dict(step, stream=(searches[n % 5]["stream"] + 1) % 3), counters=False)
    run.flush()
    assert run.cstats["rounds"] == 2    # (the collapsed searches': no later call changed them)
    index.close()


def test_weights_of_no_slot(dev):
    """Cursor and collapsed searches at T = 0 with weights given: every score
    is +0.0 and the rows are the unweighted ones; the host call passes its
    empty array's pointer and reports a weighted search, an empty tensor has
    no pointer and the device call reports a plain one (the runner pins both
    after each step).  A weighted search of T = 8 follows each."""
    index = _open("signed")
    run = Runner(index, "signed", dev, steps=())
    for n, form in enumerate(("host", "device")):
        run.run(_a_step(2, 0, 8, "page", weighted=True, i=n, form=form, stream=1))
        run.run(_c_step(2, 0, 8, tenant=True, weighted=True, ret_groups=True, form=form, stream=2))
        run.run(_step("W", 2, 8, 8, masked=False, form=form, stream=0))
    run.flush()
    index.close()
