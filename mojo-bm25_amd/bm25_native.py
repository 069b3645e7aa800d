"""Drop-in replacement of the reference's ``bm25_native`` module (BM25v).

Same class, constructor, methods, argument meaning, dtypes and error
behaviour as ``bm25_native.py:32-158`` of yuhuishi-convect/mojo-bm25, with the
scoring (posting gather, per-document fp32 scatter-add, top-k) running on an
MI355X through libbm25mi.so.  Put ``mojo-bm25_amd/`` on ``sys.path`` and
``import bm25_native`` as before.

Deliberate differences:
  * invalid query arrays raise ValueError directly (the reference first drops
    into ``breakpoint()``, bm25_native.py:113);
  * documents with equal scores are ordered by doc id ascending (the
    reference's order is numpy-implementation-defined, bm25_native.py:205-212).
Every top_k <= num_docs is served, as by the reference's argpartition
(bm25_native.py:204-214): k <= 4096 by the thresholded pipeline (tile-bound or
sampled threshold, REST lists, wave merges), larger k by the large-k list path
of csrc/bm25mi_large.hip (sampled slice-maximum threshold, REST crossing
lists, selection and row sort), and by dense score rows with a radix
selection only where lists cannot serve (signed indices, k > 131 072, a list
past its capacity).
"""
from __future__ import annotations

import logging
from typing import Optional, Tuple

import numpy as np
import scipy.sparse as sp

from bm25mi.index import GpuIndex

QueryId = np.int32
TokId = np.int32
DocId = np.int32
Score = np.float32


class BM25v:
    """BM25v(ector): BM25 over a precomputed doc x term score matrix in CSC
    form (bm25_native.py:32-38), resident on the GPU."""

    logger = logging.getLogger(__name__)

    def __init__(self, k1: float = 1.5, b: float = 0.75, device: int = 0):
        self.k1 = k1
        self.b = b
        self.dtype = np.float32
        self.device = device
        self.doc_toks: sp.csc_matrix = sp.csc_matrix(np.zeros((0,), dtype=self.dtype))
        self.doc_lengths: np.ndarray = np.zeros((0,), dtype=self.dtype)
        self.avg_doc_length: float = 0.0
        self.num_docs: int = 0
        self._gpu: GpuIndex | None = None

    def index(self, doc_toks: sp.csc_matrix, doc_lengths) -> None:
        """bm25_native.py:59-74.  Copies the CSC matrix into HBM (the doc
        lengths are kept but, as in the reference, not used for scoring)."""
        self.doc_toks = doc_toks
        self.doc_lengths = doc_lengths
        self.avg_doc_length = np.mean(doc_lengths)
        self.num_docs = doc_toks.shape[0]
        if self._gpu is not None:
            self._gpu.close()
        self._gpu = GpuIndex.from_csc(doc_toks, device=self.device)

    @classmethod
    def from_bm25s(cls, path: str, device: int = 0, k1: Optional[float] = None,
                   b: Optional[float] = None) -> "BM25v":
        """A BM25v over a bm25s index directory (indptr/indices/data
        .csc.index.npy + params.index.json, bm25_test.py:35-42), with doc
        lengths of ones (bm25s does not store them; unused for scoring)."""
        from bm25mi.bm25s_io import load_bm25s
        ix = load_bm25s(path)
        m = cls(k1=ix.params.get("k1", 1.5) if k1 is None else k1,
                b=ix.params.get("b", 0.75) if b is None else b, device=device)
        m.vocab = ix.vocab
        n = ix.num_docs
        m.index(sp.csc_matrix((ix.data, ix.indices, ix.indptr), shape=(n, ix.n_terms)),
                np.ones(n, np.float32))
        return m

    def search(self, queries, top_k: int = 100) -> Tuple[np.ndarray, np.ndarray]:
        """bm25_native.py:76-103: sorted top-k doc ids (int32) and scores (f32)."""
        if self.num_docs is None:
            raise ValueError("BM25v index not built. Call index() first.")
        if len(queries) == 0:
            self.logger.info(
                msg="The query is empty. This will result in a zero score for all documents.")
            return np.zeros((0, 0), dtype=self.dtype), np.zeros((0, 0), dtype=self.dtype)
        return self.get_scores(queries, top_k)

    def get_scores(self, queries, top_k: int) -> Tuple[np.ndarray, np.ndarray]:
        """bm25_native.py:105-127 (validation), then the GPU path."""
        if (not isinstance(queries, np.ndarray) or queries.ndim != 2
                or not isinstance(queries[0][0], TokId)):
            raise ValueError("The queries must be a list of list of query token IDs.")
        max_token_id = int(queries.max(initial=0))
        n_terms = self._gpu.n_terms if self._gpu is not None else len(self.doc_toks.indptr) - 1
        if max_token_id >= n_terms:
            raise ValueError(
                f"The maximum token ID in the query ({max_token_id}) is higher than the number "
                "of tokens in the index.")
        return self._compute_relevance_from_scores(queries=queries, top_k=top_k,
                                                   dtype=self.dtype)

    def score(self, queries, docs) -> np.ndarray:
        """Scores of given candidates (not in the reference, whose search is
        top-k only): ``queries`` as for search, ``docs`` an int32 [Q, C] array
        of doc ids (negative = padding, scored 0) -> float32 [Q, C]; each
        score is the one search reports for that document."""
        if len(queries) == 0:
            return np.zeros((0, 0), dtype=self.dtype)
        if (not isinstance(queries, np.ndarray) or queries.ndim != 2
                or not isinstance(queries[0][0], TokId)):
            raise ValueError("The queries must be a list of list of query token IDs.")
        docs = np.asarray(docs)
        if docs.ndim != 2 or docs.shape[0] != queries.shape[0]:
            raise ValueError("docs must be a 2-D [Q, C] array with one row per query.")
        max_token_id = int(queries.max(initial=0))
        n_terms = self._gpu.n_terms if self._gpu is not None else len(self.doc_toks.indptr) - 1
        if max_token_id >= n_terms:
            raise ValueError(
                f"The maximum token ID in the query ({max_token_id}) is higher than the number "
                "of tokens in the index.")
        if self._gpu is None:
            raise ValueError("BM25v index not built. Call index() first.")
        return self._gpu.score_docs(queries, docs)

    def search_filtered(self, queries, top_k: int, allow) -> Tuple[np.ndarray, np.ndarray]:
        """search restricted to the documents ``allow`` lets through (not in
        the reference, whose search has no filter): ``allow`` is a bool
        [n_docs] mask for every query, or [Q, n_docs] with one row per query
        (packed uint32 rows of bm25mi.pack_mask work too).  Returns search's
        tuple: doc ids (int32) and scores (f32), [Q, top_k]; rows with fewer
        than top_k allowed documents end in doc -1 / NaN-bit scores."""
        if len(queries) == 0:
            return np.zeros((0, 0), dtype=self.dtype), np.zeros((0, 0), dtype=self.dtype)
        if (not isinstance(queries, np.ndarray) or queries.ndim != 2
                or not isinstance(queries[0][0], TokId)):
            raise ValueError("The queries must be a list of list of query token IDs.")
        allow = np.asarray(allow)
        if allow.ndim not in (1, 2) or (allow.ndim == 2 and allow.shape[0] != queries.shape[0]):
            raise ValueError("allow must be a [n_docs] mask or a [Q, n_docs] array with one "
                             "row per query.")
        if top_k < 0:
            raise ValueError("negative dimensions are not allowed")
        max_token_id = int(queries.max(initial=0))
        n_terms = self._gpu.n_terms if self._gpu is not None else len(self.doc_toks.indptr) - 1
        if max_token_id >= n_terms:
            raise ValueError(
                f"The maximum token ID in the query ({max_token_id}) is higher than the number "
                "of tokens in the index.")
        if self._gpu is None:
            raise ValueError("BM25v index not built. Call index() first.")
        if allow.ndim == 1:
            return self._gpu.search_filtered(queries, top_k, allow)
        return self._gpu.search_filtered(queries, top_k, allow,
                                         np.arange(queries.shape[0], dtype=np.int32))

    def search_weighted(self, queries, weights, top_k: int) -> Tuple[np.ndarray, np.ndarray]:
        """search with a weight per query term (not in the reference, whose
        search takes no weights): term boosts, expansion terms at fractional
        weight, learned sparse queries, negative feedback.  ``weights`` is a
        float [Q, T] array beside ``queries``; a document's score is the fp32
        sum, in query order, of float32(weight * value) over the terms it
        holds.  Weights of 1.0 give search's result bit for bit; the weight of
        a padding slot is ignored, the others must be finite.  Returns
        search's tuple: doc ids (int32) and scores (f32), [Q, top_k]."""
        if len(queries) == 0:
            return np.zeros((0, 0), dtype=self.dtype), np.zeros((0, 0), dtype=self.dtype)
        if (not isinstance(queries, np.ndarray) or queries.ndim != 2
                or not isinstance(queries[0][0], TokId)):
            raise ValueError("The queries must be a list of list of query token IDs.")
        weights = np.asarray(weights)
        if weights.ndim != 2 or weights.shape != queries.shape:
            raise ValueError(f"weights must be a float array of the queries' shape "
                             f"{queries.shape}, got shape {weights.shape}")
        if top_k < 0:
            raise ValueError("negative dimensions are not allowed")
        max_token_id = int(queries.max(initial=0))
        n_terms = self._gpu.n_terms if self._gpu is not None else len(self.doc_toks.indptr) - 1
        if max_token_id >= n_terms:
            raise ValueError(
                f"The maximum token ID in the query ({max_token_id}) is higher than the number "
                "of tokens in the index.")
        if self._gpu is None:
            raise ValueError("BM25v index not built. Call index() first.")
        return self._gpu.search_weighted(queries, weights, top_k)

    def search_after(self, queries, top_k: int, after=None, allow=None,
                     weights=None) -> Tuple[np.ndarray, np.ndarray]:
        """The next top_k results after a cursor (not in the reference, whose
        search has no cursor): exact deep paging without searching the whole
        prefix.  ``after`` is None (the first page) or the pair (scores [Q]
        float32, docs [Q] int32) that bm25mi.page_cursor makes of the previous
        page; a row whose previous page ended in padding (doc -1) comes back
        all padding.  ``allow`` as in search_filtered, ``weights`` as in
        search_weighted, both optional.  Returns search's tuple: doc ids
        (int32) and scores (f32), [Q, top_k]."""
        if len(queries) == 0:
            return np.zeros((0, 0), dtype=self.dtype), np.zeros((0, 0), dtype=self.dtype)
        if (not isinstance(queries, np.ndarray) or queries.ndim != 2
                or not isinstance(queries[0][0], TokId)):
            raise ValueError("The queries must be a list of list of query token IDs.")
        Q = queries.shape[0]
        if weights is not None:
            weights = np.asarray(weights)
            if weights.ndim != 2 or weights.shape != queries.shape:
                raise ValueError(f"weights must be a float array of the queries' shape "
                                 f"{queries.shape}, got shape {weights.shape}")
        if allow is not None:
            allow = np.asarray(allow)
            if allow.ndim not in (1, 2) or (allow.ndim == 2 and allow.shape[0] != Q):
                raise ValueError("allow must be a [n_docs] mask or a [Q, n_docs] array with one "
                                 "row per query.")
        if after is not None:
            if not isinstance(after, (tuple, list)) or len(after) != 2 \
                    or after[0] is None or after[1] is None:
                raise ValueError("after must be None or a pair (scores [Q], docs [Q])")
            if np.shape(after[0]) != (Q,) or np.shape(after[1]) != (Q,):
                raise ValueError(f"after must hold one cursor per query ({Q})")
            after = (np.ascontiguousarray(after[0], dtype=np.float32),
                     np.ascontiguousarray(after[1], dtype=np.int32))
        if top_k < 0:
            raise ValueError("negative dimensions are not allowed")
        max_token_id = int(queries.max(initial=0))
        n_terms = self._gpu.n_terms if self._gpu is not None else len(self.doc_toks.indptr) - 1
        if max_token_id >= n_terms:
            raise ValueError(
                f"The maximum token ID in the query ({max_token_id}) is higher than the number "
                "of tokens in the index.")
        if self._gpu is None:
            raise ValueError("BM25v index not built. Call index() first.")
        qm = None
        if allow is not None:
            qm = (np.zeros(Q, np.int32) if allow.ndim == 1 else np.arange(Q, dtype=np.int32))
        return self._gpu.search_after(queries, top_k, after, weights, allow, qm)

    def search_collapsed(self, queries, top_k: int, groups, per_group: int = 1,
                         allow=None) -> Tuple[np.ndarray, np.ndarray]:
        """search with at most ``per_group`` hits of every group (not in the
        reference, whose search has no grouping): "one hit per site".
        ``groups`` is an integer [n_docs] array, one group per document (the
        codes of bm25mi.facet_codes; a value < 0: no group).  Each row is the
        walk of search's full order that keeps a document while its group has
        room; rows with fewer hits end in padding (doc -1).  ``allow`` as in
        search_filtered.  top_k <= 4096.  Returns search's tuple: doc ids
        (int32) and scores (f32), [Q, top_k]."""
        if len(queries) == 0:
            return np.zeros((0, 0), dtype=self.dtype), np.zeros((0, 0), dtype=self.dtype)
        if (not isinstance(queries, np.ndarray) or queries.ndim != 2
                or not isinstance(queries[0][0], TokId)):
            raise ValueError("The queries must be a list of list of query token IDs.")
        Q = queries.shape[0]
        if allow is not None:
            allow = np.asarray(allow)
            if allow.ndim not in (1, 2) or (allow.ndim == 2 and allow.shape[0] != Q):
                raise ValueError("allow must be a [n_docs] mask or a [Q, n_docs] array with one "
                                 "row per query.")
        groups = np.asarray(groups)
        if groups.ndim != 1 or groups.dtype.kind not in "iu":
            raise ValueError("groups must be a 1-D integer array with one group per document.")
        if per_group < 1:
            raise ValueError(f"per_group={per_group} must be >= 1")
        if top_k < 0:
            raise ValueError("negative dimensions are not allowed")
        if top_k > 4096:
            raise ValueError(f"top_k={top_k}: a collapsed search is limited to top_k <= 4096")
        max_token_id = int(queries.max(initial=0))
        n_terms = self._gpu.n_terms if self._gpu is not None else len(self.doc_toks.indptr) - 1
        if max_token_id >= n_terms:
            raise ValueError(
                f"The maximum token ID in the query ({max_token_id}) is higher than the number "
                "of tokens in the index.")
        if self._gpu is None:
            raise ValueError("BM25v index not built. Call index() first.")
        qm = None
        if allow is not None:
            qm = (np.zeros(Q, np.int32) if allow.ndim == 1 else np.arange(Q, dtype=np.int32))
        return self._gpu.search_collapsed(queries, top_k, groups, per_group, None, allow, qm)

    def search_boolean(self, queries, top_k: int, must=None, any=None, must_not=None,
                       base=None, *, min_match=None, total_hits: bool = False, facets=None,
                       ranges=None, sort=None, after_ranks=None):
        """search under boolean term filters (not in the reference, whose
        search has no term filter): query q ranks only the documents that hold
        every term of ``must[q]``, at least one of ``any[q]`` (when it names
        one) and none of ``must_not[q]`` — "+a +b -c" — and that ``base``
        allows (a bool [n_docs] mask for every query or [Q, n_docs], or packed
        rows of bm25mi.pack_mask).  Clauses are int32 [Q, width] arrays or
        ragged lists of lists of token ids (negative = padding), or None.
        ``min_match``: query q needs min_match[q] of the terms ``any[q]``
        names instead of one (an int, an int [Q] array or "NN%", as
        bm25mi.min_match_rows; 0: the clause is optional).  Returns
        search_filtered's tuple, with ``total_hits=True`` followed by the
        int64 [Q] number of documents each query's filter lets through; the
        masks are built and counted on the GPU.  ``facets=(groups, n_groups)``
        (groups: an integer group id per document, negative = none, as
        bm25mi.facet_codes makes them of labels) appends, as the last element,
        the int64 [Q, n_groups] count of those documents per group.
        ``ranges=(values, fields, lo, hi)`` (or ``(values, lo, hi)`` for one
        field; GpuIndex.range_masks describes them, bm25mi.range_rows makes the
        last three of dicts) also asks, per query, for numeric fields of the
        documents within inclusive bounds: a date or price range, tested on
        the GPU.  ``sort=(ranks, perm)`` (GpuIndex.sort_ranks makes the pair
        of a column, once per column and direction) returns each query's hits
        in that column's order instead of by score — "newest first" — with
        their int32 [Q, top_k] ranks after the scores; ``after_ranks`` (a
        page's last ranks column) continues after a page."""
        if facets is not None and (not isinstance(facets, (tuple, list)) or len(facets) != 2):
            raise ValueError("facets must be a pair (groups, n_groups)")
        if ranges is not None and (not isinstance(ranges, (tuple, list))
                                   or len(ranges) not in (3, 4)):
            raise ValueError("ranges must be a quadruple (values, fields, lo, hi) or, for one "
                             "field, a triple (values, lo, hi)")
        if len(queries) == 0:
            empty = np.zeros((0, 0), dtype=self.dtype), np.zeros((0, 0), dtype=self.dtype)
            if sort is not None:
                empty += (np.zeros((0, 0), np.int32),)
            if total_hits:
                empty += (np.zeros(0, np.int64),)
            if facets is not None:
                empty += (np.zeros((0, max(int(facets[1]), 0)), np.int64),)
            return empty
        if (not isinstance(queries, np.ndarray) or queries.ndim != 2
                or not isinstance(queries[0][0], TokId)):
            raise ValueError("The queries must be a list of list of query token IDs.")
        from bm25mi.index import min_match_rows, pad_clause
        Q = queries.shape[0]
        clauses = []
        for name, c in (("must", must), ("any", any), ("must_not", must_not)):
            c = None if c is None else pad_clause(c)
            if c is not None and c.shape[0] != Q:
                raise ValueError(f"{name} must have one row per query ({Q}), got {c.shape[0]}.")
            clauses.append(c)
        if base is not None:
            base = np.asarray(base)
            if base.ndim not in (1, 2) or (base.ndim == 2 and base.shape[0] not in (1, Q)):
                raise ValueError("base must be a [n_docs] mask or a [Q, n_docs] array with one "
                                 "row per query.")
        if min_match is not None:
            min_match = min_match_rows(np.zeros((Q, 0), np.int32) if clauses[1] is None
                                       else clauses[1], min_match, "query")
        if top_k < 0:
            raise ValueError("negative dimensions are not allowed")
        max_token_id = max([int(queries.max(initial=0))]
                           + [int(c.max(initial=0)) for c in clauses if c is not None])
        n_terms = self._gpu.n_terms if self._gpu is not None else len(self.doc_toks.indptr) - 1
        if max_token_id >= n_terms:
            raise ValueError(
                f"The maximum token ID in the query ({max_token_id}) is higher than the number "
                "of tokens in the index.")
        if self._gpu is None:
            raise ValueError("BM25v index not built. Call index() first.")
        more = {}  # (only what the caller gave: the call without them is the earlier one)
        if facets is not None:
            more["facets"] = facets
        if ranges is not None:
            more["ranges"] = ranges
        if sort is not None:
            more["sort"] = sort
        if after_ranks is not None:
            more["after_ranks"] = after_ranks
        return self._gpu.search_boolean(queries, top_k, clauses[0], clauses[1], clauses[2], base,
                                        min_match=min_match, total_hits=total_hits, **more)

    def _compute_relevance_from_scores(self, queries, top_k: int, dtype=np.float32):
        """bm25_native.py:129-158 on the GPU: per query, negative ids dropped,
        postings gathered, fp32 sums in query order, top-k."""
        if top_k < 0:
            raise ValueError("negative dimensions are not allowed")
        return self._gpu.search(queries, top_k)
