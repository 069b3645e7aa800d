/*
 * bm25mi.h — C-ABI of libbm25mi.so, the MI355X-native BM25 CSC query engine.
 *
 * This is the drop-in boundary for the reference's batched BM25 scoring path
 * (SURVEY.md §8(b)).  Every entry point is plain C: pointers, sizes and error
 * codes, no torch / HIP types in the signatures.  Each function cites the
 * reference interface it replaces (paths relative to the reference checkout
 * yuhuishi-convect/mojo-bm25 @ 2025-06-20).
 *
 * Conventions
 *   - Return 0 on success, a BM25_E* code otherwise; the message of the last
 *     failure on the calling thread is bm25_last_error().
 *   - Host buffers are C-order numpy-compatible arrays owned by the caller.
 *     A synchronous call that returns an error has finished reading and
 *     writing the caller's arrays.
 *   - Device buffers (the *_device entry points) are caller-owned HIP device
 *     allocations on the index's device; `stream` is a hipStream_t passed as
 *     void* (NULL = the legacy default stream).  *_device calls are
 *     asynchronous with respect to the host.
 *   - One index handle is not re-entrant: calls on the same handle are
 *     serialised by an internal mutex.
 *   - Doc ids are int32, scores float32, token ids int32; negative token ids
 *     are padding and are skipped (bm25_native.py:151).
 *   - Results are sorted by score descending; equal scores are ordered by doc
 *     id ascending (the deterministic rule of the MAX CPU top-k,
 *     operations/topk.mojo:234-258 / test_topk.mojo:222-238; bm25_native's
 *     own tie order is numpy-implementation-defined).
 */
#ifndef BM25MI_H
#define BM25MI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BM25MI_ABI_VERSION 1

enum {
  BM25_OK = 0,
  BM25_EINVAL = 1, /* bad argument (bad shape, token id >= n_terms, k > n_docs ...) */
  BM25_EHIP = 2,   /* HIP runtime failure, or no usable GPU */
  /* 3 is unused: the one-process sharded handle moves its keys and lists with
   * peer copies, and the multi-process path's collectives run in the caller
   * (torch.distributed over RCCL, bm25mi.dist), not in this library */
  BM25_ENOMEM = 4  /* device or host allocation failed */
};

typedef struct bm25_index bm25_index;

/* ABI version of the loaded library (== BM25MI_ABI_VERSION it was built with). */
int bm25_abi_version(void);

/* Message of the last failing call on this thread ("" if none).  The pointer
 * stays valid until the next failing call on the same thread. */
const char* bm25_last_error(void);

/* Number of HIP devices visible to the process (0 on a host without a GPU;
 * never fails). */
int bm25_device_count(void);

/*
 * Build a device-resident index from a CSC doc x term score matrix.
 * Replaces: BM25v.index(doc_toks: scipy csc_matrix, doc_lengths)
 *           (bm25_native.py:59-74) and the host->device copy of the MAX path
 *           (gpu_bm25/common.py:38).
 *   indptr  [n_terms+1]  int32 (indptr_is_i64 = 0) or int64 (= 1), indptr[0]=0,
 *                        indptr[n_terms] = nnz, non-decreasing
 *   indices [nnz] int32  doc ids of each column, sorted ascending and unique
 *                        within a column (canonical CSC, as bm25s writes it)
 *   data    [nnz] f32    precomputed per-(doc, term) BM25 scores
 * The arrays are copied; the caller may free them when this returns.
 * doc_offset is added to every doc id the index returns (shards of a larger
 * collection pass the global id of their first document; 0 otherwise).
 */
int bm25_index_create(int device, int64_t n_docs, int64_t n_terms, int64_t nnz,
                      const void* indptr, int indptr_is_i64,
                      const int32_t* indices, const float* data,
                      int64_t doc_offset, bm25_index** out);

/* Release every device allocation and stream of the handle (the index
 * arrays once no fork of the handle is left). */
int bm25_index_destroy(bm25_index* idx);

/*
 * A second search context on the same device-resident index: it shares the
 * CSC arrays, segment table and tile bounds of `base` (no copy) and has its
 * own workspace, staging buffers, options (copied from base) and internal
 * stream, so searches on base and on its forks may run concurrently on
 * different streams (the doc-sharded search pipelines the parts of a batch
 * this way: bm25mi.dist.sharded_search(parts=2)).  Each handle is destroyed
 * on its own; the index arrays are released with the last one.
 * Replaces no reference call: BM25v.search is stateless per call
 * (bm25_native.py:76-158), which a fork per concurrent caller restores.
 */
int bm25_index_fork(bm25_index* base, bm25_index** out);

/* Geometry of a built index (any pointer may be NULL). */
int bm25_index_info(const bm25_index* idx, int64_t* n_docs, int64_t* n_terms,
                    int64_t* nnz, int32_t* tile_docs, int64_t* n_tiles,
                    int64_t* device_bytes);

/*
 * Segment table of a built index: *sparse = 0 for the dense
 * V x (n_tiles+1) table, 1 for per-term tile lists (chosen at create time:
 * env BM25_SEGMENTS=dense|sparse, else dense unless it would exceed twice the
 * posting arrays); *n_pairs = non-empty (term, tile) pairs held (sparse).
 */
int bm25_index_segments(const bm25_index* idx, int32_t* sparse, int64_t* n_pairs);

/*
 * Tile bounds of a built index: *has_bounds = 1 when it keeps
 * each (term, tile)'s largest score (a dense, non-negative index whose table
 * fit in device memory) — the tile-bound threshold and the REST tile skip
 * need it; *bytes = the table's device bytes.  Any pointer may be NULL.
 */
int bm25_index_bounds(const bm25_index* idx, int32_t* has_bounds, int64_t* bytes);

/*
 * Batched top-k search, host buffers, synchronous.
 * Replaces: BM25v.search / get_scores / _compute_relevance_from_scores / _topk
 *           (bm25_native.py:76-158, 204-214).
 *   queries    [Q, T] int32, negative = padding, every id < n_terms
 *   out_docs   [Q, k] int32
 *   out_scores [Q, k] f32
 * Every 0 <= k <= n_docs is served (k > 4096 by the exact large-k path: a
 * sampled threshold, the keys above it listed, selected and sorted — or
 * dense score rows with a radix selection where lists cannot serve).  That
 * path's scratch (up to a quarter of the free device memory, at most 4 GiB)
 * stays with the handle after its first such search, for the next ones,
 * until bm25_index_destroy.
 * Errors: EINVAL when a token id >= n_terms (message matches
 * bm25_native.py:118-121), when k < 0 or k > n_docs.
 */
int bm25_search(bm25_index* idx, const int32_t* queries, int64_t Q, int64_t T,
                int32_t k, int32_t* out_docs, float* out_scores);

/*
 * Same as bm25_search with device-resident queries and results, enqueued on
 * `stream` without host synchronisation (the bench's timed step: inputs
 * already resident in HBM).  Token ids are NOT validated here: ids >=
 * n_terms are treated as padding by the kernels (bm25_max_token_device is
 * the opt-in check).
 */
int bm25_search_device(bm25_index* idx, const int32_t* d_queries, int64_t Q,
                       int64_t T, int32_t k, int32_t* d_docs, float* d_scores,
                       void* stream);

/*
 * Opt-in validation of a device-resident batch: *max_token = the largest
 * token id of d_queries[Q, T] (0 when none is positive), computed on the
 * device on `stream`, which is synchronised.  A caller of bm25_search_device
 * that wants the reference's check raises when *max_token >= n_terms.
 * Replaces: bm25_native.py:91-96 (queries.max(initial=0) >= n_terms ->
 *           ValueError).
 */
int bm25_max_token_device(bm25_index* idx, const int32_t* d_queries, int64_t Q,
                          int64_t T, int32_t* max_token, void* stream);

/*
 * GPU index build: (doc, term, tf) triples + document lengths -> the CSC
 * score matrix (term-major, doc ids ascending per term = what
 * bm25_index_create and the bm25s on-disk format hold).
 * Replaces: the scoring half of the bm25s writer that produced the
 *           reference's index (animal_index_bm25/, params.index.json:1-11,
 *           bm25_test.py:19-38; method 0) and BM25.fit's matrix
 *           (bm25.py:30-121; method 1).
 *   docs/terms [n] int32, tfs [n] f32 (> 0), any order, one triple per
 *   (doc, term); doc_len [n_docs] int32; avgdl = the mean document length
 *   (bm25.py:62 / bm25s); idf [n_terms] f32 or NULL (computed on the device:
 *   ln(1 + (N - df + 0.5) / (df + 0.5)), df = triples per term);
 *   method 0 = lucene: idf * tf / (tf + k1 * (1 - b + b * dl / avgdl)),
 *   method 1 = bm25.py: idf * tf * (k1 + 1) / (tf + k1 * (1 - b + b * dl / avgdl)).
 *   Outputs (host): out_indptr [n_terms+1] int64, out_indices [n] int32,
 *   out_data [n] f32, out_data64 [n] f64 or NULL (method 1: the float64
 *   bm25_matrix entries).  Operation order and precision follow the code each
 *   method stands in for (bm25mi_build.hip), so the values are bit-identical.
 * Errors: EINVAL for ids out of range, tf <= 0, duplicate (doc, term).
 */
int bm25_build_scores(int device, int64_t n_docs, int64_t n_terms, int64_t n_triples,
                      const int32_t* docs, const int32_t* terms, const float* tfs,
                      const int32_t* doc_len, double avgdl, double k1, double b, int method,
                      const float* idf, int64_t* out_indptr, int32_t* out_indices,
                      float* out_data, double* out_data64);

/*
 * Dense per-document scores of one query (all n_docs fp32 sums, query-term
 * order, zero for untouched documents), host buffers.
 * Replaces: the dense gather+sum of the MAX graph (gpu_bm25/common.py:64-74)
 *           and BM25.get_scores (bm25.py:124-145) over a CSC index.
 */
int bm25_scores_dense(bm25_index* idx, const int32_t* query, int64_t T,
                      float* out_scores);

/*
 * Scores of given (query, document) pairs: the candidates of a reranker, the
 * documents another shard returned, a returned score to check.
 * Replaces no reference call: BM25v.search is top-k only
 * (bm25_native.py:76-158); this is the point lookup beside it.
 *   queries    [Q, T] int32 as in bm25_search (negative = padding)
 *   docs       [Q, C] int32 GLOBAL doc ids — the ids a search on this handle
 *              returns, doc_offset included; negative = padding; a document
 *              may appear several times in a row
 *   out_scores [Q, C] f32
 * out[q][c] is the fp32 sum, starting from +0.0f, over the valid token ids of
 * query q in query order (a repeated id is added each time it occurs) of the
 * index value of (term, docs[q][c]) where the document has that term: bit for
 * bit bm25_scores_dense(queries[q])[docs[q][c] - doc_offset], and therefore the
 * score bm25_search reports for that document.  Padding scores +0.0f (bits
 * 0x00000000).
 *   bm25_score_docs: host buffers, validated, synchronous; staged through
 *     device buffers of the call's own on the handle's stream.  Q == 0 or
 *     C == 0 returns BM25_OK without device work.
 *     Errors: EINVAL when a token id >= n_terms (message matches
 *     bm25_native.py:118-121, as bm25_search), when a non-negative doc id is
 *     outside [doc_offset, doc_offset + n_docs) (the message names it), for
 *     negative Q, T or C and NULL pointers with non-empty shapes.
 *   bm25_score_docs_device: device buffers, enqueued on `stream`, validates
 *     nothing and never synchronises.  Token ids >= n_terms are padding (as
 *     bm25_search_device); doc ids outside the handle's range score +0.0f —
 *     so doc shards add up: exactly one shard holds a document, the others
 *     write +0.0f, and the element-wise fp32 sum of the shards' outputs is the
 *     single-index output bit for bit.  It reads the immutable index arrays
 *     only — not the search workspace — and is not ordered against the
 *     handle's searches: it may run on its own stream while a search of the
 *     same handle is in flight on another.
 */
int bm25_score_docs(bm25_index* idx, const int32_t* queries, int64_t Q, int64_t T,
                    const int32_t* docs, int64_t C, float* out_scores);
int bm25_score_docs_device(bm25_index* idx, const int32_t* d_queries, int64_t Q, int64_t T,
                           const int32_t* d_docs, int64_t C, float* d_scores, void* stream);

/*
 * Filtered search: the top-k among the documents an allow-mask lets through
 * (a tenant, a date range, a language, "not deleted").
 * Replaces no reference call: BM25v.search has no filter
 * (bm25_native.py:76-158); the result is what its scorer and top-k give on
 * the allowed documents alone.
 *   queries    [Q, T] int32 as in bm25_search (negative = padding)
 *   masks      [M, W] uint32, W = ceil(n_docs / 32), rows contiguous: document
 *              doc_offset + d is allowed when bit d & 31 of word d >> 5 is set.
 *              Bits are indexed by the handle's own documents (a doc shard
 *              takes its slice of a collection's mask).  Bits at or past
 *              n_docs in the last word are ignored and never produce a
 *              document; no kernel reads a word at index >= W.
 *   query_mask [Q] int32: query q uses mask query_mask[q] in [0, M); -1 = no
 *              filter (the row equals bm25_search's bit for bit).  NULL = every
 *              query uses mask 0.  M == 0 is valid only when every entry is -1.
 *   out_docs / out_scores [Q, k]: row q = the first k of query q's allowed
 *              documents by (fp32 score descending, doc id ascending); scores
 *              are the bits bm25_scores_dense gives, ids are global.  Allowed
 *              documents no query term touches are candidates at +0.0f, as in
 *              bm25_search: an all-padding query returns its k smallest
 *              allowed ids, and on an index with negative values zero-score
 *              documents outrank negative ones.  Where fewer than k documents
 *              are allowed the rest of the row is padding, doc -1 / score bits
 *              0xFFFFFFFF — the padding of doc shards' lists, so the shards'
 *              filtered lists merge through bm25_merge_topk_device unchanged.
 *   0 <= k <= n_docs; k == 0 or Q == 0 returns BM25_OK without device work.
 * k <= 4096 takes the tile passes (option filter_tiles): the best allowed
 * keys of every tile — a tile without an allowed document reads no posting —
 * their k-th as the threshold, the tiles that reach it scored again into
 * per-query lists (capacity: option list_cap), sorted.  A query whose list
 * overflows, every query of k > 4096 and every query when filter_tiles is 0
 * take the dense path: dense score rows and a radix selection with the mask
 * applied.  Every path gives the same bits.
 *   bm25_search_filtered: host buffers, validated, synchronous.
 *     Errors: EINVAL when a token id >= n_terms (message matches
 *     bm25_native.py:118-121, as bm25_search), k out of range, a query_mask
 *     entry outside [-1, M), negative shapes and NULL pointers with non-empty
 *     shapes.
 *   bm25_search_filtered_device: device buffers, enqueued on `stream`,
 *     validates nothing (token ids >= n_terms are padding).  It is a search
 *     of the handle: it takes the handle's mutex and uses its workspace,
 *     ordered against the previous search's stream as bm25_search_device.  It
 *     synchronises `stream` at most once per call, after the tile passes, to
 *     count the queries handed to the dense path (as the large-k list path
 *     does); a search served by the dense path alone never synchronises.  It
 *     retains scratch with the handle, as the large-k path: 4 M (tiles + 1)
 *     bytes for the census, and — only once queries took the dense path —
 *     that path's chunk of score rows (4 B per document and query), at most
 *     the large-k scratch budget (a quarter of the free device memory at
 *     first use, at most 4 GiB).
 */
int bm25_search_filtered(bm25_index* idx, const int32_t* queries, int64_t Q, int64_t T, int32_t k,
                         const uint32_t* masks, int64_t M, const int32_t* query_mask,
                         int32_t* out_docs, float* out_scores);
int bm25_search_filtered_device(bm25_index* idx, const int32_t* d_queries, int64_t Q, int64_t T,
                                int32_t k, const uint32_t* d_masks, int64_t M,
                                const int32_t* d_query_mask, int32_t* d_docs, float* d_scores,
                                void* stream);
/* Counters of the last filtered search, the first n (1..3) of:
 *   [0] queries served by the dense path, [1] (query, tile) pairs pass A
 *   skipped because the query's mask allows no document of the tile, [2]
 *   (query, tile) pairs pass B scored again.
 * Waits for the last search, like bm25_search_stats. */
int bm25_search_filtered_stats(bm25_index* idx, int64_t* out, int32_t n);

/*
 * Weighted query terms: term boosts ("rust^2 gpu^0.5"), query expansion at
 * fractional weight, learned sparse queries (uniCOIL, SPLADE, DeepImpact: the
 * document impacts are the index values, the query is a weighted vector) and
 * negative feedback.
 * Replaces no reference call: BM25v.search takes no weights
 * (bm25_native.py:76-158).
 *   queries    [Q, T] int32 as in bm25_search (negative = padding)
 *   weights    [Q, T] f32, weights[q][j] belongs to queries[q][j]
 * The score of handle-local document d under query row q is the fold
 *     acc = +0.0f
 *     for j = 0 .. T-1, in query order:
 *       if queries[q][j] is a valid id and the index stores a posting
 *       (queries[q][j], d) with value v:
 *         p   = weights[q][j] * v    rounded to fp32 on its own
 *         acc = acc + p              a separate fp32 add: never an FMA
 *     score(q, d) = acc
 * A repeated id is added each time it occurs, each time with its own weight.
 * The weight of a padding slot (a negative id; in the device calls also an id
 * >= n_terms) is never read into a score and may hold anything, NaN included.
 * Two identities follow from the fold:
 *   - a weight of exactly 1.0f gives p == v, so a row of all-1.0f weights has
 *     the bits of bm25_search_filtered — and of bm25_search, bm25_scores_dense
 *     and bm25_score_docs;
 *   - a weight of +0.0f or -0.0f leaves acc as it is (acc starts at +0.0f and
 *     never becomes -0.0f), so weight 0.0f is bit for bit the same as padding.
 * Weights must be finite.  The host calls reject a non-finite weight on a
 * non-padding slot with BM25_EINVAL (the message names row, column and
 * value).  The device calls validate nothing: a row with a non-finite weight
 * has unspecified contents, the other rows are unaffected and nothing outside
 * the caller's buffers is read or written.
 * Documents no valid term touches are candidates at +0.0f, as everywhere
 * else; with negative weights zero-score documents outrank negative ones.
 * Order: score descending, then doc id ascending; padding is doc -1 / score
 * bits 0xFFFFFFFF.
 *
 *   bm25_search_weighted(_device): bm25_search_filtered(_device) with the fold
 *     above in place of the plain sum.  masks [M, W], query_mask [Q] (-1 = no
 *     filter), padding rows, 0 <= k <= n_docs, the filter_tiles and list_cap
 *     options, the one possible stream synchronisation, the retained scratch
 *     and bm25_search_filtered_stats are as documented there.  One
 *     difference: with M == 0 a NULL query_mask means "no filter for every
 *     query" (the common case needs no array of -1); with M >= 1 NULL still
 *     means mask 0.  The search always takes the filtered search's exact
 *     passes; the tile-bound threshold of bm25_search is not used: weight *
 *     bound is no upper bound of weight * value when the weight is negative,
 *     and those passes need no bound (their threshold is a candidate's own
 *     key), so they are exact for weights and values of either sign.
 *     bm25_search_dispatch reports the flag 8192 after a weighted search.
 *     Host call: validates as bm25_search_filtered, plus the finite-weight
 *     rule.  Device call: shapes and NULL pointers only; token ids >= n_terms
 *     are padding.
 *   bm25_score_docs_weighted(_device): bm25_score_docs(_device) under the same
 *     fold: out[q][c] is bit for bit the score bm25_search_weighted reports
 *     for docs[q][c].  A posting that is absent adds +0.0f (not weight * 0).
 *     The device call keeps the properties of bm25_score_docs_device: it reads
 *     the index arrays only, is not ordered against the handle's searches,
 *     never synchronises, and doc ids outside the handle's range score +0.0f,
 *     so doc shards' outputs add up element-wise.  Host call: validates as
 *     bm25_score_docs, plus the finite-weight rule.
 * Subnormal products follow the device's fp32 denormal mode.
 */
int bm25_search_weighted(bm25_index* idx, const int32_t* queries, const float* weights, int64_t Q,
                         int64_t T, int32_t k, const uint32_t* masks, int64_t M,
                         const int32_t* query_mask, int32_t* out_docs, float* out_scores);
int bm25_search_weighted_device(bm25_index* idx, const int32_t* d_queries, const float* d_weights,
                                int64_t Q, int64_t T, int32_t k, const uint32_t* d_masks,
                                int64_t M, const int32_t* d_query_mask, int32_t* d_docs,
                                float* d_scores, void* stream);
int bm25_score_docs_weighted(bm25_index* idx, const int32_t* queries, const float* weights,
                             int64_t Q, int64_t T, const int32_t* docs, int64_t C,
                             float* out_scores);
int bm25_score_docs_weighted_device(bm25_index* idx, const int32_t* d_queries,
                                    const float* d_weights, int64_t Q, int64_t T,
                                    const int32_t* d_docs, int64_t C, float* d_scores,
                                    void* stream);

/*
 * Cursor pagination ("search after"): the next k results after a given
 * (score, doc) pair — exact deep paging for export jobs, infinite scroll,
 * rerankers that pull candidates until a budget is spent and doc shards that
 * resume a scan — at the cost of a k-sized search instead of a search of the
 * whole prefix.
 * Replaces no reference call: BM25v.search has no cursor
 * (bm25_native.py:76-158).
 *   queries, weights, masks, M, query_mask, k, out_docs / out_scores: exactly
 *              bm25_search_weighted(_device).  weights may be NULL: plain
 *              sums, bit for bit what a row of 1.0f weights gives.  With
 *              M == 0 a NULL query_mask means no filter for every query; with
 *              M >= 1 NULL means mask 0; -1 = no filter for that row.
 *              0 <= k <= n_docs.  Padding is doc -1 / score bits 0xFFFFFFFF.
 *   after_scores [Q] f32, after_docs [Q] int32: one cursor (s, c) per query
 *              row, c a global doc id.  A document d (handle-local, allowed by
 *              the row's mask) is eligible iff
 *                  score_key(score(q, d)) <  score_key(s), or
 *                  score_key(score(q, d)) == score_key(s) and doc_offset + d > c
 *              compared in 64 bits: a c outside [doc_offset, doc_offset +
 *              n_docs) is legal and means what the inequality says, so every
 *              doc shard of a collection searches after the collection's
 *              cursor and the shards' lists merge through
 *              bm25_merge_topk_device unchanged.  The cursor need not name an
 *              existing or an allowed document.  Row q is the first k eligible
 *              documents in the usual order (score descending, doc id
 *              ascending), padded where fewer exist.
 *              score_key is the engine's order of fp32 scores: the numeric
 *              order, with -0.0f just below +0.0f.  Returned scores are never
 *              -0.0f, so a cursor taken from a result never is.
 *   after_docs[q] == BM25_AFTER_NONE (-2): no cursor; after_scores[q] is not
 *              read and the row is bit for bit bm25_search_weighted's.
 *   after_docs[q] == -1 (the doc id of a padding slot): the previous page ended
 *              in padding, so the list is exhausted: the row is all padding
 *              and no posting is read for it.  Feeding the last column of any
 *              page back in is therefore always safe; -1 never means
 *              "restart".
 *   Both after_* pointers NULL: no cursor for every row.  Exactly one NULL:
 *              BM25_EINVAL.
 * The search takes the filtered search's passes with the cursor as one more
 * per-document predicate (their threshold is an eligible document's own key,
 * so they stay exact); the dense path clamps a row to its eligible documents.
 * Every path gives the same bits.  A row with an exhausted cursor counts in
 * bm25_search_filtered_stats [1] once per tile (pass A skips it as it skips an
 * empty census).
 *   bm25_search_after: host buffers, validated, synchronous.  Validates as
 *     bm25_search_weighted (the finite-weight rule when weights are given),
 *     plus: an after_docs entry < -2, and a NaN after_scores entry on a row
 *     with after_docs >= 0, give BM25_EINVAL (the message names row and
 *     value).
 *   bm25_search_after_device: device buffers, enqueued on `stream`; checks
 *     shapes and NULL pointers only.  An after_docs entry < -1 is "no cursor".
 *     A row with a NaN cursor score has unspecified contents, the other rows
 *     are unaffected and nothing outside the caller's buffers is read or
 *     written (the rule of a non-finite weight).
 * Both are searches of the handle: mutex, workspace, stream ordering, the one
 * possible synchronisation, the retained scratch (plus 8 + 4 T bytes per query
 * for the cursor keys and the query copy) and bm25_search_filtered_stats are
 * as documented for bm25_search_filtered.  bm25_search_dispatch reports the
 * flag 16384 after a search through either call, whatever its cursors, with
 * 4096 / 64 / 8192 as the passes taken.
 */
#define BM25_AFTER_NONE (-2) /* after_docs[q]: no cursor, row q starts at rank 1 */
int bm25_search_after(bm25_index* idx, const int32_t* queries, const float* weights, int64_t Q,
                      int64_t T, int32_t k, const uint32_t* masks, int64_t M,
                      const int32_t* query_mask, const float* after_scores,
                      const int32_t* after_docs, int32_t* out_docs, float* out_scores);
int bm25_search_after_device(bm25_index* idx, const int32_t* d_queries, const float* d_weights,
                             int64_t Q, int64_t T, int32_t k, const uint32_t* d_masks, int64_t M,
                             const int32_t* d_query_mask, const float* d_after_scores,
                             const int32_t* d_after_docs, int32_t* d_docs, float* d_scores,
                             void* stream);

/*
 * Field collapsing (result diversification): at most per_group hits of every
 * group in a row's top-k — "one hit per site", "at most two per author" —
 * exact, on the device.  Over-fetching k x results and deduplicating on the
 * host is wrong whenever one group holds more than k x of the best documents.
 * Replaces no reference call: BM25v.search has no grouping
 * (bm25_native.py:76-158).
 *   queries, weights, masks, M, query_mask, out_docs / out_scores: exactly
 *              bm25_search_after(_device): weights may be NULL (plain sums);
 *              with M == 0 a NULL query_mask means no filter, with M >= 1 it
 *              means mask 0; -1 = no filter for that row.
 *   groups [n_docs] int32, by the handle's own documents: a value >= 0 is the
 *              document's group, any non-negative int32 (there is no group
 *              count and no table of groups: a hashed host name works; the
 *              codes of bm25mi.facet_codes work too); a value < 0: the document
 *              has no group.
 *   per_group >= 1: the most hits of one group in a row.
 * Row q: take the full result order of bm25_search_weighted under the row's
 * mask (fp32 score descending, doc id ascending, zero-score allowed documents
 * included) and walk it from rank 1 with a counter per group value:
 *   a document with groups[d] < 0 is always kept;
 *   a document with groups[d] = g >= 0 is kept iff fewer than per_group
 *              documents of g were kept before it, and then g's counter goes up;
 *   the row is the first k kept documents as (doc + doc_offset, score bits),
 *              padded (doc -1 / score bits 0xFFFFFFFF) where fewer are kept.
 * per_group >= k changes nothing: with it, with all groups negative or all
 * distinct, every row is bit for bit bm25_search_weighted's (bm25_search's
 * under NULL weights and no mask).  Returned scores are never -0.0f.
 *   out_groups [Q, k] int32, optional (NULL: not wanted): groups[d] of each
 *              hit, -1 in padding (a hit without a group reads as its own
 *              negative value).  A doc-shard merge needs it.
 *   0 <= k <= min(n_docs, 4096).  k > 4096 is BM25_EINVAL: collapse is limited
 *              to 4096 because the per-row group table lives in LDS (8192 slots
 *              of (group, count), 64 KiB).  k == 0 or Q == 0: BM25_OK, no
 *              device work.
 *   There is no cursor argument: paging collapsed results is out of scope (the
 *              next page depends on the groups the earlier pages filled, which
 *              a (score, doc) cursor does not carry).
 * Doc shards: groups are by the handle's own documents and the ids come back
 * global.  A document of the collection's collapsed top-k is inside its
 * shard's collapsed top-k, so the shards' (doc, score, group) lists merged in
 * key order and collapsed once more are exact:
 * bm25_merge_collapsed_device below does that on the device, and
 * bm25mi.dist.sharded_search_collapsed is the search on top of it.
 * How: rounds.  Round 1 is one cursor-search page of p results for every row
 * (option "collapse_page"), walked in rank order against the row's group
 * counters.  The rows that are neither full nor out of documents go on in
 * compact sub-batches (option "collapse_chunk"): each round a page after the
 * row's cursor under the row's mask minus every document of a saturated
 * group, built on the device.  Such a round keeps at least one new hit, and
 * where it leaves the row unfinished it saturated a new group: at most k + 1
 * rounds a row; a filter that leaves one group ends in two.  Every round
 * synchronises `stream` once, to read the number of unfinished rows (beside
 * the filtered search's own possible synchronisation).
 * Memory: the handle retains 8 p + 16 bytes per row of the largest batch
 * (pages, cursors, counts, row ids; + 4 k where out_groups is NULL), like the
 * large-k scratch; the rounds under exclusion masks take a buffer of the
 * call's own, (8 T + 12 + 4 ceil(n_docs / 32)) bytes per sub-batch row, at
 * most 1 GiB of mask words by default, released before the call returns.
 *   bm25_search_collapsed: host buffers, validated, synchronous.  Validates as
 *     bm25_search_after (token ids, finite weights, query_mask range, shapes,
 *     NULLs); in addition NULL groups, per_group < 1 and k > 4096 are
 *     BM25_EINVAL and the message names the value.  On an error the outputs
 *     are untouched.
 *   bm25_search_collapsed_device: device buffers, enqueued on `stream` (and
 *     synchronising it as said above); checks shapes, NULLs, k > 4096 and
 *     per_group < 1 only.
 *   bm25_search_collapsed_stats: the first n (1..4) of, for the handle's last
 *     collapsed search: [0] rounds (the most any row took), [1] rows
 *     unfinished after round 1, [2] page entries dropped as over-quota (ahead
 *     of their row's last hit), [3] rows served under exclusion masks, summed
 *     over the rounds.  No device wait.
 * Both are searches of the handle: mutex, workspace and stream ordering as
 * bm25_search_after.  bm25_search_dispatch reports the flag 262144 after a
 * search through either call, with 16384 / 4096 / 64 / 8192 as the last round
 * set them; bm25_search_filtered_stats describes the last round.  Results
 * never depend on "collapse_page" or "collapse_chunk".
 */
int bm25_search_collapsed(bm25_index* idx, const int32_t* queries, const float* weights,
                          int64_t Q, int64_t T, int32_t k, const uint32_t* masks, int64_t M,
                          const int32_t* query_mask, const int32_t* groups, int32_t per_group,
                          int32_t* out_docs, float* out_scores, int32_t* out_groups);
int bm25_search_collapsed_device(bm25_index* idx, const int32_t* d_queries,
                                 const float* d_weights, int64_t Q, int64_t T, int32_t k,
                                 const uint32_t* d_masks, int64_t M, const int32_t* d_query_mask,
                                 const int32_t* d_groups, int32_t per_group, int32_t* d_docs,
                                 float* d_scores, int32_t* d_groups_out, void* stream);
int bm25_search_collapsed_stats(bm25_index* idx, int64_t* out, int32_t n);

/*
 * Boolean term filters: the allow-masks of "+rust -java" — must contain all
 * of these terms, at least one of those, none of these — built on the device
 * from the index's own postings, in exactly the layout
 * bm25_search_filtered_device reads.
 * Replaces no reference call: BM25v.search has no term filter
 * (bm25_native.py:76-158).
 *   has(t, d) is true when the CSC index stores a posting for (term t,
 *   handle-local document d); a stored 0.0f or a negative value counts.
 *   Mask row m, from three clause rows of token ids and an optional base mask:
 *     allowed(m, d) =  d < n_docs
 *                  and base(m, d)                              (absent base: true)
 *                  and for every id t >= 0 in must[m]:      has(t, d)
 *                  and (any[m] holds no id >= 0  or  some id t >= 0 in any[m] has(t, d))
 *                  and no id t >= 0 in must_not[m]:         has(t, d)
 *   must [M, A], any [M, B], must_not [M, N] int32, rows contiguous.  Negative
 *              ids are padding; duplicate ids are harmless; a width of 0 (the
 *              pointer may then be NULL) is an empty clause.  A term in both
 *              must and must_not gives an empty mask; all three clauses empty
 *              give base, or every document when there is no base.
 *   base       [Mb, W] uint32, Mb = 0 (NULL: no base), 1 (applied to every
 *              row) or M; the bit layout of bm25_search_filtered: document d
 *              at bit d & 31 of word d >> 5, handle-local documents.
 *   out_masks  [M, W] uint32, W = ceil(n_docs / 32).  Every word of every row
 *              is written (the caller need not zero the buffer); the bits at
 *              or past n_docs of the last word are written 0 even where base
 *              has them set; no word at index >= W of a row is read or
 *              written, nothing past M * W words is touched.
 * Memory: the masks take M * W * 4 bytes — 1.25 MB per mask at 10M documents;
 * built here they never cross the host link.
 * Doc shards: bits are by the handle's own documents, so a shard builds its
 * slice of the collection's mask from its own postings, and the shards'
 * filtered lists still merge through bm25_merge_topk_device unchanged.
 *   bm25_term_masks: host buffers, validated, synchronous; staged through
 *     device buffers of the call's own.  M == 0 returns BM25_OK without device
 *     work.  Errors: EINVAL for a NULL index, negative shapes, NULL pointers
 *     with non-empty shapes, Mb not in {0, 1, M}, and an id >= n_terms (the
 *     message matches bm25_native.py:118-121, as bm25_search).
 *   bm25_term_masks_device: device buffers, enqueued on `stream`; validates no
 *     id and never synchronises (shapes and NULL pointers are checked as
 *     above).  Here an id >= n_terms is a term that no document has: in must
 *     it empties the row, in any it makes the clause active and matches
 *     nothing, in must_not it removes nothing — on purpose NOT the "padding"
 *     of bm25_search_device, where dropping an unknown term only loses its
 *     score; dropping it from must would let every document through.  The call
 *     reads the immutable index arrays only — not the search workspace — and
 *     is not ordered against the handle's searches: it may run on its own
 *     stream while a search of the same handle is in flight on another (as
 *     bm25_score_docs_device).  No global atomics, no scratch: the result
 *     does not depend on scheduling.
 *   bm25_search_boolean: bm25_search_filtered under the masks of Q clause
 *     rows (M = Q, Mb in {0, 1, Q}), host buffers, validated, synchronous: row
 *     q is bit for bit the row bm25_search_filtered returns for query q under
 *     the mask of clause row q, padding included (doc -1 / score bits
 *     0xFFFFFFFF where fewer than k documents qualify).  The masks are built
 *     on the device and never move to the host.  The batch is served in
 *     chunks of queries so that the call's mask buffer — its own, allocated
 *     and released inside the call — stays bounded: option "bool_chunk"
 *     queries per chunk, automatically at most 1 GiB of mask words and at
 *     least one query.  Errors: those of bm25_search_filtered and of
 *     bm25_term_masks.
 */
int bm25_term_masks(bm25_index* idx, const int32_t* must, int64_t A, const int32_t* any, int64_t B,
                    const int32_t* must_not, int64_t N, int64_t M, const uint32_t* base,
                    int64_t Mb, uint32_t* out_masks);
int bm25_term_masks_device(bm25_index* idx, const int32_t* d_must, int64_t A, const int32_t* d_any,
                           int64_t B, const int32_t* d_must_not, int64_t N, int64_t M,
                           const uint32_t* d_base, int64_t Mb, uint32_t* d_out_masks,
                           void* stream);
int bm25_search_boolean(bm25_index* idx, const int32_t* queries, int64_t Q, int64_t T, int32_t k,
                        const int32_t* must, int64_t A, const int32_t* any, int64_t B,
                        const int32_t* must_not, int64_t N, const uint32_t* base, int64_t Mb,
                        int32_t* out_docs, float* out_scores);

/*
 * Minimum-should-match and hit counts: "at least m of these terms" in the any
 * clause of the boolean term filters, and the number of documents a mask
 * allows, both on the device.  Replaces no reference call.
 *   The definitions of "Boolean term filters" above hold as they are.  One
 *   more input per row, min_match [M] int32, changes only the any line of
 *   allowed(m, d):
 *     n_any(m)    = number of slots j of any[m] with any[m][j] >= 0
 *     count(m, d) = number of slots j with any[m][j] >= 0 and has(any[m][j], d)
 *     any-clause(m, d) =  n_any(m) == 0        (no id: the clause is absent,
 *                                               min_match[m] is not read into the result)
 *                      or min_match[m] <= 0    (the clause is optional: no constraint)
 *                      or count(m, d) >= min_match[m]
 *   Every non-negative slot is a clause of its own: a repeated id counts each
 *   time it occurs (as a repeated query id is scored each time it occurs), so
 *   any = [t, t] with min_match 2 is has(t, .); duplicates stay harmless at
 *   min_match 1.  min_match[m] > n_any(m) allows no document: the row is all
 *   zeros and no posting is read for it.  min_match[m] == 1, or a NULL
 *   min_match pointer: the row is bit for bit bm25_term_masks' row.  must,
 *   must_not, base (Mb in {0, 1, M}), the cleared tail bits, "every word of
 *   every row is written" and "nothing at index >= W is touched" are unchanged.
 *   bm25_term_masks_min_match: bm25_term_masks with min_match; host buffers,
 *     validated, synchronous.  Errors: those of bm25_term_masks;
 *     min_match[m] < 0 (the message names row and value); B > 65535 together
 *     with a non-NULL min_match (the width of the per-document counter).
 *     M == 0 returns BM25_OK without device work.
 *   bm25_term_masks_min_match_device: bm25_term_masks_device with
 *     d_min_match [M] on the device; checks shapes (B > 65535 with a non-NULL
 *     d_min_match among them) and NULL pointers only, never synchronises,
 *     retains no scratch, reads the immutable index arrays only and is not
 *     ordered against the handle's searches.  An entry <= 0 means "optional".
 *     An id >= n_terms in any is, as there, a term that no document has: it
 *     counts in n_any and never in count.
 *   bm25_mask_count / bm25_mask_count_device: masks [M, W] uint32 ->
 *     out_counts [M] int64, out_counts[m] = the number of set bits of row m
 *     among bits 0 .. n_docs - 1.  Bits at or past n_docs in the last word
 *     are ignored even when set (a caller's own mask may carry garbage there;
 *     the search ignores those bits too).  The caller need not zero the
 *     counts; M may pass 65535; the result is an integer sum and does not
 *     depend on scheduling.  On doc shards the bits are the handle's own
 *     documents, so the shards' counts add up to the collection's.  The
 *     device call reads the caller's masks only, never synchronises, retains
 *     no scratch and is not ordered against the handle's searches.
 *   Neither the mask calls nor the counts are searches: they leave
 *   bm25_search_dispatch, the counters and bm25_search_filtered_stats alone.
 *   bm25_search_boolean_min_match: bm25_search_boolean with the new clause:
 *     row q is bit for bit bm25_search_filtered's row under the mask of clause
 *     row q, and out_total_hits [Q] int64 (or NULL) receives that mask's
 *     count.  Same chunking (option "bool_chunk", at most 1 GiB of mask
 *     words); each chunk's counts are taken on the device before its mask
 *     buffer is reused, so the masks still never move to the host.  k == 0
 *     with a non-NULL out_total_hits still builds and counts the masks ("how
 *     many match" is a query of its own; queries, out_docs and out_scores may
 *     then be NULL).  With min_match NULL and out_total_hits NULL the outputs
 *     equal bm25_search_boolean's.
 */
int bm25_term_masks_min_match(bm25_index* idx, const int32_t* must, int64_t A, const int32_t* any,
                              int64_t B, const int32_t* must_not, int64_t N,
                              const int32_t* min_match, int64_t M, const uint32_t* base,
                              int64_t Mb, uint32_t* out_masks);
int bm25_term_masks_min_match_device(bm25_index* idx, const int32_t* d_must, int64_t A,
                                     const int32_t* d_any, int64_t B, const int32_t* d_must_not,
                                     int64_t N, const int32_t* d_min_match, int64_t M,
                                     const uint32_t* d_base, int64_t Mb, uint32_t* d_out_masks,
                                     void* stream);
int bm25_mask_count(bm25_index* idx, const uint32_t* masks, int64_t M, int64_t* out_counts);
int bm25_mask_count_device(bm25_index* idx, const uint32_t* d_masks, int64_t M, int64_t* d_counts,
                           void* stream);
int bm25_search_boolean_min_match(bm25_index* idx, const int32_t* queries, int64_t Q, int64_t T,
                                  int32_t k, const int32_t* must, int64_t A, const int32_t* any,
                                  int64_t B, const int32_t* must_not, int64_t N,
                                  const int32_t* min_match, const uint32_t* base, int64_t Mb,
                                  int32_t* out_docs, float* out_scores, int64_t* out_total_hits);

/*
 * Facet counts: the hit count of every allow-mask broken down by a
 * per-document field (a "terms aggregation": how many match per language,
 * tenant, year or source), on the device.  Replaces no reference call.
 *   groups [n_docs] int32: groups[d] = the group (category id) of handle-local
 *              document d, in [0, G); a negative value = the document has no group.
 *   masks  [M, W] uint32, W = ceil(n_docs / 32), the layout of bm25_search_filtered.
 *   out    [M, G] int64, rows contiguous:
 *     out[m][g] = number of d in [0, n_docs) with bit d of mask row m set and groups[d] == g
 *   Every entry of out is written; the caller need not zero it.  Bits at or
 *   past n_docs in the last word are ignored even when set.  No mask word at
 *   index >= W of a row is read, no entry of groups at index >= n_docs is
 *   read, nothing past M * G counts is written.  M may pass 65535; G == 0 or
 *   M == 0 returns BM25_OK without device work; G lies in [0, 2^31 - 1].  The
 *   sums are integer, so the result does not depend on scheduling.
 *   Identity: sum_g out[m][g] + (allowed documents of row m with a negative
 *   group) == bm25_mask_count of row m.  On doc shards the bits and the groups
 *   are by the handle's own documents, so the shards' [M, G] outputs add up
 *   element-wise to the collection's.
 *   The facet calls are not searches: they leave bm25_search_dispatch,
 *   bm25_search_counters and bm25_search_filtered_stats alone.
 *   bm25_mask_facets: host buffers, validated, synchronous.  BM25_EINVAL for
 *     a NULL index, a negative M or G (or G > 2^31 - 1), a NULL pointer with a
 *     non-empty shape, and a groups[d] >= G (the message names d and the
 *     value).  On any error the outputs are untouched.
 *   bm25_mask_facets_device: device buffers, enqueued on `stream`; checks
 *     shapes and NULL pointers only, never synchronises, retains no scratch,
 *     reads the caller's masks and groups only (no workspace, no index array)
 *     and is not ordered against the handle's searches: it may run on its own
 *     stream while a search of the same handle is in flight, as
 *     bm25_mask_count_device may.  A groups[d] >= G counts nowhere, exactly
 *     like a negative value; nothing outside the caller's buffers is touched.
 *   bm25_search_boolean_facets: bm25_search_boolean_min_match plus the
 *     per-query facet rows, out_facets [Q, G] int64 = the facet counts of each
 *     query's mask.  The groups (validated as bm25_mask_facets validates them)
 *     are uploaded once per call; each chunk's facets are taken on the device
 *     where its hit counts are taken, before its mask buffer is reused, so the
 *     masks still never move to the host.  k == 0 with a non-NULL out_facets or
 *     out_total_hits builds the masks and counts alone (queries, out_docs and
 *     out_scores may then be NULL).  With groups NULL and out_facets NULL every
 *     output equals bm25_search_boolean_min_match's, which is this call
 *     without them; exactly one of the two with G > 0 is BM25_EINVAL.
 */
int bm25_mask_facets(bm25_index* idx, const uint32_t* masks, int64_t M, const int32_t* groups,
                     int64_t G, int64_t* out_counts);
int bm25_mask_facets_device(bm25_index* idx, const uint32_t* d_masks, int64_t M,
                            const int32_t* d_groups, int64_t G, int64_t* d_counts, void* stream);
int bm25_search_boolean_facets(bm25_index* idx, const int32_t* queries, int64_t Q, int64_t T,
                               int32_t k, const int32_t* must, int64_t A, const int32_t* any,
                               int64_t B, const int32_t* must_not, int64_t N,
                               const int32_t* min_match, const uint32_t* base, int64_t Mb,
                               const int32_t* groups, int64_t G, int32_t* out_docs,
                               float* out_scores, int64_t* out_total_hits, int64_t* out_facets);

/*
 * Numeric range filters: allow-masks made on the device from per-document
 * numeric fields (a date range, a price range, a tenant id), the one common
 * filter that otherwise has to be compared and packed on the host.  Replaces
 * no reference call.
 *
 *   values  [F, n_docs]  one dtype per call, rows contiguous: values[f][d] = field f of
 *                        handle-local document d.  kind: BM25_FIELD_I32 (0) int32,
 *                        BM25_FIELD_F32 (1) float32, BM25_FIELD_I64 (2) int64.
 *   fields  [M, C] int32 clause c of mask row m tests field fields[m][c]; negative = padding
 *   lo, hi  [M, C]       of the values' dtype: the clause's bounds, both inclusive
 *   base    [Mb, W]      Mb = 0 (NULL), 1 or M — exactly bm25_term_masks' base
 *   out     [M, W] uint32, W = ceil(n_docs / 32), the layout of bm25_search_filtered
 *
 *   allowed(m, d) = d < n_docs and base(m, d)
 *                   and for every c with fields[m][c] >= 0:
 *                       lo[m][c] <= values[fields[m][c]][d] <= hi[m][c]
 *
 *   Comparisons are the dtype's own: int64 is compared as int64, never through
 *   a float.  float32 is compared as IEEE: a NaN value fails every clause, and
 *   -0.0f equals +0.0f.  Bounds may be +-inf or the integer limits: these are
 *   the open ends.  lo > hi is an empty clause, and the row is all zeros.  A
 *   row with no clause gives base, or every document when there is no base.
 *   Clauses of one row are ANDed; several clauses may name the same field.
 *   The mask guarantees of bm25_term_masks hold: Every word of every row is
 *   written.  Bits at or past n_docs of the last word are written 0 even where
 *   base has them set.  No word at index >= W of a row is read or written.  No
 *   values entry at index >= n_docs of a field row is read.  M may pass 65535.
 *   There are no global atomics and no scratch; the result does not depend on
 *   scheduling.  base and out must not overlap.
 *   Doc shards: values and bits are by the handle's own documents, so a shard
 *   builds its slice of the collection's mask.
 *   None of the three calls is a search on its own: bm25_range_masks and
 *   bm25_range_masks_device leave bm25_search_dispatch, bm25_search_counters
 *   and bm25_search_filtered_stats alone.
 *   bm25_range_masks: host buffers, validated, synchronous.  BM25_EINVAL for a
 *     NULL index, a bad kind, negative shapes, NULL pointers with non-empty
 *     shapes, Mb not in {0, 1, M}, a fields entry >= F (the message names row,
 *     column and value) and, float32 only, a NaN bound on a non-padding clause
 *     (the message names it).  On any error the outputs are untouched.
 *     M == 0 returns BM25_OK without device work.
 *   bm25_range_masks_device: device buffers, enqueued on `stream`; checks
 *     shapes and NULL pointers only, never synchronises, retains no scratch,
 *     reads the caller's buffers only (no workspace, no index array) and is
 *     not ordered against the handle's searches, as bm25_mask_facets_device is
 *     not.  A field id >= F is a field that no document has: the clause
 *     matches nothing and nothing out of bounds is read (the rule of an unknown
 *     term in must, for the same reason).  A NaN bound matches nothing, which
 *     is what the comparison gives anyway.
 *   bm25_search_boolean_ranges: bm25_search_boolean_facets plus (values, kind,
 *     F, fields, lo, hi, C) with the rows [Q, C]: row q is, bit for bit, the
 *     row bm25_search_filtered returns under the mask range(q) AND term
 *     clauses(q) AND base; totals and facets are taken of that same mask.  The
 *     columns (validated as bm25_range_masks validates them) go up once per
 *     call; each chunk's range masks are built on the device into a second
 *     buffer of the call's own, which is the chunk's per-row base of the term
 *     masks, so the masks still never move to the host.  With ranges present
 *     the automatic chunk halves, so the two buffers together stay within
 *     1 GiB; an explicit bool_chunk keeps its meaning, queries per chunk.  With
 *     F == 0, C == 0 or NULL values the call is bm25_search_boolean_facets,
 *     chunk size included, which is this call without them.
 */
enum { BM25_FIELD_I32 = 0, BM25_FIELD_F32 = 1, BM25_FIELD_I64 = 2 };
int bm25_range_masks(bm25_index* idx, const void* values, int32_t kind, int64_t F,
                     const int32_t* fields, const void* lo, const void* hi, int64_t C, int64_t M,
                     const uint32_t* base, int64_t Mb, uint32_t* out_masks);
int bm25_range_masks_device(bm25_index* idx, const void* d_values, int32_t kind, int64_t F,
                            const int32_t* d_fields, const void* d_lo, const void* d_hi, int64_t C,
                            int64_t M, const uint32_t* d_base, int64_t Mb, uint32_t* d_out_masks,
                            void* stream);
int bm25_search_boolean_ranges(bm25_index* idx, const int32_t* queries, int64_t Q, int64_t T,
                               int32_t k, const int32_t* must, int64_t A, const int32_t* any,
                               int64_t B, const int32_t* must_not, int64_t N,
                               const int32_t* min_match, const uint32_t* base, int64_t Mb,
                               const int32_t* groups, int64_t G, const void* values, int32_t kind,
                               int64_t F, const int32_t* fields, const void* lo, const void* hi,
                               int64_t C, int32_t* out_docs, float* out_scores,
                               int64_t* out_total_hits, int64_t* out_facets);

/*
 * Field statistics: count, min, max and exact sum of a per-document column
 * over the documents every allow-mask allows, per mask row and per group (a
 * "stats" aggregation, and the "terms" + avg / min / max sub-aggregation:
 * price range and average price of the hits, average rating per category,
 * oldest and newest matching document per tenant), on the device.  Replaces no
 * reference call.
 *   masks  [M, W] uint32, W = ceil(n_docs / 32), the layout of bm25_search_filtered.
 *          Bits at or past n_docs are ignored even when set.  No word at
 *          index >= W of a row is read.
 *   values [n_docs] of kind (BM25_FIELD_I32 / _F32 / _I64), by the handle's own
 *          documents.  No entry at index >= n_docs is read.
 *   groups [n_docs] int32 with G buckets.  groups == NULL and G == 0 together
 *          mean one bucket per row that holds every allowed document; write
 *          B = 1.  Otherwise B = G.  A document with a negative group, or in
 *          the device call a group >= G, is in no bucket.  Exactly one of
 *          (groups == NULL, G == 0) is BM25_EINVAL.
 *   A document d contributes to bucket (m, b) if and only if bit d of row m is
 *   set, its bucket is b, and its value is a number: for float32, NaN is "no
 *   value", the rule of the sort and range calls; +-inf are numbers.
 *   Outputs, all [M, B], rows contiguous.  Every entry is written and the
 *   caller need not clear them.  Nothing past M * B entries is touched.
 *     out_count int64: the number of contributing documents.
 *     out_min, out_max of the column's dtype.  The comparison is the dtype's
 *       own: int64 never goes through a float; float32 is compared by the
 *       order key of "Sort-by-field search over doc shards" below, so
 *       -0.0f == +0.0f, and a zero result is written as +0.0f.
 *     out_sum: int32 column: int64, the exact sum.  int64 column: int64, the
 *       sum modulo 2^64 (numpy's sum(dtype=int64)).  float32 column: float64,
 *       the exact real sum of the finite contributing values rounded to
 *       nearest-even once; +0.0 when that sum is zero or nothing contributes;
 *       if +inf contributes and -inf does not, +inf; the mirror case gives
 *       -inf; both contributing gives NaN.  The sum cannot overflow: fewer
 *       than 2^32 addends below 2^128.
 *     Where out_count is 0, min, max and sum are written as 0 of their type.
 *     out_min, out_max and out_sum may each be NULL (not wanted); out_count is
 *     required.
 *   The float32 sum is computed with integer accumulators only: a finite value
 *   of biased exponent e is sig * 2^(E - 150) with E = max(e, 1) and sig the
 *   24-bit significand (the 23-bit field when e = 0); it adds
 *   +-(sig << (E & 7)), a magnitude below 2^31, to int64 bin E >> 3 of its
 *   bucket's 32 bins.  A bin of weight 2^(8 b - 150) cannot overflow int64
 *   below 2^32 addends.  The bins are carry-normalised from low to high into a
 *   signed multi-limb integer whose magnitude's top 53 bits are rounded to
 *   nearest-even on the rest, once.  Count, sums and bins are integer adds,
 *   min and max are integer maxima of order keys: there are no float atomics,
 *   and the result does not depend on scheduling — it is bit-identical across
 *   runs, streams, grids and routes, and Python's math.fsum is its oracle.
 *   Identities: with no NaN in the column, ungrouped out_count ==
 *   bm25_mask_count; with no NaN in the column, grouped out_count ==
 *   bm25_mask_facets; for integer kinds, sum_g out_sum[m][g] plus the sum over
 *   the allowed documents without a group == the ungrouped sum, in wrapping
 *   int64.
 *   Doc shards: values, groups and bits are by the handle's own documents.
 *   Counts add, min and max combine, integer sums add (wrapping).  The float32
 *   sums of shards are each rounded once: their float64 sum is not bit-equal
 *   to the collection's.
 *   The stats calls are not searches: they leave bm25_search_dispatch,
 *   bm25_search_counters and bm25_search_filtered_stats alone.
 *   bm25_mask_stats_scratch: *bytes = the scratch of the device call for
 *     (kind, M, G) = 8 * M * B * (36 for float32, 4 for the integer kinds): at
 *     most 288 bytes per bucket plus a constant (the constant is 0 today).
 *   bm25_mask_stats: host buffers, validated, synchronous; allocates its
 *     scratch itself.  BM25_EINVAL for a NULL index, a bad kind, a negative M
 *     or G (or G > 2^31 - 1), a NULL pointer with a non-empty shape, the
 *     groups / G mismatch above, and a groups[d] >= G (the message names d and
 *     the value, as bm25_mask_facets does).  On any error the outputs are
 *     untouched.  M == 0 returns BM25_OK without device work; n_docs == 0
 *     writes zeros.
 *   bm25_mask_stats_device: device buffers, enqueued on `stream`; checks
 *     shapes, NULL pointers, the kind and scratch_bytes >=
 *     bm25_mask_stats_scratch(...) (d_scratch 8-byte aligned), never
 *     synchronises, retains nothing, reads the caller's buffers only (no
 *     workspace, no index array) and is not ordered against the handle's
 *     searches: it may run on its own stream while a search of the same handle
 *     is in flight.  M may pass 65535.
 *   Out of scope: a stats= argument of the boolean search (the device calls
 *   compose: bm25_term_masks_device -> bm25_mask_stats_device), a sharded or
 *   distributed form, percentiles, variance and histograms, several columns
 *   per call.
 */
int bm25_mask_stats_scratch(const bm25_index* idx, int32_t kind, int64_t M, int64_t G,
                            int64_t* bytes);
int bm25_mask_stats(bm25_index* idx, const uint32_t* masks, int64_t M, const void* values,
                    int32_t kind, const int32_t* groups, int64_t G, int64_t* out_count,
                    void* out_min, void* out_max, void* out_sum);
int bm25_mask_stats_device(bm25_index* idx, const uint32_t* d_masks, int64_t M,
                           const void* d_values, int32_t kind, const int32_t* d_groups, int64_t G,
                           int64_t* d_count, void* d_min, void* d_max, void* d_sum,
                           void* d_scratch, int64_t scratch_bytes, void* stream);

/*
 * Sort-by-field search: the documents a mask allows in the order of a
 * per-document column ("newest first", "cheapest first", by tenant id)
 * instead of by score — the exact top-k of a mask by a column, ties broken by
 * doc id, independent of scheduling.  Replaces no reference call.
 *
 * A column's order does not depend on the query, so the work is split: the
 * rank build, once per column and direction, and the selection, per batch.
 *
 *   Order of a column (kind: BM25_FIELD_I32 / _F32 / _I64, as the range
 *   filters): int32 and int64 are compared as themselves; int64 never goes
 *   through a float.  float32 is numeric order with -0.0f == +0.0f, as the
 *   range filters compare.  NaN is "no value": it comes after every number in
 *   both directions.  descending != 0 reverses the order of the numbers only;
 *   NaN stays last.  Equal values are ordered by doc id ascending in both
 *   directions: +-0, all NaNs and repeated integers included.
 *
 *   values  [n_docs]     of `kind`, by the handle's own documents
 *   ranks   [n_docs] int32  ranks[d] = the rank of document d in that order
 *   perm    [n_docs] int32  perm[r] = the handle-local document at rank r
 *   masks   [M, W] uint32, W = ceil(n_docs / 32), the layout of
 *                        bm25_search_filtered; NULL: every document is allowed
 *                        for all M rows
 *   after_ranks [M] int32  row m's cursor, or NULL: no cursor for any row
 *   out_docs, out_ranks [M, k] int32
 *
 * bm25_sort_ranks / bm25_sort_ranks_device: both outputs are permutations of
 *   [0, n_docs) and inverses of each other.  No values entry at index >=
 *   n_docs is read; n_docs == 0 returns BM25_OK without device work.  Ranks
 *   are unique 32-bit keys that already contain the direction, the dtype's
 *   comparison, the NaN rule and the doc-id tie-break.  The device call is a
 *   setup call, like bm25_index_set_world_bounds: it allocates and frees a
 *   buffer of its own — the sort's key/value double buffers, 24 bytes per
 *   document, and its histogram, 1 KiB per 4096 documents — and synchronises
 *   `stream` before it returns.  It reads the caller's buffers only and is
 *   not a search.  BM25_EINVAL for a NULL index, a bad kind, or NULL pointers
 *   with n_docs > 0.
 *
 * bm25_search_sorted / bm25_search_sorted_device: document d is eligible for
 *   row m iff mask m allows it and ranks[d] > after_ranks[m].  Row m of the
 *   outputs is the k eligible documents of smallest rank, in rank order, as
 *   (perm[rank] + doc_offset, rank); where fewer are eligible the rest of the
 *   row is padding: doc -1 and rank -1.  Without masks row m is
 *   perm[after + 1 .. after + k].  Bits at or past n_docs are ignored, and no
 *   word at index >= W of a row is read.
 *   Cursors: after_ranks[m] == BM25_AFTER_NONE (-2), or a NULL pointer, means
 *   no cursor.  -1 is the rank of a padding slot: the row is all padding and
 *   reads no mask word, so feeding back any page's last column is always
 *   safe.  Entries < -2 are "no cursor" in the device call and BM25_EINVAL in
 *   the host call.  The last column of out_ranks is the next page's cursor.
 *   0 <= k <= min(n_docs, 4096); k > 4096 is BM25_EINVAL, the limit of the
 *   collapsed search, for the same LDS reason (a row's list is sorted in one
 *   workgroup's LDS).  k == 0 or M == 0 returns BM25_OK without device work.
 *   M may pass 65535.  The result is integer and depends neither on
 *   scheduling nor on any option; the global atomics are integer adds.
 *   Host call: validated, synchronous.  It checks that ranks and perm are
 *   inverse permutations (the message names the first offending index),
 *   shapes, NULLs and cursor entries.  On an error the outputs are untouched.
 *   Device call: it checks shapes, NULLs, k, and scratch_bytes against
 *   bm25_search_sorted_scratch (scratch 4-byte aligned; none is needed
 *   without masks).  It never synchronises and retains nothing.  It reads
 *   only the caller's buffers and writes only the outputs and d_scratch.  It
 *   is not ordered against the handle's searches.  It leaves
 *   bm25_search_dispatch, the counters and bm25_search_filtered_stats alone.
 *   A ranks entry outside [0, n_docs) is never eligible.  With arrays that
 *   are not inverse permutations the affected rows are unspecified, and
 *   nothing outside the caller's buffers is touched.
 *   Method: a row's rank interval, [0, n_docs) at first, is narrowed by
 *   histograms over rank bits — a pass over the mask words and ranks counts
 *   the row's eligible documents per bin of its interval, the interval
 *   becomes the bin that holds the k-th — until it is at most Wmax = 2048
 *   ranks wide; one more pass lists every eligible rank below the interval's
 *   end (fewer than k below it, at most Wmax inside), the list is sorted and
 *   its first k written.  levels + 1 passes over the masks, no fallback path.
 * bm25_search_sorted_scratch: *bytes = 4 M (4 + 1 + 256 + min(k + 2048,
 *   n_docs)): per row the interval state, the list count, the histogram of at
 *   most 256 bins and the list.  The same k and M rules (BM25_EINVAL).
 * Option "sorted_bins" (below) sets the bins per level.
 *
 * bm25_search_boolean_sorted: every argument of bm25_search_boolean_ranges,
 *   then (ranks, perm, after_ranks [Q], out_ranks [Q, k]).  With ranks == NULL
 *   it is bm25_search_boolean_ranges, bit for bit, chunk size included.  With
 *   ranks, each chunk's mask is built exactly as there — range AND terms AND
 *   base — and totals and facets are taken of it; rows are then selected by
 *   rank instead of by score.  out_scores[q][j] is bm25_score_docs_device's
 *   bits for (queries[q], hit j).  Padding slots are doc -1, score bits
 *   0xFFFFFFFF and rank -1, the padding of every other search.  ranks and
 *   perm (validated as bm25_search_sorted validates them) go up once per
 *   call, as the groups and columns do; the masks still never move to the
 *   host.  k > 4096 with ranks is BM25_EINVAL.
 *
 * Out of scope: merging sorted lists of doc shards by their ranks (ranks are
 * per handle; the keyed merge of "Sort-by-field search over doc shards" below
 * serves shards with (value, doc) keys); secondary sort keys other than doc
 * id; an early-terminating walk of perm for dense masks; k > 4096.
 */
int bm25_sort_ranks(bm25_index* idx, const void* values, int32_t kind, int32_t descending,
                    int32_t* out_ranks, int32_t* out_perm);
int bm25_sort_ranks_device(bm25_index* idx, const void* d_values, int32_t kind, int32_t descending,
                           int32_t* d_ranks, int32_t* d_perm, void* stream);
int bm25_search_sorted_scratch(const bm25_index* idx, int64_t M, int32_t k, int64_t* bytes);
int bm25_search_sorted(bm25_index* idx, const uint32_t* masks, int64_t M, const int32_t* ranks,
                       const int32_t* perm, int32_t k, const int32_t* after_ranks,
                       int32_t* out_docs, int32_t* out_ranks);
int bm25_search_sorted_device(bm25_index* idx, const uint32_t* d_masks, int64_t M,
                              const int32_t* d_ranks, const int32_t* d_perm, int32_t k,
                              const int32_t* d_after_ranks, int32_t* d_docs, int32_t* d_out_ranks,
                              void* d_scratch, int64_t scratch_bytes, void* stream);
int bm25_search_boolean_sorted(bm25_index* idx, const int32_t* queries, int64_t Q, int64_t T,
                               int32_t k, const int32_t* must, int64_t A, const int32_t* any,
                               int64_t B, const int32_t* must_not, int64_t N,
                               const int32_t* min_match, const uint32_t* base, int64_t Mb,
                               const int32_t* groups, int64_t G, const void* values, int32_t kind,
                               int64_t F, const int32_t* fields, const void* lo, const void* hi,
                               int64_t C, int32_t* out_docs, float* out_scores,
                               int64_t* out_total_hits, int64_t* out_facets, const int32_t* ranks,
                               const int32_t* perm, const int32_t* after_ranks,
                               int32_t* out_ranks);

/*
 * Sort-by-field search over doc shards: order keys, collection cursors and a
 * keyed merge.  A rank is a position in one handle's permutation: rank 17 of
 * shard 0 and rank 17 of shard 1 say nothing about each other, and a rank
 * cursor of one shard means nothing on another.  Shards therefore exchange a
 * collection-wide order key per hit.  Replaces no reference call.
 *
 * The order key K(v, kind, descending) is a uint64, the key the rank build of
 * bm25_sort_ranks sorts by:
 *   BM25_FIELD_I32: u = (uint32)v ^ 0x80000000; descending: ~u in 32 bits;
 *                   zero-extended.
 *   BM25_FIELD_F32, in this order: (1) NaN gives 1 << 32 in both directions;
 *                   (2) otherwise +-0.0 become bits 0; (3) u = sign ? ~bits :
 *                   bits | 0x80000000; (4) descending: (uint32)~u.
 *   BM25_FIELD_I64: u = (uint64)v ^ (1 << 63); descending: ~u.
 * The collection-wide order of a column is (K ascending, global doc id
 * ascending); within one handle it is exactly the order bm25_sort_ranks builds.
 * All ranks of a collection must use the same kind and direction.
 *
 * A key travels as two uint32 planes, key_hi = K >> 32 and key_lo = K &
 * 0xFFFFFFFF, never as an 8-byte word: a packed [3][Q][k] int32 buffer (docs |
 * key_hi | key_lo) needs no 8-byte alignment and one all-gather moves docs and
 * keys together (the layout idea of bm25_merge_collapsed_device).
 * Padding is doc -1 with key_hi = key_lo = 0xFFFFFFFF.  Padding is recognised
 * by the doc id, never by the key: a real document whose int64 value is
 * INT64_MAX ascending has the all-ones key and is still returned, ahead of
 * padding.
 *
 * All three calls are device-only and enqueued on `stream`; they never
 * synchronise, take no scratch and retain nothing, use no atomics on global
 * memory, are not searches (bm25_search_dispatch, the counters and
 * bm25_search_filtered_stats stay as they were) and are not ordered against
 * the handle's searches.  Every argument check runs before any device call.
 *
 * bm25_sort_keys_device: d_docs [n] holds global doc ids as
 *   bm25_search_sorted_device writes them; element i of d_key_hi / d_key_lo
 *   [n] gets K(values[d_docs[i] - doc_offset]).  A negative doc id, or one
 *   outside [doc_offset, doc_offset + n_docs), gets the padding key and reads
 *   no value.  Nothing past n elements is written.  BM25_EINVAL for a NULL
 *   index, a bad kind, negative n, or a NULL pointer with n > 0; n == 0 is
 *   BM25_OK without device work.
 *
 * bm25_sort_cursor_device: a collection cursor (key, global doc) per row m <
 *   M into this handle's rank cursor for bm25_search_sorted_device:
 *     d_after_docs[m] == -1 (the doc of a padding slot: exhausted)  -> -1
 *     d_after_docs[m] <  -1 (no cursor)            -> BM25_AFTER_NONE (-2)
 *     d_after_docs[m] >=  0                        -> from c, below
 *   c = the number of handle-local documents d with (K(values[d]), doc_offset
 *   + d) <= (key, d_after_docs[m]), the doc part compared in 64 bits, so a
 *   cursor document of another shard is legal and means what the inequality
 *   says.  c == 0 gives -2 — not -1, which would end the row — otherwise c - 1.
 *   A document is then eligible on this shard iff it is strictly after the
 *   cursor in the collection's order; the cursor need not name an existing
 *   document.  Method: one binary search per row over d_perm, which is sorted
 *   by exactly this pair (about log2(n_docs) dependent pairs of loads, one
 *   thread per row).  M may pass 65535.  d_perm is the caller's and is not
 *   validated: an entry outside [0, n_docs) makes that row unspecified, no
 *   value outside the column is read, the other rows are unaffected.
 *   BM25_EINVAL for a NULL index, a bad kind, negative M, or NULL pointers with
 *   M > 0; M == 0 is BM25_OK without device work.
 *
 * bm25_merge_sort_keys_device: takes no handle.  List w of row q starts at
 *   element w * rank_stride + q * k of each input pointer: rank_stride = Q * k
 *   for plain [W, Q, k] arrays, 3 * Q * k with the pointers Q * k apart for the
 *   packed buffer one all-gather moves.  Each list is strictly ascending by
 *   (key, doc) with real entries first; the first doc < 0 and everything after
 *   it is padding and is never read into a result.  Doc ids are unique across
 *   the lists.  Row q of the outputs [Q, k] is the first k of the union in
 *   (key, doc) order, the rest padded with doc -1 and keys 0xFFFFFFFF; every
 *   output slot is written.  W = 1 returns its input, with padding made
 *   canonical.  The last column (doc, key) of a page is the next page's
 *   collection cursor.  BM25_EINVAL, the message naming the value: W outside
 *   1..64 (W > 64: merge in stages), negative Q or k, k > 4096 (the sorted
 *   search's own limit), rank_stride < Q * k, a NULL input or output pointer
 *   with a non-empty shape.  k == 0 or Q == 0 is BM25_OK with no device work.
 *   Q may pass 65535.  A list that breaks the order precondition gives that
 *   row unspecified contents; the other rows are unaffected, nothing outside
 *   the caller's buffers is touched, and the kernel ends.
 *   Method: a workgroup per row folds the lists one after another into an
 *   accumulator of at most k (key, doc) entries in LDS, each fold a two-way
 *   merge by ranking truncated at k: about W k log k steps a row.
 *
 * Out of scope: secondary sort keys, ordering by several columns, a
 * host-buffer form of the three calls, W > 64 in one merge, k > 4096.
 */
int bm25_sort_keys_device(bm25_index* idx, const void* d_values, int32_t kind, int32_t descending,
                          const int32_t* d_docs, int64_t n, uint32_t* d_key_hi,
                          uint32_t* d_key_lo, void* stream);
int bm25_sort_cursor_device(bm25_index* idx, const void* d_values, int32_t kind,
                            int32_t descending, const int32_t* d_perm,
                            const uint32_t* d_after_key_hi, const uint32_t* d_after_key_lo,
                            const int32_t* d_after_docs, int64_t M, int32_t* d_after_ranks,
                            void* stream);
int bm25_merge_sort_keys_device(int device, const int32_t* d_docs, const uint32_t* d_key_hi,
                                const uint32_t* d_key_lo, int64_t W, int64_t Q, int32_t k,
                                int64_t rank_stride, int32_t* d_out_docs, uint32_t* d_out_key_hi,
                                uint32_t* d_out_key_lo, void* stream);

/*
 * bm25.BM25's float64 path (the dense model's API keeps the reference's
 * precision).  bm25_index_set_values_f64 keeps a float64 copy of the index's
 * values beside it (the same CSC order; bm25_build_scores method 1 returns
 * them as out_data64 — the reference's bm25_matrix entries).
 *   bm25_scores_dense_f64: every document's float64 sum over the query's
 *     valid ids in query order from 0 — numpy's np.sum(bm25_matrix[:, ids],
 *     axis=1) bit for bit (column by column; a one-document corpus: numpy's
 *     pairwise order).  Replaces BM25.get_scores (bm25.py:124-145).
 *   bm25_topn_f64: the n best documents of those sums by (score desc, doc
 *     asc), 0 <= n <= n_docs.  Replaces the ranking of BM25.get_top_n
 *     (bm25.py:147-178: argsort(scores)[::-1][:n]; its order among equal
 *     scores is numpy-implementation-defined).
 * Errors: EINVAL when no float64 values were set, a token id >= n_terms
 * (bm25_native's message), n out of range.
 */
int bm25_index_set_values_f64(bm25_index* idx, const double* data64);
int bm25_scores_dense_f64(bm25_index* idx, const int32_t* query, int64_t T, double* out_scores);
int bm25_topn_f64(bm25_index* idx, const int32_t* query, int64_t T, int64_t n, int32_t* out_docs,
                  double* out_scores);

/*
 * Merge W per-shard top-k lists (global doc ids) into one top-k, device
 * buffers: d_docs/d_scores are [W, Q, k], outputs [Q, k].  Used after the
 * RCCL all-gather of the doc-sharded search; the order rule
 * is the same (score desc, doc asc), so the result equals a single-index
 * search over the whole collection.
 */
int bm25_merge_topk_device(int device, const int32_t* d_docs,
                           const float* d_scores, int64_t W, int64_t Q,
                           int32_t k, int32_t* d_out_docs, float* d_out_scores,
                           void* stream);

/*
 * The same merge for the lists bm25_search_finish_device (world > 1) and
 * bm25_search_shard_device write — a shard's keys in any order, padding
 * (doc -1) anywhere — in one buffer per rank: rank w's [Q, k] docs and scores start at element
 * w * rank_stride of d_docs / d_scores (rank_stride = Q * k for plain
 * [W, Q, k] arrays, 2 * Q * k for the packed [W][docs|scores][Q][k] buffer
 * one all-gather moves).  A W-way merge, one wavefront per query.
 * Replaces: the reference is single-device (main.py:205); SURVEY.md §8(e).
 */
int bm25_merge_sorted_device(int device, const int32_t* d_docs,
                             const float* d_scores, int64_t W, int64_t Q,
                             int32_t k, int64_t rank_stride, int32_t* d_out_docs,
                             float* d_out_scores, void* stream);

/*
 * The merge of collapsed searches over doc shards: the W-way merge of
 * bm25_merge_sorted_device with the walk of bm25_search_collapsed run over the
 * merged order, so the quota holds across shards (two shards can each return a
 * hit of one group; a plain merge of collapsed lists would keep both).
 * Replaces no reference call: the reference is single-device (main.py:205) and
 * BM25v.search has no grouping (bm25_native.py:76-158).
 *   d_docs / d_scores / d_groups: list w of row q starts at element
 *              w * rank_stride + q * k of each of the three pointers:
 *              rank_stride = Q * k for plain [W, Q, k] arrays; 3 * Q * k, with
 *              the pointers Q * k apart, for the packed
 *              [W][docs|scores|groups][Q][k] buffer that one all-gather moves.
 *              Each list is what bm25_search_collapsed(_device) writes with
 *              out_groups: global doc ids, strictly in result order (score
 *              descending, doc ascending, by the engine's key), real entries
 *              first; the first doc < 0 and everything after it is padding and
 *              is never read into a result.  A negative group on a real entry
 *              means "no group".  Doc ids are unique across the lists.
 *   Row q of the outputs [Q, k]: the first k kept entries of the walk of the
 *              merged order under per_group (the walk rule of
 *              bm25_search_collapsed: an entry without a group is always kept,
 *              one of group g iff fewer than per_group of g were kept before
 *              it), as (doc, score bits, group); padding is doc -1, score bits
 *              0xFFFFFFFF, group -1.  Every output slot is written.
 *              d_out_groups may be NULL (not wanted).
 * Identities:
 *   every input a shard's collapsed list at the same k and per_group (masks and
 *              weights included): the output is bit for bit the single-index
 *              bm25_search_collapsed row over the collection;
 *   per_group >= k, or all groups negative: docs and scores are bit for bit
 *              those of bm25_merge_sorted_device on the same lists;
 *   W = 1 returns its input (padding made canonical).
 * Errors (BM25_EINVAL, the message names the value, checked before any device
 * call): W < 1 or W > 64 (merge wider worlds in stages), negative Q or k,
 * k > 4096 (the group table lives in LDS, as bm25_search_collapsed's),
 * per_group < 1, rank_stride < Q * k, a NULL input or output pointer with a
 * non-empty shape (d_out_groups alone may be NULL).  k == 0 or Q == 0: BM25_OK
 * without device work.  Q may pass 65535.
 * A list that breaks the order precondition gives that row unspecified
 * contents: the other rows are unaffected, nothing outside the caller's
 * buffers is touched, and the kernel ends (at most W * k + 1 rounds a row).
 * How: one wavefront per row, in rounds: a window of every list (W * B <= 512
 * keys, B = 64 at W <= 8 down to 8 at W = 64), the window entries at or above
 * the best last window key of the lists that go on are next in the merged
 * order; they are ranked by binary searches of the other windows and walked
 * 64 at a time against the row's group table in LDS.  No scratch, no atomics
 * on global memory, no host synchronisation; enqueued on `stream`.
 * Not a search: it takes no handle and leaves every handle's dispatch and
 * stats alone.
 */
int bm25_merge_collapsed_device(int device, const int32_t* d_docs, const float* d_scores,
                                const int32_t* d_groups, int64_t W, int64_t Q, int32_t k,
                                int64_t rank_stride, int32_t per_group, int32_t* d_out_docs,
                                float* d_out_scores, int32_t* d_out_groups, void* stream);

/*
 * Doc-sharded search with a GLOBAL threshold, one rank per GPU (the
 * multi-process form of bm25_search_device).  Every rank
 * holds one doc shard (bm25_index_create with its doc_offset) and searches
 * the same query batch in two halves around one all-gather:
 *   bm25_sample_width(idx, shard_docs_max, world, k, &S): keys per query each
 *     rank samples (the same on every rank: shard_docs_max = the largest
 *     shard's document count; S = 0: shards too small to sample, or
 *     k > 4096 — then the finish half lists the shard's exact top-k; the
 *     same S serves the tile-bound threshold, whose keys need no sampling);
 *   bm25_search_sample_device(...): this shard's sample keys -> d_keys
 *     (u64 [Q][S], zero-padded: a SAMPLE pass, or — theta_bound — the best S
 *     tile-bound keys, read from the tile bounds without scoring);
 *   (caller) all-gather d_keys of every rank -> d_all_keys [world][Q][S];
 *   bm25_search_finish_device(...): theta = the k-th best key of the world's
 *     sample (k real documents score at least this), then every key >= theta
 *     of this shard -> [Q, k] (global doc ids; padded with doc -1 / score bits
 *     0xFFFFFFFF where the shard holds fewer), or the shard's exact top-k for
 *     queries the threshold cannot serve.
 * Merging the world's [Q, k] lists with bm25_merge_topk_device (padding
 * sorts last) gives exactly the single-index top-k.  world = 1 is a plain
 * search.  Replaces no reference call: the reference is single-device.
 */
int bm25_sample_width(const bm25_index* idx, int64_t shard_docs_max, int32_t world, int32_t k,
                      int64_t* width);
int bm25_search_sample_device(bm25_index* idx, const int32_t* d_queries, int64_t Q, int64_t T,
                              int32_t k, int32_t world, int64_t shard_docs_max,
                              uint64_t* d_keys, void* stream);
int bm25_search_finish_device(bm25_index* idx, const int32_t* d_queries, int64_t Q, int64_t T,
                              int32_t k, int32_t world, int64_t shard_docs_max,
                              const uint64_t* d_all_keys, int32_t* d_docs, float* d_scores,
                              void* stream);
/*
 * The finish half on three streams, for a caller that pipelines batches
 * (bm25mi.dist.ShardPipeline): theta on stream_theta, the REST pass on
 * stream_rest (after theta), the merges into d_docs / d_scores on
 * stream_select (after REST); the library orders the three with events.
 * The workspace is released on stream_select: the handle's next search on
 * another stream waits for it.  Same results as bm25_search_finish_device
 * (which is this with one stream).  The score pass of a profiled handle is
 * timed on stream_rest from the REST pass's start.
 */
int bm25_search_finish_streams_device(bm25_index* idx, const int32_t* d_queries, int64_t Q,
                                      int64_t T, int32_t k, int32_t world,
                                      int64_t shard_docs_max, const uint64_t* d_all_keys,
                                      int32_t* d_docs, float* d_scores, void* stream_theta,
                                      void* stream_rest, void* stream_select);

/*
 * Doc-sharded search with ONE collective (the multi-process form used by
 * bm25mi.dist when the collection's tile bounds fit one selection block:
 * <= 30720 tiles).  Every rank exports its tile bounds, the ranks all-gather
 * them once (at index build), and each rank's search takes the whole
 * collection's tile-bound threshold by itself:
 *   bm25_index_bounds_export(idx, d_out, stride, stream): this index's tile
 *     bounds [n_terms][stride] u16 (stride: a multiple of 4 >= its tiles,
 *     rounded up to 4; the same on every rank; zero past its tiles);
 *   (caller) all-gather -> d_world [world][n_terms][stride], kept alive;
 *   bm25_index_set_world_bounds(idx, d_world, world, stride, world_tiles):
 *     world_tiles = the collection's tiles (NULL d_world clears); the call
 *     waits for the device (d_world written on any stream before it is
 *     complete) and reads the table once into a pooled copy the handle owns (the max of every 4 tiles, a quarter
 *     of the size: the threshold's input where the collection has >= 8k such
 *     groups — option bound_pool) and keeps the pointer for the rest;
 *   bm25_search_shard_device(...): this shard's keys >= the collection's
 *     threshold (k real documents score at least it) as a [Q, k] list in no
 *     particular order (global doc ids, padding doc -1 / score bits
 *     0xFFFFFFFF last), or its exact top-k for k > 4096 / queries the
 *     threshold cannot serve;
 *   (caller) all-gather the lists, bm25_merge_sorted_device (any order in).
 * The result is exactly the single-index top-k.  Replaces no reference call:
 * the reference is single-device (main.py:205).
 */
int bm25_index_bounds_export(bm25_index* idx, uint16_t* d_out, int64_t stride, void* stream);
/* Diagnostics: the sub-block presence masks beside the tile bounds,
 * [n_terms][stride] u32 with the stride rules of bm25_index_bounds_export —
 * bit s of (term, tile): the term has a posting in the tile's s-th sub-block
 * of tile_docs / 32 documents.  EINVAL where the index keeps none (no tile
 * bounds, BM25_TILE_MASK=0 at create, or no memory for the table). */
int bm25_index_masks_export(bm25_index* idx, uint32_t* d_out, int64_t stride, void* stream);
int bm25_index_set_world_bounds(bm25_index* idx, const uint16_t* d_world, int32_t world,
                                int64_t stride, int64_t world_tiles);
int bm25_search_shard_device(bm25_index* idx, const int32_t* d_queries, int64_t Q, int64_t T,
                             int32_t k, int32_t* d_docs, float* d_scores, void* stream);

/*
 * Doc-sharded index over several devices of ONE process.
 * The reference is single-device (DEVICE_ID = 0, main.py:205, graph.py:95);
 * this is the build's multi-GPU form of BM25v.index / BM25v.search
 * (bm25_native.py:59-103) for callers that own all local GPUs.  The multi-
 * process form (one rank per GPU, RCCL all-gather) is bm25mi.dist + the
 * *_device calls above.
 *   bm25_sharded_create: same CSC arguments as bm25_index_create; documents
 *     are split into n_dev contiguous, 2048-doc-aligned ranges, shard s on
 *     devices[s] (a device may be listed more than once).
 *   bm25_sharded_search: same contract as bm25_search; the global-threshold
 *     protocol of the *_device calls above with peer copies (xGMI) in place of
 *     the all-gathers: every shard samples on its own stream, every shard's
 *     keys are copied to every device, every shard computes the world's theta
 *     and lists its keys >= theta, and the [Q, k] lists are copied to
 *     devices[0] and merged there; the result equals a single-index search.
 *     Errors as bm25_search (k may exceed a shard's documents: its list is
 *     padded).
 *   bm25_sharded_info: shard count and [lo, hi) doc ranges (arrays of n_dev).
 */
typedef struct bm25_sharded bm25_sharded;

int bm25_sharded_create(int n_dev, const int* devices, int64_t n_docs, int64_t n_terms,
                        int64_t nnz, const void* indptr, int indptr_is_i64,
                        const int32_t* indices, const float* data, bm25_sharded** out);
int bm25_sharded_search(bm25_sharded* s, const int32_t* queries, int64_t Q, int64_t T,
                        int32_t k, int32_t* out_docs, float* out_scores);
int bm25_sharded_info(const bm25_sharded* s, int64_t* n_shards, int64_t* shard_lo,
                      int64_t* shard_hi);
int bm25_sharded_destroy(bm25_sharded* s);

/*
 * Timing of the score pass (sample + theta + rest score kernels, the HBM
 * bound part of a search), measured with HIP events recorded on the search
 * stream around it in every search while enabled.
 * bm25_profile_enable(idx, on) resets the accumulators; on = 1: two events
 * per search (score pass start and end: total_ms reports the score pass);
 * on = 2: a third at the search's end (total_ms = the whole search).  Each
 * event record costs the device a marker packet (~4 us).
 */
int bm25_profile_enable(bm25_index* idx, int on);
int bm25_profile_read(bm25_index* idx, double* score_ms_total,
                      int64_t* score_launches, double* total_ms,
                      int64_t* searches, int64_t* rescored_tiles);

/*
 * Selection statistics of the last search on the handle (diagnostics; waits
 * for the device): tiles whose exact top-k had to be recomputed, and queries
 * that took the exact fallback stage (candidate list overflow).
 */
int bm25_search_stats(bm25_index* idx, int64_t* rescored_tiles,
                      int64_t* fallback_queries);
/* The same plus *bound_skipped: (query, tile) pairs the REST pass skipped
 * because the sum of the query terms' largest scores in the tile (the tile
 * bounds of a dense, non-negative index) is below the query's threshold —
 * counted only by a search with the count_skips option on, else -1.
 * Any pointer may be NULL. */
int bm25_search_stats_ex(bm25_index* idx, int64_t* rescored_tiles,
                         int64_t* fallback_queries, int64_t* bound_skipped);
/* Every selection counter of the last search, the first n of (in order):
 *   [0] tiles re-scored exactly, [1] queries sent to the exact fallback
 *   stage, [2] (query, tile) pairs the REST pass skipped by their tile
 *   bound, [3] the postings of those skipped (query, tile) segments (what
 *   the skip saved of the algorithmic bytes, 8 B each) — [2] and [3]
 *   counted only by a search with the count_skips option on, else -1 —
 *   [4] queries left to
 *   the block merge (lists longer than one wavefront's registers), [5] k >
 *   4096: queries the list path handed to dense score rows (-1: the dense
 *   path served the whole search; 0 after a search of k <= 4096),
 *   [6] non-empty term segments the REST pass dropped in tiles it scored
 *   (seg_skip: the term has no posting in a sub-block that can reach the
 *   threshold), [7] their postings, [8] double rows (128 postings) the
 *   REST pass dropped in the segments it kept (row_skip: all of the row's
 *   postings lie in sub-blocks that cannot reach the threshold), [9] their
 *   postings — counted as [2] and [3], else -1.
 * n must be in 1..10. */
int bm25_search_counters(bm25_index* idx, int64_t* out, int32_t n);

/*
 * Search options of one handle.  A new handle takes them from the
 * environment (BM25_FLAT, BM25_FLAT_BW, BM25_ITEMS_PER_WAVE, BM25_SAMPLE_P,
 * BM25_LIST_CAP, BM25_CLAIM_CH, BM25_CLAIM_M, BM25_TILE_BOUND, BM25_THETA_BOUND,
 * BM25_GRID_PCT, BM25_LARGE_LISTS, BM25_COUNT_SKIPS, BM25_REST_SPLIT,
 * BM25_BOUND_POOL, BM25_FILTER_TILES, BM25_BOOL_CHUNK) and, for "tile_mask"
 * "seg_skip", "row_skip", "row_mask_kb", "collapse_page" and "collapse_chunk",
 * from BM25_TILE_MASK, BM25_SEG_SKIP, BM25_ROW_SKIP, BM25_ROW_MASK_KB,
 * BM25_COLLAPSE_PAGE and BM25_COLLAPSE_CHUNK, at bm25_index_create; these
 * calls change or read them afterwards, effective from the next search.
 * Results never depend on them (every setting is bit-exact); they choose
 * kernels and geometry:
 *   "flat"           1 (default): the flat score kernel for queries of 1..64
 *                    terms; 0: score_wave_kernel for every phase
 *   "flat_bw"        tiles per flat-kernel item: 0 = automatic, 1, 2, 4, 8
 *   "items_per_wave" automatic flat_bw: halved while a phase gives the
 *                    resident waves fewer items each (default 4; config 2:
 *                    4-tile items 0.089 ms per batch, 2-tile items at 8: 0.105)
 *   "sample_p"       largest sampling stride, a power of two (default 8;
 *                    1 = no threshold: the exact pass over every tile)
 *   "list_cap"       candidate-list capacity per query (0 = automatic; small
 *                    values force queries through the exact fallback stage)
 *   "claim_ch", "claim_m"  flat-kernel item claims: items per claim (1),
 *                    counters per XCD (4)
 *   "tile_bound"     1 (default): the REST pass skips tiles whose query-term
 *                    maxima (f16 bounds kept per (term, tile) by a dense,
 *                    non-negative index) sum below the threshold;
 *                    0: every tile is scored
 *   "theta_bound"    1 (default): the threshold comes from those tile bounds
 *                    (per tile, its largest query-term maximum is a real
 *                    document's score lower bound) with no SAMPLE pass;
 *                    0: the sampled threshold.  Every shard of a multi-rank
 *                    search needs the same setting (bm25_sample_width).  A
 *                    handle whose tile-bound searches overflowed switches
 *                    itself to the sampled threshold for a while, decided per
 *                    handle from a host-mapped report read without waiting —
 *                    so ranks may mix the two kinds of keys in one search:
 *                    that is exact (both are keys of real documents, the
 *                    width S is the same), only the work differs
 *   "large_lists"    1 (default): k > 4096 takes the list path where it
 *                    applies (a sampled threshold, keys above it listed by the
 *                    REST pass, selected and sorted — no dense score rows);
 *                    0: dense score rows for every query
 *   "count_skips"    1: the REST pass also counts the (query, tile) pairs its
 *                    tile bound skips and their postings (bm25_search_counters
 *                    [2], [3]) — a kernel build of its own: the two counts'
 *                    registers cost the pass 13 % on an 8-way doc shard;
 *                    0 (default): not counted
 *   "rest_split"     1: where the REST pass gives each resident wave few
 *                    items (< 48: a doc shard of a few-GPU collection), a
 *                    heavy query's 8-tile band is split into 2..8 items (a
 *                    per-search table built by the threshold kernel);
 *                    0 (default: measured no faster at W = 8)
 *   "bound_pool"     1 (default): the tile-bound threshold reads the bounds
 *                    pooled over groups of 4 tiles (a group's largest query-
 *                    term maximum is still a lower bound of one of its
 *                    documents' scores) where there are >= 8k groups — a
 *                    quarter of the threshold kernel's bytes; 0: the per-tile
 *                    bounds
 *   "filter_tiles"   1 (default): a filtered search of k <= 4096 takes the tile
 *                    passes; 0: dense score rows for every query
 *   "bool_chunk"     bm25_search_boolean: queries per chunk of device-built
 *                    masks (env BM25_BOOL_CHUNK); 0 (default) = automatic: at
 *                    most 1 GiB of mask words per chunk, at least one query
 *   "tile_mask"      1 (default): the REST pass's tile bound is refined by the
 *                    sub-block presence masks (a u32 per (term, tile) beside
 *                    the tile bounds: bm25_index_masks_export); 0: the
 *                    whole-tile bound alone.  Read at bm25_index_create too:
 *                    a handle created under BM25_TILE_MASK=0 keeps no mask
 *                    table, and the option then changes nothing
 *   "seg_skip"       1 (default): in a tile the REST pass scores, it drops the
 *                    segment of every query term that has no posting in a
 *                    sub-block whose masked bound reaches the threshold (the
 *                    pre-pass marks them: a byte per (query, tile)); needs
 *                    "tile_mask" and its table; 0: whole tiles only
 *   "row_skip"       1 (default): of a kept segment of two or more double rows
 *                    (128 postings each) the REST pass runs only the rows with
 *                    a posting in such a sub-block (the pre-pass writes a u16
 *                    per (query, tile, term lane) from the index's row masks);
 *                    needs "seg_skip" and the row-mask table; 0: whole segments
 *   "row_mask_kb"    budget of the row-mask table in KiB (default 262144), read
 *                    at bm25_index_create only: terms with a segment of two or
 *                    more rows take a slot of 64 B per tile, the most frequent
 *                    first; a term past the budget keeps all its rows; 0: no table
 *   "collapse_page"  bm25_search_collapsed: results per page of a round, 0..4096
 *                    (clamped to [1, min(n_docs, 4096)]); 0 (default) =
 *                    automatic: 2 k
 *   "collapse_chunk" bm25_search_collapsed: rows per sub-batch of the rounds
 *                    under exclusion masks; 0 (default) = automatic: at most
 *                    1 GiB of mask words per sub-batch, at least one row
 *   "sorted_bins"    bm25_search_sorted: histogram bins per level of the rank
 *                    selection, 0..256 (env BM25_SORTED_BINS); 0 (default) or
 *                    1 = automatic: 256.  Fewer bins take more levels
 *   "grid_pct"      percent of the device's resident workgroup slots the
 *                    persistent score kernels launch (1..100, default 100):
 *                    below 100 leaves slots for kernels of another stream
 *                    (a concurrent search on a fork, the collectives)
 * Replaces no reference call (the reference has no tuning surface; its MAX
 * custom op takes compile-time parameters, graph.py:72).
 */
int bm25_index_set_option(bm25_index* idx, const char* name, int64_t value);
int bm25_index_get_option(const bm25_index* idx, const char* name, int64_t* value);

/*
 * What the last search on the handle launched (diagnostics, no device wait):
 *   *kernels     bit mask of score kernels: 1 flat SAMPLE, 2 flat REST,
 *                4 flat ALL (exact pass / fallback stage), 8 wave SAMPLE,
 *                16 wave REST, 32 wave ALL, 64 large-k path, 128 tile-bound
 *                threshold keys; 256 (a flag, not a kernel): the tile-bound
 *                threshold was off for this search because earlier searches
 *                on the handle that used it overflowed their candidate lists
 *                (more than 1/16 of their queries took the exact fallback) —
 *                it is retried after 64, 128, ... 4096 searches; 512 (a
 *                flag): REST counted its skipped postings (count_skips);
 *                1024 (a flag): REST ran over split items (rest_split);
 *                2048 (a flag): the threshold read the pooled bounds (bound_pool);
 *                4096: the filtered search's tile passes (its dense path sets 64);
 *                8192 (a flag): the last search was weighted
 *                (bm25_search_weighted; it sets 4096 and / or 64 as well);
 *                16384 (a flag): the last search was called through
 *                bm25_search_after(_device), whatever its cursors;
 *                32768: tile_skip_kernel, the tile bounds' pre-pass of a flat
 *                REST launch; 65536 (a flag): the pre-pass also marked the
 *                dead term segments of scored tiles (seg_skip); 131072 (a
 *                flag): ... and the dead rows of kept segments (row_skip);
 *                262144 (a flag): the last search was called through
 *                bm25_search_collapsed(_device); the other bits are its last
 *                round's
 *   *term_lanes  flat kernel: term lanes per tile (8, 16, 32 or 64)
 *   band_tiles   [3]: flat kernel tiles per item of ALL, SAMPLE, REST
 *   *sample_p    sampling stride of the search (1: exact pass, 0: tile-bound
 *                threshold keys, no SAMPLE pass)
 * Any pointer may be NULL.
 */
int bm25_search_dispatch(bm25_index* idx, uint32_t* kernels, int32_t* term_lanes,
                         int32_t* band_tiles, int32_t* sample_p);

#ifdef __cplusplus
}
#endif

#endif /* BM25MI_H */
