// bm25mi_internal.h — shared declarations between the C-ABI host code
// (bm25mi_capi.cpp) and the gfx950 kernels (bm25mi_kernels.hip).
//
// Device layout of one index, tiles of D = 2^S docs (S = 11):
//   val   f32 [nnz+64]       the CSC `data` array, unchanged order (term-major,
//                            doc-ascending inside a term)
//   ldoc  u16 [nnz+64]       the doc's tile-local id (= its LDS accumulator
//                            slot); the tile of a posting is implied by its
//                            position
//   indptr i64 [V+1]         CSC column pointers
//   rel   u32 [V][ntiles+1]  rel[t][j] = first posting of term t whose doc is
//                            in tile j or later, relative to indptr[t]
// so the postings of term t inside tile j are
//   [indptr[t] + rel[t][j], indptr[t] + rel[t][j+1]).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

namespace bm25mi {

// Candidate key: (sortable f32 score bits) << 32 | (0xFFFFFFFF - doc).
// Larger key == better: higher score first, then smaller doc id.
// Key 0 never encodes a real (non-NaN) score and marks an empty slot.
__host__ __device__ inline uint32_t score_key(float s) {
  uint32_t u;
  __builtin_memcpy(&u, &s, 4);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__host__ __device__ inline float key_score(uint32_t k) {
  uint32_t u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
  float s;
  __builtin_memcpy(&s, &u, 4);
  return s;
}
__host__ __device__ inline uint64_t make_key(float s, uint32_t doc) {
  return ((uint64_t)score_key(s) << 32) | (uint64_t)(0xFFFFFFFFu - doc);
}

// Exact candidates kept per sample tile.
constexpr int kTileM = 4;
// Keys per sample tile of the large-k list path (the best of each 256-doc slice).
constexpr int kLargeM = 8;
constexpr int kSplitM = 3;  // the REST build over split items (bm25mi_kernels.hip)
constexpr int kSplitItemsPerWave = 48;  // split REST items below this many items per wave
// Largest k of the sampled-threshold pipeline; larger k (up to n_docs) take
// the large-k path (bm25mi_large.hip).
constexpr int kMaxK = 4096;
// Merge kernel LDS: number of u64 keys sorted at once.
constexpr int kMergeP = 8192;
// Posting arrays carry a small tail (so posting 0 exists for an empty index).
constexpr int64_t kPostingPad = 64;
// Tile: 2^11 = 2048 docs, one wavefront's LDS accumulator (8 KB).
constexpr int kDefaultTileShift = 11;

// Item claims of the flat score kernel (bm25mi_kernels.hip): counters per
// XCD (allocated), int32 stride between counters (256 B).
constexpr int kClaimM = 8;
constexpr int kCtrStride = 64;
// Sample tiles come in groups of kSampleGroup consecutive tiles (sample_geom).
constexpr int kSampleGroup = 8;
constexpr int kWctrInts = 8 * kClaimM * kCtrStride;
// Finished-wave count of a claim counter's waves: 128 B past the counter.
constexpr int kDoneOff = 32;
// Claim-counter regions of a search: SAMPLE, REST (or the exact pass), fallback.
constexpr int kWctrRegions = 3;

// Search dispatch options of one index handle: a snapshot of the BM25_*
// environment at bm25_index_create, changed by bm25_index_set_option
// (include/bm25mi.h lists the names).  Read per search — never cached in
// function statics — so every option takes effect on the next search.
struct SearchOpts {
  int flat = 1;            // 0: score_wave_kernel for every phase
  int flat_bw = 0;         // tiles per flat item: 0 = auto, else 1, 2, 4 or 8
  int items_per_wave = 4;  // auto flat_bw: halve while a phase gives fewer items per wave (c2: 4 > 8)
  int sample_p = 8;        // largest sampling stride (1: the exact pass over every tile)
  int list_cap = 0;        // candidate-list capacity per query (0: auto)
  int claim_ch = 1;        // flat items per claim
  int claim_m = 4;         // claim counters per XCD (1..kClaimM)
  int tile_bound = 1;      // REST skips tiles whose term-maxima sum is below theta (needs bmax)
  int theta_bound = 1;     // threshold keys from the tile bounds instead of a SAMPLE pass
                           // (needs bmax; search_geom)
  int count_skips = 0;     // REST counts the postings its tile bound skips (a build of its own)
  int grid_pct = 100;      // percent of the resident slots the persistent score kernels take
  int large_lists = 1;     // k > kMaxK: the list path (0: dense score rows for every query)
  int rest_split = 0;      // REST over split items where the waves get few items (measured: no gain)
  int bound_pool = 1;      // the tile-bound threshold from the pooled bounds (bpool / wbpool) where
                           // they hold >= kPoolGroupsPerK * k groups
  int filter_tiles = 1;    // filtered search, k <= kMaxK: the tile passes (0: dense score rows
                           // for every query)
  int bool_chunk = 0;      // boolean search: queries per chunk of masks (0: auto, <= 1 GiB of words)
  int tile_mask = 1;       // the tile bound refined by the sub-block presence masks (needs tmask;
                           // read at index build too: 0 there keeps the handle without the table)
  int seg_skip = 1;        // REST drops the term segments of a scored tile that lie in dead
                           // sub-blocks only (the pre-pass's per-lane bits; needs tile_mask)
  int row_skip = 1;        // ... and, of a heavy term's kept segment, the double rows whose
                           // postings all lie in dead sub-blocks (needs seg_skip and rowmask)
  int row_mask_kb = 262144;  // budget of the row-mask table in KiB, read at index build: the
                           // lightest heavy terms past it get no slot and keep all their rows
  int collapse_page = 0;   // collapsed search: results per page of a round (0: auto; clamped to
                           // [1, min(n_docs, kMaxK)])
  int collapse_chunk = 0;  // ... rows per sub-batch of the rounds under exclusion masks (0: auto,
                           // <= 1 GiB of mask words)
  int sorted_bins = 0;     // sorted search: histogram bins per level (0 or 1: auto, kSortedBins)
};

// What the last search launched (bm25_search_dispatch).
enum {
  kKFlatSample = 1, kKFlatRest = 2, kKFlatAll = 4,
  kKWaveSample = 8, kKWaveRest = 16, kKWaveAll = 32,
  kKLarge = 64,  // the large-k path (k > kMaxK): dense scores + radix selection
  kKBound = 128, // tile-bound threshold keys (bound_keys_kernel) instead of a SAMPLE pass
  kKBoundOff = 256,  // (not a kernel) the tile-bound threshold was off for this search:
                     // earlier ones overflowed with it (DevIndex::bound_weak)
  kKCountSkips = 512,  // (a flag) REST counted the postings its tile bound skipped
  kKRestSplit = 1024,  // (a flag) REST ran over split items (heavy queries' bands in pieces)
  kKBoundPool = 2048,  // (a flag) the tile-bound threshold came from the pooled bounds
  kKFiltered = 4096,   // the filtered search's tile passes (bm25mi_filter.hip)
  kKWeighted = 8192,   // (a flag) the search was weighted (bm25_search_weighted)
  kKAfter = 16384,     // (a flag) the search came through bm25_search_after(_device)
  kKTileSkip = 32768,  // tile_skip_kernel: the tile bounds' pre-pass of a flat REST launch
  kKSegSkip = 65536,   // (a flag) ... and it marked the dead term segments of scored tiles
  kKRowSkip = 131072,  // (a flag) ... and the dead rows of the heavy terms' kept segments
  kKCollapsed = 262144,  // (a flag) the search came through bm25_search_collapsed(_device)
};
struct Dispatch {
  uint32_t kernels = 0;       // kK* bits of the score kernels launched
  int32_t term_lanes = 0;     // flat kernel: term lanes per tile (8, 16, 32, 64)
  int32_t band_tiles[3] = {0, 0, 0};  // flat kernel: tiles per item of ALL, SAMPLE, REST
  int32_t sample_p = 0;       // sampling stride (1: exact pass, 0: tile-bound keys)
};

// Row stride of the tile-bound table: whole groups of four tiles (8 B).
__host__ __device__ inline int64_t bmax_stride(int64_t ntiles) { return (ntiles + 3) & ~(int64_t)3; }

// Row tiles of the REST pass's tile-skip table (eight u16 per tile), whole groups of four.
__host__ __device__ inline int64_t tskip_stride(int64_t ntiles) { return (ntiles + 3) & ~(int64_t)3; }

struct DevIndex {
  int device = 0;
  int64_t n_docs = 0, n_terms = 0, nnz = 0, doc_offset = 0;
  int tile_shift = kDefaultTileShift;
  bool nonneg = false;  // every CSC value is 0 or >= FLT_MIN (running sums are monotone)
  int64_t ntiles = 0;
  int64_t* indptr = nullptr;
  // Segment table, dense or sparse: the postings of term t in
  // tile j are [indptr[t] + r(t, j), indptr[t] + r(t, j + 1)) where
  //   dense:  r(t, j) = rel[t * (ntiles + 1) + j]          (V x (ntiles+1) u32)
  //   sparse: the term's non-empty tiles tl_tile[tl_ptr[t] .. tl_ptr[t+1])
  //           (ascending u16) with their first postings tl_start (u32,
  //           relative to indptr[t]) — O(non-empty (term, tile) pairs).
  bool sparse = false;
  uint32_t* rel = nullptr;
  int64_t* tl_ptr = nullptr;
  uint16_t* tl_tile = nullptr;
  uint32_t* tl_start = nullptr;
  int64_t n_pairs = 0;
  uint16_t* ldoc = nullptr;
  float* val = nullptr;
  double* val64 = nullptr;  // float64 values of the same postings (bm25.BM25's path; optional)
  // Tile bounds (dense segment table, non-negative index): each (term,
  // tile)'s largest score as f16 bits rounded DOWN, [V][bmax_stride] — a lower
  // bound of that score (threshold keys) and, one f16 step up, an upper bound
  // (the REST pass's tile skip)
  uint16_t* bmax = nullptr;
  // Sub-block presence masks beside bmax, [V][bmax_stride]: bit s of (term,
  // tile) is set when the term has a posting in the tile's s-th sub-block of
  // 2^(tile_shift - 5) documents (zero past the last tile).  A document only
  // collects terms whose bit of its sub-block is set, which tightens the tile
  // bound (tile_skip_kernel); null: the whole-tile bound alone
  uint32_t* tmask = nullptr;
  // Row presence masks of the heavy terms (row_skip; built where tmask is): a
  // term is heavy when one of its segments has two or more of REST's double
  // rows.  hslot[V]: the term's table slot h, -1 for a term that is not heavy
  // or that the table's budget (row_mask_kb; slots go by document frequency)
  // left out; rowmask[n_heavy][ntiles][kRowEntries]: bit s of entry r = row r
  // of the term's segment in the tile has a posting in sub-block s (all ones
  // in every entry of a segment of more than kRowEntries rows)
  int32_t* hslot = nullptr;
  uint32_t* rowmask = nullptr;
  int64_t n_heavy = 0;
  // The same bounds pooled over groups of kPool consecutive tiles (the max of
  // each group's entries, [V][pstride], pstride = bmax_stride(ceil(ntiles /
  // kPool))): the threshold kernel's input where it holds enough groups — a
  // group's bound is still <= one of its documents' scores, and distinct
  // groups hold distinct documents, at a quarter of the bytes
  uint16_t* bpool = nullptr;
  int64_t pstride = 0;
  // The tile-bound threshold is off for this handle's next searches: the
  // last ones that used it overflowed their candidate lists (weak bounds —
  // an index whose terms weigh alike); set by the host per search
  // (bm25mi_capi.cpp: bound_ok), read by search_geom
  bool bound_weak = false;
  // World tile bounds of a doc-sharded collection (bm25_index_set_world_
  // bounds): every shard's bmax rows, [wW][V][wstride] (a caller-owned device
  // buffer, zero past each shard's tiles), so a shard's search
  // (bm25_search_shard_device) takes the whole collection's tile-bound
  // threshold by itself — no key exchange; wtiles = the collection's tiles
  const uint16_t* wbmax = nullptr;
  int32_t wW = 0;
  int64_t wstride = 0;
  int64_t wtiles = 0;
  // ... and pooled as bpool (handle-owned, built by bm25_index_set_world_bounds):
  // [wW][V][wpstride], wpstride = bmax_stride(wstride / kPool); wgroups = the
  // collection's groups (each shard's ceil(tiles / kPool), summed)
  uint16_t* wbpool = nullptr;
  int64_t wpstride = 0;
  int64_t wgroups = 0;
  SearchOpts opt;
  mutable Dispatch disp;  // written by the launchers (callers hold the handle's mutex)
};

constexpr int kCounters = 16;  // Workspace::counters
constexpr int kRowEntries = 16;  // row masks of a (heavy term, tile)

// A handle's reusable scratch for the large-k paths (bm25mi_large.hip): one
// device allocation, bump-allocated by each search (nested uses stack), sized
// by the host before a search to what the last searches asked for — so a
// search makes no allocation of its own once the handle has seen its shape.
struct LargeArena {
  char* base = nullptr;
  size_t bytes = 0;
  size_t used = 0;     // bump offset of the live scratch users
  size_t need = 0;     // the most the last searches asked for
  int64_t budget = 0;  // bytes one search may take (large_budget(), fixed at first use)
};

// Scratch of one launch sequence.  With a handle's arena (LargeArena) the
// buffers come from it; what does not fit is allocated stream-ordered,
// released on `st` after everything enqueued so far, and counted, so the host
// grows the arena before the handle's next search: a large-k search then
// allocates nothing (each stream-ordered allocation and free cost the host
// ~0.1 ms: ~2 ms per search at c3, k = 10 000, before its first kernel).  The
// device's default pool keeps its default release threshold (the process's
// other users of the pool are not affected); what a handle retains is its
// arena, at most its budget (large_budget at first use), plus what the first
// search allocated stream-ordered until the pool trims it at a
// synchronisation.  At most budget bytes at a time: a nested launch sequence
// (the list path's dense rows) gets what its caller's scratch leaves.
struct Scratch {
  hipStream_t st;
  std::vector<void*> ptrs;
  LargeArena* ar;
  size_t start, total = 0;
  explicit Scratch(hipStream_t s, LargeArena* a = nullptr)
      : st(s), ar(a), start(a ? a->used : 0) {}
  template <class T>
  hipError_t get(T** p, int64_t n) {
    *p = nullptr;
    const size_t size = (sizeof(T) * (size_t)std::max<int64_t>(n, 1) + 255) & ~(size_t)255;
    total += size;
    if (ar && ar->base && ar->used + size <= ar->bytes) {
      *p = reinterpret_cast<T*>(ar->base + ar->used);
      ar->used += size;
      return hipSuccess;
    }
    const hipError_t e = hipMallocAsync((void**)p, size, st);
    if (e == hipSuccess) ptrs.push_back((void*)*p);
    return e;
  }
  ~Scratch() {
    if (ar) {
      ar->need = std::max(ar->need, start + total);
      ar->used = start;
    }
    for (void* p : ptrs) hipFreeAsync(p, st);
  }
};

struct Workspace {
  int64_t cap_q = 0, cap_k = 0;
  LargeArena* arena = nullptr;   // the handle's large-k scratch (null: per-search allocations)
  uint64_t* cand = nullptr;      // [Q][ntiles][kTileM] exact top-kTileM keys of sample (or all) tiles
  uint64_t* theta = nullptr;     // [Q] k-th best sample key
  uint64_t* list = nullptr;      // [Q][list_cap] keys above theta of the other tiles
  int32_t* list_cnt = nullptr;   // [Q] keys appended (> list_cap: overflow)
  int32_t list_cap = 0;
  int32_t* fb = nullptr;         // [Q] queries whose list overflowed (fallback stage)
  uint64_t* cand2 = nullptr;     // [Q][maxflag][k] exact top-k of re-scored tiles
  int32_t* flag_tiles = nullptr; // [Q][maxflag]
  int32_t* nflag = nullptr;      // [Q]
  int32_t* queue = nullptr;      // [Q*maxflag] items = qi*maxflag + i
  int32_t* counters = nullptr;   // [kCounters]: [0]/[1] rescore queue length / pop cursor,
                                 // [2] fallback queries, [3] tiles re-scored this search,
                                 // [4] queries left to the block merge (slow),
                                 // [5] (query, tile) pairs REST skipped by their tile bound,
                                 // [6..7] (a u64) the postings of those pairs,
                                 // [8] term segments REST dropped in the tiles it scored,
                                 // [10..11] (a u64) their postings,
                                 // [9] double rows REST dropped in the segments it kept,
                                 // [12..13] (a u64) their postings
  int32_t* slow = nullptr;       // [Q] those queries
  // the large-k list path's REST (bm25mi_large.hip sets them on its copy):
  // per-(query, tile) slots of slot_cap keys and their counts; null otherwise
  uint64_t* slots = nullptr;
  int32_t* slot_cnt = nullptr;
  int32_t slot_cap = 0;
  int32_t* wctr = nullptr;       // [kWctrRegions][kWctrInts] item-claim counters: zeroed once
                                 // at allocation; the last wave of each counter's sharers
                                 // re-zeroes it (and its finished count) at the end of every
                                 // flat launch, so each launch finds its region zeroed
  int32_t* report = nullptr;     // host-mapped [2]: merge_tail_kernel writes the search's
                                 // fallback query count, then `seq` (null: no report)
  int32_t seq = 0;               // the search's sequence number on its handle
  // split REST items (bound_keys_kernel builds the table per search): per
  // query its weight, then the band's item table (<= 8 per query), the items
  // per band, and the finished-block count of the build (self-resetting)
  uint32_t* qw = nullptr;
  uint32_t* sub = nullptr;
  int32_t* sub_ipb = nullptr;
  int32_t* sub_done = nullptr;
  uint16_t* tskip = nullptr;     // [Q][tskip_stride(ntiles)][8]: a u16 per (query, tile, term
                                 // lane) — 0 = REST drops the lane's segment (all eight: it
                                 // skips the tile), 0xFFFF = every row runs, else bit r = row r
                                 // runs (tile_skip_kernel writes every word of the searched
                                 // rows before each REST launch)
  uint64_t* seg = nullptr;       // sparse index: [Q][tiles/8][TT][8] segment of each (query,
                                 // term position, tile) (start | len << 32), built per search
  int64_t cap_seg = 0;           // u64 entries of seg
};

// Flag slots per query: a flagged tile holds kTileM keys of the top-(k-1), so
// at most (k-1)/kTileM tiles (and never more than the candidate tiles).
inline int64_t maxflag_for(int k, int64_t ntiles) {
  const int64_t m = (k + kTileM - 1) / kTileM;
  return m < ntiles ? m : (ntiles > 0 ? ntiles : 1);
}

// Threshold geometry of a search over W doc shards of ntiles tiles each:
// stride P (1 = no sampling), m keys per sample tile, S keys per query per
// shard, sample tiles in groups of G consecutive tiles (one group per G*P).
// P = 0: no SAMPLE pass — each shard's S best tile-bound keys
// (bound_keys_kernel).
struct SampleGeom {
  int P, m;
  int64_t S;
  int G;  // sample tiles come in groups of G consecutive tiles (bm25mi_kernels.hip)
};
SampleGeom sample_geom(int64_t ntiles, int k, int W, int pmax);
// The geometry a search of T-term queries takes: tile-bound keys when the
// handle has tile bounds (and the theta_bound option) and the queries are
// short, else sample_geom; the key width S is sample_geom's either way.
// ntiles: the widest shard's tiles (every shard of a search must take the
// same geometry).
SampleGeom search_geom(const DevIndex& ix, int64_t ntiles, int k, int W, int64_t T);
// Most tiles a shard may have for tile-bound keys (one wave's LDS per query).
constexpr int64_t kBoundMaxTiles = 30720;
// ... and at least this many tiles per wanted key over the whole collection.
constexpr int64_t kBoundTilesPerK = 16;
// Pooled bounds: tiles per group, and the groups per wanted key the pooled
// threshold needs (else the per-tile bounds: top-k tiles sharing a group
// lower the threshold by about k^2 (kPool - 1) / (2 ntiles) ranks).
constexpr int64_t kPool = 4;
constexpr int64_t kPoolGroupsPerK = 8;
// ... and queries of at most this many terms (search_geom; the bound kernel's
// per-tile loads in flight).
#ifndef BM25_BOUND_TERMS
#define BM25_BOUND_TERMS 16
#endif
constexpr int64_t kBoundMaxTerms = BM25_BOUND_TERMS;

// Kernel launchers (bm25mi_kernels.hip).  All enqueue on `stream`.
hipError_t launch_build_tables(const DevIndex& ix, const int32_t* d_indices,
                               int32_t* d_err, hipStream_t stream);
// Tile bounds ix.bmax from the dense segment table and the scores.
hipError_t launch_build_bmax(const DevIndex& ix, hipStream_t stream);
// Sub-block presence masks ix.tmask from the dense segment table and ldoc.
hipError_t launch_build_tmask(const DevIndex& ix, hipStream_t stream);
// Row presence masks (row_skip): heavy[t] = term t has a segment of two or
// more double rows; then ix.rowmask for the ix.n_heavy terms d_hterm lists.
hipError_t launch_heavy_terms(const DevIndex& ix, int32_t* d_heavy, hipStream_t stream);
hipError_t launch_build_rowmask(const DevIndex& ix, const int32_t* d_hterm, hipStream_t stream);
// out[r][g] = the max of in[r][kPool g .. kPool g + kPool - 1] (u16 f16 bits,
// all >= 0) for rows r < rows, g < out_stride (zero past in_stride).
hipError_t launch_pool_bounds(const uint16_t* in, int64_t rows, int64_t in_stride, uint16_t* out,
                              int64_t out_stride, hipStream_t stream);
// Sparse segment table: non-empty tiles per term -> d_cnt[V] (also writes
// ldoc and validates, as launch_build_tables), then (after the caller's scan
// into ix.tl_ptr) the tile lists.
hipError_t launch_count_tiles(const DevIndex& ix, const int32_t* d_indices, int64_t* d_cnt,
                              int32_t* d_err, hipStream_t stream);
hipError_t launch_fill_tiles(const DevIndex& ix, const int32_t* d_indices, hipStream_t stream);
// u64 entries of Workspace::seg a search of Q queries of T terms needs (0:
// dense index, or a search the flat kernel does not serve).
int64_t seg_entries(const DevIndex& ix, int64_t Q, int64_t T);
// Score pass of a single-index search: SAMPLE + theta + REST (or the exact
// pass when the index is too small to sample).
// The threshold geometry of a search; world (a shard with world bounds): the
// collection's tile-bound threshold when it serves (P = 0), else the shard's own.
SampleGeom shard_geom_world(const DevIndex& ix, int k, int64_t T, bool world);
// world: the threshold from the world tile bounds (ix.wbmax; a shard's
// search for the W-way merge), else from this index's own.
hipError_t launch_score(const DevIndex& ix, const int32_t* d_queries, int64_t Q, int64_t T,
                        int k, const Workspace& ws, hipStream_t stream, bool world = false);
// The same in two halves for W doc shards searched together: each shard's
// sample keys [Q][g.S] -> (all-gather across shards) -> theta over [W][Q][g.S]
// + REST.
hipError_t launch_sample(const DevIndex& ix, const int32_t* d_queries, int64_t Q, int64_t T,
                         const SampleGeom& g, uint64_t* keys, const Workspace& ws,
                         hipStream_t stream);
// rest_stream (when not null and not `stream`): the REST pass runs there,
// after theta (join: recorded on `stream`, waited on rest_stream); rest_timing
// (optional) is recorded on rest_stream just before the REST pass.
hipError_t launch_finish(const DevIndex& ix, const int32_t* d_queries, int64_t Q, int64_t T,
                         int k, const SampleGeom& g, int W, const uint64_t* all_keys,
                         const Workspace& ws, hipStream_t stream,
                         hipStream_t rest_stream = nullptr, hipEvent_t join = nullptr,
                         hipEvent_t rest_timing = nullptr);
// Merge (+ rescore + final merge), then the exact fallback stage; P = the
// search's sampling stride.  unsorted: a doc shard's list for the W-way merge
// (the keys >= its k-th key in no order, padding last: merge_fast skips the
// sort; the fallback stages still write sorted lists).
hipError_t launch_select(const DevIndex& ix, const int32_t* d_queries,
                         int64_t Q, int64_t T, int k, int P, const Workspace& ws,
                         int32_t* d_docs, float* d_scores, hipStream_t stream, bool unsorted = false);
hipError_t launch_scores_dense(const DevIndex& ix, const int32_t* d_query,
                               int64_t T, float* d_out, hipStream_t stream);
// Scores of given (query, document) pairs (bm25mi_lookup.hip): d_out[q * C + c]
// = the fp32 sum, in query order from +0.0f, of the index values of
// (d_queries[q][*], d_docs[q * C + c]) — element d_docs[..] - doc_offset of
// launch_scores_dense's row.  d_docs holds global ids; a negative id or one
// outside [doc_offset, doc_offset + n_docs) scores +0.0f.  Reads the index
// arrays only (no workspace).  d_weights [Q][T] (or null): every value found
// enters as the fp32 product weight * value (bm25_score_docs_weighted).
hipError_t launch_score_docs(const DevIndex& ix, const int32_t* d_queries, int64_t Q, int64_t T,
                             const int32_t* d_docs, int64_t C, float* d_out, hipStream_t stream,
                             const float* d_weights = nullptr);
// W lists [Q, k] at element w * rank_stride (docs and scores alike) -> [Q, k];
// sorted: every list is already best-first (W-way merge instead of a sort).
hipError_t launch_merge_lists(const int32_t* d_docs, const float* d_scores,
                              int64_t W, int64_t Q, int k, int64_t rank_stride, bool sorted,
                              int32_t* d_out_docs, float* d_out_scores, hipStream_t stream);

// Dense scores of G queries (rows of T terms) into d_out[g * stride + doc];
// stride >= ntiles << tile_shift (whole tiles are stored; docs past n_docs
// hold 0).  G <= 65535.  d_weights [G][T] (or null): the terms' weights of the
// weighted search, every posting entering as the fp32 product weight * value.
hipError_t launch_scores_batch(const DevIndex& ix, const int32_t* d_queries, int64_t G, int64_t T,
                               int64_t stride, float* d_out, hipStream_t stream,
                               const float* d_weights = nullptr);

// Exact top-k for any k (the path of k > kMaxK, bm25mi_large.hip): per chunk
// of queries the dense scores, a radix selection of the k-th key, the keys
// >= it compacted and sorted.  k > n_docs (a doc shard smaller than k) pads
// each row with doc -1 / score bits 0xFFFFFFFF.  Scratch comes from the
// handle's arena; what does not fit is taken stream-ordered (hipMallocAsync)
// and released at the end of the launch sequence.  budget: the bytes this
// call may take (<= 0: the arena's budget; a nested call passes what its
// caller leaves).
hipError_t launch_search_large(const DevIndex& ix, const int32_t* d_queries, int64_t Q, int64_t T,
                               int k, int32_t* d_docs, float* d_scores, hipStream_t stream,
                               LargeArena* arena = nullptr, int64_t budget = 0);
// The large-k list path's passes (bm25mi_kernels.hip; used by
// bm25mi_large.hip): SAMPLE with kLargeM keys per sample tile into keys[Q][g.S]
// (g.m == kLargeM), and REST into the workspace's theta / list / list_cnt /
// list_cap (the caller's buffers).  large_list_supported: the flat kernel
// serves the batch and the index is non-negative.
hipError_t launch_sample_large(const DevIndex& ix, const int32_t* d_queries, int64_t Q, int64_t T,
                               const SampleGeom& g, uint64_t* keys, const Workspace& ws,
                               hipStream_t stream);
hipError_t launch_rest_lists(const DevIndex& ix, const int32_t* d_queries, int64_t Q, int64_t T,
                             const SampleGeom& g, const Workspace& ws, hipStream_t stream);
bool large_list_supported(const DevIndex& ix, int64_t T, int64_t Q);

// The large-k list path (bm25mi_large.hip) for kMaxK < k <= kLargeListMaxK:
// large_geom's SAMPLE (P = 0: not applicable), theta, REST into lists, the
// k-th key of each list, compaction and a row sort; queries the lists cannot
// serve go through launch_search_large on their own (*n_fallback of them;
// the path synchronises the stream once to count them).  ws: the handle's
// workspace (claim counters, counters, segment table).
constexpr int64_t kLargeListMaxK = 131072;
SampleGeom large_geom(const DevIndex& ix, int64_t k);
hipError_t launch_search_large_lists(const DevIndex& ix, const int32_t* d_queries, int64_t Q,
                                     int64_t T, int k, const Workspace& ws, int32_t* d_docs,
                                     float* d_scores, int64_t* n_fallback, hipStream_t stream);

// W lists [Q, k] (docs and scores at element w * rank_stride) -> the best k
// of each query by (score desc, doc asc), for any k (a segmented sort of the
// W k keys of each query).  Padding (doc -1, score bits ~0) sorts last.
hipError_t launch_merge_large(const int32_t* d_docs, const float* d_scores, int64_t W, int64_t Q,
                              int k, int64_t rank_stride, int32_t* d_out_docs,
                              float* d_out_scores, hipStream_t stream);

// Filtered search (bm25_search_filtered).  Masks are [M][W] u32, W =
// ceil(n_docs / 32), bit d & 31 of word d >> 5 = handle-local document d;
// d_query_mask [Q] picks each query's mask (-1: no filter; null: mask 0 for
// every query).  No kernel reads a mask word at index >= W, and bits at or
// past n_docs never count.  d_weights [Q][T] (or null) makes the search the
// weighted one (bm25_search_weighted): every launch below scores with the
// fp32 products weight * value in place of the values; then M == 0 with a null
// d_query_mask means no filter for every query.
//
// The tile passes (bm25mi_kernels.hip): the allowed documents of every (mask,
// tile) into d_census[M][ntiles] and of every mask into d_total[M] (zeroed by
// the caller); pass A: the best kTileM allowed keys of every (query, tile)
// into d_cand[Q][ntiles][kTileM] (handle-local ids), no posting read where the
// census is 0 (*d_skipped += those pairs); pass B: the pairs whose best key
// is >= d_theta[q] scored again (*d_rescored += them), their allowed keys >=
// theta appended to d_list[q][C] (d_list_cnt[q] counts past C: overflow).
// d_ckey [Q] (or null; bm25_search_after): the cursor instantiations — only
// keys < d_ckey[q] are candidates (pass A) and emitted (pass B); a row whose
// key is 0 reads no posting and counts in *d_skipped.
hipError_t launch_filter_census(const DevIndex& ix, const uint32_t* d_masks, int64_t M,
                                int32_t* d_census, uint32_t* d_total, hipStream_t stream);
hipError_t launch_filter_pass_a(const DevIndex& ix, const int32_t* d_queries, int64_t Q, int64_t T,
                                const uint32_t* d_masks, const int32_t* d_query_mask,
                                const int32_t* d_census, uint64_t* d_cand, int32_t* d_skipped,
                                hipStream_t stream, const float* d_weights = nullptr,
                                const uint64_t* d_ckey = nullptr);
hipError_t launch_filter_pass_b(const DevIndex& ix, const int32_t* d_queries, int64_t Q, int64_t T,
                                const uint32_t* d_masks, const int32_t* d_query_mask,
                                const uint64_t* d_cand, const uint64_t* d_theta, uint64_t* d_list,
                                int32_t* d_list_cnt, int32_t C, int32_t* d_rescored,
                                hipStream_t stream, const float* d_weights = nullptr,
                                const uint64_t* d_ckey = nullptr);
// The dense path (bm25mi_large.hip), exact for every k, index and mask: per
// chunk of queries the dense scores, the radix selection with the mask
// applied where keys are formed and k_q = min(k, allowed documents of the
// query's mask) (d_total, as launch_filter_census wrote it), the row sort and
// the padded write.  d_ids (or null) names the nq rows of the batch to serve
// (a device array): their queries are gathered and their results scattered
// into d_docs / d_scores [Q][k]; otherwise nq = Q rows in order.  d_ckey [Q]
// (or null): the batch's cursor keys, gathered with the rows; k_q is then
// clamped to the row's eligible keys by the selection's first digit pass.
hipError_t launch_search_filtered_dense(const DevIndex& ix, const int32_t* d_queries, int64_t T,
                                        int k, const uint32_t* d_masks,
                                        const int32_t* d_query_mask, const uint32_t* d_total,
                                        const int32_t* d_ids, int64_t nq, int32_t* d_docs,
                                        float* d_scores, hipStream_t stream, LargeArena* arena,
                                        const float* d_weights = nullptr,
                                        const uint64_t* d_ckey = nullptr);
// The whole filtered search (bm25mi_filter.hip): the census, then the tile
// passes (k <= kMaxK and the filter_tiles option), theta, the lists' sort and
// padded write, and the dense path for the queries whose list overflowed —
// their number is read with the one host synchronisation of the call — or
// the dense path for every query.  ws: the handle's workspace sized for (Q, T,
// min(k, kMaxK)); counters [2] / [5] / [3] = queries handed to the dense path
// by the tile passes / pairs pass A skipped / pairs pass B re-scored.
// *n_dense: queries the dense path served.
// d_after_scores / d_after_docs [Q] (both or neither; bm25_search_after): row
// q returns the documents strictly after the cursor (score, global doc id) in
// the result order; d_after_docs[q] < -1: no cursor, -1: an exhausted list
// (all padding, no posting read).  Then M == 0 with a null d_query_mask means
// no filter for every query, as with weights.
hipError_t launch_search_filtered(const DevIndex& ix, const int32_t* d_queries, int64_t Q,
                                  int64_t T, int k, const uint32_t* d_masks, int64_t M,
                                  const int32_t* d_query_mask, const Workspace& ws,
                                  int32_t* d_docs, float* d_scores, int64_t* n_dense,
                                  hipStream_t stream, const float* d_weights = nullptr,
                                  const float* d_after_scores = nullptr,
                                  const int32_t* d_after_docs = nullptr);

// Boolean term filters as allow-masks (bm25mi_termmask.hip): d_out[M][W] in
// the layout above, row m = the documents d < n_docs that d_base allows
// ([Mb][W], Mb = 0 (null: every document), 1 (one row for every mask) or M),
// that every id >= 0 of d_must[m][A] has, that some id >= 0 of d_any[m][B] has
// (when it holds one) and that no id >= 0 of d_must_not[m][N] has.  has(t, d):
// the index stores a posting of (t, d), whatever its value; negative ids are
// padding, an id >= n_terms is a term that no document has.  Every word of
// every row is written (bits at or past n_docs as 0), no word at index >= W
// is read or written.  Reads the index arrays only (no workspace).
// d_min_match [M] (null: the kernel of the calls without it): row m's any
// clause asks for d_min_match[m] of its slots with an id >= 0 — a repeated id
// counts each time — and for nothing where that is <= 0; B <= 65535 then.
hipError_t launch_term_masks(const DevIndex& ix, const int32_t* d_must, int64_t A,
                             const int32_t* d_any, int64_t B, const int32_t* d_must_not, int64_t N,
                             int64_t M, const uint32_t* d_base, int64_t Mb, uint32_t* d_out,
                             hipStream_t stream, const int32_t* d_min_match = nullptr);

// d_counts[m] = the set bits of d_masks[m][W] among bits 0 .. n_docs - 1 (the
// bits at or past n_docs of the last word are ignored).  d_counts need not be
// zeroed; integer sums, so the result does not depend on scheduling.
hipError_t launch_mask_count(const DevIndex& ix, const uint32_t* d_masks, int64_t M,
                             int64_t* d_counts, hipStream_t stream);

// Facet counts (bm25mi_facets.hip): d_counts[m][g], [M, G] int64 with
// contiguous rows, = the documents d < n_docs with bit d of d_masks[m][W] set
// and d_groups[d] == g; a d_groups[d] outside [0, G) counts nowhere.  Every
// entry is written (d_counts need not be zeroed), bits at or past n_docs of
// the last word are ignored, no mask word at index >= W of a row and no
// d_groups entry at index >= n_docs is read.  Integer sums.  G <= kFacetBins:
// facet_rows(G) rows share one read of a chunk's groups, their bins in LDS;
// wider G: a row per pass, global atomics.  facet_chunk_docs: the documents
// of a workgroup's chunk on the route that (G, M) takes.
constexpr int64_t kFacetBins = 8192;          // u32 LDS bins of a workgroup (32 KiB)
constexpr int64_t kFacetMaxRows = 64;         // mask rows of a row block, at most
constexpr int64_t kFacetMinChunk = 8192;      // documents of a chunk, LDS route: 8 per bin,
constexpr int64_t kFacetMaxChunk = 65536;     //   within these,
constexpr int64_t kFacetChunkStep = 1024;     //   rounded up to a multiple of this
constexpr int64_t kFacetGlobalChunk = 16384;  // documents of a chunk, global route
int64_t facet_rows(int64_t G);
int64_t facet_chunk_docs(int64_t G, int64_t M);
hipError_t launch_mask_facets(const DevIndex& ix, const uint32_t* d_masks, int64_t M,
                              const int32_t* d_groups, int64_t G, int64_t* d_counts,
                              hipStream_t stream);

// Field statistics (bm25mi_stats.hip; bm25_mask_stats of include/bm25mi.h):
// count, min, max and sum of d_values (kind: kField* below) over the documents
// each row of d_masks[M][W] allows, per bucket: B = 1 bucket a row holding
// every allowed document (d_groups null and G == 0), else B = G buckets by
// d_groups[d] (an id outside [0, G) is in no bucket).  A float32 NaN is no
// value.  Outputs [M][B], every entry written: d_count int64; d_min / d_max of
// the column's type; d_sum int64 (integer kinds, wrapping) or float64 (the
// exact sum rounded once, bm25mi_stats_sum.h); the last three may be null.
// Bits at or past n_docs are ignored, no mask word at index >= W of a row and
// no d_values / d_groups entry at index >= n_docs is read.  d_scratch:
// stats_scratch_bytes(kind, M, G) bytes, 8-byte aligned — a record of
// stats_slots(kind) u64 per bucket (count, ~min key, max key, sum or inf
// counters, then the 32 float bins), cleared by the launch on its stream,
// accumulated with integer atomics only and turned into the outputs by a
// finalise kernel.  B <= stats_lds_buckets(kind): stats_rows(kind, B) rows
// share one read of a chunk's column, their records in LDS; wider: a row per
// item, global atomics.  A chunk is kStatsChunk documents on both routes.
constexpr int64_t kStatsLdsSlots = 4608;   // u64 LDS slots of a workgroup (36 KiB)
constexpr int64_t kStatsMaxRows = 64;      // mask rows of a row block, at most
constexpr int64_t kStatsChunk = 8192;      // documents of a workgroup's chunk
constexpr int64_t kStatsIntSlots = 4;      // count, ~min key, max key, sum
constexpr int64_t kStatsF32Slots = 36;     // count, ~min key, max key, infs, 32 bins (288 B)
inline int64_t stats_slots(int kind) { return kind == 1 ? kStatsF32Slots : kStatsIntSlots; }
inline int64_t stats_lds_buckets(int kind) { return kStatsLdsSlots / stats_slots(kind); }
inline int64_t stats_rows(int kind, int64_t B) {
  return std::max<int64_t>(1, std::min<int64_t>(kStatsMaxRows, stats_lds_buckets(kind) / B));
}
// (-1: M * B records do not fit an int64 of bytes)
inline int64_t stats_scratch_bytes(int kind, int64_t M, int64_t G) {
  const int64_t B = G > 0 ? G : 1, rec = 8 * stats_slots(kind);
  if (M > 0 && B > (int64_t)0x7FFFFFFFFFFFFFFFll / rec / M) return -1;
  return std::max<int64_t>(M, 0) * B * rec;
}
hipError_t launch_mask_stats(const DevIndex& ix, const uint32_t* d_masks, int64_t M,
                             const void* d_values, int kind, const int32_t* d_groups, int64_t G,
                             int64_t* d_count, void* d_min, void* d_max, void* d_sum,
                             void* d_scratch, hipStream_t stream);

// Numeric range filters (bm25mi_range.hip): d_out[M][W] in the layout above,
// row m = the documents d < n_docs that d_base allows ([Mb][W], Mb = 0 (null:
// every document), 1 or M, exactly launch_term_masks' base) and whose fields
// pass every clause of the row: for every c with f = d_fields[m][c] >= 0,
// d_lo[m][c] <= d_values[f][d] <= d_hi[m][c] in the values' own type (kind:
// BM25_FIELD_I32 / _F32 / _I64; d_values [F][n_docs], d_lo and d_hi [M][C] of
// that type).  A field id >= F is a field that no document has: the clause
// matches nothing and no value is read.  Every word of every row is written
// (bits at or past n_docs as 0, even where d_base has them set), no word at
// index >= W of a row is read or written, no d_values entry at index >= n_docs
// of a field row is read.  Reads the caller's buffers only; no atomics, no
// scratch.  d_base and d_out must not overlap.  A workgroup takes a chunk of
// kRangeChunkDocs documents and a block of up to kRangeRows rows; each of its
// waves walks spans of kRangeSpanDocs documents in steps of 64.  Rows of up
// to kRangeRegClauses clauses stay in the lanes' registers (kernels for 1, 2,
// 4 and 8 of them); wider rows are read from memory per (step, row).
enum { kFieldI32 = 0, kFieldF32 = 1, kFieldI64 = 2 };  // BM25_FIELD_* (include/bm25mi.h)
constexpr int64_t kRangeRows = 64;          // mask rows of a row block (a lane per row)
constexpr int64_t kRangeSpanDocs = 256;      // documents of a wave's span (8 words per lane)
constexpr int64_t kRangeChunkDocs = 4096;    // documents of a workgroup's chunk (4 spans a wave)
constexpr int64_t kRangeRegClauses = 8;      // clauses a row up to which a lane keeps them in registers
hipError_t launch_range_masks(const DevIndex& ix, const void* d_values, int kind, int64_t F,
                              const int32_t* d_fields, const void* d_lo, const void* d_hi,
                              int64_t C, int64_t M, const uint32_t* d_base, int64_t Mb,
                              uint32_t* d_out, hipStream_t stream);

// Sort-by-field search (bm25mi_sorted.hip; bm25_sort_ranks / bm25_search_sorted,
// include/bm25mi.h).
//   launch_sort_ranks: the order of the n_docs documents by (d_values' column
//     order, doc id ascending) as d_perm[r] = the document at rank r and
//     d_ranks[d] = the rank of document d (kind: kField*; descending reverses
//     the numbers only, NaN stays last).  A setup call: it allocates the sort's
//     buffers (24 B per document, two (u64 key, u32 value) arrays, plus
//     radix_sort_scratch_bytes), synchronises `stream` and frees them.
//   launch_search_sorted: row m of d_docs / d_out_ranks [M][k] = the k documents
//     of smallest rank among those d_masks[m][W] allows (null: every document)
//     with d_ranks[d] > d_after[m] (null or < -1: no cursor; -1: an all-padding
//     row), as (d_perm[rank] + doc_offset, rank), padded with -1 / -1.  Reads no
//     mask word at index >= W of a row, ignores bits at or past n_docs, treats a
//     rank outside [0, n_docs) as never eligible, and writes nothing outside
//     the outputs and d_scratch (sorted_scratch_bytes(n_docs, M, k) bytes, 4-byte
//     aligned) whatever d_ranks and d_perm hold.  Integer only; the global
//     atomics are integer adds.  0 < k <= min(n_docs, kMaxK).  bins: histogram
//     bins per level (< 2: kSortedBins; at most kSortedBins).
//   launch_sorted_pad_scores: d_scores[i] = bits 0xFFFFFFFF where d_docs[i] < 0.
// Selection geometry: a workgroup takes a slice of documents and a block of
// kSortedRows mask rows; each of its waves walks spans of kSortedSpanDocs
// documents in steps of 64; a row's rank interval is narrowed level by level
// until it is at most kSortedWmax ranks wide, then collected and sorted in LDS.
constexpr int64_t kSortedRows = 32;        // mask rows of a row block (LDS bins per row)
constexpr int64_t kSortedSpanDocs = 256;   // documents of a wave's span (8 words per lane)
constexpr int64_t kSortedRoundDocs = 1024; // documents of a workgroup's round (4 spans)
constexpr int64_t kSortedBins = 256;       // histogram bins per level, at most (and automatic)
constexpr int64_t kSortedWmax = 2048;      // a row's interval is collected at this width
constexpr int64_t kSortedSortP = 8192;     // keys the row sort holds in LDS
static_assert(kMaxK + kSortedWmax <= kSortedSortP, "a row's list fits the LDS sort");
inline int64_t sorted_list_cap(int64_t n_docs, int64_t k) {
  return std::min<int64_t>(k + kSortedWmax, n_docs);
}
// bytes = 4 M (4 state + 1 count + kSortedBins histogram + sorted_list_cap list)
inline int64_t sorted_scratch_bytes(int64_t n_docs, int64_t M, int64_t k) {
  return 4 * M * (4 + 1 + kSortedBins + sorted_list_cap(n_docs, k));
}
hipError_t launch_sort_ranks(const DevIndex& ix, const void* d_values, int kind, bool descending,
                             int32_t* d_ranks, int32_t* d_perm, hipStream_t stream);
hipError_t launch_search_sorted(const DevIndex& ix, const uint32_t* d_masks, int64_t M,
                                const int32_t* d_ranks, const int32_t* d_perm, int32_t k,
                                const int32_t* d_after, int32_t* d_docs, int32_t* d_out_ranks,
                                void* d_scratch, int bins, hipStream_t stream);
hipError_t launch_sorted_pad_scores(const int32_t* d_docs, float* d_scores, int64_t n,
                                    hipStream_t stream);

// Field collapsing (bm25mi_collapse.hip; the loop is run_collapsed of
// bm25mi_capi.cpp).  State by row q of the call: d_count[q] hits kept so far
// in d_docs / d_scores / d_out_groups [Q][k], and the row's next cursor
// (d_cur_scores[q], d_cur_docs[q]) — a doc of -1: the row is finished, and
// every kernel below leaves such a row alone; before the first page the
// cursors' docs are < -1 and the counts 0.
//   launch_collapse_page: rows r < R of a batch of pages ([R][p] global docs
//     and scores in rank order, padded as the cursor search pads) walked into
//     rows d_row_map[r] (null: r) under groups [n_docs] and per_group; the
//     rest of a row that finished short of k is padded (doc -1, score bits ~0,
//     group -1).  d_ctr[0] += rows left unfinished, d_ctr[1] += over-quota page
//     entries ahead of a row's last kept one (plain sums).  k <= kMaxK.
//   launch_collapse_compact: d_rows[0 .. U) = the unfinished rows, ascending.
//   launch_collapse_gather: compact rows r < R (rows d_rows[r]): their queries
//     [R][T], weights (when d_weights), cursors and mask ids (r).
//   launch_collapse_exclude: d_excl[R][W] = row d_rows[r]'s own mask (d_masks
//     [M][W] by d_query_mask, as the filtered search reads them; all ones
//     without one) minus every document of a group with per_group kept hits;
//     zeros for a finished row.  Every word is written, bits at or past n_docs
//     are 0, no word at index >= W of a row and no d_groups entry at index >=
//     n_docs is touched.
int collapse_slots(int k);  // slots of the LDS group table at k (8 B each)
hipError_t launch_collapse_page(const int32_t* d_page_docs, const float* d_page_scores, int32_t p,
                                const int32_t* d_row_map, int64_t R, const int32_t* d_groups,
                                int64_t n_docs, int64_t doc_offset, int32_t per_group, int32_t k,
                                int32_t* d_count, int32_t* d_docs, float* d_scores,
                                int32_t* d_out_groups, float* d_cur_scores, int32_t* d_cur_docs,
                                unsigned long long* d_ctr, hipStream_t stream);
hipError_t launch_collapse_compact(const int32_t* d_cur_docs, int64_t Q, int32_t* d_rows,
                                   hipStream_t stream);
hipError_t launch_collapse_gather(const int32_t* d_rows, int64_t R, const int32_t* d_queries,
                                  const float* d_weights, int64_t T, const float* d_cur_scores,
                                  const int32_t* d_cur_docs, int32_t* d_cq, float* d_cw,
                                  float* d_as, int32_t* d_ad, int32_t* d_ids, hipStream_t stream);
hipError_t launch_collapse_exclude(const int32_t* d_rows, int64_t R, const uint32_t* d_masks,
                                   int64_t M, const int32_t* d_query_mask, const int32_t* d_groups,
                                   int64_t n_docs, int32_t per_group, int32_t k,
                                   const int32_t* d_count, const int32_t* d_out_groups,
                                   const int32_t* d_cur_docs, uint32_t* d_excl,
                                   hipStream_t stream);

// The doc-shard merge of collapsed lists (bm25mi_merge_collapse.hip;
// bm25_merge_collapsed_device): W best-first lists [Q, k] of (doc, score,
// group) at element w * rank_stride of the three inputs, padding (doc < 0)
// last -> row q = the first k kept entries of the walk of the merged order
// under per_group, padded (doc -1, score bits ~0, group -1); d_out_groups may
// be null.  Every output slot is written.  1 <= W <= 64, k <= kMaxK.
hipError_t launch_merge_collapsed(const int32_t* d_docs, const float* d_scores,
                                  const int32_t* d_groups, int64_t W, int64_t Q, int32_t k,
                                  int64_t rank_stride, int32_t per_group, int32_t* d_out_docs,
                                  float* d_out_scores, int32_t* d_out_groups, hipStream_t stream);

// Sort-by-field search over doc shards (bm25mi_sorted_shards.hip;
// bm25_sort_keys_device / bm25_sort_cursor_device / bm25_merge_sort_keys_device).
// The order key K of a value is sort_key() of bm25mi_sort_key_dev.h, carried as
// two uint32 planes (hi, lo); the collection's order is (K, global doc id).
//   launch_sort_keys: element i < n of the planes = K(d_values[d_docs[i] -
//     doc_offset]); a doc id < 0 or outside the handle's documents gets the
//     padding key (all ones) and reads no value.
//   launch_sort_cursor: d_after_ranks[m] = the rank cursor of
//     launch_search_sorted for the collection cursor (key, d_after_docs[m]):
//     -1 for doc -1, -2 for doc < -1, else c - 1 (-2 when c == 0) with c = the
//     handle's documents at or before the cursor, by a binary search of d_perm.
//     A d_perm entry outside [0, n_docs) reads no value.
//   launch_merge_sort_keys: W lists [Q, k] of (doc, key) at element w *
//     rank_stride of the three inputs, each ascending by (key, doc) up to its
//     first doc < 0 -> row q = the first k of the union, padded (doc -1, key all
//     ones).  Every output slot is written.  1 <= W <= 64, k <= kMaxK.
hipError_t launch_sort_keys(const DevIndex& ix, const void* d_values, int kind, bool descending,
                            const int32_t* d_docs, int64_t n, uint32_t* d_key_hi,
                            uint32_t* d_key_lo, hipStream_t stream);
hipError_t launch_sort_cursor(const DevIndex& ix, const void* d_values, int kind, bool descending,
                              const int32_t* d_perm, const uint32_t* d_after_hi,
                              const uint32_t* d_after_lo, const int32_t* d_after_docs, int64_t M,
                              int32_t* d_after_ranks, hipStream_t stream);
hipError_t launch_merge_sort_keys(const int32_t* d_docs, const uint32_t* d_key_hi,
                                  const uint32_t* d_key_lo, int64_t W, int64_t Q, int32_t k,
                                  int64_t rank_stride, int32_t* d_out_docs, uint32_t* d_out_key_hi,
                                  uint32_t* d_out_key_lo, hipStream_t stream);

// Largest token id of [n] device ids (0 if none is positive) into *d_out.
hipError_t launch_max_token(const int32_t* d_queries, int64_t n, int32_t* d_out,
                            hipStream_t stream);

// Tile shifts with compiled kernels, and the one a new index takes.
bool tile_shift_supported(int s);
int build_tile_shift();

// Device sort and scan (bm25mi_sort.hip; hand-written, no hipCUB).
// Stable LSD radix sort of n (u64 key, u32 value) pairs: by the key bits
// [key_bits_lo, key_bits_hi) (descending: of ~key), then by the value bits
// [0, val_bits_hi) (vals may be null when val_bits_hi == 0).  keys_alt /
// vals_alt are same-sized buffers; *result_in_alt tells which pair of buffers
// holds the result.  scratch: radix_sort_scratch_bytes(n) bytes.
size_t radix_sort_scratch_bytes(int64_t n);
hipError_t radix_sort_pairs(uint64_t* keys, uint32_t* vals, uint64_t* keys_alt, uint32_t* vals_alt,
                            int64_t n, int key_bits_lo, int key_bits_hi, bool descending,
                            int val_bits_hi, void* scratch, bool* result_in_alt, hipStream_t st);
// G rows of n keys each ([G][n]), every row sorted descending in place of
// the segmented sort (rows / rows_alt: G * n u32 of scratch values).
hipError_t radix_sort_rows_desc(uint64_t* keys, uint64_t* keys_alt, uint32_t* rows,
                                uint32_t* rows_alt, int64_t G, int64_t n, void* scratch,
                                bool* result_in_alt, hipStream_t st);
// out[i] = in[0] + ... + in[i - 1] (out[0] = 0) for n u64 counts.
size_t exclusive_scan_scratch_bytes(int64_t n);
hipError_t exclusive_scan_u64(const unsigned long long* in, int64_t* out, int64_t n, void* scratch,
                              hipStream_t st);

// bm25.BM25's float64 path (bm25mi_dense.hip): dense sums of one query from
// the index's float64 values (numpy's order), and the n best of a dense
// float64 vector by (score desc, doc asc).
hipError_t launch_dense_f64(const DevIndex& ix, const double* val64, const int32_t* d_query,
                            int64_t T, double* d_out, hipStream_t st);
size_t topn_f64_scratch_bytes(int64_t n_docs);
hipError_t launch_topn_f64(const double* d_scores, int64_t n_docs, int64_t n, void* scratch,
                           int32_t* d_docs, double* d_out_scores, hipStream_t st);

// GPU index build (bm25mi_build.hip): scoring rules of bm25_build_scores.
enum { kLucene = 0, kBm25Py = 1 };
// (doc, term, tf) triples + document lengths -> CSC indptr [n_terms+1] (i64),
// indices/data [n] (+ f64 data when d_data64 != null), all on the device;
// d_err |= 1 (id out of range), 2 (tf not positive finite), 4 (duplicate
// (doc, term)).  Synchronises `stream` before returning.
hipError_t build_scores(int64_t n_docs, int64_t n_terms, int64_t n, const int32_t* d_docs,
                        const int32_t* d_terms, const float* d_tfs, const int32_t* d_doc_len,
                        double avgdl, double k1, double b, int method, const float* d_idf,
                        int64_t* d_indptr, int32_t* d_indices, float* d_data, double* d_data64,
                        int32_t* d_err, hipStream_t stream);

}  // namespace bm25mi
