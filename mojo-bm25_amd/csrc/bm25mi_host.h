// bm25mi_host.h — host-only helpers of the C-ABI boundary (bm25mi_capi.cpp;
// tests/asan/host_check.cpp drives them without a device): the error
// reporters, the staging helper of the synchronous host-pointer calls, the
// table of the search options and the argument rules that read host arrays.
// No .hip file includes this.
//
// A host entry point reads: validate, Enter (bm25mi_capi.cpp), HostCall,
// finish.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/bm25mi.h"
#include "bm25mi_internal.h"

namespace bm25mi {

// Set bm25_last_error of the calling thread and return the code.
int fail(int code, const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);  // "<what>: <HIP's text> (<name>)": EHIP or ENOMEM

// One synchronous host-pointer call on one stream.  It owns the device
// buffers it allocates, holds the first failure — a hipError_t, or the
// return code of a device pipeline (run_search), which wins — and turns every
// step after it into a no-op, so a call body reads top to bottom; guard a
// launch that takes the buffers with ok().  finish() always waits for the
// stream before a buffer is freed and before the caller gets its arrays
// back: copies in flight read and write them.
class HostCall {
 public:
  explicit HostCall(hipStream_t st) : st_(st) {}
  HostCall(const HostCall&) = delete;
  HostCall& operator=(const HostCall&) = delete;
  ~HostCall() {
    if (!finished_) hipStreamSynchronize(st_);
    for (void* p : bufs_) hipFree(p);
  }

  bool ok() const { return rc_ == BM25_OK && err_ == hipSuccess; }
  // Holds e if it is the first failure (what: its label in the error text,
  // finish's by default).
  void run(hipError_t e, const char* what = nullptr) {
    if (ok() && e != hipSuccess) {
      err_ = e;
      what_ = what;
    }
  }
  // Holds a failed call's return code (its message is already set).
  void hold(int rc) {
    if (rc_ == BM25_OK) rc_ = rc;
  }
  template <class T>
  T* alloc(int64_t n, const char* what = nullptr) {
    void* p = nullptr;
    if (ok()) run(hipMalloc(&p, sizeof(T) * (size_t)std::max<int64_t>(n, 1)), what);
    if (p) bufs_.push_back(p);
    return (T*)p;
  }
  // Host to device, into a buffer of the caller's (n <= 0: nothing).
  template <class T>
  void upload_to(T* dst, const T* src, int64_t n, const char* what = nullptr) {
    if (ok() && n > 0)
      run(hipMemcpyAsync(dst, src, sizeof(T) * (size_t)n, hipMemcpyHostToDevice, st_), what);
  }
  // A device copy of src[0..n) (null for n <= 0).
  template <class T>
  T* upload(const T* src, int64_t n, const char* what = nullptr) {
    if (n <= 0) return nullptr;
    T* d = alloc<T>(n, what);
    upload_to(d, src, n, what);
    return d;
  }
  template <class T>
  void download(T* dst, const T* src, int64_t n, const char* what = nullptr) {
    if (ok() && n > 0)
      run(hipMemcpyAsync(dst, src, sizeof(T) * (size_t)n, hipMemcpyDeviceToHost, st_), what);
  }
  int finish(const char* what) {
    const hipError_t es = hipStreamSynchronize(st_);
    finished_ = true;
    if (rc_) return rc_;
    run(es);
    return err_ == hipSuccess ? BM25_OK : hip_fail(err_, what_ ? what_ : what);
  }

 private:
  hipStream_t st_;
  std::vector<void*> bufs_;
  hipError_t err_ = hipSuccess;
  const char* what_ = nullptr;
  int rc_ = BM25_OK;
  bool finished_ = false;
};

// The search options (SearchOpts; include/bm25mi.h describes them): name, the
// variable a new handle reads, the field, and the values set_opt accepts — a
// bool, lo..hi, or a power of two in lo..hi (lo = 0: 0 too).  msg: the error
// text where it does not follow from those.  The environment is looser than
// set_opt, as it always was: a bool is value != 0, env_clamp bounds an
// integer from below (1) or on both sides (2), the others are taken as given.
enum OptKind { kOptBool, kOptRange, kOptPow2 };
struct OptDesc {
  const char* name;
  const char* env;
  int SearchOpts::*field;
  OptKind kind;
  int lo, hi;
  int env_clamp;
  const char* msg;
};
inline constexpr OptDesc kOpts[] = {
    {"flat", "BM25_FLAT", &SearchOpts::flat, kOptBool, 0, 1, 0, nullptr},
    {"flat_bw", "BM25_FLAT_BW", &SearchOpts::flat_bw, kOptPow2, 0, 8, 0,
     "flat_bw must be 0, 1, 2, 4 or 8"},
    {"items_per_wave", "BM25_ITEMS_PER_WAVE", &SearchOpts::items_per_wave, kOptRange, 1, 1024, 0,
     nullptr},
    {"sample_p", "BM25_SAMPLE_P", &SearchOpts::sample_p, kOptPow2, 1, 64, 0, nullptr},
    {"list_cap", "BM25_LIST_CAP", &SearchOpts::list_cap, kOptRange, 0, 1 << 20, 0,
     "list_cap must be in 0..2^20"},
    {"claim_ch", "BM25_CLAIM_CH", &SearchOpts::claim_ch, kOptRange, 1, 64, 0, nullptr},
    {"claim_m", "BM25_CLAIM_M", &SearchOpts::claim_m, kOptRange, 1, kClaimM, 0, nullptr},
    {"tile_bound", "BM25_TILE_BOUND", &SearchOpts::tile_bound, kOptBool, 0, 1, 0, nullptr},
    {"theta_bound", "BM25_THETA_BOUND", &SearchOpts::theta_bound, kOptBool, 0, 1, 0, nullptr},
    {"grid_pct", "BM25_GRID_PCT", &SearchOpts::grid_pct, kOptRange, 1, 100, 2, nullptr},
    {"count_skips", "BM25_COUNT_SKIPS", &SearchOpts::count_skips, kOptBool, 0, 1, 0, nullptr},
    {"large_lists", "BM25_LARGE_LISTS", &SearchOpts::large_lists, kOptBool, 0, 1, 0, nullptr},
    {"rest_split", "BM25_REST_SPLIT", &SearchOpts::rest_split, kOptBool, 0, 1, 0, nullptr},
    {"bound_pool", "BM25_BOUND_POOL", &SearchOpts::bound_pool, kOptBool, 0, 1, 0, nullptr},
    {"filter_tiles", "BM25_FILTER_TILES", &SearchOpts::filter_tiles, kOptBool, 0, 1, 0, nullptr},
    {"bool_chunk", "BM25_BOOL_CHUNK", &SearchOpts::bool_chunk, kOptRange, 0, 1 << 30, 1,
     "bool_chunk must be in 0..2^30"},
};
// Options added since: a table of their own with the same rows, so the
// first one stays the sixteen options its host check pins by count.  set_opt,
// get_opt and a new handle's environment read both.
inline constexpr OptDesc kOptsMore[] = {
    {"tile_mask", "BM25_TILE_MASK", &SearchOpts::tile_mask, kOptBool, 0, 1, 0, nullptr},
    {"seg_skip", "BM25_SEG_SKIP", &SearchOpts::seg_skip, kOptBool, 0, 1, 0, nullptr},
    {"row_skip", "BM25_ROW_SKIP", &SearchOpts::row_skip, kOptBool, 0, 1, 0, nullptr},
    {"row_mask_kb", "BM25_ROW_MASK_KB", &SearchOpts::row_mask_kb, kOptRange, 0, 1 << 30, 2,
     nullptr},
    {"collapse_page", "BM25_COLLAPSE_PAGE", &SearchOpts::collapse_page, kOptRange, 0, kMaxK, 2,
     nullptr},
    {"collapse_chunk", "BM25_COLLAPSE_CHUNK", &SearchOpts::collapse_chunk, kOptRange, 0, 1 << 30, 1,
     "collapse_chunk must be in 0..2^30"},
    {"sorted_bins", "BM25_SORTED_BINS", &SearchOpts::sorted_bins, kOptRange, 0, (int)kSortedBins, 2,
     nullptr},
};

// The order arrays and cursors of the sorted search as the host calls check
// them (bm25_search_sorted, bm25_search_boolean_sorted): ranks and perm inverse
// permutations of [0, n_docs) — the message names the first offending index —
// and no cursor below BM25_AFTER_NONE.
// (inline, so tests/asan/sorted_check.cpp drives them under the sanitizers with
// a fail() of its own and no device)
inline int check_sort_order(const int32_t* ranks, const int32_t* perm, int64_t n_docs) {
  for (int64_t d = 0; d < n_docs; ++d) {  // (perm[ranks[d]] == d for every d shows both)
    const int32_t r = ranks[d];
    if (r < 0 || r >= n_docs)
      return fail(BM25_EINVAL, "ranks[%lld] = %d is outside [0, %lld)", (long long)d, (int)r,
                  (long long)n_docs);
    if (perm[r] != d)
      return fail(BM25_EINVAL,
                  "ranks[%lld] = %d but perm[%d] = %d: ranks and perm are not inverse permutations",
                  (long long)d, (int)r, (int)r, (int)perm[r]);
  }
  return BM25_OK;
}
inline int check_after_ranks(const int32_t* after, int64_t M) {
  for (int64_t m = 0; after && m < M; ++m)
    if (after[m] < BM25_AFTER_NONE)
      return fail(BM25_EINVAL, "after_ranks[%lld] = %d is below BM25_AFTER_NONE (-2)", (long long)m,
                  (int)after[m]);
  return BM25_OK;
}

// k of a top-k call.  shard = true: the index is one doc shard of a larger
// collection, whose [Q, k] lists are padded (doc -1, score bits ~0) where it
// holds fewer than k documents; otherwise k > n_docs is numpy's argpartition
// error (the reference's behaviour, bm25_native.py:205).
inline int check_k(int64_t n_docs, int64_t k, bool shard = false) {
  if (k < 0) return fail(BM25_EINVAL, "negative dimensions are not allowed (top_k=%lld)", (long long)k);
  if (!shard && k > n_docs)
    return fail(BM25_EINVAL, "kth(=%lld) out of bounds (%lld)", (long long)(n_docs - k),
                (long long)n_docs);
  return BM25_OK;
}

// max(ids, initial = mx), and the reference's check of it
// (bm25_native.py:116-121: max(initial=0) >= n_terms -> ValueError).
inline int64_t max_token(int64_t mx, const int32_t* ids, int64_t n) {
  for (int64_t i = 0; i < n; ++i) mx = std::max<int64_t>(mx, ids[i]);
  return mx;
}

inline int check_token_ids(int64_t n_terms, int64_t mx0, const int32_t* ids, int64_t n) {
  const int64_t mx = max_token(mx0, ids, n);
  if (mx >= n_terms)
    return fail(BM25_EINVAL,
                "The maximum token ID in the query (%lld) is higher than the number of tokens in "
                "the index.",
                (long long)mx);
  return BM25_OK;
}

// The weighted calls' finite-weight rule: a weight on a non-padding slot (a
// token id >= 0; ids >= n_terms were rejected before) must be finite.
inline int check_weights(const int32_t* ids, const float* w, int64_t Q, int64_t T) {
  for (int64_t i = 0; i < Q * T; ++i)
    if (ids[i] >= 0 && !std::isfinite(w[i]))
      return fail(BM25_EINVAL, "weights[%lld][%lld] = %g is not finite", (long long)(i / T),
                  (long long)(i % T), (double)w[i]);
  return BM25_OK;
}

// The arguments of a ranked call — the filtered, weighted, cursor and collapsed
// searches, host or device form — and the rules in which the calls differ.  A
// call leaves what it does not take at its default, validates with its rule set
// (check_ranked_shape, the early return for Q == 0 or k == 0, then
// check_ranked_content or, of device pointers, check_ranked_pointers) and
// stages from the same struct; a new ranked call adds a field and a rule, not
// a copy.  (tests/asan/ranked_check.cpp drives every rule set under the
// sanitizers, without a device)
struct RankedArgs {
  const int32_t* queries = nullptr;  // [Q, T]
  const float* weights = nullptr;    // [Q, T], or null: plain sums
  int64_t Q = 0, T = 0;
  int32_t k = 0;
  const uint32_t* masks = nullptr;  // [M, W]
  int64_t M = 0;
  const int32_t* query_mask = nullptr;  // [Q], or null
  const float* after_scores = nullptr;  // [Q] each, or both null
  const int32_t* after_docs = nullptr;
  const int32_t* groups = nullptr;  // [n_docs]
  int32_t per_group = 1;
  int32_t* out_docs = nullptr;  // [Q, k]
  float* out_scores = nullptr;
};
enum RankedRules : unsigned {
  kRankedWeights = 1,    // weights are required, not optional
  kRankedNeedsMask = 2,  // without masks, query_mask must be given (and name -1 only)
  kRankedCursor = 4,     // takes after_scores / after_docs
  kRankedCollapse = 8,   // takes groups / per_group; k <= kMaxK
};

// What a call checks before its early return: no pointer is looked at.
inline int check_ranked_shape(int64_t n_docs, const RankedArgs& a, unsigned rules) {
  if (a.Q < 0 || a.T < 0 || a.M < 0) return fail(BM25_EINVAL, "negative query or mask shape");
  if (rules & kRankedCollapse) {
    if (a.k > kMaxK)
      return fail(BM25_EINVAL,
                  "k=%d: a collapsed search is limited to k <= %d (the per-row group table lives "
                  "in LDS)",
                  a.k, kMaxK);
    if (a.per_group < 1) return fail(BM25_EINVAL, "per_group=%d must be >= 1", a.per_group);
  }
  const int rc = check_k(n_docs, a.k);
  if (rc) return rc;
  if ((rules & kRankedCursor) && (a.after_scores != nullptr) != (a.after_docs != nullptr))
    return fail(BM25_EINVAL, "after_scores and after_docs must both be given or both be NULL");
  return BM25_OK;
}

// The NULL rules of a call with Q > 0 and k > 0; nothing is dereferenced.
inline int check_ranked_pointers(const RankedArgs& a, unsigned rules) {
  if (a.T > 0 && !a.queries) return fail(BM25_EINVAL, "NULL queries");
  if ((rules & kRankedWeights) && a.T > 0 && !a.weights) return fail(BM25_EINVAL, "NULL weights");
  if (a.M > 0 && !a.masks) return fail(BM25_EINVAL, "NULL masks");
  if ((rules & kRankedNeedsMask) && a.M == 0 && !a.query_mask)
    return fail(BM25_EINVAL, "no masks: query_mask must name -1 (no filter) for every query");
  if ((rules & kRankedCollapse) && !a.groups)
    return fail(BM25_EINVAL, "NULL groups (one int32 per document; < 0: no group)");
  if (!a.out_docs || !a.out_scores) return fail(BM25_EINVAL, "NULL output");
  return BM25_OK;
}

// The host calls' check of their arrays, after the early return: the NULL
// rules, then token ids, finite weights, mask ids in [-1, M) and cursors (a doc
// id >= 0 with a score that is no NaN, -1 or BM25_AFTER_NONE).
inline int check_ranked_content(int64_t n_terms, const RankedArgs& a, unsigned rules) {
  int rc = check_ranked_pointers(a, rules);
  if (rc) return rc;
  rc = check_token_ids(n_terms, 0, a.queries, a.Q * a.T);
  if (rc) return rc;
  if (a.weights) {
    rc = check_weights(a.queries, a.weights, a.Q, a.T);
    if (rc) return rc;
  }
  for (int64_t i = 0; a.query_mask && i < a.Q; ++i)
    if (a.query_mask[i] < -1 || a.query_mask[i] >= a.M)
      return fail(BM25_EINVAL, "query_mask[%lld] = %d is outside [-1, %lld)", (long long)i,
                  a.query_mask[i], (long long)a.M);
  for (int64_t i = 0; a.after_docs && i < a.Q; ++i) {
    if (a.after_docs[i] < BM25_AFTER_NONE)
      return fail(BM25_EINVAL,
                  "after_docs[%lld] = %d is below BM25_AFTER_NONE (-2): a cursor names a doc "
                  "id >= 0, -1 (exhausted) or BM25_AFTER_NONE",
                  (long long)i, a.after_docs[i]);
    if (a.after_docs[i] >= 0 && std::isnan(a.after_scores[i]))
      return fail(BM25_EINVAL, "after_scores[%lld] = %g is not a score (the cursor of doc %d)",
                  (long long)i, (double)a.after_scores[i], a.after_docs[i]);
  }
  return BM25_OK;
}

// Sets / reads one option by name (EINVAL names the accepted values).
int set_opt(SearchOpts& o, const char* name, int64_t v);
int get_opt(const SearchOpts& o, const char* name, int64_t* v);

}  // namespace bm25mi
