// bm25mi_filter.hip — filtered top-k search: the best k among the documents a
// per-query allow-mask lets through (bm25_search_filtered, include/bm25mi.h).
//
// Replaces no reference call: BM25v.search has no filter (bm25_native.py:
// 76-158).  The result is what the reference's scorer and top-k (bm25_native.py:
// 149-158, 204-214) give on the allowed documents alone.  DESIGN.md §4.
//
// The unfiltered search's threshold machinery does not carry over: a tile
// bound (or a sample key) belongs to a document that the mask may exclude, so
// k of them no longer prove that k candidates reach the threshold, and the
// merges' zero fill takes the smallest doc ids whether or not they are
// allowed.  The filtered search is therefore a pass of its own over every
// tile that holds an allowed document:
//
//   census   allowed documents per (mask, tile) and per mask
//   pass A   one wave per (query, tile): the tile's best kTileM allowed keys
//            (add_item / take_entries / select_top, the same fp32 adds in
//            query-term order); a tile whose census is 0 reads no posting
//   theta    per query: the k-th largest of those keys — an allowed
//            document's own key, so at least k allowed documents reach it
//            (0 when fewer than k keys exist: everything allowed qualifies)
//   pass B   the (query, tile) pairs whose best key reaches theta are scored
//            again; every allowed key >= theta goes to the query's list
//   finish   per query: the k best of the list, sorted, written with global
//            ids; the rest of the row padded with doc -1 / score bits ~0
//   dense    the queries whose list overflowed (typically zero-fill queries,
//            whose theta is a zero-score key) take the dense path of
//            bm25mi_large.hip on their own, as does every query when k > kMaxK
//            or the filter_tiles option is 0
//
// The weighted search (bm25_search_weighted) is this pass with a weight row
// beside every query row: add_item's weighted instantiation multiplies each
// posting by its term's weight before the add.  Nothing above
// relies on a tile bound or on the values' sign, which is what weights of
// either sign need.
//
// The cursor search (bm25_search_after; replaces no reference call:
// BM25v.search has no cursor, bm25_native.py:76-158) is the same pass with one
// more per-document predicate: a result is the total order of one u64 key, so
// "strictly after (score, doc)" is key < ckey[q].  cursor_keys_kernel builds
// the keys in the handle-local frame once per call; pass A's candidates are
// then the tiles' best eligible keys, theta an eligible document's own key,
// pass B emits eligible keys only, and the dense path clamps a row's need to
// its eligible count (bm25mi_large.hip).
#include "bm25mi_internal.h"

namespace bm25mi {

namespace {

constexpr int kFinT = 256;      // threads of the per-query kernels
constexpr int kFinMax = kMaxK;  // keys the finish kernel sorts (a power of two)
static_assert((kFinMax & (kFinMax - 1)) == 0, "the bitonic sort runs on a power of two");

// The need-th largest non-zero key of r[0..n) (one workgroup of kFinT
// threads; need >= 1), 8 bits per pass from the top; 0 when there are fewer
// than `need`.  A row decided early (every key of the prefix is needed)
// returns the prefix with its lower bits 0, which selects the same keys.
// h: 256 counters, ctl: 4 words of LDS.
__device__ uint64_t block_kth(const uint64_t* __restrict__ r, int64_t n, uint32_t need,
                              uint32_t* h, uint32_t* ctl) {
  const uint32_t t = threadIdx.x;
  uint64_t prefix = 0ull;
  for (int shift = 56; shift >= 0; shift -= 8) {
    h[t] = 0u;
    __syncthreads();
    const int hs = shift + 8;
    for (int64_t i = t; i < n; i += kFinT) {
      const uint64_t key = r[i];
      if (key != 0ull && (hs >= 64 || ((key ^ prefix) >> hs) == 0ull))
        atomicAdd(&h[(uint32_t)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (t == 0) {
      uint32_t above = 0u, state = 2u, digit = 0u, left = need;
      for (int d = 255; d >= 0; --d) {
        const uint32_t x = h[d];
        if (need <= above + x) {
          digit = (uint32_t)d;
          left = need - above;
          state = (x == left || shift == 0) ? 1u : 0u;
          break;
        }
        above += x;
      }
      ctl[0] = state;
      ctl[1] = digit;
      ctl[2] = left;
    }
    __syncthreads();
    const uint32_t state = ctl[0];
    if (state == 2u) return 0ull;  // (block-uniform)
    prefix |= (uint64_t)ctl[1] << shift;
    need = ctl[2];
    if (state == 1u) return prefix;
    // (the next pass's writes to h and ctl come after its first barrier)
    __syncthreads();
  }
  return prefix;
}

// theta[q] = the k-th largest pass-A key of query q (0: fewer than k); the
// query's list count is cleared for pass B.
__global__ __launch_bounds__(kFinT) void filter_theta_kernel(const uint64_t* __restrict__ cand,
                                                             int64_t per_q, uint32_t k,
                                                             uint64_t* __restrict__ theta,
                                                             int32_t* __restrict__ list_cnt) {
  __shared__ uint32_t h[256];
  __shared__ uint32_t ctl[4];
  const int64_t q = blockIdx.x;
  const uint64_t th = block_kth(cand + q * per_q, per_q, k, h, ctl);
  if (threadIdx.x == 0) {
    theta[q] = th;
    list_cnt[q] = 0;
  }
}

// The k best keys of each query's list, best first, as docs (+ doc_offset)
// and scores; the columns past the list's keys are padding (doc -1, score
// bits ~0).  A query whose list overflowed writes nothing and is appended to
// ids (*n_ids of them): the dense path serves it.
__global__ __launch_bounds__(kFinT) void filter_finish_kernel(
    const uint64_t* __restrict__ list, const int32_t* __restrict__ list_cnt, int32_t C, int32_t k,
    int64_t doc_offset, int32_t* __restrict__ docs, float* __restrict__ scores,
    int32_t* __restrict__ ids, int32_t* __restrict__ n_ids) {
  __shared__ uint64_t buf[kFinMax];
  __shared__ uint32_t h[256];
  __shared__ uint32_t ctl[4];
  __shared__ int32_t s_pos;
  const int64_t q = blockIdx.x;
  const uint32_t t = threadIdx.x;
  const int32_t n = list_cnt[q];
  if (n > C) {  // block-uniform; before the barriers
    if (t == 0) ids[atomicAdd(n_ids, 1)] = (int32_t)q;
    return;
  }
  const uint64_t* r = list + q * C;
  const int32_t take = min(n, k);
  uint32_t P2 = 1u;
  while ((int32_t)P2 < take) P2 <<= 1;
  // n > k: the list holds at least k (non-zero) keys, so the k-th exists
  const uint64_t kth = n > k ? block_kth(r, n, (uint32_t)k, h, ctl) : 0ull;
  if (t == 0) s_pos = 0;
  for (uint32_t i = t; i < P2; i += kFinT) buf[i] = 0ull;
  __syncthreads();
  for (int32_t i = t; i < n; i += kFinT) {
    const uint64_t key = r[i];
    if (key >= kth) {  // exactly `take` keys: keys are unique
      const int32_t p = n > k ? atomicAdd(&s_pos, 1) : i;
      if (p < take) buf[p] = key;
    }
  }
  __syncthreads();
  for (uint32_t size = 2; size <= P2; size <<= 1) {
    for (uint32_t j = size >> 1; j > 0; j >>= 1) {
      for (uint32_t p = t; p < P2 / 2; p += kFinT) {
        const uint32_t i = ((p & ~(j - 1u)) << 1) | (p & (j - 1u));  // bit j of i clear
        const bool asc = (i & size) != 0u;  // (the last merge: descending everywhere)
        const uint64_t x = buf[i], y = buf[i + j];
        if (asc ? (x > y) : (x < y)) {
          buf[i] = y;
          buf[i + j] = x;
        }
      }
      __syncthreads();
    }
  }
  for (int32_t i = t; i < k; i += kFinT) {
    const uint64_t key = i < take ? buf[i] : 0ull;
    const int64_t e = q * k + i;
    if (key == 0ull) {
      docs[e] = -1;
      scores[e] = __uint_as_float(0xFFFFFFFFu);
    } else {
      docs[e] = (int32_t)((int64_t)(0xFFFFFFFFu - (uint32_t)key) + doc_offset);
      scores[e] = key_score((uint32_t)(key >> 32));
    }
  }
}

// The cursor keys of a call, in the handle-local doc frame: key (score_key(s),
// 0xFFFFFFFF - d) is eligible iff it is < ckey[q].  after_docs[q] < -1: no
// cursor (~0: every real key is below it); -1: the list is exhausted (0: no
// key is below it) — and the row's copy of the query is blanked to padding, so
// no pass reads a posting for it; otherwise the cursor (after_scores[q],
// after_docs[q]) with the doc moved from the global frame, carrying into the
// score field where it falls outside the frame's 32 bits (as row_kth_kernel<0>
// of bm25mi_large.hip): a doc below doc_offset precedes every local document,
// so the whole run of equal scores is still eligible.  One workgroup per row;
// qcopy [Q][T] is the queries with the exhausted rows blanked.
__global__ __launch_bounds__(64) void cursor_keys_kernel(const float* __restrict__ after_scores,
                                                         const int32_t* __restrict__ after_docs,
                                                         int64_t doc_offset,
                                                         const int32_t* __restrict__ queries,
                                                         int64_t T, uint64_t* __restrict__ ckey,
                                                         int32_t* __restrict__ qcopy) {
  const int64_t q = blockIdx.x;
  const int32_t c = after_docs[q];
  uint64_t key;
  if (c < -1) {
    key = ~0ull;
  } else if (c == -1) {
    key = 0ull;
  } else {
    const uint64_t hi = (uint64_t)score_key(after_scores[q]);
    const int64_t cl = (int64_t)c - doc_offset;  // (< 2^31: c is an int32, doc_offset >= 0)
    if (cl < 0)  // before every local document: all of the equal scores follow it
      key = hi == 0xFFFFFFFFull ? ~0ull : (hi + 1ull) << 32;
    else
      key = (hi << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)cl);
  }
  if (threadIdx.x == 0) ckey[q] = key;
  for (int64_t j = threadIdx.x; j < T; j += 64)
    qcopy[q * T + j] = key == 0ull ? -1 : queries[q * T + j];
}

#define FL_TRY(expr)                    \
  do {                                  \
    const hipError_t e_ = (expr);       \
    if (e_ != hipSuccess) return e_;    \
  } while (0)

}  // namespace

hipError_t launch_search_filtered(const DevIndex& ix, const int32_t* d_queries, int64_t Q,
                                  int64_t T, int k, const uint32_t* d_masks, int64_t M,
                                  const int32_t* d_query_mask, const Workspace& ws,
                                  int32_t* d_docs, float* d_scores, int64_t* n_dense,
                                  hipStream_t st, const float* d_weights,
                                  const float* d_after_scores, const int32_t* d_after_docs) {
  *n_dense = 0;
  if (Q == 0 || k == 0) return hipSuccess;
  if (k > ix.n_docs) return hipErrorInvalidValue;
  // the census: M (ntiles + 1) counts of the handle's scratch
  Scratch sc(st, ws.arena);
  int32_t* census = nullptr;
  uint32_t* total = nullptr;
  if ((d_after_scores != nullptr) != (d_after_docs != nullptr)) return hipErrorInvalidValue;
  uint64_t* ckey = nullptr;
  if (d_after_docs) {
    int32_t* qcopy = nullptr;
    FL_TRY(sc.get(&ckey, Q));
    FL_TRY(sc.get(&qcopy, Q * T));
    hipLaunchKernelGGL(cursor_keys_kernel, dim3((unsigned)Q), dim3(64), 0, st, d_after_scores,
                       d_after_docs, ix.doc_offset, d_queries, T, ckey, qcopy);
    d_queries = qcopy;
  }
  if (d_weights) ix.disp.kernels |= kKWeighted;
  // no masks and no mask ids (the weighted and the cursor search allow it):
  // no filter for every query, as mask ids of -1 (the kernels read a null
  // d_query_mask as mask 0)
  if (M == 0 && !d_query_mask) {
    int32_t* none = nullptr;
    FL_TRY(sc.get(&none, Q));
    FL_TRY(hipMemsetAsync(none, 0xFF, sizeof(int32_t) * Q, st));
    d_query_mask = none;
  }
  FL_TRY(sc.get(&census, M * ix.ntiles));
  FL_TRY(sc.get(&total, M));
  if (M > 0) {
    FL_TRY(hipMemsetAsync(total, 0, sizeof(uint32_t) * M, st));
    FL_TRY(launch_filter_census(ix, d_masks, M, census, total, st));
  }
  FL_TRY(hipMemsetAsync(ws.counters, 0, sizeof(int32_t) * kCounters, st));
  if (!ix.opt.filter_tiles || k > kMaxK) {
    *n_dense = Q;
    return launch_search_filtered_dense(ix, d_queries, T, k, d_masks, d_query_mask, total, nullptr,
                                        Q, d_docs, d_scores, st, ws.arena, d_weights, ckey);
  }
  ix.disp.kernels |= kKFiltered;
  FL_TRY(launch_filter_pass_a(ix, d_queries, Q, T, d_masks, d_query_mask, census, ws.cand,
                              ws.counters + 5, st, d_weights, ckey));
  hipLaunchKernelGGL(filter_theta_kernel, dim3((unsigned)Q), dim3(kFinT), 0, st, ws.cand,
                     ix.ntiles * kTileM, (uint32_t)k, ws.theta, ws.list_cnt);
  FL_TRY(launch_filter_pass_b(ix, d_queries, Q, T, d_masks, d_query_mask, ws.cand, ws.theta,
                              ws.list, ws.list_cnt, ws.list_cap, ws.counters + 3, st, d_weights,
                              ckey));
  hipLaunchKernelGGL(filter_finish_kernel, dim3((unsigned)Q), dim3(kFinT), 0, st, ws.list,
                     ws.list_cnt, ws.list_cap, (int32_t)k, ix.doc_offset, d_docs, d_scores,
                     ws.slow, ws.counters + 2);
  FL_TRY(hipGetLastError());
  // the queries whose list overflowed: the dense path, on their own (the one
  // host synchronisation of the call: their number sizes that pass)
  int32_t nfb = 0;
  FL_TRY(hipMemcpyAsync(&nfb, ws.counters + 2, sizeof nfb, hipMemcpyDeviceToHost, st));
  FL_TRY(hipStreamSynchronize(st));
  *n_dense = nfb;
  if (nfb == 0) return hipSuccess;
  return launch_search_filtered_dense(ix, d_queries, T, k, d_masks, d_query_mask, total, ws.slow,
                                      nfb, d_docs, d_scores, st, ws.arena, d_weights, ckey);
}

}  // namespace bm25mi
