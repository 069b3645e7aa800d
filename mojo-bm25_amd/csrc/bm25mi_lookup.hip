// bm25mi_lookup.hip — BM25 scores of given (query, document) pairs
// (bm25_score_docs / bm25_score_docs_device, include/bm25mi.h): a sparse
// point lookup, not a streamed scatter-add.
//
//   out[q][c] = +0.0f + v(q[0], d) + v(q[1], d) + ...   d = docs[q][c]
//
// over the query's token ids in query order, v(t, d) = the index value of
// (term t, document d), or +0.0f where the document lacks the term or the id
// is padding.  The running sum starts at +0.0f and so is never -0.0f; adding
// +0.0f leaves every bit as it is, hence the result is element d of
// scores_dense_kernel's row (bm25mi_kernels.hip), which adds the present
// postings only, in the same order.
//
// What the lookup relies on (bm25mi_internal.h): the postings
// of term t in tile j are [indptr[t] + r(t, j), indptr[t] + r(t, j + 1)) by
// either segment table, and ldoc inside one segment is strictly ascending
// (tile-local id << 2), so a (term, document) pair is one segment lookup and
// one binary search over at most 2^tile_shift u16.
//
// One lane per (pair, term slot), 2^TL term slots per pair: each lane's chain
// of dependent loads is its own term's, about 3 + log2(segment length) long,
// and the wave holds 64 of them in flight.  The 2^TL values of a pair are then
// added one by one from term slot 0 upward (the rounding sequence is the
// contract: no tree reduction).
//
// The weighted form (bm25_score_docs_weighted) multiplies a value that was
// found by its term's weight, rounded to fp32 on its own, before that sum:
// the fold of bm25_search_weighted, so the bits agree with its scores.  A
// posting that is absent adds +0.0f, not weight * 0.
#include "bm25mi_internal.h"

#include <algorithm>
#include <atomic>

namespace bm25mi {

namespace {

constexpr int kLookupNT = 256;  // threads per workgroup (4 waves)

struct LookupArgs {
  const int64_t* indptr;
  const uint32_t* rel;
  const int64_t* tl_ptr;
  const uint16_t* tl_tile;
  const uint32_t* tl_start;
  const uint16_t* ldoc;
  const float* val;
  int64_t V, ntiles, n_docs, doc_offset;
  int32_t sparse, tile_shift;
};

// The index value of (term, local document id), both in range; +0.0f where the
// document does not hold the term (*found, if given, tells the two apart).
__device__ __forceinline__ float posting_value(const LookupArgs& a, int64_t term, int64_t local,
                                               bool* found = nullptr) {
  if (found) *found = false;
  const int64_t tile = local >> a.tile_shift;
  const uint32_t slot = ((uint32_t)local & ((1u << a.tile_shift) - 1u)) << 2;
  const int64_t p0 = a.indptr[term];
  uint32_t r0, r1;
  if (!a.sparse) {  // two adjacent u32 of the term's row: one 8-byte load
    uint32_t r[2];
    __builtin_memcpy(r, a.rel + term * (a.ntiles + 1) + tile, sizeof r);
    r0 = r[0];
    r1 = r[1];
  } else {  // binary search of the term's non-empty tiles (as segment())
    const int64_t b = a.tl_ptr[term], e = a.tl_ptr[term + 1];
    int64_t lo = b, hi = e;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)a.tl_tile[mid] < tile) lo = mid + 1;
      else hi = mid;
    }
    if (lo >= e || (int64_t)a.tl_tile[lo] != tile) return 0.f;
    r0 = a.tl_start[lo];
    r1 = lo + 1 < e ? a.tl_start[lo + 1] : (uint32_t)(a.indptr[term + 1] - p0);
  }
  const uint16_t* seg = a.ldoc + p0;
  uint32_t lo = r0, hi = r1;  // the first posting of [r0, r1) with ldoc >= slot
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if ((uint32_t)seg[mid] < slot) lo = mid + 1;
    else hi = mid;
  }
  if (lo < r1 && (uint32_t)seg[lo] == slot) {
    if (found) *found = true;
    return a.val[p0 + lo];
  }
  return 0.f;
}

// Pairs g = q * C + c, 64 >> TL of them per wave step, grid-stride; the lanes
// of a pair share g, so its shuffles stay inside wholly active groups (the
// loops' trip counts are wave-uniform).  WT: weights [Q][T] beside the queries.
__device__ __forceinline__ float weight_times(float w, float v) {
#pragma clang fp contract(off)
  return w * v;  // rounded on its own: never fused with the sum's add
}

template <int TL, bool WT = false>
__global__ __launch_bounds__(kLookupNT) void score_docs_kernel(
    LookupArgs a, const int32_t* __restrict__ queries, int64_t T,
    const int32_t* __restrict__ docs, int64_t C, int64_t n_pairs, float* __restrict__ out,
    const float* __restrict__ weights) {
  constexpr int G = 1 << TL;
  constexpr int kPerWave = 64 / G;
  const int lane = (int)(threadIdx.x & 63u);
  const int j = lane & (G - 1);  // term slot
  const int64_t stride = (int64_t)gridDim.x * (kLookupNT / G);
  for (int64_t wbase = (int64_t)blockIdx.x * (kLookupNT / G) + (int64_t)(threadIdx.x >> 6) * kPerWave;
       wbase < n_pairs; wbase += stride) {
    const int64_t g = wbase + (lane >> TL);
    const bool live = g < n_pairs;
    int64_t local = -1;
    const int32_t* qrow = queries;
    const float* wrow = weights;
    if (live) {
      const int32_t doc = docs[g];
      // a negative id is padding; an id outside the handle's range scores +0.0f
      local = doc < 0 ? -1 : (int64_t)doc - a.doc_offset;
      qrow = queries + (g / C) * T;
      if constexpr (WT) wrow = weights + (g / C) * T;
    }
    const bool have = local >= 0 && local < a.n_docs;
    float acc = 0.f;
    for (int64_t t0 = 0; t0 < T; t0 += G) {
      float v = 0.f;
      if (have && t0 + j < T) {
        const int32_t term = qrow[t0 + j];
        if constexpr (WT) {
          if (term >= 0 && (int64_t)term < a.V) {  // (a padding slot's weight is not read)
            bool found;
            const float x = posting_value(a, term, local, &found);
            if (found) v = weight_times(wrow[t0 + j], x);
          }
        } else {
          if (term >= 0 && (int64_t)term < a.V) v = posting_value(a, term, local);
        }
      }
      const int n = T - t0 < G ? (int)(T - t0) : G;
      for (int i = 0; i < n; ++i) acc += __shfl(v, i, G);  // query order
    }
    if (live && j == 0) out[g] = acc;
  }
}

}  // namespace

hipError_t launch_score_docs(const DevIndex& ix, const int32_t* d_queries, int64_t Q, int64_t T,
                             const int32_t* d_docs, int64_t C, float* d_out, hipStream_t st,
                             const float* d_weights) {
  const int64_t n_pairs = Q * C;
  if (n_pairs == 0) return hipSuccess;
  if (ix.tile_shift < 1 || ix.tile_shift > 14) return hipErrorInvalidValue;  // (ldoc is u16)
  static std::atomic<int> s_cus{0};
  int cus = s_cus.load(std::memory_order_relaxed);
  if (cus == 0) {
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ix.device) != hipSuccess ||
        cus <= 0)
      cus = 256;
    s_cus.store(cus, std::memory_order_relaxed);
  }
  const LookupArgs a{ix.indptr, ix.rel, ix.tl_ptr, ix.tl_tile, ix.tl_start, ix.ldoc, ix.val,
                     ix.n_terms, ix.ntiles, ix.n_docs, ix.doc_offset, ix.sparse ? 1 : 0,
                     ix.tile_shift};
  // term slots per pair: 8, 16, 32, 64 (longer queries: groups of 64 terms)
  const int tl = T <= 8 ? 3 : T <= 16 ? 4 : T <= 32 ? 5 : 6;
  const int64_t per_block = kLookupNT >> tl;
  // 8 workgroups (32 waves) per CU hold the chip; more pairs take more steps
  const unsigned grid = (unsigned)std::max<int64_t>(
      1, std::min<int64_t>((n_pairs + per_block - 1) / per_block, (int64_t)cus * 8));
#define BM25_LOOKUP(TL_)                                                                       \
  if (d_weights)                                                                               \
    hipLaunchKernelGGL((score_docs_kernel<TL_, true>), dim3(grid), dim3(kLookupNT), 0, st, a,  \
                       d_queries, T, d_docs, C, n_pairs, d_out, d_weights);                    \
  else                                                                                         \
    hipLaunchKernelGGL((score_docs_kernel<TL_>), dim3(grid), dim3(kLookupNT), 0, st, a,        \
                       d_queries, T, d_docs, C, n_pairs, d_out, d_weights)
  switch (tl) {
    case 3: BM25_LOOKUP(3); break;
    case 4: BM25_LOOKUP(4); break;
    case 5: BM25_LOOKUP(5); break;
    default: BM25_LOOKUP(6); break;
  }
#undef BM25_LOOKUP
  return hipGetLastError();
}

}  // namespace bm25mi
