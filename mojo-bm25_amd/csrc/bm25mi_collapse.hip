// bm25mi_collapse.hip — field collapsing (bm25_search_collapsed /
// bm25_search_collapsed_device, include/bm25mi.h): at most per_group hits of
// every group in a row's top-k.
//
// Replaces no reference call: BM25v.search has no grouping (bm25_native.py:
// 76-158).  The result is the walk of the weighted search's full order with a
// counter per group value; the score passes are the cursor
// search's, untouched.  The host loop (bm25mi_capi.cpp, run_collapsed) pages
// through each row's order and these kernels do the walk:
//
//   collapse_page_kernel     one wave per row: the page's entries, 64 at a
//                            time in rank order, against the row's group
//                            counters (an LDS hash rebuilt from the hits kept
//                            so far); kept entries are appended to the row
//   collapse_compact_kernel  the unfinished rows' ids, ascending (one
//                            workgroup, a block prefix: no atomic picks a slot)
//   collapse_gather_kernel   those rows' queries, weights and cursors as a
//                            compact batch
//   collapse_exclude_kernel  the compact rows' allow-masks: the row's own mask
//                            minus every document of a saturated group
//
// The group table and the step that decides a 64-entry chunk live in
// bm25mi_collapse_dev.h, shared with the doc-shard merge
// (bm25mi_merge_collapse.hip).
//
// Nothing here depends on scheduling: a row is one wave's, the lanes of a
// chunk decide from ballots, LDS atomics only insert keys and sum counts (the
// lookups read the same values whatever the order), and the two global
// counters are plain sums.  Plain C++ and vector memory operations throughout.
#include "bm25mi_collapse_dev.h"
#include "bm25mi_internal.h"

#include <algorithm>

namespace bm25mi {

namespace {

constexpr int kExT = 256;          // threads of the exclusion kernel: 4 waves, 64 words each
constexpr int kExStepWords = 256;  // mask words of a workgroup's step
constexpr int kCompactT = 1024;    // threads of the compaction kernel

// One wave per row r of a batch of pages (row q = row_map[r] of the call, or r
// itself).  A row whose cursor says "exhausted" was finished by an earlier
// round and is left alone.  ctr[0] += 1 for a row that stays unfinished,
// ctr[1] += the page's over-quota entries ahead of the row's last kept one.
__global__ __launch_bounds__(64) void collapse_page_kernel(
    const int32_t* __restrict__ page_docs, const float* __restrict__ page_scores, int32_t p,
    const int32_t* __restrict__ row_map, const int32_t* __restrict__ groups, int64_t n_docs,
    int64_t doc_offset, int32_t per_group, int32_t k, int slots, int lg,
    int32_t* __restrict__ count, int32_t* __restrict__ out_docs, float* __restrict__ out_scores,
    int32_t* __restrict__ out_groups, float* __restrict__ cur_scores,
    int32_t* __restrict__ cur_docs, unsigned long long* __restrict__ ctr) {
  extern __shared__ int32_t tab[];
  const int64_t r = blockIdx.x;
  const int64_t q = row_map ? row_map[r] : r;
  if (cur_docs[q] == -1) return;  // (block-uniform, before the barriers)
  const int lane = threadIdx.x;
  int32_t cnt = count[q];
  int32_t* od = out_docs + q * k;
  float* os = out_scores + q * k;
  int32_t* og = out_groups + q * k;
  tab_clear(tab, slots, lane, 64);
  __syncthreads();
  for (int32_t i = lane; i < cnt; i += 64) {
    const int32_t g = og[i];
    if (g >= 0) tab_add(tab, slots, lg, g);
  }
  __syncthreads();
  const int32_t* pd = page_docs + r * p;
  const float* ps = page_scores + r * p;
  uint32_t dropped = 0;
  bool ended = false;  // the page ran into padding
  for (int32_t c0 = 0; c0 < p && cnt < k && !ended; c0 += 64) {
    const int32_t i = c0 + lane;
    const int32_t d = i < p ? pd[i] : -1;
    const int64_t dl = (int64_t)d - doc_offset;
    const bool real = d >= 0 && dl >= 0 && dl < n_docs;
    ended = __builtin_amdgcn_ballot_w64(i < p && !real) != 0ull;
    const float s = real ? ps[i] : 0.f;
    const int32_t g = real ? groups[dl] : -1;
    const ChunkStep c = chunk_step(tab, slots, lg, real, g, per_group, cnt, k, lane);
    // over-quota entries ahead of the chunk's last taken entry (all of them
    // when the row does not fill here)
    const uint64_t ahead =
        c.total >= k && c.tm ? (1ull << (63 - __builtin_clzll(c.tm))) - 1ull : ~0ull;
    dropped += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(real && !c.keep) & ahead);
    if (c.take) {
      od[c.pos] = d;
      os[c.pos] = s;
      og[c.pos] = g;
    }
    chunk_commit(tab, slots, lg, c.take, g);  // (the lookups above, before the table changes)
    cnt = min(c.total, k);
  }
  const int32_t last = pd[p - 1];
  const bool done = cnt >= k || ended || last < 0;
  if (done)  // the rest of a row that cannot fill: padding
    for (int32_t i = cnt + lane; i < k; i += 64) {
      od[i] = -1;
      os[i] = __uint_as_float(0xFFFFFFFFu);
      og[i] = -1;
    }
  if (lane == 0) {
    count[q] = cnt;
    cur_docs[q] = done ? -1 : last;
    cur_scores[q] = ps[p - 1];
    if (!done) atomicAdd(&ctr[0], 1ull);
    if (dropped) atomicAdd(&ctr[1], (unsigned long long)dropped);
  }
}

// rows[0 .. *n_rows) = the rows q < Q with cur_docs[q] != -1, ascending.
__global__ __launch_bounds__(kCompactT) void collapse_compact_kernel(
    const int32_t* __restrict__ cur_docs, int64_t Q, int32_t* __restrict__ rows) {
  __shared__ int32_t wsum[kCompactT / 64];
  __shared__ int32_t base;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (t == 0) base = 0;
  __syncthreads();
  for (int64_t q0 = 0; q0 < Q; q0 += kCompactT) {
    const int64_t q = q0 + t;
    const bool live = q < Q && cur_docs[q] != -1;
    const uint64_t m = __builtin_amdgcn_ballot_w64(live);
    if (lane == 0) wsum[wv] = (int32_t)__popcll(m);
    __syncthreads();
    int32_t at = base;
    for (int w = 0; w < wv; ++w) at += wsum[w];
    if (live) rows[at + (int32_t)__popcll(m & ((1ull << lane) - 1ull))] = (int32_t)q;
    __syncthreads();
    if (t == 0) {
      int32_t all = 0;
      for (int w = 0; w < kCompactT / 64; ++w) all += wsum[w];
      base += all;
    }
    __syncthreads();
  }
}

// Compact row r = row rows[r] of the call: its query, weights (when given),
// cursor, and its mask id (r: the exclusion masks are by compact row).
__global__ __launch_bounds__(64) void collapse_gather_kernel(
    const int32_t* __restrict__ rows, const int32_t* __restrict__ queries,
    const float* __restrict__ weights, int64_t T, const float* __restrict__ cur_scores,
    const int32_t* __restrict__ cur_docs, int32_t* __restrict__ cq, float* __restrict__ cw,
    float* __restrict__ c_as, int32_t* __restrict__ c_ad, int32_t* __restrict__ ids) {
  const int64_t r = blockIdx.x;
  const int64_t q = rows[r];
  for (int64_t j = threadIdx.x; j < T; j += 64) {
    cq[r * T + j] = queries[q * T + j];
    if (weights) cw[r * T + j] = weights[q * T + j];
  }
  if (threadIdx.x == 0) {
    c_as[r] = cur_scores[q];
    c_ad[r] = cur_docs[q];
    ids[r] = (int32_t)r;
  }
}

// excl[r][W] for compact row r (row q = rows[r] of the call): the words of the
// row's own mask (all ones without one), minus every document whose group has
// per_group hits among the row's count[q] kept ones; a finished row: zeros.
// Every word is written, bits at or past n_docs are 0, no word at index >= W
// and no groups entry at index >= n_docs is touched.  blockIdx.x: the row;
// blockIdx.y strides over steps of kExStepWords words; a wave takes 64 words:
// 32 coalesced reads of 64 groups, a ballot each, whose halves go to the two
// lanes that own those words.
__global__ __launch_bounds__(kExT) void collapse_exclude_kernel(
    const int32_t* __restrict__ rows, const uint32_t* __restrict__ masks, int64_t M,
    const int32_t* __restrict__ query_mask, const int32_t* __restrict__ groups, int64_t n_docs,
    int64_t W, int32_t per_group, int32_t k, int slots, int lg, const int32_t* __restrict__ count,
    const int32_t* __restrict__ out_groups, const int32_t* __restrict__ cur_docs,
    uint32_t* __restrict__ excl) {
  extern __shared__ int32_t tab[];
  const int64_t r = blockIdx.x;
  const int64_t q = rows[r];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  uint32_t* orow = excl + r * W;
  const int64_t steps = (W + kExStepWords - 1) / kExStepWords;
  if (cur_docs[q] == -1) {  // (block-uniform)
    for (int64_t s = blockIdx.y; s < steps; s += gridDim.y) {
      const int64_t w = s * kExStepWords + t;
      if (w < W) orow[w] = 0u;
    }
    return;
  }
  tab_clear(tab, slots, t, kExT);
  __syncthreads();
  const int32_t cnt = count[q];
  for (int32_t i = t; i < cnt; i += kExT) {
    const int32_t g = out_groups[q * k + i];
    if (g >= 0) tab_add(tab, slots, lg, g);
  }
  __syncthreads();
  const int64_t m = M == 0 ? -1 : (query_mask ? (int64_t)query_mask[q] : 0);
  const uint32_t* brow = m < 0 ? nullptr : masks + m * W;
  for (int64_t s = blockIdx.y; s < steps; s += gridDim.y) {
    const int64_t w0 = s * kExStepWords + wv * 64;  // the wave's first word
    uint32_t mine = 0u;
    for (int j = 0; j < 32; ++j) {
      const int64_t d0 = (w0 + 2 * j) * 32;  // (wave-uniform)
      if (d0 >= n_docs) break;
      const int64_t d = d0 + lane;
      const int32_t g = d < n_docs ? groups[d] : -1;
      const bool open = d < n_docs && (g < 0 || tab_count(tab, slots, lg, g) < per_group);
      const uint64_t b = __builtin_amdgcn_ballot_w64(open);
      mine = lane == 2 * j ? (uint32_t)b : lane == 2 * j + 1 ? (uint32_t)(b >> 32) : mine;
    }
    const int64_t w = w0 + lane;
    if (w < W) orow[w] = brow ? (brow[w] & mine) : mine;
  }
}

int log2_ceil(int64_t x) {
  int lg = 0;
  while (((int64_t)1 << lg) < x) ++lg;
  return lg;
}

}  // namespace

// Slots of the group table of a search at k: twice the keys it may hold, at
// least 128 — 8 B each, so 64 KiB of LDS at k = kMaxK.
int collapse_slots(int k) { return 1 << std::max(7, log2_ceil(2 * (int64_t)k)); }

hipError_t launch_collapse_page(const int32_t* d_page_docs, const float* d_page_scores, int32_t p,
                                const int32_t* d_row_map, int64_t R, const int32_t* d_groups,
                                int64_t n_docs, int64_t doc_offset, int32_t per_group, int32_t k,
                                int32_t* d_count, int32_t* d_docs, float* d_scores,
                                int32_t* d_out_groups, float* d_cur_scores, int32_t* d_cur_docs,
                                unsigned long long* d_ctr, hipStream_t st) {
  if (R <= 0 || k <= 0 || p <= 0) return hipSuccess;
  if (k > kMaxK || per_group < 1) return hipErrorInvalidValue;
  const int slots = collapse_slots(k);
  hipLaunchKernelGGL(collapse_page_kernel, dim3((unsigned)R), dim3(64), sizeof(int32_t) * 2 * slots,
                     st, d_page_docs, d_page_scores, p, d_row_map, d_groups, n_docs, doc_offset,
                     per_group, k, slots, log2_ceil(slots), d_count, d_docs, d_scores, d_out_groups,
                     d_cur_scores, d_cur_docs, d_ctr);
  return hipGetLastError();
}

hipError_t launch_collapse_compact(const int32_t* d_cur_docs, int64_t Q, int32_t* d_rows,
                                   hipStream_t st) {
  if (Q <= 0) return hipSuccess;
  hipLaunchKernelGGL(collapse_compact_kernel, dim3(1), dim3(kCompactT), 0, st, d_cur_docs, Q,
                     d_rows);
  return hipGetLastError();
}

hipError_t launch_collapse_gather(const int32_t* d_rows, int64_t R, const int32_t* d_queries,
                                  const float* d_weights, int64_t T, const float* d_cur_scores,
                                  const int32_t* d_cur_docs, int32_t* d_cq, float* d_cw,
                                  float* d_as, int32_t* d_ad, int32_t* d_ids, hipStream_t st) {
  if (R <= 0) return hipSuccess;
  hipLaunchKernelGGL(collapse_gather_kernel, dim3((unsigned)R), dim3(64), 0, st, d_rows, d_queries,
                     d_weights, T, d_cur_scores, d_cur_docs, d_cq, d_cw, d_as, d_ad, d_ids);
  return hipGetLastError();
}

hipError_t launch_collapse_exclude(const int32_t* d_rows, int64_t R, const uint32_t* d_masks,
                                   int64_t M, const int32_t* d_query_mask, const int32_t* d_groups,
                                   int64_t n_docs, int32_t per_group, int32_t k,
                                   const int32_t* d_count, const int32_t* d_out_groups,
                                   const int32_t* d_cur_docs, uint32_t* d_excl, hipStream_t st) {
  const int64_t W = (n_docs + 31) >> 5;
  if (R <= 0 || W <= 0) return hipSuccess;
  if (k > kMaxK || per_group < 1) return hipErrorInvalidValue;
  const int slots = collapse_slots(k);
  // a workgroup rebuilds the row's table once: eight steps each where the row
  // is that long, so the rebuild stays a small share
  const int64_t steps = (W + kExStepWords - 1) / kExStepWords;
  const unsigned gy = (unsigned)std::min<int64_t>(std::max<int64_t>(1, (steps + 7) / 8), 65535);
  hipLaunchKernelGGL(collapse_exclude_kernel, dim3((unsigned)R, gy), dim3(kExT),
                     sizeof(int32_t) * 2 * slots, st, d_rows, d_masks, M, d_query_mask, d_groups,
                     n_docs, W, per_group, k, slots, log2_ceil(slots), d_count, d_out_groups,
                     d_cur_docs, d_excl);
  return hipGetLastError();
}

}  // namespace bm25mi
