// bm25mi_merge_collapse.hip — the doc-shard merge of collapsed searches
// (bm25_merge_collapsed_device, include/bm25mi.h): W best-first lists of
// (doc, score, group) per row, merged in the engine's key order and walked
// once more under per_group.
//
// Replaces no reference call: the reference is single-device (main.py:205) and
// BM25v.search has no grouping (bm25_native.py:76-158).
//
//   merge_collapsed_kernel  one wave (one workgroup) per row, in rounds: a
//     window of B entries of every list (W * B <= 512 keys), the threshold t =
//     the best last window key among the lists that may go on past their
//     window, the window entries >= t put in merged order by rank — an entry's
//     rank is its place in its own list's window plus, by a binary search of
//     every other window, the keys above it — and that order walked 64 at a
//     time against the row's group table (chunk_step / chunk_commit of
//     bm25mi_collapse_dev.h, the walk of collapse_page_kernel).  Everything
//     outside a window is worse than its own window's last key, so the entries
//     >= t are the next of the merged order; the list that sets t gives its
//     whole window, so a round always advances.
//
// A group travels with its entry (the merging rank does not hold the other
// shards' group columns); docs and scores come back out of the u64 keys, whose
// halves are bijections of them.  No global scratch, no global atomics, no host
// synchronisation; a row is one wave's, so nothing depends on scheduling.
// Plain C++ and vector memory operations throughout.
//
// Bounds, whatever the input holds: a rank is < W * B (a sum of W terms <= B,
// the entry's own < B), the heads never pass k (a list advances by at most its
// window's valid entries), every round but the last advances some head — the
// entry that sets t is itself >= t — so there are at most W * k + 1 rounds,
// and the table takes at most k keys of its >= 2 k slots, so a probe ends.
#include "bm25mi_collapse_dev.h"
#include "bm25mi_internal.h"

namespace bm25mi {

namespace {

constexpr int kWin = 512;  // keys of a round's windows

// LDS of a workgroup: the windows' keys and their merged order (u64 [kWin]
// each), the merged groups (i32 [kWin]), the lists' heads (i32 [64]) and the
// group table (8 B a slot): 10.25 KiB + 2, 16 or 64 KiB.
template <int SLOTS>
__global__ __launch_bounds__(64) void merge_collapsed_kernel(
    const int32_t* __restrict__ in_docs, const float* __restrict__ in_scores,
    const int32_t* __restrict__ in_groups, int32_t W, int32_t k, int64_t rstride,
    int32_t per_group, int lb, int slots, int lg, int32_t* __restrict__ out_docs,
    float* __restrict__ out_scores, int32_t* __restrict__ out_groups) {
  __shared__ uint64_t stage[kWin];
  __shared__ uint64_t skey[kWin];
  __shared__ int32_t sgrp[kWin];
  __shared__ int32_t head[64];
  __shared__ int32_t tab[2 * SLOTS];
  const int lane = threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x * k;
  const int B = 1 << lb;
  const int ne = W << lb;                   // window entries of a round
  const int sh = lane & ~(B - 1);           // the first lane of this lane's list in a column
  const uint64_t bm = B == 64 ? ~0ull : (1ull << B) - 1ull;
  int32_t* od = out_docs + row;
  float* os = out_scores + row;
  int32_t* og = out_groups ? out_groups + row : nullptr;
  head[lane] = 0;
  tab_clear(tab, slots, lane, 64);
  __syncthreads();
  int32_t cnt = 0;
  for (int64_t round = 0; round <= (int64_t)W * k && cnt < k; ++round) {
    // the windows: entry e = list e >> lb, place e & (B - 1) past its head; a
    // list's B lanes are neighbours in one column.  Each load unconditional at
    // a valid address and masked after it
    uint64_t key[kWin / 64];
    int32_t grp[kWin / 64];
    uint64_t t = 0ull;
#pragma unroll
    for (int i = 0; i < kWin / 64; ++i) {
      key[i] = 0ull;
      grp[i] = -1;
      if (i * 64 >= ne) continue;  // (wave-uniform)
      const int e = i * 64 + lane;
      const int w = e >> lb, j = e & (B - 1);
      const bool in = e < ne;
      const int32_t idx = head[in ? w : 0] + j;
      const bool ok = in && idx < k;
      const int64_t off = ok ? (int64_t)w * rstride + row + idx : row;
      const int32_t d = in_docs[off];
      const float s = in_scores[off];
      const int32_t g = in_groups[off];
      // the list's entries of this window before its first padding
      const uint64_t bad = (__builtin_amdgcn_ballot_w64(!ok || d < 0) >> sh) & bm;
      const int nv = bad ? (int)__builtin_ctzll(bad) : B;
      const bool valid = j < nv;
      key[i] = valid ? make_key(s, (uint32_t)d) : 0ull;
      grp[i] = g;
      if (in) stage[e] = key[i];
      // a full window short of the list's end: the list may go on, every entry
      // past the window below this key
      if (valid && j == B - 1 && idx + 1 < k && key[i] > t) t = key[i];
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) {
      const uint64_t y = __shfl_xor(t, o);
      t = y > t ? y : t;
    }
    __syncthreads();  // (the windows' keys; the heads read above)
    int32_t nsel = 0;
#pragma unroll
    for (int i = 0; i < kWin / 64; ++i) {
      if (i * 64 >= ne) continue;
      const int e = i * 64 + lane;
      const int w = e >> lb, j = e & (B - 1);
      const uint64_t x = key[i];
      const bool sel = x != 0ull && x >= t;
      const uint64_t sm = __builtin_amdgcn_ballot_w64(sel);
      nsel += (int32_t)__popcll(sm);
      if (e < ne && j == 0) head[w] += (int32_t)__popcll((sm >> sh) & bm);
      if (sel) {
        int r = j;
        for (int w2 = 0; w2 < W; ++w2) {
          if (w2 == w) continue;
          const uint64_t* a = stage + (w2 << lb);  // descending, 0 past its valid entries
          int p = 0;
          for (int st = B >> 1; st; st >>= 1)
            if (a[p + st - 1] > x) p += st;
          if (a[p] > x) ++p;
          r += p;
        }
        skey[r] = x;
        sgrp[r] = grp[i];
      }
    }
    if (nsel == 0) break;  // every list is exhausted
    __syncthreads();       // (the merged order; the heads)
    for (int32_t c0 = 0; c0 < nsel && cnt < k; c0 += 64) {
      const int32_t i = c0 + lane;
      const bool real = i < nsel;
      const uint64_t x = skey[real ? i : 0];
      const int32_t g = real ? sgrp[i] : -1;
      const ChunkStep c = chunk_step(tab, slots, lg, real, g, per_group, cnt, k, lane);
      if (c.take) {
        od[c.pos] = (int32_t)(0xFFFFFFFFu - (uint32_t)x);
        os[c.pos] = key_score((uint32_t)(x >> 32));
        if (og) og[c.pos] = g;
      }
      chunk_commit(tab, slots, lg, c.take, g);
      cnt = min(c.total, k);
    }
  }
  for (int32_t i = cnt + lane; i < k; i += 64) {  // padding
    od[i] = -1;
    os[i] = __uint_as_float(0xFFFFFFFFu);
    if (og) og[i] = -1;
  }
}

}  // namespace

hipError_t launch_merge_collapsed(const int32_t* d_docs, const float* d_scores,
                                  const int32_t* d_groups, int64_t W, int64_t Q, int32_t k,
                                  int64_t rank_stride, int32_t per_group, int32_t* d_out_docs,
                                  float* d_out_scores, int32_t* d_out_groups, hipStream_t st) {
  if (Q <= 0 || k <= 0) return hipSuccess;
  if (W < 1 || W > 64 || k > kMaxK || per_group < 1 || Q > 0x7FFFFFFF)
    return hipErrorInvalidValue;
  const int lb = W <= 8 ? 6 : W <= 16 ? 5 : W <= 32 ? 4 : 3;  // W << lb <= kWin
  const int slots = collapse_slots(k);
  int lg = 0;
  while ((1 << lg) < slots) ++lg;
  const dim3 grid((unsigned)Q), block(64);
#define BM25_MERGE_COLLAPSED(S)                                                                  \
  hipLaunchKernelGGL(merge_collapsed_kernel<S>, grid, block, 0, st, d_docs, d_scores, d_groups, \
                     (int32_t)W, k, rank_stride, per_group, lb, slots, lg, d_out_docs,          \
                     d_out_scores, d_out_groups)
  if (slots <= 256)
    BM25_MERGE_COLLAPSED(256);
  else if (slots <= 2048)
    BM25_MERGE_COLLAPSED(2048);
  else
    BM25_MERGE_COLLAPSED(8192);
#undef BM25_MERGE_COLLAPSED
  return hipGetLastError();
}

}  // namespace bm25mi
