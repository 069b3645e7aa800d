// bm25mi_sorted.hip — sort-by-field search (bm25_sort_ranks /
// bm25_search_sorted, include/bm25mi.h): the k allowed documents of a mask row
// that come first in a column's order.
//
// Rank build, once per column and direction.  sort_key_kernel maps a value to
// an order-preserving unsigned key (sign flips, -0.0f as +0.0f, the NaN flag
// above the value bits, the value bits complemented for a descending order)
// with the identity document as the pair's value; the stable radix_sort_pairs
// (bm25mi_sort.hip) sorts over exactly the key bits used, so equal keys keep
// the doc id order; rank_scatter_kernel writes perm[r] and ranks[perm[r]] = r.
// Everything after it is dtype-free: a rank is a unique 32-bit key.
//
// Selection, per batch.  Row m's state is a rank interval [lo, end), the
// count `below` of its eligible documents under lo, and its cursor thr
// (eligible: allowed and rank > thr).  Every row starts at [0, n_docs); a
// level splits the intervals into `bins` bins of 2^shift ranks — the same
// shift for every row, so the host knows the number of levels —
//   sorted_pass_kernel<false>  a workgroup takes (slice of documents, block of
//       kSortedRows rows): lane r loads row r's mask words of a wave's span,
//       the span is walked in steps of 64 documents with one coalesced read
//       of ranks per step, rows without a bit in the step are skipped, the
//       eligible documents of the row's interval are counted per bin in LDS
//       and the non-zero bins added to hist[M][kSortedBins];
//   sorted_pick_kernel         per row a prefix sum over the bins: the
//       interval becomes the bin that holds the k-th eligible document, below
//       grows by the bins before it (a row with fewer than k eligible
//       documents keeps [0, n_docs) and is finished);
// until the intervals are at most kSortedWmax wide.  Then
//   sorted_pass_kernel<true>   appends every eligible rank below the row's end
//       to the row's list: fewer than k under the interval and at most
//       kSortedWmax inside it, so the capacity sorted_list_cap never overflows
//       (a store past it is dropped all the same: ranks and perm are the
//       caller's);
//   sorted_write_kernel        one workgroup per row sorts the list in LDS and
//       writes the first k as (perm[rank] + doc_offset, rank), padded.
// The list's order depends on scheduling, its content and so the sorted
// output do not.  Global atomics are integer adds (histogram bins, list
// counts).  Plain C++ and vector memory operations throughout.
#include "bm25mi_internal.h"
#include "bm25mi_sort_key_dev.h"

#include <algorithm>
#include <atomic>
#include <type_traits>

namespace bm25mi {

namespace {

constexpr int kSoNT = 256;  // threads per workgroup (4 waves)
constexpr int kSoSpanWords = (int)kSortedSpanDocs / 32;
constexpr int kSoSteps = (int)kSortedSpanDocs / 64;
static_assert(kSortedRows <= 64, "a lane per row of the block");
static_assert(kSortedRoundDocs == (kSoNT / 64) * kSortedSpanDocs, "a round is the waves' spans");
static_assert(kSortedBins <= kSoNT, "the pick kernel holds a bin per thread");

// ---- rank build (sort_key: bm25mi_sort_key_dev.h) ---------------------------

template <class T>
__global__ __launch_bounds__(256) void sort_key_kernel(const T* __restrict__ values, int64_t n,
                                                       int desc, uint64_t* __restrict__ keys,
                                                       uint32_t* __restrict__ vals) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    keys[i] = sort_key(values[i], desc != 0);
    vals[i] = (uint32_t)i;
  }
}

__global__ __launch_bounds__(256) void rank_scatter_kernel(const uint32_t* __restrict__ sorted,
                                                           int64_t n, int32_t* __restrict__ ranks,
                                                           int32_t* __restrict__ perm) {
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
    const uint32_t d = sorted[r];
    perm[r] = (int32_t)d;
    ranks[d] = (int32_t)r;  // (d < n: a value of the identity the sort permuted)
  }
}

template <class T>
hipError_t sort_ranks_typed(const T* d_values, int64_t n, bool desc, int32_t* d_ranks,
                            int32_t* d_perm, hipStream_t st) {
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t kb = al(8 * (size_t)n), vb = al(4 * (size_t)n);
  char* buf = nullptr;
  hipError_t e = hipMalloc((void**)&buf, 2 * kb + 2 * vb + al(radix_sort_scratch_bytes(n)));
  if (e != hipSuccess) return e;
  uint64_t* keys = (uint64_t*)buf;
  uint64_t* keys_alt = (uint64_t*)(buf + kb);
  uint32_t* vals = (uint32_t*)(buf + 2 * kb);
  uint32_t* vals_alt = (uint32_t*)(buf + 2 * kb + vb);
  void* scratch = buf + 2 * kb + 2 * vb;
  const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 8192);
  hipLaunchKernelGGL(sort_key_kernel<T>, dim3(grid), dim3(256), 0, st, d_values, n, desc ? 1 : 0,
                     keys, vals);
  e = hipGetLastError();
  bool in_alt = false;
  if (e == hipSuccess)
    e = radix_sort_pairs(keys, vals, keys_alt, vals_alt, n, 0, sort_key_bits<T>(), false, 0,
                         scratch, &in_alt, st);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(rank_scatter_kernel, dim3(grid), dim3(256), 0, st,
                       in_alt ? vals_alt : vals, n, d_ranks, d_perm);
    e = hipGetLastError();
  }
  // the buffers are this call's own: the stream is done with them before they go
  const hipError_t es = hipStreamSynchronize(st);
  hipFree(buf);
  return e != hipSuccess ? e : es;
}

// ---- selection ------------------------------------------------------------

// Row state, four int32 per row.
enum { kStLo = 0, kStEnd = 1, kStBelow = 2, kStThr = 3 };

__global__ __launch_bounds__(256) void sorted_init_kernel(const int32_t* __restrict__ after,
                                                          int64_t M, int32_t n, int32_t k,
                                                          int32_t* __restrict__ st,
                                                          int32_t* __restrict__ cnt) {
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const int32_t c = after ? after[m] : -2;
  const bool dead = c == -1;  // the cursor of a padding slot: nothing follows
  st[4 * m + kStLo] = 0;
  st[4 * m + kStEnd] = dead ? 0 : n;
  st[4 * m + kStBelow] = dead ? k : 0;  // (below >= k: the row is finished)
  st[4 * m + kStThr] = c < -1 ? -1 : c;
  cnt[m] = 0;
}

__device__ __forceinline__ uint32_t lanes_below(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// kCollect = false: a level's histogram (bins B of 2^shift ranks from each
// row's lo).  kCollect = true: the eligible ranks below each row's end into
// lists[M][cap], counted in cnt[M].
template <bool kCollect>
__global__ __launch_bounds__(kSoNT) void sorted_pass_kernel(
    const uint32_t* __restrict__ masks, const int32_t* __restrict__ ranks, int64_t W,
    int64_t n_docs, int64_t M, int64_t blocks, int64_t slice_docs, int B, int shift, int32_t k,
    const int32_t* __restrict__ st, uint32_t* __restrict__ hist, int32_t* __restrict__ cnt,
    int32_t* __restrict__ lists, int32_t cap) {
  __shared__ uint32_t h[kCollect ? 1 : kSortedRows * kSortedBins];
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  // (row blocks of one slice are neighbours: they share the slice's ranks in L2)
  const int64_t sl = (int64_t)blockIdx.x / blocks, b = (int64_t)blockIdx.x - sl * blocks;
  const int64_t m0 = b * kSortedRows;
  const int rows = M - m0 < kSortedRows ? (int)(M - m0) : (int)kSortedRows;
  const bool mine = lane < rows;
  const int64_t m = m0 + (mine ? lane : 0);
  const int32_t lo = kCollect ? 0 : st[4 * m + kStLo];
  const int32_t end = st[4 * m + kStEnd];
  const int32_t thr = st[4 * m + kStThr];
  // a finished row of a level, or an all-padding row: no word is read
  const bool live_row = mine && end > lo && (kCollect || st[4 * m + kStBelow] < k);
  const uint32_t* mrow = masks + m * W;
  if (!kCollect) {
    for (int i = (int)threadIdx.x; i < rows * B; i += kSoNT) h[i] = 0u;
    __syncthreads();
  }
  const int64_t doc0 = sl * slice_docs;
  const int64_t doc_end = doc0 + slice_docs < n_docs ? doc0 + slice_docs : n_docs;
  for (int64_t s0 = doc0 + (int64_t)wave * kSortedSpanDocs; s0 < doc_end; s0 += kSortedRoundDocs) {
    const int64_t w0 = s0 >> 5;
    uint32_t x[kSoSpanWords];
#pragma unroll
    for (int j = 0; j < kSoSpanWords; ++j) x[j] = (live_row && w0 + j < W) ? mrow[w0 + j] : 0u;
#pragma unroll
    for (int s = 0; s < kSoSteps; ++s) {
      uint64_t live = __ballot((x[2 * s] | x[2 * s + 1]) != 0u);
      if (live == 0) continue;  // (wave-uniform: no row allows a document of the step)
      const int64_t d = s0 + 64 * s + lane;
      const bool in_docs = d < n_docs;  // (bits at or past n_docs never count)
      const int32_t rank = in_docs ? ranks[d] : -1;
      while (live) {
        const int r = (int)__builtin_ctzll(live);
        live &= live - 1;
        const uint64_t bits = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)x[2 * s], r) |
                              ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)x[2 * s + 1], r)
                               << 32);
        const int32_t rlo = __builtin_amdgcn_readlane(lo, r);
        const int32_t rend = __builtin_amdgcn_readlane(end, r);
        const int32_t rthr = __builtin_amdgcn_readlane(thr, r);
        // (a rank outside [0, n_docs) lies in no interval: never eligible)
        const bool e = in_docs && ((bits >> lane) & 1ull) != 0ull && rank > rthr &&
                       (uint32_t)(rank - rlo) < (uint32_t)(rend - rlo);
        const uint64_t em = __ballot(e);
        if (em == 0) continue;
        const int first = (int)__builtin_ctzll(em);
        if (kCollect) {
          int32_t base = 0;
          if (lane == first) base = atomicAdd(&cnt[m0 + r], (int32_t)__popcll(em));
          base = __builtin_amdgcn_readlane(base, first);
          const int64_t pos = (int64_t)base + lanes_below(em);
          if (e && pos < cap) lists[(m0 + r) * cap + pos] = rank;
        } else {
          const uint32_t bin = (uint32_t)(rank - rlo) >> shift;
          // documents in id order often share a bin (a column that grows with
          // the id): one add for the step then
          const uint32_t bin0 = (uint32_t)__builtin_amdgcn_readlane((int)bin, first);
          if (__ballot(e && bin == bin0) == em) {
            if (lane == first && bin0 < (uint32_t)B) atomicAdd(&h[r * B + bin0], (uint32_t)__popcll(em));
          } else if (e && bin < (uint32_t)B) {
            atomicAdd(&h[r * B + bin], 1u);
          }
        }
      }
    }
  }
  if (!kCollect) {
    __syncthreads();
    for (int i = (int)threadIdx.x; i < rows * B; i += kSoNT) {
      const uint32_t v = h[i];
      if (v) atomicAdd(&hist[(m0 + i / B) * kSortedBins + i % B], v);
    }
  }
}

// Exclusive scan of one value per thread over the workgroup; *total = the sum.
__device__ __forceinline__ uint32_t block_excl(uint32_t x, uint32_t* wsum, uint32_t* total) {
  const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  uint32_t incl = x;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t y = (uint32_t)__shfl_up((int)incl, o, 64);
    if ((int)lane >= o) incl += y;
  }
  if (lane == 63u) wsum[w] = incl;
  __syncthreads();
  uint32_t pre = 0u;
  for (uint32_t j = 0; j < w; ++j) pre += wsum[j];
  *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  return pre + incl - x;
}

// One workgroup per row: the row's interval becomes the bin of its k-th
// eligible document; the row's bins are zeroed for the next level.
__global__ __launch_bounds__(kSoNT) void sorted_pick_kernel(uint32_t* __restrict__ hist, int B,
                                                            int shift, int32_t k,
                                                            int32_t* __restrict__ st) {
  __shared__ uint32_t wsum[4];
  const int64_t m = blockIdx.x;
  const int t = (int)threadIdx.x;
  const int32_t lo = st[4 * m + kStLo], end = st[4 * m + kStEnd], below = st[4 * m + kStBelow];
  uint32_t v = 0u;
  if (t < B) {
    v = hist[m * kSortedBins + t];
    hist[m * kSortedBins + t] = 0u;
  }
  uint32_t total = 0u;
  const uint32_t ex = block_excl(v, wsum, &total);
  if (below >= k || end <= lo) return;  // (finished: the pass counted nothing for it)
  const uint32_t need = (uint32_t)(k - below);
  if (total < need) {  // fewer than k eligible documents: all of them, the interval stays
    if (t == 0) st[4 * m + kStBelow] = k;
    return;
  }
  if (ex < need && need <= ex + v) {  // (one thread: the bins' prefix sums are monotone)
    const int64_t nlo = (int64_t)lo + ((int64_t)t << shift);
    const int64_t nend = std::min<int64_t>(end, nlo + ((int64_t)1 << shift));
    st[4 * m + kStLo] = (int32_t)nlo;
    st[4 * m + kStEnd] = (int32_t)nend;
    st[4 * m + kStBelow] = below + (int32_t)ex;
  }
}

// One workgroup per row: the list sorted ascending in LDS (bitonic over the
// next power of two), the first k written with their documents, the rest of
// the row padded.
__global__ __launch_bounds__(kSoNT) void sorted_write_kernel(
    const int32_t* __restrict__ lists, const int32_t* __restrict__ cnt, int32_t cap,
    const int32_t* __restrict__ perm, int32_t doc_offset, int32_t k, int32_t* __restrict__ out_docs,
    int32_t* __restrict__ out_ranks) {
  __shared__ int32_t buf[kSortedSortP];
  const int64_t m = blockIdx.x;
  const int t = (int)threadIdx.x;
  int32_t c = cnt[m];
  c = c < 0 ? 0 : (c > cap ? cap : c);
  int P = 1;
  while (P < c) P <<= 1;  // (c <= cap <= kSortedSortP)
  for (int i = t; i < P; i += kSoNT) buf[i] = i < c ? lists[m * cap + i] : 0x7FFFFFFF;
  for (int size = 2; size <= P; size <<= 1)
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int i = t; i < (P >> 1); i += kSoNT) {
        const int a = 2 * i - (i & (stride - 1)), bI = a + stride;
        const bool up = (a & size) == 0;
        const int32_t va = buf[a], vb = buf[bI];
        if ((va > vb) == up) {
          buf[a] = vb;
          buf[bI] = va;
        }
      }
    }
  __syncthreads();
  for (int j = t; j < k; j += kSoNT) {
    const bool has = j < c;
    const int32_t r = has ? buf[j] : -1;  // (a listed rank is in [0, n_docs))
    out_docs[m * k + j] = has ? perm[r] + doc_offset : -1;
    out_ranks[m * k + j] = r;
  }
}

// No mask: row m is perm[thr + 1 .. thr + k].
__global__ __launch_bounds__(256) void sorted_all_kernel(const int32_t* __restrict__ after,
                                                         int64_t M, int32_t n, int32_t k,
                                                         const int32_t* __restrict__ perm,
                                                         int32_t doc_offset,
                                                         int32_t* __restrict__ out_docs,
                                                         int32_t* __restrict__ out_ranks) {
  const int64_t total = M * k;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * 256) {
    const int64_t m = i / k;
    const int32_t c = after ? after[m] : -2;
    const int64_t r = (int64_t)(c < -1 ? -1 : c) + 1 + (i - m * k);
    const bool has = c != -1 && r < n;
    out_docs[i] = has ? perm[r] + doc_offset : -1;
    out_ranks[i] = has ? (int32_t)r : -1;
  }
}

__global__ __launch_bounds__(256) void sorted_pad_scores_kernel(const int32_t* __restrict__ docs,
                                                                uint32_t* __restrict__ scores,
                                                                int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    if (docs[i] < 0) scores[i] = 0xFFFFFFFFu;
}

int device_cus(int device) {
  static std::atomic<int> s_cus{0};
  int cus = s_cus.load(std::memory_order_relaxed);
  if (cus == 0) {
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess ||
        cus <= 0)
      cus = 256;
    s_cus.store(cus, std::memory_order_relaxed);
  }
  return cus;
}

}  // namespace

hipError_t launch_sort_ranks(const DevIndex& ix, const void* d_values, int kind, bool descending,
                             int32_t* d_ranks, int32_t* d_perm, hipStream_t st) {
  const int64_t n = ix.n_docs;
  if (n <= 0) return hipSuccess;
  switch (kind) {
    case kFieldI32:
      return sort_ranks_typed((const int32_t*)d_values, n, descending, d_ranks, d_perm, st);
    case kFieldF32:
      return sort_ranks_typed((const float*)d_values, n, descending, d_ranks, d_perm, st);
    case kFieldI64:
      return sort_ranks_typed((const int64_t*)d_values, n, descending, d_ranks, d_perm, st);
    default:
      return hipErrorInvalidValue;
  }
}

hipError_t launch_search_sorted(const DevIndex& ix, const uint32_t* d_masks, int64_t M,
                                const int32_t* d_ranks, const int32_t* d_perm, int32_t k,
                                const int32_t* d_after, int32_t* d_docs, int32_t* d_out_ranks,
                                void* d_scratch, int bins, hipStream_t st) {
  const int64_t n = ix.n_docs;
  if (M <= 0 || k <= 0) return hipSuccess;
  if (n <= 0 || n > 0x7FFFFFFFll || k > kMaxK || k > n) return hipErrorInvalidValue;
  if (!d_masks) {
    const unsigned grid = (unsigned)std::min<int64_t>((M * k + 255) / 256, 65536);
    hipLaunchKernelGGL(sorted_all_kernel, dim3(grid), dim3(256), 0, st, d_after, M, (int32_t)n, k,
                       d_perm, (int32_t)ix.doc_offset, d_docs, d_out_ranks);
    return hipGetLastError();
  }
  const int B = bins < 2 ? (int)kSortedBins : std::min<int>(bins, (int)kSortedBins);
  const int64_t W = (n + 31) >> 5;
  const int32_t cap = (int32_t)sorted_list_cap(n, k);
  // the scratch of sorted_scratch_bytes: state, list counts, histogram, lists
  int32_t* state = (int32_t*)d_scratch;
  int32_t* cnt = state + 4 * M;
  uint32_t* hist = (uint32_t*)(cnt + M);
  int32_t* lists = (int32_t*)(hist + M * kSortedBins);
  hipLaunchKernelGGL(sorted_init_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st,
                     d_after, M, (int32_t)n, k, state, cnt);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // (slice of documents, block of rows) items: about 8 workgroups per CU, a
  // slice is whole rounds of the workgroup (M may pass 65535: the grid is 1-D)
  const int64_t blocks = (M + kSortedRows - 1) / kSortedRows;
  const int64_t rounds = (n + kSortedRoundDocs - 1) / kSortedRoundDocs;
  const int64_t want = std::max<int64_t>(1, ((int64_t)device_cus(ix.device) * 8) / blocks);
  const int64_t slice_rounds = (rounds + std::min(want, rounds) - 1) / std::min(want, rounds);
  const int64_t slice_docs = slice_rounds * kSortedRoundDocs;
  const int64_t slices = (n + slice_docs - 1) / slice_docs;
  const dim3 grid((unsigned)(slices * blocks));
  int64_t width = n;
  if (width > kSortedWmax) {
    e = hipMemsetAsync(hist, 0, sizeof(uint32_t) * M * kSortedBins, st);
    if (e != hipSuccess) return e;
  }
  while (width > kSortedWmax) {
    int shift = 0;
    while (((int64_t)B << shift) < width) ++shift;
    hipLaunchKernelGGL(sorted_pass_kernel<false>, grid, dim3(kSoNT), 0, st, d_masks, d_ranks, W, n,
                       M, blocks, slice_docs, B, shift, k, state, hist, cnt, lists, cap);
    hipLaunchKernelGGL(sorted_pick_kernel, dim3((unsigned)M), dim3(kSoNT), 0, st, hist, B, shift, k,
                       state);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    width = (int64_t)1 << shift;  // (B >= 2: strictly narrower)
  }
  hipLaunchKernelGGL(sorted_pass_kernel<true>, grid, dim3(kSoNT), 0, st, d_masks, d_ranks, W, n, M,
                     blocks, slice_docs, B, 0, k, state, hist, cnt, lists, cap);
  hipLaunchKernelGGL(sorted_write_kernel, dim3((unsigned)M), dim3(kSoNT), 0, st, lists, cnt, cap,
                     d_perm, (int32_t)ix.doc_offset, k, d_docs, d_out_ranks);
  return hipGetLastError();
}

hipError_t launch_sorted_pad_scores(const int32_t* d_docs, float* d_scores, int64_t n,
                                    hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 65536);
  hipLaunchKernelGGL(sorted_pad_scores_kernel, dim3(grid), dim3(256), 0, st, d_docs,
                     (uint32_t*)d_scores, n);
  return hipGetLastError();
}

}  // namespace bm25mi
