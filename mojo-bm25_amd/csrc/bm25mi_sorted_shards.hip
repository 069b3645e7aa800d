// bm25mi_sorted_shards.hip — sort-by-field search over doc shards
// (bm25_sort_keys_device / bm25_sort_cursor_device /
// bm25_merge_sort_keys_device, include/bm25mi.h): a rank is a position in one
// handle's permutation, so shards exchange the collection-wide order key
// K(value) of bm25mi_sort_key_dev.h instead, as two uint32 planes beside the
// global doc ids, and everything here orders by (K, doc).
//
// Replaces no reference call: the reference is single-device (main.py:205) and
// has no sort-by-field search.
//
//   sort_keys_kernel     a thread per hit: K(values[doc - doc_offset]) split into
//     key_hi / key_lo; a doc outside the handle's range (padding included) gets
//     the all-ones key and reads no value.
//   sort_cursor_kernel   a thread per row: the collection cursor (key, doc)
//     counted into this handle's order by one binary search over perm — perm
//     is sorted by exactly (K(values[perm[r]]), doc_offset + perm[r]) — as the
//     rank cursor of bm25_search_sorted_device.
//   merge_keys_kernel    a workgroup per row folds the W lists one after
//     another into an accumulator of at most k entries in LDS: the list is
//     staged in LDS up to its first padding, every entry of the accumulator and
//     of the list finds its place in the union by a binary search of the other
//     side (a two-way merge by ranking, both searches in LDS), places >= k are
//     dropped, the two accumulator buffers swap.  W k log k steps a row.  Three
//     buffers of KCAP (u64 key, i32 doc) entries: 36 * KCAP bytes of static LDS
//     (4.5, 36 and 144 KiB at KCAP 128, 1024 and 4096).
//
// No global scratch, no global atomics (the list length is a minimum in LDS),
// no host synchronisation; a row is one workgroup's, so nothing depends on
// scheduling.  Plain C++ and vector memory operations throughout.
//
// Bounds, whatever the input holds: a place is written only when < k <= KCAP,
// a search runs over [0, length) with length <= k and halves its interval each
// step, the lengths never pass k, and perm entries are range-checked before a
// value is read.
#include "bm25mi_internal.h"
#include "bm25mi_sort_key_dev.h"

#include <algorithm>

namespace bm25mi {

namespace {

// ---- keys of a page ---------------------------------------------------------

template <class T>
__global__ __launch_bounds__(256) void sort_keys_kernel(const T* __restrict__ values,
                                                        int64_t n_docs, int64_t doc_offset,
                                                        int desc, const int32_t* __restrict__ docs,
                                                        int64_t n, uint32_t* __restrict__ key_hi,
                                                        uint32_t* __restrict__ key_lo) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int64_t d = (int64_t)docs[i] - doc_offset;
    uint64_t key = ~0ull;  // padding, or a document of another shard
    if (docs[i] >= 0 && d >= 0 && d < n_docs) key = sort_key(values[d], desc != 0);
    key_hi[i] = (uint32_t)(key >> 32);
    key_lo[i] = (uint32_t)key;
  }
}

// ---- collection cursor -> rank cursor ---------------------------------------

template <class T>
__global__ __launch_bounds__(256) void sort_cursor_kernel(
    const T* __restrict__ values, int64_t n_docs, int64_t doc_offset, int desc,
    const int32_t* __restrict__ perm, const uint32_t* __restrict__ after_hi,
    const uint32_t* __restrict__ after_lo, const int32_t* __restrict__ after_docs, int64_t M,
    int32_t* __restrict__ after_ranks) {
  const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const int32_t ad = after_docs[m];
  if (ad < 0) {  // -1: the doc of a padding slot, the row is exhausted; below: no cursor
    after_ranks[m] = ad == -1 ? -1 : -2;
    return;
  }
  const uint64_t key = ((uint64_t)after_hi[m] << 32) | after_lo[m];
  // c = the documents of this handle at or before the cursor: perm is sorted
  // by the pair, so the first rank after the cursor
  int64_t lo = 0, hi = n_docs;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    const int32_t p = perm[mid];
    bool le = false;  // (an entry outside the column: as if after the cursor, no value read)
    if (p >= 0 && p < n_docs) {
      const uint64_t kp = sort_key(values[p], desc != 0);
      le = kp < key || (kp == key && doc_offset + (int64_t)p <= (int64_t)ad);
    }
    if (le) lo = mid + 1; else hi = mid;
  }
  // (nothing at or before the cursor: everything is eligible, which is "no
  // cursor" — -1 would end the row)
  after_ranks[m] = lo == 0 ? -2 : (int32_t)(lo - 1);
}

// ---- W-way merge on (key, doc) ----------------------------------------------

// Entries of a[0 .. n) before (k, d) in (key, doc) order — or, with kOrEqual,
// at or before it (the two sides of a fold break a tie one way).
template <bool kOrEqual>
__device__ __forceinline__ int count_before(const uint64_t* akey, const int32_t* adoc, int n,
                                            uint64_t k, int32_t d) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const uint64_t km = akey[mid];
    const int32_t dm = adoc[mid];
    const bool before = km < k || (km == k && (kOrEqual ? dm <= d : dm < d));
    if (before) lo = mid + 1; else hi = mid;
  }
  return lo;
}

template <int KCAP, int NT>
__global__ __launch_bounds__(NT) void merge_keys_kernel(
    const int32_t* __restrict__ in_docs, const uint32_t* __restrict__ in_hi,
    const uint32_t* __restrict__ in_lo, int32_t W, int32_t k, int64_t rstride,
    int32_t* __restrict__ out_docs, uint32_t* __restrict__ out_hi,
    uint32_t* __restrict__ out_lo) {
  __shared__ uint64_t skey[3][KCAP];
  __shared__ int32_t sdoc[3][KCAP];
  __shared__ int32_t s_len[2];  // (by fold parity: a fold's length is read while the next is set)
  const int t = (int)threadIdx.x;
  const int64_t row = (int64_t)blockIdx.x * k;
  int a = 0, o = 1;  // the accumulator and the fold's output; buffer 2 stages a list
  int32_t la = 0;    // entries of the accumulator
  uint64_t* lkey = skey[2];
  int32_t* ldoc = sdoc[2];
  for (int32_t w = 0; w < W; ++w) {
    int32_t* len = &s_len[w & 1];
    if (t == 0) *len = k;
    __syncthreads();  // (the length; the last fold's reads of the stage)
    const int64_t base = (int64_t)w * rstride + row;
    for (int32_t i = t; i < k; i += NT) {
      const int32_t d = in_docs[base + i];
      lkey[i] = ((uint64_t)in_hi[base + i] << 32) | in_lo[base + i];
      ldoc[i] = d;
      if (d < 0) atomicMin(len, i);  // (LDS: the list ends at its first padding)
    }
    __syncthreads();
    const int32_t ll = *len;
    if (ll == 0) continue;  // (uniform)
    const uint64_t* akey = skey[a];
    const int32_t* adoc = sdoc[a];
    uint64_t* okey = skey[o];
    int32_t* odoc = sdoc[o];
    for (int32_t i = t; i < la; i += NT) {
      const uint64_t x = akey[i];
      const int32_t d = adoc[i];
      const int32_t r = i + count_before<false>(lkey, ldoc, ll, x, d);
      if (r < k) {
        okey[r] = x;
        odoc[r] = d;
      }
    }
    for (int32_t j = t; j < ll; j += NT) {
      const uint64_t x = lkey[j];
      const int32_t d = ldoc[j];
      const int32_t r = j + count_before<true>(akey, adoc, la, x, d);
      if (r < k) {
        okey[r] = x;
        odoc[r] = d;
      }
    }
    la = min(k, la + ll);
    a ^= 1;
    o ^= 1;
  }
  __syncthreads();  // (the last fold's output)
  for (int32_t i = t; i < k; i += NT) {
    const bool has = i < la;
    const uint64_t x = has ? skey[a][i] : ~0ull;
    out_docs[row + i] = has ? sdoc[a][i] : -1;
    out_hi[row + i] = (uint32_t)(x >> 32);
    out_lo[row + i] = (uint32_t)x;
  }
}

}  // namespace

hipError_t launch_sort_keys(const DevIndex& ix, const void* d_values, int kind, bool descending,
                            const int32_t* d_docs, int64_t n, uint32_t* d_key_hi,
                            uint32_t* d_key_lo, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 65536);
#define BM25_SORT_KEYS(T)                                                                       \
  hipLaunchKernelGGL(sort_keys_kernel<T>, dim3(grid), dim3(256), 0, st, (const T*)d_values,    \
                     ix.n_docs, ix.doc_offset, descending ? 1 : 0, d_docs, n, d_key_hi, d_key_lo)
  switch (kind) {
    case kFieldI32: BM25_SORT_KEYS(int32_t); break;
    case kFieldF32: BM25_SORT_KEYS(float); break;
    case kFieldI64: BM25_SORT_KEYS(int64_t); break;
    default: return hipErrorInvalidValue;
  }
#undef BM25_SORT_KEYS
  return hipGetLastError();
}

hipError_t launch_sort_cursor(const DevIndex& ix, const void* d_values, int kind, bool descending,
                              const int32_t* d_perm, const uint32_t* d_after_hi,
                              const uint32_t* d_after_lo, const int32_t* d_after_docs, int64_t M,
                              int32_t* d_after_ranks, hipStream_t st) {
  if (M <= 0) return hipSuccess;
  if ((M + 255) / 256 > 0x7FFFFFFFll) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((M + 255) / 256));  // (M may pass 65535: the grid is 1-D)
#define BM25_SORT_CURSOR(T)                                                                      \
  hipLaunchKernelGGL(sort_cursor_kernel<T>, grid, dim3(256), 0, st, (const T*)d_values,         \
                     ix.n_docs, ix.doc_offset, descending ? 1 : 0, d_perm, d_after_hi,           \
                     d_after_lo, d_after_docs, M, d_after_ranks)
  switch (kind) {
    case kFieldI32: BM25_SORT_CURSOR(int32_t); break;
    case kFieldF32: BM25_SORT_CURSOR(float); break;
    case kFieldI64: BM25_SORT_CURSOR(int64_t); break;
    default: return hipErrorInvalidValue;
  }
#undef BM25_SORT_CURSOR
  return hipGetLastError();
}

hipError_t launch_merge_sort_keys(const int32_t* d_docs, const uint32_t* d_key_hi,
                                  const uint32_t* d_key_lo, int64_t W, int64_t Q, int32_t k,
                                  int64_t rank_stride, int32_t* d_out_docs, uint32_t* d_out_key_hi,
                                  uint32_t* d_out_key_lo, hipStream_t st) {
  if (Q <= 0 || k <= 0) return hipSuccess;
  if (W < 1 || W > 64 || k > kMaxK || Q > 0x7FFFFFFF) return hipErrorInvalidValue;
  const dim3 grid((unsigned)Q);  // (Q may pass 65535: the grid is 1-D)
#define BM25_MERGE_KEYS(KCAP, NT)                                                              \
  hipLaunchKernelGGL((merge_keys_kernel<KCAP, NT>), grid, dim3(NT), 0, st, d_docs, d_key_hi,  \
                     d_key_lo, (int32_t)W, k, rank_stride, d_out_docs, d_out_key_hi,           \
                     d_out_key_lo)
  if (k <= 128)
    BM25_MERGE_KEYS(128, 64);
  else if (k <= 1024)
    BM25_MERGE_KEYS(1024, 256);
  else
    BM25_MERGE_KEYS(4096, 1024);
#undef BM25_MERGE_KEYS
  return hipGetLastError();
}

}  // namespace bm25mi
