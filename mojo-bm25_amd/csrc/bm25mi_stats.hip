// bm25mi_stats.hip — field statistics (bm25_mask_stats / bm25_mask_stats_device,
// include/bm25mi.h): count, min, max and exact sum of a per-document column
// over the documents every allow-mask row allows, ungrouped or per group id,
//
//   bucket (m, b) = the d < n_docs with bit d of mask row m set, groups[d] == b
//                   (ungrouped: b = 0 for every d) and values[d] a number
//
// The fourth reader of (masks, column, groups) and the geometry of
// bm25mi_facets.hip: a lane per document, a wave owns a span of
// kStatsSpanWords mask words (256 documents), lane r holds the span's words of
// row r of the row block, the span is walked in four steps of 64 documents and
// a step's column and groups are loaded — one coalesced read each — only when
// some row of the block has a bit there.  A grid-stride loop runs over the
// (chunk, row block) items.
//
// A bucket's record is stats_slots(kind) u64 slots, every one updated by an
// integer add or an integer max, so the result does not depend on scheduling:
//   [0] count            add
//   [1] ~min key         max  (the order key of bm25mi_sort_key_dev.h,
//   [2] max key          max   complemented in its width for the minimum)
//   [3] int kinds: the wrapping int64 sum;  float32: the +inf count in the low
//       and the -inf count in the high 32 bits        add
//   [4 .. 35] float32 only: the 32 int64 bins of bm25mi_stats_sum.h   add
// A record of zeros is the empty bucket: the launch clears the scratch with
// one memset, and a key slot that stays 0 next to a count > 0 decodes to the
// extreme value that alone can leave it there.
//
// Per (step, live row): the count is one add of the ballot's popcount and the
// integer sum one add of the wave's sum where the row's documents of the step
// share a bucket (always when ungrouped; G == 1, a dominant category), else a
// lane adds its own.  Min and max: a lane issues its atomic max only where its
// key beats the slot's current value (LDS route), which after a row's first
// steps of a chunk is rare.  The float bins depend on the data: where the
// step's finite values of the row share bucket and bin the wave adds their sum
// once, else every lane adds to its own bin — 64-bit integer LDS adds, never
// a per-lane register array of bins (it would live in scratch memory).
//
// Two routes, chosen on the host (launch_mask_stats):
//   LDS (B <= stats_lds_buckets(kind)): stats_rows(kind, B) rows per block,
//     their records in LDS, cleared per item and flushed with one integer
//     global atomic per non-zero slot onto the scratch.
//   global (wider B): one row per item, the same updates as global atomics
//     straight onto the scratch.  Categories this wide are sparse per row.
// The finalise kernel, a thread per bucket, turns keys back into values,
// copies the integer sums and rounds the float bins once (stats_sum_round).
// Reads the caller's buffers only; plain C++ and vector memory operations.
#include "bm25mi_internal.h"
#include "bm25mi_sort_key_dev.h"
#include "bm25mi_stats_sum.h"

#include <algorithm>
#include <atomic>
#include <type_traits>

namespace bm25mi {

namespace {

using u64 = unsigned long long;

constexpr int kStatsNT = 256;        // threads per workgroup (4 waves)
constexpr int kStatsSpanWords = 8;   // mask words of a wave's span (256 documents)
constexpr int kStatsSpanDocs = kStatsSpanWords * 32;
static_assert(kStatsChunk % ((kStatsNT / 64) * kStatsSpanDocs) == 0, "a chunk is whole spans");
static_assert(kStatsMaxRows <= 64, "a lane per row of the block");
static_assert(kStatsF32Slots == 4 + kStatsSumBins, "a float record: 4 slots and the bins");
static_assert(kStatsLdsSlots * 8 <= 65536, "the records of a row block fit a workgroup's LDS");

template <class T>
constexpr int slots_of() {
  return std::is_floating_point<T>::value ? (int)kStatsF32Slots : (int)kStatsIntSlots;
}

__device__ __forceinline__ bool is_number(float v) { return v == v; }
__device__ __forceinline__ bool is_number(int32_t) { return true; }
__device__ __forceinline__ bool is_number(int64_t) { return true; }

// Keys back to values (the inverse of sort_key(v, false)).
__device__ __forceinline__ void key_value(u64 k, int32_t* v) {
  *v = (int32_t)((uint32_t)k ^ 0x80000000u);
}
__device__ __forceinline__ void key_value(u64 k, int64_t* v) {
  *v = (int64_t)(k ^ 0x8000000000000000ull);
}
__device__ __forceinline__ void key_value(u64 k, float* v) {
  const uint32_t u = (uint32_t)k;
  *v = __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}
// The complement of a key in its width: the key of the opposite direction.
template <class T>
__device__ __forceinline__ u64 key_flip(u64 k) {
  return sizeof(T) == 8 ? ~k : (u64)(uint32_t)~(uint32_t)k;
}

// The sum of v over the wave (every lane gets it).
__device__ __forceinline__ int64_t wave_sum(int64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <class T, bool GLOBAL>
__global__ __launch_bounds__(kStatsNT) void mask_stats_kernel(
    const uint32_t* __restrict__ masks, int64_t M, int64_t W, int64_t n_docs, uint32_t last_mask,
    const T* __restrict__ values, const int32_t* __restrict__ groups, int64_t B, int R,
    int64_t chunks, int64_t blocks, u64* __restrict__ scratch) {
  constexpr int S = slots_of<T>();
  constexpr bool F32 = std::is_floating_point<T>::value;
  extern __shared__ u64 lds_acc[];
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  const int64_t items = chunks * blocks;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    // (row blocks of one chunk are neighbours: they share the chunk's column in L2)
    const int64_t c = it / blocks, b = it - c * blocks;
    const int64_t m0 = b * R;
    const int rows = M - m0 < (int64_t)R ? (int)(M - m0) : R;
    const int ns = GLOBAL ? 0 : rows * (int)B * S;
    if (!GLOBAL) {
      for (int i = (int)threadIdx.x; i < ns; i += kStatsNT) lds_acc[i] = 0ull;
      __syncthreads();
    }
    const int64_t doc0 = c * kStatsChunk;
    const int64_t doc_end = doc0 + kStatsChunk < n_docs ? doc0 + kStatsChunk : n_docs;
    const uint32_t* row = masks + (m0 + (lane < rows ? lane : rows - 1)) * W;
    for (int64_t s0 = doc0 + (int64_t)wave * kStatsSpanDocs; s0 < doc_end;
         s0 += (int64_t)(kStatsNT / 64) * kStatsSpanDocs) {
      const int64_t w0 = s0 >> 5;
      uint32_t x[kStatsSpanWords];
#pragma unroll
      for (int j = 0; j < kStatsSpanWords; ++j) {
        const int64_t w = w0 + j;
        uint32_t v = lane < rows && w < W ? row[w] : 0u;
        if (w == W - 1) v &= last_mask;
        x[j] = v;
      }
#pragma unroll
      for (int s = 0; s < kStatsSpanWords / 2; ++s) {
        const uint32_t lo = x[2 * s], hi = x[2 * s + 1];
        uint64_t live = __ballot((lo | hi) != 0u);
        if (live == 0) continue;  // (wave-uniform: no row allows a document of the step)
        const int64_t d = s0 + 64 * s + lane;
        const bool inb = d < n_docs;
        const T v = inb ? values[d] : T(0);
        const int32_t gv = groups ? (inb ? groups[d] : -1) : 0;
        const bool ok = inb && gv >= 0 && (int64_t)gv < B && is_number(v);
        const u64 kmax = sort_key(v, false), kmin = sort_key(v, true);
        const int64_t boff = ok ? (int64_t)gv * S : 0;  // the document's record in its row
        int bin = 0;
        int64_t add = 0;
        bool inf = false;
        if (F32) {
          const uint32_t u = __float_as_uint((float)v);
          inf = (u & 0x7F800000u) == 0x7F800000u;  // (a NaN is not ok)
          if (!inf) stats_addend(u, &bin, &add);
          if (inf) add = (u & 0x80000000u) ? (int64_t)1 << 32 : 1;  // the inf counters' addend
        } else {
          add = (int64_t)v;
        }
        while (live) {
          const int r = (int)__builtin_ctzll(live);
          live &= live - 1;
          const uint32_t rlo = (uint32_t)__builtin_amdgcn_readlane((int)lo, r);
          const uint32_t rhi = (uint32_t)__builtin_amdgcn_readlane((int)hi, r);
          const bool on = ok && (((lane < 32 ? rlo : rhi) >> (lane & 31)) & 1u) != 0u;
          const uint64_t mb = __ballot(on);
          if (mb == 0) continue;  // (wave-uniform)
          const int first = (int)__builtin_ctzll(mb);
          // do the row's documents of the step share a bucket?
          bool uni = true;
          if (groups) {
            const int32_t g0 = __builtin_amdgcn_readlane(gv, first);
            uni = __ballot(on && gv != g0) == 0;
          }
          u64* rec = (GLOBAL ? scratch + (m0 + r) * B * S : lds_acc + (int64_t)r * B * S) + boff;
          if (uni) {
            if (lane == first) atomicAdd(rec, (u64)__popcll(mb));
          } else if (on) {
            atomicAdd(rec, 1ull);
          }
          if (on) {
            if (GLOBAL) {
              atomicMax(rec + 1, kmin);
              atomicMax(rec + 2, kmax);
            } else {
              // (a stale read only costs an atomic that changes nothing)
              if (kmin > __atomic_load_n(rec + 1, __ATOMIC_RELAXED)) atomicMax(rec + 1, kmin);
              if (kmax > __atomic_load_n(rec + 2, __ATOMIC_RELAXED)) atomicMax(rec + 2, kmax);
            }
          }
          if (!F32) {
            if (uni) {
              const int64_t sv = wave_sum(on ? add : 0);
              if (lane == first) atomicAdd(rec + 3, (u64)sv);
            } else if (on) {
              atomicAdd(rec + 3, (u64)add);
            }
          } else {
            if (on && inf) atomicAdd(rec + 3, (u64)add);  // (rare: lane by lane)
            const bool fin = on && !inf;
            const uint64_t mf = __ballot(fin);
            if (mf == 0) continue;  // (wave-uniform)
            const int f1 = (int)__builtin_ctzll(mf);
            const int b0 = __builtin_amdgcn_readlane(bin, f1);
            if (uni && __ballot(fin && bin != b0) == 0) {
              // (64 magnitudes below 2^31: the wave's sum is far inside int64)
              const int64_t sv = wave_sum(fin ? add : 0);
              if (lane == f1) atomicAdd(rec + 4 + bin, (u64)sv);
            } else if (fin) {
              atomicAdd(rec + 4 + bin, (u64)add);
            }
          }
        }
      }
    }
    if (!GLOBAL) {
      __syncthreads();
      u64* dst = scratch + m0 * B * S;  // rows m0 .. m0 + rows - 1 are contiguous
      for (int i = (int)threadIdx.x; i < ns; i += kStatsNT) {
        const u64 v = lds_acc[i];
        if (v == 0ull) continue;
        const int slot = i % S;
        if (slot == 1 || slot == 2)
          atomicMax(dst + i, v);
        else
          atomicAdd(dst + i, v);
      }
      __syncthreads();  // (the records are cleared for the next item)
    }
  }
}

// A thread per bucket: the record -> the outputs (null: not wanted).
template <class T>
__global__ __launch_bounds__(256) void mask_stats_finalise_kernel(
    const u64* __restrict__ scratch, int64_t n, int64_t* __restrict__ out_count,
    T* __restrict__ out_min, T* __restrict__ out_max, void* __restrict__ out_sum) {
  constexpr int S = slots_of<T>();
  constexpr bool F32 = std::is_floating_point<T>::value;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const u64* rec = scratch + i * S;
    const u64 cnt = rec[0];
    out_count[i] = (int64_t)cnt;
    T vmin = T(0), vmax = T(0);
    if (cnt) {
      key_value(key_flip<T>(rec[1]), &vmin);
      key_value(rec[2], &vmax);
    }
    if (out_min) out_min[i] = vmin;
    if (out_max) out_max[i] = vmax;
    if (!out_sum) continue;
    if (F32) {
      int64_t bins[kStatsSumBins];
#pragma unroll
      for (int j = 0; j < kStatsSumBins; ++j) bins[j] = (int64_t)rec[4 + j];
      ((double*)out_sum)[i] =
          cnt ? stats_sum_round(bins, rec[3] & 0xFFFFFFFFull, rec[3] >> 32) : 0.0;
    } else {
      ((int64_t*)out_sum)[i] = cnt ? (int64_t)rec[3] : 0;
    }
  }
}

int stats_device_cus(int device) {
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

template <class T>
hipError_t launch_typed(const DevIndex& ix, const uint32_t* d_masks, int64_t M, const T* d_values,
                        int kind, const int32_t* d_groups, int64_t B, int64_t* d_count, T* d_min,
                        T* d_max, void* d_sum, u64* scratch, hipStream_t st) {
  const int64_t n_docs = ix.n_docs, W = (n_docs + 31) >> 5;
  const int cus = stats_device_cus(ix.device);
  if (W > 0) {
    const uint32_t tail = (uint32_t)(n_docs & 31);
    const uint32_t last_mask = tail ? (1u << tail) - 1u : 0xFFFFFFFFu;
    const bool global = B > stats_lds_buckets(kind);
    const int64_t R = global ? 1 : stats_rows(kind, B);
    const int64_t chunks = (n_docs + kStatsChunk - 1) / kStatsChunk;
    const int64_t blocks = (M + R - 1) / R;
    // items flattened into a grid-stride loop (M may pass 65535)
    const unsigned grid =
        (unsigned)std::max<int64_t>(1, std::min<int64_t>(chunks * blocks, (int64_t)cus * 8));
    if (global) {
      hipLaunchKernelGGL((mask_stats_kernel<T, true>), dim3(grid), dim3(kStatsNT), 0, st, d_masks,
                         M, W, n_docs, last_mask, d_values, d_groups, B, 1, chunks, blocks,
                         scratch);
    } else {
      const size_t lds = sizeof(u64) * (size_t)(std::min<int64_t>(R, M) * B * slots_of<T>());
      hipLaunchKernelGGL((mask_stats_kernel<T, false>), dim3(grid), dim3(kStatsNT), lds, st,
                         d_masks, M, W, n_docs, last_mask, d_values, d_groups, B, (int)R, chunks,
                         blocks, scratch);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  const int64_t n = M * B;
  const unsigned fgrid =
      (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, (int64_t)cus * 8));
  hipLaunchKernelGGL(mask_stats_finalise_kernel<T>, dim3(fgrid), dim3(256), 0, st, scratch, n,
                     d_count, d_min, d_max, d_sum);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_mask_stats(const DevIndex& ix, const uint32_t* d_masks, int64_t M,
                             const void* d_values, int kind, const int32_t* d_groups, int64_t G,
                             int64_t* d_count, void* d_min, void* d_max, void* d_sum,
                             void* d_scratch, hipStream_t st) {
  if (M <= 0) return hipSuccess;
  if (G < 0 || G > 0x7FFFFFFFll || (G > 0) != (d_groups != nullptr)) return hipErrorInvalidValue;
  const int64_t B = G > 0 ? G : 1;
  const int64_t bytes = stats_scratch_bytes(kind, M, G);
  if (bytes < 0) return hipErrorInvalidValue;
  // a record of zeros is the empty bucket: the kernels add and max onto them
  const hipError_t e = hipMemsetAsync(d_scratch, 0, (size_t)bytes, st);
  if (e != hipSuccess) return e;
  u64* scratch = reinterpret_cast<u64*>(d_scratch);
  switch (kind) {
    case kFieldI32:
      return launch_typed<int32_t>(ix, d_masks, M, (const int32_t*)d_values, kind, d_groups, B,
                                   d_count, (int32_t*)d_min, (int32_t*)d_max, d_sum, scratch, st);
    case kFieldF32:
      return launch_typed<float>(ix, d_masks, M, (const float*)d_values, kind, d_groups, B, d_count,
                                 (float*)d_min, (float*)d_max, d_sum, scratch, st);
    case kFieldI64:
      return launch_typed<int64_t>(ix, d_masks, M, (const int64_t*)d_values, kind, d_groups, B,
                                   d_count, (int64_t*)d_min, (int64_t*)d_max, d_sum, scratch, st);
  }
  return hipErrorInvalidValue;
}

}  // namespace bm25mi
