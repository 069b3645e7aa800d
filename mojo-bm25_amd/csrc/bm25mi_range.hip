// bm25mi_range.hip — numeric range filters (bm25_range_masks /
// bm25_range_masks_device, include/bm25mi.h): allow-masks made from
// per-document numeric fields,
//
//   allowed(m, d) = d < n_docs and base(m, d)
//                   and for every c with fields[m][c] >= 0:
//                       lo[m][c] <= values[fields[m][c]][d] <= hi[m][c]
//
// The columns are the read traffic (4 or 8 B per document and field against
// 1/8 B per document and mask row written), so a workgroup takes a chunk of
// documents and serves a block of up to kRangeRows rows from one pass over the
// chunk's values: the mirror image of mask_facets_kernel (bm25mi_facets.hip).
//
// Layout: a lane per document for the compare, a lane per row for the words.
// A wave owns a span of kRangeSpanDocs documents (8 mask words).  Lane r first
// loads the span's base words of row r of the row block, one by one (m * W
// words is no multiple of 4 when W is odd, and the caller's pointer need not
// be 16-byte aligned; a word at index >= W of a row is never read, the last
// word is ANDed with the tail mask); without a base they are all ones.  The
// span is then walked in four steps of 64 documents.  A ballot finds the rows
// with a base bit in the step; a (step, row) without one is skipped before any
// compare, and a step that no row of the block allows loads no value.  For
// each live row the clause's field id and bounds are wave-uniform — read from
// lane r, which keeps row r's clauses in registers for the whole item when
// C <= kRangeRegClauses (wider rows read them from memory) — and lane l
// holds values[f][d0 + l] — one coalesced read per field and step, kept in a
// wave-uniform register cache of kRangeCache columns, so rows that name the
// same fields do not reload — and compares; a compare leaves its 64 lanes'
// bits in a wave-uniform mask, the row's clauses are ANDed there, and the mask
// goes to lane r, which ANDs it into its two words of the step.  After
// the span's steps lane r stores its contiguous words of row r with plain
// vector stores, never at index >= W.
//
// A field id >= F matches nothing and reads nothing.  Comparisons are the
// value type's own (the kernel is a template on it): int64 as int64, float32
// as IEEE, so a NaN value or bound fails and -0.0f equals +0.0f.
// No atomics, no LDS, no scratch: every word has one writer, so the result
// does not depend on scheduling.  Reads the caller's buffers only; plain C++
// and vector memory operations throughout.
#include "bm25mi_internal.h"

#include <algorithm>
#include <atomic>

namespace bm25mi {

namespace {

constexpr int kRangeNT = 256;                           // threads per workgroup (4 waves)
constexpr int kRangeSpanWords = (int)kRangeSpanDocs / 32;  // words a lane keeps of its row
constexpr int kRangeSteps = (int)kRangeSpanDocs / 64;
constexpr int kRangeCache = 2;  // columns of a step kept in registers
// a clause's field id as lane r keeps it: >= 0 a field, or one of
constexpr int32_t kPadding = -1;  // no clause in the slot
constexpr int32_t kNoField = -2;  // an id >= F: a field that no document has, matches nothing
static_assert(kRangeRows <= 64, "a lane per row of the block");
static_assert(kRangeSpanDocs % 64 == 0 && kRangeSpanWords == 2 * kRangeSteps, "steps of 64");
static_assert(kRangeChunkDocs % ((kRangeNT / 64) * kRangeSpanDocs) == 0,
              "a chunk is whole rounds of the workgroup's spans");

// Lane r's v as a wave-uniform value (r is wave-uniform).
__device__ __forceinline__ int32_t from_lane(int32_t v, int r) {
  return __builtin_amdgcn_readlane(v, r);
}
__device__ __forceinline__ float from_lane(float v, int r) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), r));
}
__device__ __forceinline__ int64_t from_lane(int64_t v, int r) {
  const uint32_t l = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, r);
  const uint32_t h = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), r);
  return (int64_t)(((uint64_t)h << 32) | l);
}

// The step's column f (wave-uniform, in [0, F)) for this lane's document: from
// the register cache (cf = the field ids held, cv = the values; the column
// just used stays in front), or one coalesced read of values[f][d0 + lane].
template <class T>
__device__ __forceinline__ T column(const T* __restrict__ values, int32_t f, int64_t n_docs,
                                    int64_t d, bool in_docs, int32_t (&cf)[kRangeCache],
                                    T (&cv)[kRangeCache]) {
  static_assert(kRangeCache == 2, "the swap below is written for two columns");
  if (f != cf[0]) {
    if (f == cf[1]) {
      const T t = cv[0];
      cv[0] = cv[1];
      cv[1] = t;
    } else {
      cv[1] = cv[0];
      cv[0] = in_docs ? values[(int64_t)f * n_docs + d] : T(0);
    }
    cf[1] = cf[0];
    cf[0] = f;
  }
  return cv[0];
}

// CM > 0: the rows hold at most CM clauses, and lane r keeps row r's field
// ids and bounds in registers for the whole item, so the inner loop reads no
// clause from memory (a readlane each).  CM == 0: any C, the clause table is
// read from global memory per (step, row) — wave-uniform loads.
template <class T, int CM>
__global__ __launch_bounds__(kRangeNT) void range_masks_kernel(
    const T* __restrict__ values, int64_t F, const int32_t* __restrict__ fields,
    const T* __restrict__ lo, const T* __restrict__ hi, int64_t C, int64_t M,
    const uint32_t* __restrict__ base, int64_t Mb, int64_t W, int64_t n_docs, uint32_t last_mask,
    int64_t chunks, int64_t blocks, uint32_t* __restrict__ out) {
  constexpr int CR = CM > 0 ? CM : 1;
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  const int64_t items = chunks * blocks;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    // (row blocks of one chunk are neighbours: they share the chunk's values in L2)
    const int64_t c = it / blocks, b = it - c * blocks;
    const int64_t m0 = b * kRangeRows;
    const int rows = M - m0 < kRangeRows ? (int)(M - m0) : (int)kRangeRows;
    const bool mine = lane < rows;
    const int64_t m = m0 + (mine ? lane : 0);
    const uint32_t* brow = Mb == 0 ? nullptr : base + (Mb == 1 ? 0 : m) * W;
    uint32_t* orow = out + m * W;
    int32_t rf[CR];
    T rl[CR], rh[CR];
#pragma unroll
    for (int k = 0; k < CR; ++k) {
      const bool has = CM > 0 && mine && k < C;
      const int32_t f = has ? fields[m * C + k] : -1;
      rf[k] = f < 0 ? kPadding : ((int64_t)f < F ? f : kNoField);
      rl[k] = has ? lo[m * C + k] : T(0);
      rh[k] = has ? hi[m * C + k] : T(0);
    }
    const int64_t doc0 = c * kRangeChunkDocs;
    const int64_t doc_end = doc0 + kRangeChunkDocs < n_docs ? doc0 + kRangeChunkDocs : n_docs;
    for (int64_t s0 = doc0 + (int64_t)wave * kRangeSpanDocs; s0 < doc_end;
         s0 += (int64_t)(kRangeNT / 64) * kRangeSpanDocs) {
      const int64_t w0 = s0 >> 5;
      uint32_t x[kRangeSpanWords];
#pragma unroll
      for (int j = 0; j < kRangeSpanWords; ++j) {
        const int64_t w = w0 + j;
        uint32_t v = 0u;
        if (mine && w < W) v = brow ? brow[w] : 0xFFFFFFFFu;
        if (w == W - 1) v &= last_mask;
        x[j] = v;
      }
#pragma unroll
      for (int s = 0; s < kRangeSteps; ++s) {
        uint64_t live = __ballot((x[2 * s] | x[2 * s + 1]) != 0u);
        if (live == 0) continue;  // (wave-uniform: no row allows a document of the step)
        const int64_t d = s0 + 64 * s + lane;
        const bool in_docs = d < n_docs;
        const uint64_t docs_in = __builtin_amdgcn_ballot_w64(in_docs);
        int32_t cf[kRangeCache];
        T cv[kRangeCache];
        uint32_t keep_lo = 0u, keep_hi = 0u;  // lane r: the ballot of row r's clauses
#pragma unroll
        for (int i = 0; i < kRangeCache; ++i) {
          cf[i] = -1;
          cv[i] = T(0);
        }
        while (live) {
          const int r = (int)__builtin_ctzll(live);
          live &= live - 1;
          // the row's documents of the step as a wave-uniform 64-bit mask: a
          // compare writes its lanes' bits straight into it
          uint64_t pass = docs_in;
          if constexpr (CM > 0) {
#pragma unroll
            for (int k = 0; k < CM; ++k) {
              const int32_t f = __builtin_amdgcn_readlane(rf[k], r);  // (wave-uniform)
              if (f < 0) {  // padding, or a field that no document has
                if (f != kPadding) pass = 0;
                continue;
              }
              const T v = column(values, f, n_docs, d, in_docs, cf, cv);
              pass &= __builtin_amdgcn_ballot_w64(from_lane(rl[k], r) <= v) &
                      __builtin_amdgcn_ballot_w64(v <= from_lane(rh[k], r));
            }
          } else {
            const int64_t q0 = (m0 + r) * C;
            for (int64_t k = 0; k < C; ++k) {
              const int32_t f = fields[q0 + k];  // (wave-uniform)
              if (f < 0) continue;               // padding
              if ((int64_t)f >= F) {             // a field that no document has
                pass = 0;
                break;
              }
              const T v = column(values, f, n_docs, d, in_docs, cf, cv);
              pass &= __builtin_amdgcn_ballot_w64(lo[q0 + k] <= v) &
                      __builtin_amdgcn_ballot_w64(v <= hi[q0 + k]);
            }
          }
          keep_lo = lane == r ? (uint32_t)pass : keep_lo;
          keep_hi = lane == r ? (uint32_t)(pass >> 32) : keep_hi;
        }
        x[2 * s] &= keep_lo;  // (a row that was not live: its words are 0 already)
        x[2 * s + 1] &= keep_hi;
      }
      if (mine) {
#pragma unroll
        for (int j = 0; j < kRangeSpanWords; ++j)
          if (w0 + j < W) orow[w0 + j] = x[j];
      }
    }
  }
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

template <class T>
hipError_t launch_typed(const DevIndex& ix, const void* d_values, int64_t F,
                        const int32_t* d_fields, const void* d_lo, const void* d_hi, int64_t C,
                        int64_t M, const uint32_t* d_base, int64_t Mb, uint32_t* d_out,
                        hipStream_t st) {
  const int64_t n_docs = ix.n_docs, W = (n_docs + 31) >> 5;
  const uint32_t tail = (uint32_t)(n_docs & 31);
  const uint32_t last_mask = tail ? (1u << tail) - 1u : 0xFFFFFFFFu;
  const int64_t chunks = (n_docs + kRangeChunkDocs - 1) / kRangeChunkDocs;
  const int64_t blocks = (M + kRangeRows - 1) / kRangeRows;
  // items flattened into a grid-stride loop (M may pass 65535): 8 workgroups
  // per CU hold the chip, more items take more steps
  const unsigned grid = (unsigned)std::max<int64_t>(
      1, std::min<int64_t>(chunks * blocks, (int64_t)device_cus(ix.device) * 8));
  // the narrowest kernel that holds C clauses a row in registers; wider rows
  // take the one that reads its clauses from memory
  auto kernel = C <= 1   ? range_masks_kernel<T, 1>
                : C <= 2 ? range_masks_kernel<T, 2>
                : C <= 4 ? range_masks_kernel<T, 4>
                : C <= kRangeRegClauses ? range_masks_kernel<T, (int)kRangeRegClauses>
                                        : range_masks_kernel<T, 0>;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kRangeNT), 0, st, (const T*)d_values, F, d_fields,
                     (const T*)d_lo, (const T*)d_hi, C, M, d_base, Mb, W, n_docs, last_mask,
                     chunks, blocks, d_out);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_range_masks(const DevIndex& ix, const void* d_values, int kind, int64_t F,
                              const int32_t* d_fields, const void* d_lo, const void* d_hi,
                              int64_t C, int64_t M, const uint32_t* d_base, int64_t Mb,
                              uint32_t* d_out, hipStream_t st) {
  if (M <= 0 || ix.n_docs <= 0) return hipSuccess;
  if (F < 0 || C < 0 || (Mb != 0 && Mb != 1 && Mb != M)) return hipErrorInvalidValue;
  if (!d_base) Mb = 0;
  if (!d_values) F = 0;  // (no column: every field id names a field that no document has)
  switch (kind) {
    case kFieldI32:
      return launch_typed<int32_t>(ix, d_values, F, d_fields, d_lo, d_hi, C, M, d_base, Mb, d_out,
                                   st);
    case kFieldF32:
      return launch_typed<float>(ix, d_values, F, d_fields, d_lo, d_hi, C, M, d_base, Mb, d_out,
                                 st);
    case kFieldI64:
      return launch_typed<int64_t>(ix, d_values, F, d_fields, d_lo, d_hi, C, M, d_base, Mb, d_out,
                                   st);
    default:
      return hipErrorInvalidValue;
  }
}

}  // namespace bm25mi
