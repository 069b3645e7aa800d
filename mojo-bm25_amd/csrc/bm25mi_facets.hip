// bm25mi_facets.hip — facet counts (bm25_mask_facets / bm25_mask_facets_device,
// include/bm25mi.h): the hit count of every allow-mask broken down by a
// per-document group id,
//
//   out[m][g] = number of d < n_docs with bit d of mask row m set and groups[d] == g
//
// a gather of groups[d] under a bit mask into a histogram.  The group array is
// the traffic (4 B per document against 1/8 B per document and mask row), so a
// workgroup takes a chunk of documents and serves a block of up to R mask rows
// from one read of the chunk's groups.
//
// Layout: a lane per document.  A wave owns a span of kFacetSpanWords mask
// words (256 documents).  Lane r first loads the span's words of row r of the
// row block, one by one (m * W words is no multiple of 4 when W is odd, and the
// caller's pointer need not be 16-byte aligned; a word at index >= W of a row
// is never read, the last word is ANDed with the tail mask), so after that the
// row block's mask bits of the span sit in registers.  The span is then walked
// in four steps of 64 documents: a ballot finds the rows with a set bit in the
// step; with none, the step's groups are not loaded at all (sparse masks).
// Otherwise lane l loads groups[d0 + l] — one coalesced 256-byte read — and
// for every such row the wave reads the row's two words from its lane
// (readlane, the row is wave-uniform), tests its own bit and adds 1 to the
// row's bin of its group.
//
// Hot bins: the add is wave-aggregated as hist_add of bm25mi_large.hip is —
// ballots over the bits of the group id find the lanes that share a bin, the
// first of them adds their number — so a wave whose documents all fall in one
// group (G == 1, a dominant category) issues one add, not 64 on one address.
// Sparse rows: a row with at most kFacetFewBits documents in the step skips
// the ballots — the wave walks the row's set bits (they are wave-uniform),
// reads each document's group from the lane that holds it and one lane adds.
//
// Two routes, chosen on the host (launch_mask_facets):
//   LDS (G <= kFacetBins): R = min(kFacetMaxRows, kFacetBins / G) rows per
//     block, R x G u32 bins in LDS per workgroup, cleared per (chunk, row
//     block) and flushed with one 64-bit global atomic per non-zero bin onto
//     counts that the launch zeroed on the same stream.  The chunk grows with
//     the bins (facet_chunk_docs) so the flush stays a small share of its work;
//     a chunk holds at most 65536 documents, so a u32 bin cannot overflow.
//   global (G > kFacetBins): one row per item, chunks of kFacetGlobalChunk
//     documents, the same wave-aggregated add as a 64-bit global atomic onto
//     the zeroed output.  Categories this wide are sparse per row.
// Integer sums: the result does not depend on scheduling.  Reads the caller's
// masks and groups only; plain C++ and vector memory operations throughout.
#include "bm25mi_internal.h"

#include <algorithm>
#include <atomic>

namespace bm25mi {

int64_t facet_rows(int64_t G) {
  return std::max<int64_t>(1, std::min<int64_t>(kFacetMaxRows, G > 0 ? kFacetBins / G : 1));
}

int64_t facet_chunk_docs(int64_t G, int64_t M) {
  if (G > kFacetBins) return kFacetGlobalChunk;
  const int64_t bins = std::min<int64_t>(facet_rows(G), std::max<int64_t>(M, 1)) * G;
  // 8 documents per bin, in whole rounds of the workgroup's four spans (a span
  // never straddles two chunks)
  const int64_t docs = (8 * bins + kFacetChunkStep - 1) / kFacetChunkStep * kFacetChunkStep;
  return std::min<int64_t>(kFacetMaxChunk, std::max<int64_t>(kFacetMinChunk, docs));
}

namespace {

constexpr int kFacetNT = 256;         // threads per workgroup (4 waves)
constexpr int kFacetSpanWords = 8;    // mask words of a wave's span (256 documents)
constexpr int kFacetSpanDocs = kFacetSpanWords * 32;
#ifndef BM25_FACET_FEW_BITS
#define BM25_FACET_FEW_BITS 4
#endif
// a row with at most this many documents in a 64-document step adds them one
// by one (0: always the wave-aggregated add; DESIGN.md §6 has both measured)
constexpr int kFacetFewBits = BM25_FACET_FEW_BITS;
static_assert(kFacetChunkStep == (kFacetNT / 64) * kFacetSpanDocs, "a span per wave");
static_assert(kFacetMinChunk % kFacetChunkStep == 0 && kFacetMaxChunk % kFacetChunkStep == 0 &&
                  kFacetGlobalChunk % kFacetChunkStep == 0,
              "a chunk is whole spans");
static_assert(kFacetMaxRows <= 64, "a lane per row of the block");
static_assert(kFacetMaxChunk <= 65536, "a u32 bin holds a chunk's documents");

// Wave-aggregated add of 1 to bin[g] for the lanes with `on` (g < 2^nbits on
// those): the lanes that share g add once, their number.
template <class BinT>
__device__ __forceinline__ void facet_add(BinT* bin, uint32_t g, bool on, int nbits) {
  uint64_t m = __ballot(on);
  if (m == 0) return;  // (wave-uniform)
  for (int b = 0; b < nbits; ++b) {
    const uint64_t bb = __ballot(((g >> b) & 1u) != 0u);
    m &= ((g >> b) & 1u) ? bb : ~bb;
  }
  const uint32_t below =
      __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
  if (on && below == 0u) atomicAdd(&bin[g], (BinT)__popcll(m));
}

// GLOBAL = false: a workgroup per (chunk, block of R rows), bins in LDS.
// GLOBAL = true: a workgroup per (chunk, row) (R == 1), bins = the row of out.
template <bool GLOBAL>
__global__ __launch_bounds__(kFacetNT) void mask_facets_kernel(
    const uint32_t* __restrict__ masks, int64_t M, int64_t W, int64_t n_docs, uint32_t last_mask,
    const int32_t* __restrict__ groups, int64_t G, int nbits, int R, int64_t chunk_docs,
    int64_t chunks, int64_t blocks, unsigned long long* __restrict__ out) {
  extern __shared__ uint32_t lds_bins[];
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  const int64_t items = chunks * blocks;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    // (row blocks of one chunk are neighbours: they share the chunk's groups in L2)
    const int64_t c = it / blocks, b = it - c * blocks;
    const int64_t m0 = b * R;
    const int rows = M - m0 < (int64_t)R ? (int)(M - m0) : R;
    const int nb = GLOBAL ? 0 : rows * (int)G;
    if (!GLOBAL) {
      for (int i = (int)threadIdx.x; i < nb; i += kFacetNT) lds_bins[i] = 0u;
      __syncthreads();
    }
    const int64_t doc0 = c * chunk_docs;
    const int64_t doc_end = doc0 + chunk_docs < n_docs ? doc0 + chunk_docs : n_docs;
    const uint32_t* row = masks + (m0 + (lane < rows ? lane : rows - 1)) * W;
    for (int64_t s0 = doc0 + (int64_t)wave * kFacetSpanDocs; s0 < doc_end;
         s0 += (int64_t)(kFacetNT / 64) * kFacetSpanDocs) {
      const int64_t w0 = s0 >> 5;
      uint32_t x[kFacetSpanWords];
#pragma unroll
      for (int j = 0; j < kFacetSpanWords; ++j) {
        const int64_t w = w0 + j;
        uint32_t v = lane < rows && w < W ? row[w] : 0u;
        if (w == W - 1) v &= last_mask;
        x[j] = v;
      }
#pragma unroll
      for (int s = 0; s < kFacetSpanWords / 2; ++s) {
        const uint32_t lo = x[2 * s], hi = x[2 * s + 1];
        uint64_t live = __ballot((lo | hi) != 0u);
        if (live == 0) continue;  // (wave-uniform: no row allows a document of the step)
        const int64_t d = s0 + 64 * s + lane;
        const int32_t gv = d < n_docs ? groups[d] : -1;
        const bool in_range = gv >= 0 && (int64_t)gv < G;
        const uint32_t g = in_range ? (uint32_t)gv : 0u;
        while (live) {
          const int r = (int)__builtin_ctzll(live);
          live &= live - 1;
          const uint32_t rlo = (uint32_t)__builtin_amdgcn_readlane((int)lo, r);
          const uint32_t rhi = (uint32_t)__builtin_amdgcn_readlane((int)hi, r);
          uint64_t few = ((uint64_t)rhi << 32) | rlo;  // (wave-uniform)
          if (__popcll(few) <= kFacetFewBits) {
            // a sparse row: its few documents one by one, the group read from
            // the lane that holds it, one lane adds — no ballot
            while (few) {
              const int l = (int)__builtin_ctzll(few);
              few &= few - 1;
              const int32_t gl = __builtin_amdgcn_readlane(gv, l);
              if (gl >= 0 && (int64_t)gl < G && lane == 0) {
                if (GLOBAL)
                  atomicAdd(out + (m0 + r) * G + gl, 1ull);
                else
                  atomicAdd(lds_bins + (int64_t)r * G + gl, 1u);
              }
            }
            continue;
          }
          const bool bit = (((lane < 32 ? rlo : rhi) >> (lane & 31)) & 1u) != 0u;
          if (GLOBAL)
            facet_add(out + (m0 + r) * G, g, bit && in_range, nbits);
          else
            facet_add(lds_bins + (int64_t)r * G, g, bit && in_range, nbits);
        }
      }
    }
    if (!GLOBAL) {
      __syncthreads();
      unsigned long long* dst = out + m0 * G;  // rows m0 .. m0 + rows - 1 are contiguous
      for (int i = (int)threadIdx.x; i < nb; i += kFacetNT) {
        const uint32_t v = lds_bins[i];
        if (v) atomicAdd(dst + i, (unsigned long long)v);
      }
      __syncthreads();  // (the bins are cleared for the next item)
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

}  // namespace

hipError_t launch_mask_facets(const DevIndex& ix, const uint32_t* d_masks, int64_t M,
                              const int32_t* d_groups, int64_t G, int64_t* d_counts,
                              hipStream_t st) {
  if (M <= 0 || G <= 0) return hipSuccess;
  if (G > 0x7FFFFFFFll) return hipErrorInvalidValue;
  // every entry is written: the kernels add onto zeros
  const hipError_t e = hipMemsetAsync(d_counts, 0, sizeof(int64_t) * (size_t)M * (size_t)G, st);
  if (e != hipSuccess) return e;
  const int64_t n_docs = ix.n_docs, W = (n_docs + 31) >> 5;
  if (W == 0) return hipSuccess;
  const uint32_t tail = (uint32_t)(n_docs & 31);
  const uint32_t last_mask = tail ? (1u << tail) - 1u : 0xFFFFFFFFu;
  int nbits = 0;  // bits of a group id < G
  while (nbits < 31 && ((int64_t)1 << nbits) < G) ++nbits;
  const bool global = G > kFacetBins;
  const int64_t R = global ? 1 : facet_rows(G);
  const int64_t chunk_docs = facet_chunk_docs(G, M);
  const int64_t chunks = (n_docs + chunk_docs - 1) / chunk_docs;
  const int64_t blocks = (M + R - 1) / R;
  // items flattened into a grid-stride loop (M may pass 65535): 8 workgroups
  // per CU hold the chip, more items take more steps
  const unsigned grid = (unsigned)std::max<int64_t>(
      1, std::min<int64_t>(chunks * blocks, (int64_t)device_cus(ix.device) * 8));
  auto* counts = reinterpret_cast<unsigned long long*>(d_counts);
  if (global) {
    hipLaunchKernelGGL(mask_facets_kernel<true>, dim3(grid), dim3(kFacetNT), 0, st, d_masks, M, W,
                       n_docs, last_mask, d_groups, G, nbits, 1, chunk_docs, chunks, blocks, counts);
  } else {
    const size_t lds = sizeof(uint32_t) * (size_t)(std::min<int64_t>(R, M) * G);
    hipLaunchKernelGGL(mask_facets_kernel<false>, dim3(grid), dim3(kFacetNT), lds, st, d_masks, M,
                       W, n_docs, last_mask, d_groups, G, nbits, (int)R, chunk_docs, chunks,
                       blocks, counts);
  }
  return hipGetLastError();
}

}  // namespace bm25mi
