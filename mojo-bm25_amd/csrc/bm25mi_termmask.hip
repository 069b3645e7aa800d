// bm25mi_termmask.hip — boolean term filters as allow-masks (bm25_term_masks /
// bm25_term_masks_device, include/bm25mi.h), built from the index's own
// postings in the layout the filtered search reads (bm25mi_filter.hip).
//
//   allowed(m, d) = d < n_docs and base(m, d)
//                   and every id >= 0 of must[m] has d
//                   and (any[m] holds no id >= 0 or some id >= 0 of any[m] has d)
//                   and no id >= 0 of must_not[m] has d
//
// has(t, d): the CSC index stores a posting of (term t, document d), whatever
// its value; an id >= n_terms is a term that no document has.
//
// What the kernel relies on (bm25mi_internal.h): the postings of
// term t in tile j are one segment [indptr[t] + r(t, j), indptr[t] + r(t, j + 1))
// of ldoc by either segment table, ldoc >> 2 is the document's slot in the tile
// and ascends inside a segment, and a tile is 2^(tile_shift - 5) mask words.
//
// One wavefront owns one (mask, tile) item, its lanes the tile's mask words in
// registers (word w of the tile on lane w & 63).  The segments of a clause's
// terms are looked up a lane per term (64 a step, so the dependent loads of
// the lookups overlap) and handed to the wave by shuffles.  A term's segment is streamed
// with 16-byte loads (8 u16 per lane, aligned; val is never read) and its bits
// are set in a wave-private LDS bitmap with LDS atomic OR — a lane first
// gathers the bits of its 8 ascending postings that fall in one word.  must
// terms are ANDed into the accumulator one bitmap at a time; the any terms
// share one bitmap and so do the must_not terms (OR needs no clear between
// terms).  The words are written once with plain stores, one contiguous row
// segment per wave: no global atomics, no workspace, nothing depends on
// scheduling.
//
// Before any posting is read the item's base words and the segment bounds of
// all its must terms are looked up: where the base words are all zero or a
// must term has no posting in the tile the wave stores zeros and moves on (a
// wave-uniform branch) — the tiles the filtered search's census then skips.
//
// Minimum-should-match (the MM instantiations, launched only where a min_match
// pointer is given): a row that needs two or more of its any terms gives each
// of them a bitmap pass of its own, as a must term's, and every lane adds the
// bitmap word into a bit-sliced counter of its mask words held in registers
// (tests/min_match_model.py restates the arithmetic).  Before that the wave
// counts the any terms with a segment in the tile: fewer than the row needs
// and it stores zeros without reading a posting.  Rows that need one term
// take the shared bitmap above through a wave-uniform branch per item.
//
// bm25_mask_count: a popcount reduction of [M, W] mask words, at the end of
// this file.
#include "bm25mi_internal.h"

#include <algorithm>
#include <atomic>

namespace bm25mi {

namespace {

constexpr int kMaskNT = 256;     // threads per workgroup (4 waves)
constexpr int kMaskMaxWords = 128;  // mask words of a tile (tile_shift <= 12)

struct MaskArgs {
  const int64_t* indptr;
  const uint32_t* rel;
  const int64_t* tl_ptr;
  const uint16_t* tl_tile;
  const uint32_t* tl_start;
  const uint16_t* ldoc;
  int64_t V, ntiles, n_docs, W;
  int32_t sparse, tile_shift;
};

// The postings [*s, *e) of (term, tile), 0 <= term < V (a term per lane);
// false where the tile holds none.
__device__ __forceinline__ bool term_segment(const MaskArgs& a, int64_t term, int64_t tile,
                                             int64_t* s, int64_t* e) {
  const int64_t p0 = a.indptr[term];
  uint32_t r0, r1;
  if (!a.sparse) {  // two adjacent entries of the term's row
    const uint32_t* r = a.rel + term * (a.ntiles + 1) + tile;
    r0 = r[0];
    r1 = r[1];
  } else {  // binary search of the term's non-empty tiles (as bm25mi_lookup.hip)
    const int64_t b = a.tl_ptr[term], end = a.tl_ptr[term + 1];
    int64_t lo = b, hi = end;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)a.tl_tile[mid] < tile) lo = mid + 1;
      else hi = mid;
    }
    if (lo >= end || (int64_t)a.tl_tile[lo] != tile) return false;
    r0 = a.tl_start[lo];
    r1 = lo + 1 < end ? a.tl_start[lo + 1] : (uint32_t)(a.indptr[term + 1] - p0);
  }
  *s = p0 + (int64_t)r0;
  *e = p0 + (int64_t)r1;
  return r1 > r0;
}

// ORs the slots of the postings [s, e) into the wave's bitmap.  Aligned
// 16-byte loads over [s & ~7, e): the elements outside [s, e) are masked (the
// posting arrays carry kPostingPad elements past nnz, and s & ~7 >= 0).
__device__ __forceinline__ void or_segment(const uint16_t* __restrict__ ldoc, int64_t s, int64_t e,
                                           uint32_t* bm, int lane) {
  for (int64_t v = (s & ~(int64_t)7) + (int64_t)lane * 8; v < e; v += 64 * 8) {
    const uint4 raw = *reinterpret_cast<const uint4*>(ldoc + v);
    const uint32_t x[4] = {raw.x, raw.y, raw.z, raw.w};
    uint32_t cur_w = 0, cur_bits = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int64_t p = v + j;
      if (p < s || p >= e) continue;
      const uint32_t slot = ((x[j >> 1] >> ((j & 1) * 16)) & 0xFFFFu) >> 2;
      const uint32_t w = slot >> 5;
      if (w != cur_w && cur_bits) {  // slots ascend: a word is left for good
        atomicOr(&bm[cur_w], cur_bits);
        cur_bits = 0;
      }
      cur_w = w;
      cur_bits |= 1u << (slot & 31u);
    }
    if (cur_bits) atomicOr(&bm[cur_w], cur_bits);
  }
}

// Planes of the counting any clause's bit-sliced counter (B <= 65535).
constexpr int kCountPlanes = 16;

// WPL: mask words of a tile per lane (1: tiles of up to 2048 documents, 2: 4096).
// MM: the any clause of row m needs min_match[m] of its terms (the
// min_match calls); false: the kernel of bm25_term_masks, which never reads
// min_match and compiles none of the counting code.
template <int WPL, bool MM>
__global__ __launch_bounds__(kMaskNT) void term_masks_kernel(
    MaskArgs a, const int32_t* __restrict__ must, int64_t A, const int32_t* __restrict__ any,
    int64_t B, const int32_t* __restrict__ must_not, int64_t N, int64_t M,
    const uint32_t* __restrict__ base, int64_t Mb, uint32_t* __restrict__ out,
    const int32_t* __restrict__ min_match) {
  __shared__ uint32_t bm_all[(kMaskNT / 64) * kMaskMaxWords];
  const int lane = (int)(threadIdx.x & 63u);
  const int wave = (int)(threadIdx.x >> 6);
  uint32_t* bm = bm_all + wave * kMaskMaxWords;
  const int words = 1 << (a.tile_shift - 5);  // <= 64 * WPL
  const int64_t items = M * a.ntiles;
  const int64_t stride = (int64_t)gridDim.x * (kMaskNT / 64);
  const uint32_t tail = (uint32_t)(a.n_docs & 31);
  for (int64_t it = (int64_t)blockIdx.x * (kMaskNT / 64) + wave; it < items; it += stride) {
    const int64_t m = it / a.ntiles, tile = it - m * a.ntiles;
    const int64_t w0 = tile * words;  // the tile's first word of the row
    uint32_t acc[WPL];
    bool live = false;
#pragma unroll
    for (int i = 0; i < WPL; ++i) {
      const int64_t gw = w0 + lane + 64 * i;
      uint32_t x = 0u;
      if (lane + 64 * i < words && gw < a.W) {
        x = base ? base[(Mb == 1 ? 0 : m) * a.W + gw] : 0xFFFFFFFFu;
        if (tail && gw == a.W - 1) x &= (1u << tail) - 1u;  // bits at or past n_docs
      }
      acc[i] = x;
      live = live || x != 0u;
    }
    bool alive = __ballot(live) != 0ull;
    // the bounds of every must term before any posting is read
    const int32_t* mrow = must + m * A;
    // (a lane per term, 64 terms a step: the lookups' dependent loads run side
    // by side instead of term after term)
    for (int64_t i0 = 0; alive && i0 < A; i0 += 64) {
      const int32_t t = i0 + lane < A ? mrow[i0 + lane] : -1;
      int64_t s, e;
      const bool empty = t >= 0 && ((int64_t)t >= a.V || !term_segment(a, t, tile, &s, &e));
      if (__ballot(empty) != 0ull) alive = false;
    }
    for (int64_t i0 = 0; alive && i0 < A; i0 += 64) {
      const int32_t t = i0 + lane < A ? mrow[i0 + lane] : -1;
      long long s = 0, e = 0;
      if (t >= 0) {  // (t < V and the segment is not empty: the pass above)
        int64_t s1 = 0, e1 = 0;
        term_segment(a, t, tile, &s1, &e1);
        s = s1;
        e = e1;
      }
      unsigned long long todo = __ballot(t >= 0);
      while (alive && todo != 0ull) {  // the terms one by one (wave-uniform)
        const int i = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        const int64_t si = __shfl(s, i), ei = __shfl(e, i);
#pragma unroll
        for (int k = 0; k < WPL; ++k)
          if (lane + 64 * k < words) bm[lane + 64 * k] = 0u;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        or_segment(a.ldoc, si, ei, bm, lane);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        live = false;
#pragma unroll
        for (int k = 0; k < WPL; ++k) {
          if (lane + 64 * k < words) acc[k] &= bm[lane + 64 * k];
          live = live || acc[k] != 0u;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        alive = __ballot(live) != 0ull;
      }
    }
    // any, then must_not: one bitmap per clause
    for (int clause = 0; clause < 2; ++clause) {
      const int64_t width = clause == 0 ? B : N;
      const int32_t* row = (clause == 0 ? any : must_not) + m * width;
      if constexpr (MM) {
        // need <= 0: the clause is optional; 1: the shared bitmap below; >= 2:
        // count the terms per document (a wave-uniform branch per item)
        const int32_t need = clause == 0 ? min_match[m] : 1;
        if (need <= 0) continue;
        if (need >= 2) {
          // a lane per term: the slots that hold an id, and those whose term
          // has postings in the tile — fewer than need: no posting is read
          int64_t n_any = 0, n_seg = 0;
          for (int64_t i0 = 0; alive && i0 < width; i0 += 64) {
            const int32_t t = i0 + lane < width ? row[i0 + lane] : -1;
            int64_t s, e;
            const bool found = t >= 0 && (int64_t)t < a.V && term_segment(a, t, tile, &s, &e);
            n_any += __popcll(__ballot(t >= 0));
            n_seg += __popcll(__ballot(found));
          }
          if (!alive || n_any == 0) continue;  // (no id: the clause is absent)
          if (n_seg < (int64_t)need) {
            alive = false;
            continue;
          }
          // a bit-sliced counter per mask word, P = bit_length(need) planes
          // (need <= n_seg <= B <= 65535) that start at 2^P - need: the need-th
          // term of a document carries out of the top plane into `reached`
          const int P = 32 - __builtin_clz((uint32_t)need);
          const uint32_t init = (1u << P) - (uint32_t)need;
          uint32_t cnt[WPL][kCountPlanes], reached[WPL];
#pragma unroll
          for (int k = 0; k < WPL; ++k) {
            reached[k] = 0u;
#pragma unroll
            for (int p = 0; p < kCountPlanes; ++p) cnt[k][p] = (init >> p) & 1u ? 0xFFFFFFFFu : 0u;
          }
          for (int64_t i0 = 0; i0 < width; i0 += 64) {
            const int32_t t = i0 + lane < width ? row[i0 + lane] : -1;
            long long s = 0, e = 0;
            bool found = false;
            if (t >= 0 && (int64_t)t < a.V) {
              int64_t s1 = 0, e1 = 0;
              found = term_segment(a, t, tile, &s1, &e1);
              s = s1;
              e = e1;
            }
            unsigned long long todo = __ballot(found);
            while (todo != 0ull) {  // a bitmap pass per term, as a must term's
              const int i = __builtin_ctzll(todo);
              todo &= todo - 1ull;
              const int64_t si = __shfl(s, i), ei = __shfl(e, i);
#pragma unroll
              for (int k = 0; k < WPL; ++k)
                if (lane + 64 * k < words) bm[lane + 64 * k] = 0u;
              __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
              or_segment(a.ldoc, si, ei, bm, lane);
              __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
              for (int k = 0; k < WPL; ++k) {
                uint32_t carry = lane + 64 * k < words ? bm[lane + 64 * k] : 0u;
#pragma unroll
                for (int p = 0; p < kCountPlanes; ++p) {
                  if (p < P) {  // (wave-uniform)
                    const uint32_t c = cnt[k][p] & carry;
                    cnt[k][p] ^= carry;
                    carry = c;
                  }
                }
                reached[k] |= carry;
              }
              __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            }
          }
          live = false;
#pragma unroll
          for (int k = 0; k < WPL; ++k) {
            acc[k] &= reached[k];
            live = live || acc[k] != 0u;
          }
          alive = __ballot(live) != 0ull;
          continue;
        }
      }
      bool active = false;  // the clause holds an id >= 0
      for (int64_t i0 = 0; alive && i0 < width; i0 += 64) {
        const int32_t t = i0 + lane < width ? row[i0 + lane] : -1;
        long long s = 0, e = 0;
        bool found = false;
        if (t >= 0 && (int64_t)t < a.V) {
          int64_t s1 = 0, e1 = 0;
          found = term_segment(a, t, tile, &s1, &e1);
          s = s1;
          e = e1;
        }
        if (__ballot(t >= 0) == 0ull) continue;
        if (!active) {
          active = true;
#pragma unroll
          for (int k = 0; k < WPL; ++k)
            if (lane + 64 * k < words) bm[lane + 64 * k] = 0u;
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
        unsigned long long todo = __ballot(found);
        while (todo != 0ull) {
          const int i = __builtin_ctzll(todo);
          todo &= todo - 1ull;
          or_segment(a.ldoc, __shfl(s, i), __shfl(e, i), bm, lane);
        }
      }
      if (active) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        live = false;
#pragma unroll
        for (int k = 0; k < WPL; ++k) {
          if (lane + 64 * k < words) {
            const uint32_t b = bm[lane + 64 * k];
            acc[k] &= clause == 0 ? b : ~b;
          }
          live = live || acc[k] != 0u;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        alive = __ballot(live) != 0ull;
      }
    }
#pragma unroll
    for (int k = 0; k < WPL; ++k) {
      const int64_t gw = w0 + lane + 64 * k;
      if (lane + 64 * k < words && gw < a.W) out[m * a.W + gw] = alive ? acc[k] : 0u;
    }
  }
}

// ---- bm25_mask_count: the set bits of every mask row among bits 0 .. n_docs - 1.
//
// A row is read in aligned 16-byte groups: with a = the row's first word's
// offset inside its 16 bytes (m * W words is no multiple of 4 when W is odd,
// and the caller's pointer need not be one), group g holds the words
// 4 g - a .. 4 g - a + 3 of the row.  A group that lies inside the row is one
// uint4 load; the row's first and last group load their words one by one, so
// no word outside [0, W) of a row is read.  last_mask clears the bits at or
// past n_docs of word W - 1.
constexpr int kCountNT = 256;       // threads per workgroup
constexpr int kCountGroups = 4;     // groups per thread of a workgroup's chunk
constexpr int64_t kCountWaveW = 1024;  // rows of up to this many words: a wave per row

__device__ __forceinline__ int64_t row_misalign(const uint32_t* row) {
  return (int64_t)((reinterpret_cast<uintptr_t>(row) >> 2) & 3u);
}

__device__ __forceinline__ uint32_t group_bits(const uint32_t* __restrict__ row, int64_t W,
                                               int64_t a, int64_t g, uint32_t last_mask) {
  const int64_t i0 = 4 * g - a;
  uint32_t x[4];
  if (i0 >= 0 && i0 + 4 <= W) {
    const uint4 v = *reinterpret_cast<const uint4*>(row + i0);
    x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = i0 + j >= 0 && i0 + j < W ? row[i0 + j] : 0u;
  }
  uint32_t n = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) n += __popc(i0 + j == W - 1 ? x[j] & last_mask : x[j]);
  return n;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// A wavefront per row (W <= kCountWaveW): plain stores.
__global__ __launch_bounds__(kCountNT) void mask_count_rows_kernel(
    const uint32_t* __restrict__ masks, int64_t M, int64_t W, uint32_t last_mask,
    int64_t* __restrict__ out) {
  const int lane = (int)(threadIdx.x & 63u);
  const int64_t stride = (int64_t)gridDim.x * (kCountNT / 64);
  for (int64_t m = (int64_t)blockIdx.x * (kCountNT / 64) + (threadIdx.x >> 6); m < M; m += stride) {
    const uint32_t* row = masks + m * W;
    const int64_t a = row_misalign(row), groups = (a + W + 3) >> 2;
    uint32_t n = 0;
    for (int64_t g = lane; g < groups; g += 64) n += group_bits(row, W, a, g, last_mask);
    n = wave_sum(n);
    if (lane == 0) out[m] = (int64_t)n;
  }
}

// A workgroup per (row, chunk of kCountNT * kCountGroups groups): reduced
// across each wave, then once per workgroup; chunks == 1: a plain store,
// otherwise an integer atomic onto the count the launch zeroed on the stream.
__global__ __launch_bounds__(kCountNT) void mask_count_chunks_kernel(
    const uint32_t* __restrict__ masks, int64_t M, int64_t W, int64_t chunks, uint32_t last_mask,
    int64_t* __restrict__ out) {
  __shared__ uint32_t part[kCountNT / 64];
  const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
  const int64_t items = M * chunks;
  for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
    const int64_t m = it / chunks, c = it - m * chunks;
    const uint32_t* row = masks + m * W;
    const int64_t a = row_misalign(row), groups = (a + W + 3) >> 2;
    uint32_t n = 0;
#pragma unroll
    for (int j = 0; j < kCountGroups; ++j) {
      const int64_t g = (c * kCountGroups + j) * kCountNT + (int64_t)threadIdx.x;
      if (g < groups) n += group_bits(row, W, a, g, last_mask);
    }
    n = wave_sum(n);
    if (lane == 0) part[wave] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t s = 0;
#pragma unroll
      for (int w = 0; w < kCountNT / 64; ++w) s += part[w];
      if (chunks == 1) out[m] = (int64_t)s;
      else if (s) atomicAdd(reinterpret_cast<unsigned long long*>(out + m), (unsigned long long)s);
    }
    __syncthreads();  // (part is reused by the next item)
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

hipError_t launch_term_masks(const DevIndex& ix, const int32_t* d_must, int64_t A,
                             const int32_t* d_any, int64_t B, const int32_t* d_must_not, int64_t N,
                             int64_t M, const uint32_t* d_base, int64_t Mb, uint32_t* d_out,
                             hipStream_t st, const int32_t* d_min_match) {
  const int64_t W = (ix.n_docs + 31) >> 5;
  if (M <= 0 || W == 0) return hipSuccess;
  if (ix.tile_shift < 5 || ix.tile_shift > 12) return hipErrorInvalidValue;  // (kMaskMaxWords)
  if (A < 0 || B < 0 || N < 0 || (Mb != 0 && Mb != 1 && Mb != M)) return hipErrorInvalidValue;
  if (d_min_match && B > 65535) return hipErrorInvalidValue;  // (kCountPlanes)
  const int cus = device_cus(ix.device);
  const MaskArgs a{ix.indptr, ix.rel, ix.tl_ptr, ix.tl_tile, ix.tl_start, ix.ldoc,
                   ix.n_terms, ix.ntiles, ix.n_docs, W, ix.sparse ? 1 : 0, ix.tile_shift};
  // items flattened into a grid-stride loop (M may pass 65535): 8 workgroups
  // (32 waves) per CU hold the chip, more items take more steps
  const int64_t items = M * ix.ntiles;
  const int64_t per_block = kMaskNT / 64;
  const unsigned grid = (unsigned)std::max<int64_t>(
      1, std::min<int64_t>((items + per_block - 1) / per_block, (int64_t)cus * 8));
  const uint32_t* base = Mb ? d_base : nullptr;
  // the instantiation by "is a min_match pointer given": the calls without
  // one launch the kernel they always launched (the counting instantiations
  // hold 7 or 5 waves per SIMD, not 8; a grid cut to what the chip holds of
  // them measured 6 to 7 % slower than this one, whose last workgroups start as
  // the first ones finish)
  auto* kernel = ix.tile_shift <= 11
                     ? (d_min_match ? term_masks_kernel<1, true> : term_masks_kernel<1, false>)
                     : (d_min_match ? term_masks_kernel<2, true> : term_masks_kernel<2, false>);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(kMaskNT), 0, st, a, d_must, A, d_any, B, d_must_not,
                     N, M, base, Mb, d_out, d_min_match);
  return hipGetLastError();
}

hipError_t launch_mask_count(const DevIndex& ix, const uint32_t* d_masks, int64_t M,
                             int64_t* d_counts, hipStream_t st) {
  if (M <= 0) return hipSuccess;
  const int64_t W = (ix.n_docs + 31) >> 5;
  if (W == 0) return hipMemsetAsync(d_counts, 0, sizeof(int64_t) * (size_t)M, st);
  const uint32_t tail = (uint32_t)(ix.n_docs & 31);
  const uint32_t last_mask = tail ? (1u << tail) - 1u : 0xFFFFFFFFu;
  const int64_t cus = device_cus(ix.device);
  if (W <= kCountWaveW) {
    const int64_t per_block = kCountNT / 64;
    const unsigned grid =
        (unsigned)std::max<int64_t>(1, std::min<int64_t>((M + per_block - 1) / per_block, cus * 8));
    hipLaunchKernelGGL(mask_count_rows_kernel, dim3(grid), dim3(kCountNT), 0, st, d_masks, M, W,
                       last_mask, d_counts);
    return hipGetLastError();
  }
  // (a row's groups: at most 3 words of misalignment before its W words)
  const int64_t per_chunk = (int64_t)kCountNT * kCountGroups;
  const int64_t chunks = (((W + 3 + 3) >> 2) + per_chunk - 1) / per_chunk;
  if (chunks > 1) {
    const hipError_t e = hipMemsetAsync(d_counts, 0, sizeof(int64_t) * (size_t)M, st);
    if (e != hipSuccess) return e;
  }
  const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(M * chunks, cus * 8));
  hipLaunchKernelGGL(mask_count_chunks_kernel, dim3(grid), dim3(kCountNT), 0, st, d_masks, M, W,
                     chunks, last_mask, d_counts);
  return hipGetLastError();
}

}  // namespace bm25mi

