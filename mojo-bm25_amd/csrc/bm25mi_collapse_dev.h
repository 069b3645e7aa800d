// bm25mi_collapse_dev.h — the device pieces that the walks of field collapsing
// share (bm25mi_collapse.hip: a search's pages; bm25mi_merge_collapse.hip: the
// merged order of doc shards' lists): the per-row group table in LDS and the
// step that decides one 64-entry chunk of a walk.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace bm25mi {

// The group table: `slots` (a power of two, >= 2 * the keys it may hold) int32
// keys, -1 = empty, then `slots` int32 counts.  Linear probing from a
// multiplicative hash.
__device__ inline uint32_t tab_home(int32_t g, int lg) {
  return ((uint32_t)g * 0x9E3779B1u) >> (32 - lg);
}

__device__ inline void tab_clear(int32_t* tab, int slots, int t, int nt) {
  for (int i = t; i < slots; i += nt) {
    tab[i] = -1;
    tab[slots + i] = 0;
  }
}

// Adds one to g's count (g >= 0), inserting it when new.
__device__ inline void tab_add(int32_t* tab, int slots, int lg, int32_t g) {
  uint32_t s = tab_home(g, lg);
  for (;;) {
    const int32_t was = atomicCAS(&tab[s], -1, g);
    if (was == -1 || was == g) break;
    s = (s + 1u) & (uint32_t)(slots - 1);
  }
  atomicAdd(&tab[slots + s], 1);
}

// g's count (0 when absent; g >= 0).
__device__ inline int32_t tab_count(const int32_t* tab, int slots, int lg, int32_t g) {
  uint32_t s = tab_home(g, lg);
  for (;;) {
    const int32_t key = tab[s];
    if (key == g) return tab[slots + s];
    if (key == -1) return 0;
    s = (s + 1u) & (uint32_t)(slots - 1);
  }
}

// One chunk of a row's walk: 64 entries in rank order, one per lane of the
// row's wave (real: the lane holds an entry; g: its group, < 0 = none), against
// the row's table and its cnt hits kept so far.
struct ChunkStep {
  bool keep;     // the walk keeps the lane's entry (were the row not to fill)
  bool take;     // ... and it is among the row's first k: slot pos
  int32_t pos;
  int32_t total; // cnt + every kept entry of the chunk (may pass k)
  uint64_t km;   // the keep lanes
  uint64_t tm;   // the take lanes
};

__device__ inline ChunkStep chunk_step(const int32_t* tab, int slots, int lg, bool real, int32_t g,
                                       int32_t per_group, int32_t cnt, int32_t k, int lane) {
  const uint64_t below = (1ull << lane) - 1ull;
  // the lower lanes of the chunk in the same group: the first of a group's
  // lanes are the ones kept, so a lane is kept iff its rank among them, past
  // the group's count so far, is below the quota
  int32_t same = 0;
  uint64_t todo = __builtin_amdgcn_ballot_w64(real && g >= 0);
  while (todo) {
    const int l = (int)__builtin_ctzll(todo);
    const int32_t gl = __shfl(g, l);
    const uint64_t m = __builtin_amdgcn_ballot_w64(real && g == gl);
    if (real && g == gl) same = (int32_t)__popcll(m & below);
    todo &= ~m;
  }
  ChunkStep s;
  s.keep = real && (g < 0 || (int64_t)tab_count(tab, slots, lg, g) + same < (int64_t)per_group);
  s.km = __builtin_amdgcn_ballot_w64(s.keep);
  s.pos = cnt + (int32_t)__popcll(s.km & below);
  s.take = s.keep && s.pos < k;
  s.tm = __builtin_amdgcn_ballot_w64(s.take);
  s.total = cnt + (int32_t)__popcll(s.km);
  return s;
}

// The table's update after a chunk_step: the taken entries' groups counted,
// behind a barrier (the step's lookups come first) and before one (the next
// chunk's lookups).  For workgroups of one wave: every lane calls it.
__device__ inline void chunk_commit(int32_t* tab, int slots, int lg, bool take, int32_t g) {
  __syncthreads();
  if (take && g >= 0) tab_add(tab, slots, lg, g);
  __syncthreads();
}

}  // namespace bm25mi
