// bm25mi_sort_key_dev.h — the order key of a sort column, K(v, kind,
// descending) of include/bm25mi.h ("Sort-by-field search over doc shards"):
// one definition for the rank build (bm25mi_sorted.hip) and for the keys,
// cursors and merge of doc shards (bm25mi_sorted_shards.hip).  The order of a
// column is (K ascending, doc id ascending).
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#include <type_traits>

namespace bm25mi {

__device__ __forceinline__ uint64_t sort_key(int32_t v, bool desc) {
  const uint32_t u = (uint32_t)v ^ 0x80000000u;
  return desc ? (uint32_t)~u : u;
}
__device__ __forceinline__ uint64_t sort_key(int64_t v, bool desc) {
  const uint64_t u = (uint64_t)v ^ 0x8000000000000000ull;
  return desc ? ~u : u;
}
__device__ __forceinline__ uint64_t sort_key(float v, bool desc) {
  if (v != v) return 1ull << 32;  // NaN: no value, after every number in both directions
  uint32_t u = __float_as_uint(v);
  if ((u & 0x7FFFFFFFu) == 0u) u = 0u;  // -0.0f orders as +0.0f
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return desc ? (uint32_t)~u : u;
}
// The key bits in use: what the rank build's radix sort runs over.
template <class T>
constexpr int sort_key_bits() {
  return sizeof(T) == 8 ? 64 : (std::is_floating_point<T>::value ? 33 : 32);
}

}  // namespace bm25mi
