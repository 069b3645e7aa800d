// sorted_check — the host-side arithmetic of the sorted search under
// AddressSanitizer and UBSan, without a device: the validation of the order
// arrays and cursors (check_sort_order, check_after_ranks, bm25mi_host.h) on
// exactly sized heap arrays, and the scratch-size and list-capacity
// arithmetic (sorted_scratch_bytes, sorted_list_cap, bm25mi_internal.h) at
// their limits.  Built and run by tests/test_search_sorted_host.py with the
// host compiler alone (no HIP call is made, none is linked); fail() is this
// program's own.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

#include "../../mojo-bm25_amd/csrc/bm25mi_host.h"

static std::string g_err;
int bm25mi::fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define EXPECT(cond)                                                       \
  do {                                                                     \
    if (!(cond)) {                                                         \
      fprintf(stderr, "sorted_check.cpp:%d: %s (last error: %s)\n", __LINE__, #cond, g_err.c_str()); \
      return 1;                                                            \
    }                                                                      \
  } while (0)

int main() {
  using namespace bm25mi;
  for (int64_t n : {0ll, 1ll, 2ll, 33ll, 4097ll}) {
    // a permutation and its inverse in arrays of exactly n entries
    std::vector<int32_t> perm((size_t)n), ranks((size_t)n);
    std::iota(perm.begin(), perm.end(), 0);
    for (int64_t i = n - 1; i > 0; --i) std::swap(perm[(size_t)i], perm[(size_t)((i * 7919) % (i + 1))]);
    for (int64_t r = 0; r < n; ++r) ranks[(size_t)perm[(size_t)r]] = (int32_t)r;
    EXPECT(check_sort_order(ranks.data(), perm.data(), n) == BM25_OK);
    if (n < 2) continue;
    // an entry at and past the ends: no perm entry is read for it
    for (int32_t bad : {(int32_t)n, (int32_t)-1, INT32_MAX, INT32_MIN}) {
      std::vector<int32_t> r2 = ranks;
      r2[(size_t)(n / 2)] = bad;
      EXPECT(check_sort_order(r2.data(), perm.data(), n) == BM25_EINVAL);
      char want[64];
      snprintf(want, sizeof want, "ranks[%lld] = %d is outside", (long long)(n / 2), (int)bad);
      EXPECT(g_err.find(want) != std::string::npos);
    }
    // two documents at one rank: the first one whose perm entry names the other
    std::vector<int32_t> r2 = ranks;
    r2[0] = ranks[(size_t)(n - 1)];
    EXPECT(check_sort_order(r2.data(), perm.data(), n) == BM25_EINVAL);
    EXPECT(g_err.find("ranks[0] = ") == 0 && g_err.find("not inverse permutations") != std::string::npos);
    // a perm that is no permutation
    std::vector<int32_t> p2 = perm;
    p2[(size_t)ranks[1]] = INT32_MAX;
    EXPECT(check_sort_order(ranks.data(), p2.data(), n) == BM25_EINVAL);
    EXPECT(g_err.find("ranks[1] = ") == 0);
  }
  // cursors
  EXPECT(check_after_ranks(nullptr, 1000) == BM25_OK);
  std::vector<int32_t> after = {BM25_AFTER_NONE, -1, 0, INT32_MAX};
  EXPECT(check_after_ranks(after.data(), (int64_t)after.size()) == BM25_OK);
  after.push_back(-3);
  EXPECT(check_after_ranks(after.data(), (int64_t)after.size()) == BM25_EINVAL);
  EXPECT(g_err == "after_ranks[4] = -3 is below BM25_AFTER_NONE (-2)");
  after.back() = INT32_MIN;
  EXPECT(check_after_ranks(after.data(), (int64_t)after.size()) == BM25_EINVAL);
  // the scratch: 4 M (4 + 1 + kSortedBins + min(k + kSortedWmax, n_docs)), in
  // int64 at the largest shapes (no intermediate overflows: UBSan watches)
  EXPECT(sorted_list_cap(40, 5) == 40 && sorted_list_cap(5000, 4096) == 5000);
  EXPECT(sorted_list_cap(10000000, 100) == 100 + kSortedWmax);
  EXPECT(sorted_list_cap(INT32_MAX, kMaxK) == kMaxK + kSortedWmax);
  EXPECT(sorted_scratch_bytes(40, 65537, 5) == 4ll * 65537 * (4 + 1 + 256 + 40));
  EXPECT(sorted_scratch_bytes(10000000, 1024, 100) == 4ll * 1024 * (4 + 1 + 256 + 2148));
  EXPECT(sorted_scratch_bytes(INT32_MAX, 1ll << 32, kMaxK) ==
         4ll * (1ll << 32) * (4 + 1 + 256 + 4096 + 2048));
  EXPECT(sorted_scratch_bytes(1, 0, 0) == 0 && sorted_scratch_bytes(1, 1, 1) == 4 * (261 + 1));
  EXPECT(kMaxK + kSortedWmax <= kSortedSortP);
  // the option row
  bool found = false;
  for (const OptDesc& d : kOptsMore)
    if (!strcmp(d.name, "sorted_bins"))
      found = d.lo == 0 && d.hi == kSortedBins && !strcmp(d.env, "BM25_SORTED_BINS");
  EXPECT(found);
  printf("sorted_check ok\n");
  return 0;
}
