// stats_sum_check — drives the float32 sum of the field statistics
// (mojo-bm25_amd/csrc/bm25mi_stats_sum.h: stats_addend, stats_sum_round) on the
// host, under AddressSanitizer and UBSan, with no device and no HIP call
// (tests/test_mask_stats_host.py builds it through
// bm25mi.build.build_host_program and compares its output with the Python
// model and math.fsum).
//
//   stats_sum_check FILE
// FILE: cases of (uint32 n, n float32 bit patterns), little endian.  Per case
// one line: the float64 sum's bits as 16 hex digits, then bins 0, 15 and 31
// as decimal integers.  NaN values are skipped, +-inf counted, as the
// accumulate pass does.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../mojo-bm25_amd/csrc/bm25mi_stats_sum.h"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s FILE\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  uint32_t n = 0;
  while (std::fread(&n, 4, 1, f) == 1) {
    std::vector<uint32_t> v(n);
    if (n && std::fread(v.data(), 4, n, f) != n) {
      std::fprintf(stderr, "short case\n");
      return 2;
    }
    int64_t bins[bm25mi::kStatsSumBins] = {};
    uint64_t pinf = 0, ninf = 0;
    for (uint32_t u : v) {
      if ((u & 0x7F800000u) == 0x7F800000u) {
        if (u & 0x7FFFFFu) continue;  // NaN: no value
        ++((u >> 31) ? ninf : pinf);
        continue;
      }
      int bin = 0;
      int64_t add = 0;
      bm25mi::stats_addend(u, &bin, &add);
      bins[bin] += add;
    }
    const double s = bm25mi::stats_sum_round(bins, pinf, ninf);
    uint64_t bits;
    __builtin_memcpy(&bits, &s, 8);
    std::printf("%016llx %lld %lld %lld\n", (unsigned long long)bits, (long long)bins[0],
                (long long)bins[15], (long long)bins[31]);
  }
  std::fclose(f);
  return 0;
}
