// bm25mi_stats_sum.h — the float32 sum of the field statistics (include/bm25mi.h,
// "Field statistics"): the exact real sum of float32 values, rounded once to
// float64.  One definition for the accumulate pass (the addend of a value),
// the finalise pass (the rounding) and a stand-alone host program
// (tests/asan/stats_sum_check.cpp): everything here is __host__ __device__ and
// integer until the one ldexp.
//
// A finite float32 of biased exponent e and fraction f is sig * 2^(E - 150)
// with E = max(e, 1) and sig = f | (e ? 2^23 : 0).  It is accumulated as the
// integer  +-(sig << (E & 7))  (a magnitude below 2^31) in bin E >> 3, a bin
// of weight 2^(8 b - 150): fewer than 2^32 addends keep every bin inside int64.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef __host__
#define __host__
#endif
#ifndef __device__
#define __device__
#endif

namespace bm25mi {

constexpr int kStatsSumBins = 32;

// The bin and the signed addend of a finite float32 (bits u, exponent < 255).
__host__ __device__ inline void stats_addend(uint32_t u, int* bin, int64_t* add) {
  const uint32_t e = (u >> 23) & 0xFFu;
  const uint32_t E = e ? e : 1u;
  const uint32_t sig = (u & 0x7FFFFFu) | (e ? 0x800000u : 0u);
  const int64_t mag = (int64_t)((uint64_t)sig << (E & 7u));
  *bin = (int)(E >> 3);
  *add = (u & 0x80000000u) ? -mag : mag;
}

// The 32 bins and the inf counters of one bucket -> its sum: the bins are
// carry-normalised from low to high into a signed multi-limb integer, its
// magnitude's top 53 bits are rounded to nearest-even on the rest, and the
// result is scaled by 2^-150.  +inf without -inf: +inf; the mirror: -inf;
// both: NaN.  An exact zero is +0.0.
__host__ __device__ inline double stats_sum_round(const int64_t* bins, uint64_t n_pinf,
                                                  uint64_t n_ninf) {
  if (n_pinf || n_ninf) {
    if (n_pinf && n_ninf) return (double)NAN;
    return n_pinf ? (double)INFINITY : -(double)INFINITY;
  }
  // 256 bits of digits in w[0..3], the last carry (signed) in w[4]
  uint64_t w[5] = {0, 0, 0, 0, 0};
  int64_t carry = 0;
  for (int b = 0; b < kStatsSumBins; ++b) {
    // (a wrapping add: |bin| < 2^63 and |carry| < 2^55, and t's low byte and
    // arithmetic shift are those of the true sum whenever it fits, which the
    // bound on the addends guarantees)
    const int64_t t = (int64_t)((uint64_t)bins[b] + (uint64_t)carry);
    w[b >> 3] |= (uint64_t)(t & 0xFF) << (8 * (b & 7));
    carry = t >> 8;  // arithmetic
  }
  w[4] = (uint64_t)carry;
  const bool neg = carry < 0;
  if (neg) {  // the magnitude: two's complement over the five limbs
    uint64_t c = 1;
    for (int i = 0; i < 5; ++i) {
      const uint64_t v = ~w[i] + c;
      c = (c && v == 0) ? 1 : 0;
      w[i] = v;
    }
  }
  int top = -1;  // the highest set bit
  for (int i = 4; i >= 0 && top < 0; --i)
    if (w[i]) {
      int p = 63;
      while (!((w[i] >> p) & 1)) --p;
      top = 64 * i + p;
    }
  if (top < 0) return 0.0;
  uint64_t mant;
  int shift = 0;
  if (top <= 52) {
    mant = w[0];
  } else {
    shift = top - 52;  // bits [shift, shift + 53) are kept
    const int wi = shift >> 6, bi = shift & 63;
    mant = w[wi] >> bi;
    if (bi && wi + 1 < 5) mant |= w[wi + 1] << (64 - bi);
    mant &= (1ull << 53) - 1;
    const int r = shift - 1;  // the round bit; the sticky bits lie below it
    const bool round = (w[r >> 6] >> (r & 63)) & 1;
    bool sticky = (w[r >> 6] & (((uint64_t)1 << (r & 63)) - 1)) != 0;
    for (int i = 0; i < (r >> 6); ++i) sticky = sticky || w[i] != 0;
    if (round && (sticky || (mant & 1))) ++mant;  // (2^53 is still exact in a double)
  }
  const double v = ldexp((double)mant, shift - 150);
  return neg ? -v : v;
}

}  // namespace bm25mi
