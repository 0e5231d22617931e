// scan_u8_bound.h -- the two scalar rules of the uint8 L2 matrix-core scan
// (scan_u8.hip) that tie an integer sum of squared differences S to the
// reference's float distance.  Pure: no HIP, no library state; the host test
// (tests/cxx/scan_u8_bound_host.cpp) walks every S in [0, 2^24).
//
// compareL2(const unsigned char*, ...) (PrimitiveComparator.h:200-223) sums
// integer squares in four float lanes and folds them (f0 + f1) + (f2 + f3).
// While S < 2^24 every partial sum is an integer below 2^24, exact in fp32,
// so the distance is exactly (float)sqrt((double)S).  From 2^24 on the folds
// may round: S alone no longer gives the bits, only a bound (u8_sum_threshold).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NGT_U8_BOUND_FN __host__ __device__ inline
#else
#define NGT_U8_BOUND_FN inline
#endif

namespace ngt_amd {

constexpr int32_t kU8ExactSums = 1 << 24;  // S below this: the distance is a function of S
constexpr int32_t kU8SumAll = 1 << 28;     // a threshold every real sum passes (S <= 1024 * 255^2 < 2^26)
constexpr int32_t kU8SumNever = 1 << 30;   // the norm of a removed / padding row: above every threshold

// the reference's distance of a sum S < 2^24
NGT_U8_BOUND_FN float u8_sum_distance(int32_t s) { return (float)sqrt((double)s); }

NGT_U8_BOUND_FN float u8_next_up(float d) {  // d >= 0, finite
  return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, d) + 1u);
}

// the largest S < 2^24 with u8_sum_distance(S) <= d; -1 when there is none
NGT_U8_BOUND_FN int32_t max_sum_for_distance(float d) {
  if (!(d >= 0.0f)) return -1;
  if (d >= 4096.0f) return kU8ExactSums - 1;
  // S >= next_up(d)^2 has sqrt(S) >= next_up(d) > d: start there, step down
  // (the step is d * ulp(d) <= 1 wide, so a few iterations at the most)
  const double dn = (double)u8_next_up(d);
  const double b = dn * dn;
  int32_t s = b >= (double)kU8ExactSums ? kU8ExactSums - 1 : (int32_t)b;
  while (s >= 0 && u8_sum_distance(s) > d) s--;
  return s;
}

// The filter threshold of a k-th distance d: every pair whose reference
// distance is <= d has S <= u8_sum_threshold(d).
//  * d < 4095.99f: a pair with S >= 2^24 has a reference sum of at least
//    S (1 - 2^-24)^3 > 2^24 - 4, a distance above 4095.99f: only the exact
//    range matters, and there the threshold is tight.
//  * otherwise: the reference sum R >= S (1 - 2^-24)^3; R >= next_up(d)^2
//    means a distance >= next_up(d) > d (sqrt and the float rounding are
//    monotone), so S (1 - 2^-24)^3 < next_up(d)^2 bounds the candidates; the
//    factor below is a little more than (1 - 2^-24)^-3.  Pairs it lets
//    through get the comparator's own distance.
NGT_U8_BOUND_FN int32_t u8_sum_threshold(float d) {
  if (!(d >= 0.0f)) return -1;
  if (d < 4095.99f) return max_sum_for_distance(d);
  if (d >= 16384.0f) return kU8SumAll;
  const double dn = (double)u8_next_up(d);
  const double b = dn * dn * (1.0 + 0x1p-22) + 1.0;
  return b >= (double)kU8SumAll ? kU8SumAll : (int32_t)b;
}

}  // namespace ngt_amd
