// scan_u8_bound_host.cpp -- ngt_amd/csrc/scan_u8_bound.h on the CPU, over
// every sum S in [0, 2^24): the float distance of S against the comparator's
// four float lanes, max_sum_for_distance as the exact inverse of that
// distance, and u8_sum_threshold as a bound that never drops a pair.
// tests/test_scan_u8_bound_host.py compiles and runs it.
#include <stdio.h>

#include "../../ngt_amd/csrc/scan_u8_bound.h"

using namespace ngt_amd;

static long failures = 0;
static void check(bool ok, const char* what, long s) {
  if (!ok && failures++ < 20) printf("FAIL %s at %ld\n", what, s);
}

static float prev_float(float d) { return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, d) - 1u); }

int main() {
  long sums = 0, distances = 0;
  float last = -1.0f;
  int32_t last_thr = -1;
  for (int32_t s = 0; s < kU8ExactSums; s++, sums++) {
    const float d = u8_sum_distance(s);
    // compareL2's lanes: any split of S into four integers below 2^24 folds
    // exactly; the most uneven and an even one
    const float a = (float)(s / 4), b = (float)(s - 3 * (s / 4));
    check((float)sqrt((double)((a + a) + (a + b))) == d && (float)sqrt((double)(((float)s + 0.0f) + (0.0f + 0.0f))) == d,
          "distance of the folded lanes", s);
    check(d >= last, "monotone distance", s);
    const int32_t m = max_sum_for_distance(d);
    check(m >= s && m < kU8ExactSums && u8_sum_distance(m) == d, "max_sum_for_distance holds S", s);
    check(m + 1 == kU8ExactSums || u8_sum_distance(m + 1) > d, "max_sum_for_distance is the largest", s);
    if (d != last) {
      distances++;
      // between two distances: the float just below this one belongs to the sums before S
      if (s > 0) {
        const float p = prev_float(d);
        const int32_t mp = max_sum_for_distance(p);
        check(mp == s - 1, "the float below a distance", s);
      }
      const int32_t t = u8_sum_threshold(d);
      check(t >= m && t >= last_thr, "threshold covers and grows", s);
      check(d >= 4095.99f || t == m, "threshold tight in the exact range", s);
      last_thr = t;
    }
    last = d;
  }
  check(max_sum_for_distance(-1.0f) == -1 && max_sum_for_distance(__builtin_nanf("")) == -1, "no sum", -1);
  check(max_sum_for_distance(0.0f) == 0 && max_sum_for_distance(0.99f) == 0 && max_sum_for_distance(1.0f) == 1, "small", 0);
  check(max_sum_for_distance(4096.0f) == kU8ExactSums - 1 && max_sum_for_distance(3.0e38f) == kU8ExactSums - 1, "large", 0);
  // beyond the exact range: a reference sum R >= S (1 - 2^-24)^3 at or below
  // the k-th distance d (R < next_up(d)^2) must pass the threshold
  for (float d = 4095.99f; d < 8200.0f; d += 0.37f) {
    const double dn = (double)u8_next_up(d);
    const double smax = dn * dn / ((1.0 - 0x1p-24) * (1.0 - 0x1p-24) * (1.0 - 0x1p-24));
    check((double)u8_sum_threshold(d) >= smax, "threshold beyond 2^24", (long)d);
  }
  check(u8_sum_threshold(3.0e38f) == kU8SumAll && u8_sum_threshold(-1.0f) == -1, "threshold ends", 0);
  check(1024 * 255 * 255 < kU8SumAll && kU8SumAll < kU8SumNever - (1 << 26), "sentinels", 0);
  printf("sums %ld distances %ld failures %ld\n", sums, distances, failures);
  return failures ? 1 : 0;
}
