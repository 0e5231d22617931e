// Host program of tests/test_build_host.py: the order-deciding arithmetic of a
// DVP-tree leaf split (ngt_amd/csrc/build_order.h) without a device.
//
//  * std_sort against this machine's std::sort with the same comparison
//    (distance only), for every n in 2..101 and 128 and key classes full of
//    ties: the sequence of .i must be identical.  Built with
//    -DNGT_BUILD_ORDER_COUNT, it counts how often the depth limit was reached,
//    and fails unless heap_sort ran.
//  * pivot_variance against a long double two-pass variance (bound
//    128 * 2^-53 * mean of squares) and, bit for bit, against lane_variance
//    below, a second statement of the documented lane order.
//
// Compile with -ffp-contract=off: the only fused operations are the fma calls.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <string>
#include <vector>

#include "../../ngt_amd/csrc/build_order.h"

using ngt_amd::SortItem;

namespace {

int failures = 0;

// ---- sort ---------------------------------------------------------------------
long sort_cases = 0;

void check_sort(const char* cls, const std::vector<float>& keys) {
  const size_t n = keys.size();
  std::vector<SortItem> a(n), b(n);
  for (size_t i = 0; i < n; i++) a[i] = b[i] = SortItem{keys[i], (uint32_t)i};
  ngt_amd::std_sort(a.data(), a.data() + n);
  std::sort(b.begin(), b.end(), [](const SortItem& x, const SortItem& y) { return x.d < y.d; });
  sort_cases++;
  for (size_t i = 0; i < n; i++)
    if (a[i].i != b[i].i || memcmp(&a[i].d, &b[i].d, 4) != 0) {
      if (failures++ < 10)
        printf("FAIL sort %s n=%zu: position %zu holds item %u (key %g), std::sort has item %u (key %g)\n", cls, n, i,
               a[i].i, a[i].d, b[i].i, b[i].d);
      return;
    }
}

// An input on which this machine's std::sort degrades (the adversary of
// M. D. McIlroy, "A Killer Adversary for Quicksort", 1999): the sort runs on
// item numbers whose keys are undecided until a comparison needs them; two
// undecided items compared fix the smaller key on the one likely to be a
// pivot, so every pivot ends up among the smallest keys of its range.
struct Adversary {
  std::vector<int> val;
  int gas, nsolid = 0, candidate = 0;
  explicit Adversary(int n) : val(n, n), gas(n) {}
  bool less(int x, int y) {
    if (val[x] == gas && val[y] == gas) val[x == candidate ? x : y] = nsolid++;
    if (val[x] == gas) candidate = x;
    else if (val[y] == gas) candidate = y;
    return val[x] < val[y];
  }
};

std::vector<float> killer(int n) {
  Adversary adv(n);
  std::vector<int> item(n);
  for (int i = 0; i < n; i++) item[i] = i;
  std::sort(item.begin(), item.end(), [&](int x, int y) { return adv.less(x, y); });
  return std::vector<float>(adv.val.begin(), adv.val.end());
}

// D. R. Musser's median-of-three killer (first, middle, last), "Introspective
// Sorting and Selection Algorithms", 1997; an odd n gets its largest key last.
std::vector<float> musser(int n) {
  std::vector<float> a(n, (float)n);
  const int k = n / 2;
  for (int i = 1; i <= k; i++) {
    if (i % 2 == 1) {
      a[i - 1] = (float)i;
      if (i < k) a[i] = (float)(k + i);
    }
    a[k + i - 1] = (float)(2 * i);
  }
  return a;
}

void sort_tests() {
  std::mt19937 rng(20240607u);
  std::vector<int> sizes;
  for (int n = 2; n <= 101; n++) sizes.push_back(n);
  sizes.push_back(128);
  for (int n : sizes) {
    std::vector<float> k(n);
    check_sort("all equal", std::vector<float>(n, 3.5f));
    for (int rep = 0; rep < 8; rep++) {
      for (int i = 0; i < n; i++) k[i] = (float)(rng() & 1u);
      check_sort("two values", k);
      for (int i = 0; i < n; i++) k[i] = (float)(rng() & 7u);
      check_sort("integers 0..7", k);
      // blocks of equal keys, block length 1..8, block keys in random order
      for (int i = 0; i < n;) {
        const int len = 1 + (int)(rng() % 8u);
        const float key = (float)(rng() % 16u) * 0.25f;
        for (int j = 0; j < len && i < n; j++) k[i++] = key;
      }
      check_sort("blocks", k);
    }
    for (int q = 1; q <= 4; q *= 2) {  // q > 1: the same shapes with runs of ties
      for (int i = 0; i < n; i++) k[i] = (float)(i / q);
      check_sort("ascending", k);
      for (int i = 0; i < n; i++) k[i] = (float)((n - 1 - i) / q);
      check_sort("descending", k);
      for (int i = 0; i < n; i++) k[i] = (float)(std::min(i, n - 1 - i) / q);
      check_sort("organ pipe", k);
    }
    if (n > 16) {
      const std::vector<float> kil = killer(n), mus = musser(n);
      for (int q = 1; q <= 3; q++) {
        for (int i = 0; i < n; i++) k[i] = floorf(kil[i] / (float)q);
        check_sort("killer (adversary)", k);
        for (int i = 0; i < n; i++) k[i] = floorf(mus[i] / (float)q);
        check_sort("killer (Musser)", k);
      }
    }
  }
}

// ---- variance -----------------------------------------------------------------
long variance_cases = 0;
double worst_ratio = 0.0;

// The documented order, stated once more: sums of the row and of the squared
// deviations run in four lanes over blocks of 8 (lane l takes elements l and
// l + 4 of a block), folded (l1 + l3) + (l0 + l2); a block of 4 follows if 4
// elements remain, then single elements; squares are fused:
// fma(lo, lo, hi * hi) in a block of 8, fma(y1, y1, y3 * y3) + fma(y0, y0, y2 * y2)
// in the block of 4, fma(d, d, acc) for a single element.
double lane_variance(const float* x, uint32_t n) {
  const double inv = 1.0 / (double)n;
  double total[2] = {0.0, 0.0};  // [0] the sum, [1] the sum of squared deviations
  double avg = 0.0;
  for (int pass = 0; pass < 2; pass++) {
    auto term = [&](uint32_t i) { return pass == 0 ? (double)x[i] : (double)x[i] - avg; };
    double acc = 0.0;
    uint32_t at = 0;
    if (n >= 8) {
      double lanes[4] = {0.0, 0.0, 0.0, 0.0};
      for (; at + 8 <= n; at += 8)
        for (int l = 0; l < 4; l++) {
          const double lo = term(at + l), hi = term(at + l + 4);
          lanes[l] += pass == 0 ? lo + hi : fma(lo, lo, hi * hi);
        }
      acc = (lanes[1] + lanes[3]) + (lanes[0] + lanes[2]);
      if (n - at >= 4) {
        const double y[4] = {term(at), term(at + 1), term(at + 2), term(at + 3)};
        acc += pass == 0 ? (y[1] + y[3]) + (y[0] + y[2]) : fma(y[1], y[1], y[3] * y[3]) + fma(y[0], y[0], y[2] * y[2]);
        at += 4;
      }
    }
    for (; at < n; at++) {
      const double d = term(at);
      acc = pass == 0 ? acc + d : fma(d, d, acc);
    }
    total[pass] = acc;
    if (pass == 0) avg = acc * inv;
  }
  return total[1] * inv;
}

void check_variance(const char* cls, const std::vector<float>& x) {
  const uint32_t n = (uint32_t)x.size();
  const double got = ngt_amd::pivot_variance(x.data(), n);
  long double s = 0, sq = 0, v = 0;
  for (float f : x) {
    s += f;
    sq += (long double)f * f;
  }
  const long double mean = s / n;
  for (float f : x) v += ((long double)f - mean) * ((long double)f - mean);
  const long double ref = v / n, bound = 128.0L * ldexpl(1.0L, -53) * (sq / n);
  variance_cases++;
  const long double err = fabsl((long double)got - ref);
  if (bound > 0) worst_ratio = std::max(worst_ratio, (double)(err / bound));
  if (!(err <= bound) && failures++ < 10)
    printf("FAIL variance %s n=%u: %.17g, two-pass long double %.17Lg, difference %.3Lg above the bound %.3Lg\n", cls, n,
           got, ref, err, bound);
  const double lanes = lane_variance(x.data(), n);
  if (memcmp(&got, &lanes, 8) != 0 && failures++ < 10)
    printf("FAIL variance %s n=%u: %.17g is not the lane order's %.17g\n", cls, n, got, lanes);
}

void variance_tests() {
  std::mt19937 rng(97u);
  auto unit = [&]() { return (float)(rng() >> 8) * (1.0f / 16777216.0f); };
  for (uint32_t n = 1; n <= 101; n++) {
    std::vector<float> x(n);
    for (int rep = 0; rep < 6; rep++) {
      for (auto& f : x) f = unit();
      check_variance("random in [0, 1)", x);
      for (auto& f : x) f = 1000.0f + unit();
      check_variance("random, large offset", x);
      for (auto& f : x) f = (float)(rng() % 5u);
      check_variance("small integers", x);
      for (auto& f : x) f = ldexpf(unit(), (int)(rng() % 40u) - 20);
      check_variance("random over 40 binades", x);
      // symmetric about the mean c: c - t and c + t in pairs (exact in float), shuffled
      const float c = (float)(8 + rng() % 8u);
      for (uint32_t i = 0; i + 1 < n; i += 2) {
        const float t = (float)(rng() % 1024u) * (1.0f / 256.0f);
        x[i] = c - t;
        x[i + 1] = c + t;
      }
      if (n & 1) x[n - 1] = c;
      std::shuffle(x.begin(), x.end(), rng);
      check_variance("symmetric about the mean", x);
    }
    check_variance("constant 0", std::vector<float>(n, 0.0f));
    check_variance("constant 0.1", std::vector<float>(n, 0.1f));
    check_variance("constant 3", std::vector<float>(n, 3.0f));
    check_variance("constant 1e30", std::vector<float>(n, 1e30f));
  }
}

}  // namespace

int main() {
  sort_tests();
  variance_tests();
  long heap_sorts = -1;
#ifdef NGT_BUILD_ORDER_COUNT
  heap_sorts = ngt_amd::build_order_heap_sorts();
  if (heap_sorts <= 0) {
    failures++;
    printf("FAIL sort: no input reached the depth limit, heap_sort never ran\n");
  }
#endif
  printf("sort_cases %ld heap_sorts %ld variance_cases %ld worst_error_over_bound %.3g failures %d\n", sort_cases,
         heap_sorts, variance_cases, worst_ratio, failures);
  return failures ? 1 : 0;
}
