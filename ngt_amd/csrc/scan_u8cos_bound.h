// scan_u8cos_bound.h -- the scalar rules of the uint8 Cosine / Angle
// matrix-core scan (scan_u8cos.hip): the comparator's distance of the exact
// integers (s, na, nb) = (q.x, |q|^2, |x|^2), the float filter on s and the
// threshold H_q it compares with.  Pure: no HIP, no library state;
// tests/cxx/scan_u8cos_bound_host.cpp probes the filter's boundary.
//
// The comparator (dist_u8<kCosine> / dist_u8<kAngle>, ngt_device.h):
//   c = (double)s / sqrt((double)na * (double)nb)
//   Cosine (float)(1.0 - c), Angle (float)angle_of(c).
// For Dp <= 1024, na nb <= (255^2 1024)^2 < 2^53: the product P is exact.
// With r = fl(sqrt(P)) = sqrt(P) (1 + e1) and c = fl(s / r) = (s / r) (1 + e2),
// |e1|, |e2| <= 2^-53:
//   (1)  c <= s / (sqrt(na) sqrt(nb)) (1 + 2^-51).
//
// The filter rejects the pair iff fmaf(-H_q, rx, (float)s) < 0, with
//   (float)s = s (1 + e3), |e3| <= 2^-24   (s < 2^27 can exceed 2^24),
//   rx = (float)sqrt((double)nb) = sqrt(nb) (1 + e4), |e4| <= 2^-24 + 2^-52
//        (a double sqrt, then one conversion),
// and the fused multiply-add rounds once: a result below zero means that the
// exact (float)s - H_q rx is below zero (a tiny negative that underflows to
// -0 is not below zero: the pair is kept).  So a rejected pair has
//   s (1 - 2^-24) < H_q sqrt(nb) (1 + 2^-24 + 2^-52), hence
//   (2)  s < H_q sqrt(nb) (1 + 2^-22).
// H_q is the largest float <= T sqrt(na)' (1 - 2^-20), sqrt(na)' the double
// sqrt, the two double products rounded once each, so
//   (3)  H_q <= T sqrt(na) (1 - 2^-20) (1 + 2^-51).
// (1), (2), (3): c < T (1 - 2^-20) (1 + 2^-22) (1 + 2^-51)^2 < T for T > 0, and
// strictly so: (2) is strict.  The rule:
//
//   a pair the filter rejects has the comparator's c strictly below T(kd),
//   hence (scan_dot_bound.h) a distance strictly above kd.
//
// The slack 2^-20 is 2^-22 of need and a factor of four for nothing: at
// |c - T| < 2^-20 T the filter keeps what it could reject, a few pairs in a
// million.
//
// T(kd) is dot_threshold of scan_dot_bound.h: the Angle rule as it stands, and
// for Cosine the Normalized-Cosine rule.  Cosine finishes (float)(1.0 - c)
// without the clamp at 0, so c a rounding above 1 (parallel vectors) gives a
// tiny negative distance, and a k-th distance kd can be negative.  The rule
// takes kd <= 0 as 0, T(0) = 1 - 2^-53: c < T(0) gives 1.0 - c >= 2^-53 in
// double, a positive float, which is above 0 >= kd.  For kd > 0, c < T(kd) < 1
// keeps 1 - c positive, where the clamped and the unclamped finish agree.  A
// negative kd only costs the filter the pairs with c in [T(0), 1], which it
// keeps.
//
// Every uint8 pair has s >= 0, so c >= 0 or NaN: T <= 0, "no threshold" (-inf)
// and a NaN k-th distance all become H_q = 0, which rejects nothing with a
// number for rx: (float)s >= 0.  Removed, dummy and padding rows carry rx = NaN
// and fail the comparison under every H_q, 0 included.  A row of zeros has
// rx = 0 and s = 0: it is never rejected, its NaN distance is ranked by its key.
// A query of zeros has na = 0 and H_q = 0 for good.
#pragma once

#include <math.h>
#include <stdint.h>

#include "scan_dot_bound.h"

namespace ngt_amd {

constexpr int kU8cMaxDp = 1024;            // na nb exact in double, s < 2^27
constexpr double kU8cSlack = 0x1p-20;      // relative, of T sqrt(na)

// the rule of scan_dot_bound.h that covers the metric (ngt_device.h: kAngle 3, kCosine 4)
NGT_DOT_BOUND_FN int u8cos_rule(int metric) { return metric == 3 ? kDotAngle : kDotNormalizedCosine; }

// the comparator's cosine and distance of the exact integers
NGT_DOT_BOUND_FN double u8cos_c(uint32_t s, uint32_t na, uint32_t nb) {
  return (double)s / sqrt((double)na * (double)nb);
}
NGT_DOT_BOUND_FN float u8cos_distance(int metric, uint32_t s, uint32_t na, uint32_t nb) {
  const double c = u8cos_c(s, na, nb);
  if (metric == 3) return (float)dot_angle_of(c);
  return (float)(1.0 - c);
}

// the filter's float of a live row
NGT_DOT_BOUND_FN float u8cos_rx(uint32_t nb) { return (float)sqrt((double)nb); }

// H_q of a k-th distance (or radius bound) kd
NGT_DOT_BOUND_FN float u8cos_h(int metric, float kd, uint32_t na) {
  const double t = dot_threshold(u8cos_rule(metric), kd);
  if (!(t > 0.0)) return 0.0f;
  const double h = (t * sqrt((double)na)) * (1.0 - kU8cSlack);
  return dot_round_down(h);
}

// the filter itself
NGT_DOT_BOUND_FN float u8cos_filter_value(float hq, float rx, int32_t s) {
  return __builtin_fmaf(-hq, rx, (float)s);
}
NGT_DOT_BOUND_FN bool u8cos_rejects(float hq, float rx, int32_t s) { return u8cos_filter_value(hq, rx, s) < 0.0f; }

}  // namespace ngt_amd
