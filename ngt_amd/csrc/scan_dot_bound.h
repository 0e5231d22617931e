// scan_dot_bound.h -- the scalar rules of the matrix-core scan for the float
// metrics that are a function of one dot product or cosine c (Normalized
// Cosine, Normalized L2, Normalized Angle, Angle): the comparator's finish of
// c (dot_finish, the forms of dist_f32<M> in ngt_device.h) and its inverse
// for the filter, dot_threshold(metric, kd) = T(kd):
//
//   every c strictly below T(kd) finishes strictly above kd.
//
// Pure: no HIP, no library state; tests/cxx/scan_dot_bound_host.cpp walks the
// float kd and the doubles just below T(kd).
//
// T is built from u = next_up(kd): a finish is (float)f(c) with f a double, and
// f(c) >= u (u is a double too) gives (float)f(c) >= u > kd whatever the
// rounding mode of the conversion.
//  * Normalized Cosine, f = max(0, 1 - c): c < T <= 1 - u (real numbers) gives
//    1 - c > u, and the rounded double difference is >= u because u is a double
//    and rounding is monotone.  T = next_down(fl(1 - u)), which is <= 1 - u.
//  * Normalized L2, f = sqrt(max(0, 2 - 2c)): T = next_down(fl(1 - w / 2)) with
//    w = u^2 (1 + 2^-40) (u^2 is exact in double).  c < T gives 2 - 2c >
//    u^2 (1 + 2^-41) in real numbers, the rounded difference keeps 1 - 2^-53 of
//    it, and a sqrt within 2^-45 relative (an IEEE sqrt is within 2^-53) is
//    still >= u.
//  * the angles, f = acos(c) clamped to [0, acos(-1)]: T = dot_cos(u) - 2^-40.
//    dot_cos is the Taylor series of cos to u^30 in nested form, the same
//    operations on host and device (a library cos brings its large-argument
//    reduction along, which costs the scan kernels registers they do not
//    have): on [0, 3.1416] the truncation is below pi^32 / 32! < 2^-64 and the
//    rounding of its 45 operations, amplified by at most pi^2 / 2 per step,
//    below 2^-45.  ASSUMED of the acos in use (device and host): an absolute
//    error of at most 2^-49 (4 ulp below 4, the OpenCL bound for doubles;
//    ROCm's and glibc's are tighter).  Then T < cos*(u) - 2^-41 (cos* the real
//    function), c < T gives acos*(c) > u + 2^-41 (|d acos / dc| >= 1), and the
//    computed acos(c) > u.  c <= -1 finishes at (float)acos(-1.0), the largest
//    distance, above every kd that reaches here.  The slack is absolute, not
//    relative: near c = 1 the doubles (2^-53 apart) are the coarser scale, and
//    an absolute 2^-40 of c is far below the filter's own error at both ends.
// Edges: kd at or above the largest distance (acos(-1) as a float; 2 for
// Normalized L2 -- rows that are not unit vectors can exceed it, they are then
// simply not filtered; +inf for Normalized Cosine) gives -inf, as does a NaN
// kd: nothing is rejected.  kd = 0 gives T <= 1: every c that clamps to
// distance 0 stays.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NGT_DOT_BOUND_FN __host__ __device__ inline
#else
#define NGT_DOT_BOUND_FN inline
#endif

namespace ngt_amd {

// the metric numbers of ngt_device.h (scan_mfma_common.h asserts they agree)
constexpr int kDotAngle = 3, kDotNormalizedAngle = 5, kDotNormalizedCosine = 6, kDotNormalizedL2 = 9;

constexpr double kDotAngleSlack = 0x1p-40;    // absolute, of dot_cos(u)
constexpr double kDotL2Slack = 0x1p-40;       // relative, of u^2

NGT_DOT_BOUND_FN double dot_angle_of(double c) {  // angle_of (ngt_device.h)
  if (c >= 1.0) return 0.0;
  if (c <= -1.0) return acos(-1.0);
  return acos(c);
}

// cos on [0, 3.1416] within 2^-45: 1 - z/2 (1 - z/12 (1 - z/30 ( ... ))), z = u^2, to u^30
NGT_DOT_BOUND_FN double dot_cos(double u) {
  const double z = u * u;
  double p = 1.0;
  for (int n = 15; n >= 1; n--) p = 1.0 - z * (1.0 / (double)((2 * n - 1) * (2 * n))) * p;
  return p;
}

// the comparator's distance of its dot product / cosine c
NGT_DOT_BOUND_FN float dot_finish(int metric, double c) {
  if (metric == kDotNormalizedCosine) {
    const double v = 1.0 - c;
    return (float)(v < 0.0 ? 0.0 : v);
  }
  if (metric == kDotNormalizedL2) {
    const double v = 2.0 - 2.0 * c;
    return (float)(v < 0.0 ? 0.0 : sqrt(v));
  }
  return (float)dot_angle_of(c);
}

NGT_DOT_BOUND_FN double dot_next_down(double x) {  // finite x
  const uint64_t b = __builtin_bit_cast(uint64_t, x);
  if (x > 0.0) return __builtin_bit_cast(double, b - 1);
  if (x < 0.0) return __builtin_bit_cast(double, b + 1);
  return -0x1p-1074;
}

// the largest float <= h (h = -inf stays, NaN stays NaN)
NGT_DOT_BOUND_FN float dot_round_down(double h) {
  float f = (float)h;
  if ((double)f > h) {
    const uint32_t b = __builtin_bit_cast(uint32_t, f);
    f = f > 0.0f ? __builtin_bit_cast(float, b - 1) : f < 0.0f ? __builtin_bit_cast(float, b + 1) : -0x1p-149f;
  }
  return f;
}

// T - E_q as the float the filter compares with: hb = -E_q; the double sum and
// the conversion both rounded down.  -inf and NaN (of either side) carry through.
NGT_DOT_BOUND_FN float dot_filter_threshold(double t, float hb) {
  const double h = t + (double)hb;
  return dot_round_down(h > -(double)__builtin_huge_valf() ? dot_next_down(h) : h);
}

// T(kd): see the head of the file
NGT_DOT_BOUND_FN double dot_threshold(int metric, float kd) {
  const double none = -(double)__builtin_huge_valf();
  if (kd != kd) return none;
  if (kd <= 0.0f) kd = 0.0f;  // -0, and (no distance is negative) anything below: T(0) is valid for it
  const float top = metric == kDotNormalizedCosine ? __builtin_huge_valf()
                    : metric == kDotNormalizedL2   ? 2.0f
                                                   : (float)acos(-1.0);
  if (kd >= top) return none;
  const double u = (double)__builtin_bit_cast(float, __builtin_bit_cast(uint32_t, kd) + 1u);  // next_up(kd)
  if (metric == kDotNormalizedCosine) {
    if (!(u < (double)__builtin_huge_valf())) return none;
    return dot_next_down(1.0 - u);
  }
  if (metric == kDotNormalizedL2) return dot_next_down(1.0 - 0.5 * (u * u * (1.0 + kDotL2Slack)));
  return dot_cos(u) - kDotAngleSlack;
}

}  // namespace ngt_amd
