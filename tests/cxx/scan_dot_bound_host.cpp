// The threshold rules of the dot-family matrix-core scan
// (ngt_amd/csrc/scan_dot_bound.h) on the host: for each of the four metrics,
// over a strided walk of every non-negative finite float kd and every float
// within 64 ulps of 0, 1, sqrt(2), pi/2, 2 and pi, each of the 64 doubles just
// below T(kd) finishes strictly above kd; T never rises with kd; the edges.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../ngt_amd/csrc/scan_dot_bound.h"

using namespace ngt_amd;

static const int kMetrics[4] = {kDotNormalizedCosine, kDotNormalizedL2, kDotNormalizedAngle, kDotAngle};
static long thresholds = 0, probes = 0, failures = 0;

static float f_of(uint32_t b) {
  float f;
  memcpy(&f, &b, 4);
  return f;
}
static uint32_t b_of(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return b;
}
static void fail(const char* what, int m, float kd, double t, double c) {
  if (failures++ < 20) printf("FAIL %s: metric %d kd %a T %a c %a\n", what, m, (double)kd, t, c);
}
static float top_of(int m) {
  return m == kDotNormalizedCosine ? INFINITY : m == kDotNormalizedL2 ? 2.0f : (float)acos(-1.0);
}

// one kd; prev: T of the kd before it in the walk (a smaller kd), or NaN
static double one(int m, float kd, double prev) {
  const double t = dot_threshold(m, kd);
  thresholds++;
  if (t != t || t > 1.0) fail("T is NaN or above 1", m, kd, t, 0);
  if (prev == prev && t > prev) fail("T rises with kd", m, kd, t, prev);
  // FLT_MAX under Normalized Cosine: next_up is +inf, nothing can be rejected
  const bool open = kd < top_of(m) && !(m == kDotNormalizedCosine && b_of(kd) == 0x7f7fffffu);
  if (!open) {
    if (t != -INFINITY) fail("T is not -inf at the top", m, kd, t, 0);
    return t;
  }
  if (!(t > -INFINITY)) fail("T is -inf below the top", m, kd, t, 0);
  double c = t;
  for (int i = 0; i < 64; i++) {
    c = nextafter(c, -INFINITY);
    probes++;
    if (!(dot_finish(m, c) > kd)) fail("a rejected c finishes at or below kd", m, kd, t, c);
  }
  return t;
}

int main() {
  const float marks[6] = {0.0f, 1.0f, (float)sqrt(2.0), (float)(acos(-1.0) / 2), 2.0f, (float)acos(-1.0)};
  for (int m : kMetrics) {
    double prev = NAN;
    for (uint32_t b = 0; b <= 0x7f7fffffu; b += 16411u) prev = one(m, f_of(b), prev);
    one(m, f_of(0x7f7fffffu), prev);
    for (float mark : marks) {
      const uint32_t b0 = b_of(mark);
      prev = NAN;
      for (uint32_t b = b0 > 64 ? b0 - 64 : 0; b <= b0 + 64; b++) prev = one(m, f_of(b), prev);
    }
    // edges: the top and beyond, NaN, zero of either sign
    if (dot_threshold(m, INFINITY) != -INFINITY) fail("kd = inf", m, INFINITY, dot_threshold(m, INFINITY), 0);
    if (dot_threshold(m, top_of(m)) != -INFINITY) fail("kd = top", m, top_of(m), dot_threshold(m, top_of(m)), 0);
    if (dot_threshold(m, NAN) != -INFINITY) fail("kd = NaN", m, NAN, dot_threshold(m, NAN), 0);
    const double t0 = dot_threshold(m, 0.0f);
    if (!(t0 <= 1.0 && t0 > 1.0 - 0x1p-39) || dot_threshold(m, -0.0f) != t0) fail("kd = 0", m, 0.0f, t0, 0);
    if (dot_finish(m, 1.0) != 0.0f || dot_finish(m, 1.5) != 0.0f) fail("finish of c >= 1", m, 0.0f, t0, 1.0);
    if (!(dot_finish(m, NAN) != dot_finish(m, NAN))) fail("finish of NaN", m, 0.0f, t0, NAN);
  }
  // dot_cos against the library's over [0, pi]
  for (int i = 0; i <= 1000000; i++) {
    const double u = 3.1416 * i / 1000000.0;
    probes++;
    if (!(fabs(dot_cos(u) - cos(u)) < 0x1p-45)) fail("dot_cos", 0, (float)u, dot_cos(u), cos(u));
  }
  // dot_round_down: the largest float at or below a double
  const double hs[] = {0.0, 1.0, -1.0, 0.1, -0.1, 1.0 - 0x1p-53, -1.0 - 0x1p-52, 0x1p-160, -0x1p-160, -1e300, 3.0e-39};
  for (double h : hs) {
    const float f = dot_round_down(h);
    probes++;
    if (!((double)f <= h) || (f > -INFINITY && !((double)nextafterf(f, INFINITY) > h)))
      fail("dot_round_down", 0, f, h, 0);
  }
  if (dot_round_down(-INFINITY) != -INFINITY || dot_round_down(NAN) == dot_round_down(NAN))
    fail("dot_round_down of -inf / NaN", 0, 0, 0, 0);
  printf("thresholds %ld probes %ld failures %ld\n", thresholds, probes, failures);
  return failures ? 1 : 0;
}
