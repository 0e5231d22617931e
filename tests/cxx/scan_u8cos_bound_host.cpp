// The filter rule of the uint8 Cosine / Angle matrix-core scan
// (ngt_amd/csrc/scan_u8cos_bound.h) on the host: for both metrics, over a
// strided walk of the float k-th distances kd up to the largest distance of
// uint8 rows (c >= 0: 1 for Cosine, pi/2 for Angle) plus every float within 64
// ulps of 0, of the top, of the distances of the tie fixture of
// tests/test_gpu_scan_u8cos.py and the tiny negative Cosine distances, and
// over norms (na, nb) from the Dp = 16 and Dp = 1024 extremes with exact and
// inexact roots, the integers s at and around the filter's boundary H_q rx
// (steps of 1 and of the float spacing above 2^24): no triple the filter
// rejects finishes at or below kd.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <initializer_list>

#include "../../ngt_amd/csrc/scan_u8cos_bound.h"

using namespace ngt_amd;

static long thresholds = 0, probes = 0, rejected = 0, failures = 0;

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

// |x|^2 of rows of 16 and of 1024 bytes: 1, small with an inexact root, squares, the largest of each, one below it
static const uint32_t kNorms[] = {1u,      2u,         3u,         65025u,     65026u,        1040399u,
                                  1040400u, 16777259u, 33554467u, 44100000u, 66585599u, 66585600u};
static const int kSteps[] = {-64, -16, -8, -4, -3, -2, -1, 0, 1, 2, 3, 4, 8, 16, 64};

static void one(int metric, float kd) {
  thresholds++;
  for (uint32_t na : kNorms)
    for (uint32_t nb : kNorms) {
      const float hq = u8cos_h(metric, kd, na), rx = u8cos_rx(nb);
      if (!(hq >= 0.0f) || !(hq < INFINITY)) {
        if (failures++ < 20) printf("FAIL H_q %a: metric %d kd %a na %u\n", (double)hq, metric, (double)kd, na);
        continue;
      }
      const double edge = (double)hq * (double)rx;  // s > 2^24 from edge 2^24 on
      for (int st : kSteps) {
        const double sd = floor(edge) + st;
        if (sd < 0.0 || sd > 255.0 * 255.0 * kU8cMaxDp) continue;
        const int32_t s = (int32_t)sd;
        probes++;
        if (!u8cos_rejects(hq, rx, s)) continue;
        rejected++;
        const float d = u8cos_distance(metric, (uint32_t)s, na, nb);
        if (!(d > kd) && failures++ < 20)
          printf("FAIL metric %d kd %a: rejected (s, na, nb) = (%d, %u, %u) finishes at %a, H_q %a rx %a\n", metric,
                 (double)kd, s, na, nb, (double)d, (double)hq, (double)rx);
      }
    }
}

int main() {
  for (int metric : {3, 4}) {  // kAngle, kCosine (ngt_device.h)
    const float top = metric == 3 ? (float)(acos(-1.0) / 2) : 1.0f;
    // the tie fixture's distances: 0.26874 under Cosine, 0.75063 under Angle
    const float marks[] = {0.0f, top, metric == 3 ? 0.75063f : 0.26874f, 1.0e-3f};
    for (uint32_t b = 0; b <= b_of(top); b += 65521u) one(metric, f_of(b));
    for (float mark : marks) {
      const uint32_t b0 = b_of(mark);
      for (uint32_t b = b0 > 64 ? b0 - 64 : 0; b <= b0 + 64; b++) one(metric, f_of(b));
    }
    // Cosine of c a rounding above 1: k-th distances just below zero; the edges
    for (uint32_t b = 0x80000000u; b <= 0x80000040u; b++) one(metric, f_of(b));
    for (float kd : {-0x1p-53f, -0x1p-52f, -1.0f, 2.0f, 4.0f, INFINITY, NAN}) one(metric, kd);
    if (u8cos_h(metric, NAN, 66585600u) != 0.0f || u8cos_h(metric, INFINITY, 66585600u) != 0.0f ||
        u8cos_h(metric, 0.5f, 0u) != 0.0f)
      failures++, printf("FAIL edges: metric %d\n", metric);
    // nothing is rejected at H_q = 0, a row of zeros under no H_q, a removed row's NaN never compares
    if (u8cos_rejects(0.0f, 8160.0f, 0) || u8cos_rejects(123.0f, 0.0f, 0) || u8cos_filter_value(1.0f, NAN, 5) >= 0.0f)
      failures++, printf("FAIL filter edges: metric %d\n", metric);
  }
  printf("thresholds %ld probes %ld rejected %ld failures %ld\n", thresholds, probes, rejected, failures);
  return failures ? 1 : 0;
}
