// scan_u8_lane.h -- the uint8 L2 comparator on one lane, shared by the two
// int8 matrix-core scans (scan_u8.hip: k <= 16, scan_u8_wide.hip: k <= 128)
// for the survivors whose sum S >= 2^24 no longer gives the distance's bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ngt_amd {

// The comparator on one lane: PrimitiveComparator's four float lanes (lane c:
// elements e with e mod 4 == c) as exact integers, the folds and double sqrt
// of dist_u8<kL2> (ngt_device.h).
__device__ __forceinline__ float u8_l2_lane(const uint8_t* __restrict__ q, const uint8_t* __restrict__ x, int dp) {
  const uint32_t* qw = reinterpret_cast<const uint32_t*>(q);
  const uint32_t* xw = reinterpret_cast<const uint32_t*>(x);
  int acc[4] = {0, 0, 0, 0};
  for (int i = 0; i < (dp >> 2); i++) {
    const uint32_t qv = qw[i], xv = xw[i];
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const int d = (int)((qv >> (8 * c)) & 0xff) - (int)((xv >> (8 * c)) & 0xff);
      acc[c] += d * d;
    }
  }
  // f0 + f1 of two exact lane sums (< 2^24 each for dp <= 1024) is the exact
  // integer rounded to nearest even, which is what the conversion of
  // acc[0] + acc[1] gives: one rounding either way, and no pair of float adds
  // for the compiler to pack
  const float f01 = (float)(acc[0] + acc[1]), f23 = (float)(acc[2] + acc[3]);
  return (float)sqrt((double)(f01 + f23));
}

}  // namespace ngt_amd
