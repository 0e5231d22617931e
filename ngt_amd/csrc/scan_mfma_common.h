// scan_mfma_common.h -- what the matrix-core filtered scans share
// (scan_mfma.hip: k <= 16, lists in LDS; scan_mfma_wide.hip: k <= 128, lists
// in the partial buffer): the tile constants, the comparator on one lane and
// the LDS-only barrier.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ngt_device.h"
#include "scan_dot_bound.h"

namespace ngt_amd {

// The dot family: metrics whose distance is a function of one dot product
// (kScanDot: Normalized Cosine / L2 / Angle, one instantiation, the finish
// picked at run time by MfmaScanArgs::fin) or of the comparator's cosine
// (kAngle).  Their thresholds come from scan_dot_bound.h.
constexpr int kScanDot = 1000;  // no metric's number
template <int M>
constexpr bool kIsDotFamily = M == kScanDot || M == kAngle;
static_assert(kDotAngle == kAngle && kDotNormalizedAngle == kNormalizedAngle &&
              kDotNormalizedCosine == kNormalizedCosine && kDotNormalizedL2 == kNormalizedL2);

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kMxQ = 128;    // queries per workgroup
constexpr int kMxR = 256;    // rows per tile
constexpr int kMxW = kMxR / 32;  // candidate bitmap words per query
constexpr int kMxNst = 4;    // staging ring depth (k-steps in flight: kMxNst - 1)
constexpr int kMxStage = 24576;  // one k-step: rows hi/lo 8 KiB each, queries hi/lo 4 KiB each

// squared-sum bound of a distance d (as in scan_kernels.hip): any sum whose
// (float)sqrt((double)sum) is <= d is below it
__device__ __forceinline__ float scan_sq_bound(float d) {
  if (!(d >= 0.0f) || d >= 3.0e38f) return __builtin_huge_valf();
  const double dn = (double)__uint_as_float(__float_as_uint(d) + 1u);
  const float s2 = (float)(dn * dn);
  return __uint_as_float(__float_as_uint(s2) + 1u);
}

// The comparator on one lane: PrimitiveComparator's 16 AVX-512 accumulator
// lanes as 16 registers (lane l: dims l, l+16, ...), the 16 -> 8 -> 4 folds
// and (x0 + x1) + (x2 + x3) exactly as fold16 (ngt_device.h), double sqrt /
// double cosine -- bit for bit dist_f32<M>.  kScanDot: the one dot product
// of the normalized metrics, its last four lanes summed in double (fold16_dot), and the
// finish of metric `fin`.
__device__ __forceinline__ float fold16_lane(const float* v) {
  float t8[8], t4[4];
#pragma unroll
  for (int j = 0; j < 8; j++) t8[j] = v[j + 8] + v[j];
#pragma unroll
  for (int j = 0; j < 4; j++) t4[j] = t8[j + 4] + t8[j];
  return (t4[0] + t4[1]) + (t4[2] + t4[3]);
}
// compareL1 on one lane, bit for bit dist_f32<kL1>: the 8 AVX accumulator
// lanes as 8 registers, lane j taking columns 8i + j in column order, the
// fold ((l0+l1)+(l2+l3))+((l4+l5)+(l6+l7)).  QP: the query through any pointer
// to float (scan_l1f.hip reads it through the scalar cache).
template <typename QP>
__device__ __forceinline__ float dist_lane_l1(QP q, const float* __restrict__ x, int dp) {
  const float4* x4 = reinterpret_cast<const float4*>(x);
  float l[8];
#pragma unroll
  for (int j = 0; j < 8; j++) l[j] = 0.0f;
#pragma unroll 2
  for (int i = 0; i < (dp >> 3); i++) {
    const float4 a = x4[2 * i], b = x4[2 * i + 1];
    const float xa[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int j = 0; j < 8; j++) l[j] = l[j] + __builtin_fabsf(q[8 * i + j] - xa[j]);
  }
  return ((l[0] + l[1]) + (l[2] + l[3])) + ((l[4] + l[5]) + (l[6] + l[7]));
}
template <int M>
__device__ __forceinline__ float dist_lane(const float* __restrict__ q, const float* __restrict__ x, int dp,
                                           int fin = 0) {
  const float4* q4 = reinterpret_cast<const float4*>(q);
  const float4* x4 = reinterpret_cast<const float4*>(x);
  if constexpr (M == kL1) {
    return dist_lane_l1(q, x, dp);
  } else if constexpr (M == kL2) {
    float acc[16];
#pragma unroll
    for (int l = 0; l < 16; l++) acc[l] = 0.0f;
#pragma unroll 2
    for (int i = 0; i < (dp >> 4); i++) {
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const float4 qv = q4[4 * i + c], xv = x4[4 * i + c];
        const float d0 = qv.x - xv.x, d1 = qv.y - xv.y, d2 = qv.z - xv.z, d3 = qv.w - xv.w;
        acc[4 * c + 0] = __builtin_fmaf(d0, d0, acc[4 * c + 0]);
        acc[4 * c + 1] = __builtin_fmaf(d1, d1, acc[4 * c + 1]);
        acc[4 * c + 2] = __builtin_fmaf(d2, d2, acc[4 * c + 2]);
        acc[4 * c + 3] = __builtin_fmaf(d3, d3, acc[4 * c + 3]);
      }
    }
    return (float)sqrt((double)fold16_lane(acc));
  } else if constexpr (M == kScanDot) {
    float sv[16];
#pragma unroll
    for (int l = 0; l < 16; l++) sv[l] = 0.0f;
#pragma unroll 2
    for (int i = 0; i < (dp >> 4); i++) {
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const float4 qv = q4[4 * i + c], xv = x4[4 * i + c];
        sv[4 * c + 0] = __builtin_fmaf(xv.x, qv.x, sv[4 * c + 0]);
        sv[4 * c + 1] = __builtin_fmaf(xv.y, qv.y, sv[4 * c + 1]);
        sv[4 * c + 2] = __builtin_fmaf(xv.z, qv.z, sv[4 * c + 2]);
        sv[4 * c + 3] = __builtin_fmaf(xv.w, qv.w, sv[4 * c + 3]);
      }
    }
    float t8[8], t4[4];
#pragma unroll
    for (int j = 0; j < 8; j++) t8[j] = sv[j + 8] + sv[j];
#pragma unroll
    for (int j = 0; j < 4; j++) t4[j] = t8[j + 4] + t8[j];
    return dot_finish(fin, ((double)t4[0] + (double)t4[1]) + ((double)t4[2] + (double)t4[3]));
  } else {  // kCosine, kAngle
    float na[16], nb[16], sv[16];
#pragma unroll
    for (int l = 0; l < 16; l++) na[l] = nb[l] = sv[l] = 0.0f;
#pragma unroll 2
    for (int i = 0; i < (dp >> 4); i++) {
#pragma unroll
      for (int c = 0; c < 4; c++) {
        const float4 qv = q4[4 * i + c], xv = x4[4 * i + c];
        const float qa[4] = {qv.x, qv.y, qv.z, qv.w}, xa[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
          na[4 * c + e] = __builtin_fmaf(qa[e], qa[e], na[4 * c + e]);
          nb[4 * c + e] = __builtin_fmaf(xa[e], xa[e], nb[4 * c + e]);
          sv[4 * c + e] = __builtin_fmaf(xa[e], qa[e], sv[4 * c + e]);
        }
      }
    }
    const double dna = fold16_lane(na), dnb = fold16_lane(nb), ds = fold16_lane(sv);
    const double cs = ds / sqrt(dna * dnb);
    if constexpr (M == kAngle) return dot_finish(kAngle, cs);
    else return (float)(1.0 - cs);
  }
}

// The dot family's filter threshold of a k-th distance (or radius bound) kd:
// H = T(kd) - E_q rounded down, with hb = -E_q (NaN: no such query, -inf: a
// query the filter cannot bound -- both carry through).
__device__ __forceinline__ float scan_dot_h(int fin, float hb, float kd) {
  return dot_filter_threshold(dot_threshold(fin, kd), hb);
}
// The bootstrap: k rows have a filter value of at least v, so a comparator dot
// product of at least v - hm (hm = E_q) and a distance of at most its finish.
__device__ __forceinline__ float scan_dot_boot(int fin, float hb, float hm, float v) {
  return scan_dot_h(fin, hb, dot_finish(fin, (double)v - (double)hm));
}

// Workgroup barrier for LDS only.  __syncthreads() would also drain the
// staging ring's LDS-DMA loads (vmcnt(0)); the ring is waited for by count.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

}  // namespace ngt_amd
