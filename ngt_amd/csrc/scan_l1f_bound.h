// scan_l1f_bound.h -- the scalar rules of the float L1 byte-SAD filtered scan
// (scan_l1f.hip): the one-byte quantiser, the per-vector error bounds and the
// integer threshold that tie SAD(c_q, c_x) to the reference's float distance.
// Pure: no HIP types, no library state; tests/cxx/scan_l1f_bound_host.cpp
// walks it on the CPU.
//
// Quantiser.  One affine map per version of the rows, x^_i = lo + s c_i with
// c_i in [0, 255], lo and s from the min and max over the finite elements of
// the valid rows (a constant table gets s = 1).  Every value, row or query, is
// clamped into the code range.  Columns at or past the real dimension carry
// code 0 on both sides and are left out of every sum below: their term of the
// true distance is >= 0, so leaving it out keeps a lower bound a lower bound.
//
// Bound.  For any q, x (real numbers, no range assumption)
//   |q - x|_1 >= |q^ - x^|_1 - |q - q^|_1 - |x - x^|_1,   |q^ - x^|_1 = s SAD(c_q, c_x),
// so with e_x >= |x - x^|_1 and e_q >= |q - q^|_1
//   D = |q - x|_1 >= s SAD - e_q - e_x.                                  (1)
// A clamped outlier makes its own e large and nothing else.
//
// e in double (l1f_err_up).  A term |v - (lo + s c)| takes three roundings:
// p = s c, r = lo + p, v - r; its absolute error is at most
// 2^-52 (|lo| + 255 s) + 2^-53 (the term).  The sum of n terms adds at most
// n 2^-53 relative.  sum (1 + 2^-40) + n (|lo| + 255 s) 2^-48 is far above both.
//
// The comparator (compareL1, dist_f32<kL1> in ngt_device.h; l1f_comparator
// below restates it): fl(q_i - x_i) = (q_i - x_i)(1 + d), |d| <= u = 2^-24,
// the absolute value is exact; AVX lane j sums its n = Dp / 8 terms in column
// order (the first add, to zero, is exact: n - 1 roundings), and the fold
// ((l0+l1)+(l2+l3))+((l4+l5)+(l6+l7)) adds three more.  A float sum or
// difference that lands in the subnormals is exact, so no underflow term.
// Every term is >= 0 and passes through at most m = n + 3 roundings, each
// keeping at least (1 - u) of it (rounding is monotone):
//   F >= D (1 - u)^m,   F the comparator's float distance.                (2)
// (An overflow gives F = +inf, above every finite k-th distance.)
// rho = (n + 4) u is at least (1 - u)^-m - 1:  (1 - u)^-m <= 1 / (1 - m u),
// and m u / (1 - m u) <= (m + 1) u  <=>  m (m + 1) u <= 1, true for
// m <= 4095, i.e. far beyond Dp = 256 (m = 35).
//
// The rule.  A pair is rejected iff SAD > T + E_x with integers
//   E_x >= e_x / s,   T >= (kd (1 + rho) + e_q) / s.
// Then s SAD - e_q - e_x > kd (1 + rho), by (1) D > kd (1 + rho), by (2)
// F >= D (1 - u)^m >= D / (1 + rho) > kd: a rejected pair's reference float
// distance is STRICTLY above the k-th distance kd, so no pair of equal
// distance (which a lower id would win) is ever dropped.  Both integers are
// rounded up past the three double roundings of their expression
// ((1 + 2^-50), ceil, + 1).
//
// Forced rows (a non-finite element, or E_x beyond kL1fErrCap, where the rule
// could never reject them) are always candidates; a query with a non-finite
// element, a NaN or infinite kd (no k-th distance yet, no radius) gives
// kL1fAll: everything is a candidate.  Results are then still right, only the
// speed goes.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define NGT_L1F_BOUND_FN __host__ __device__ inline
#else
#define NGT_L1F_BOUND_FN inline
#endif

namespace ngt_amd {

constexpr int32_t kL1fSadMax = 255 * 256;  // the largest SAD of two code rows (Dp <= 256)
constexpr int32_t kL1fErrCap = 1 << 16;    // E_x above this: the row is forced
constexpr int32_t kL1fAll = 1 << 17;       // a threshold every SAD passes
// Row biases of the kernel's accumulator S' = bias + SAD, survivor iff
// S' <= T + kL1fEmax: a row's bias is kL1fEmax - E_x, a forced row's 0
// (S' <= kL1fSadMax passes every T >= 0), a removed / dummy / padding row's
// kL1fNever (above kL1fAll + kL1fEmax).
constexpr int32_t kL1fEmax = 1 << 17;
constexpr int32_t kL1fNever = 1 << 30;

struct L1fQuant {
  double lo, s;
};

// lo and s of the finite minimum and maximum (any = false: no finite element)
NGT_L1F_BOUND_FN L1fQuant l1f_quant(float mn, float mx, bool any) {
  L1fQuant z = {0.0, 1.0};
  if (!any || !(mn <= mx)) return z;
  z.lo = (double)mn;
  z.s = ((double)mx - (double)mn) / 255.0;
  if (!(z.s > 0.0)) z.s = 1.0;
  return z;
}

NGT_L1F_BOUND_FN bool l1f_finite(float v) { return (__builtin_bit_cast(uint32_t, v) & 0x7f800000u) != 0x7f800000u; }

// the code of a finite v: nearest, clamped
NGT_L1F_BOUND_FN uint32_t l1f_code(L1fQuant z, float v) {
  const double c = rint(((double)v - z.lo) / z.s);
  return c >= 255.0 ? 255u : c >= 0.0 ? (uint32_t)c : 0u;
}

// |v - x^| of code c, as computed (its error: l1f_err_up)
NGT_L1F_BOUND_FN double l1f_term(L1fQuant z, float v, uint32_t c) { return fabs((double)v - (z.lo + z.s * (double)c)); }

// an upper bound of the real sum of n terms whose computed sum is `sum`
NGT_L1F_BOUND_FN double l1f_err_up(L1fQuant z, double sum, int n) {
  return sum * (1.0 + 0x1p-40) + (double)n * (fabs(z.lo) + 255.0 * z.s) * 0x1p-48;
}

// the comparator's rounding: see the head of the file
NGT_L1F_BOUND_FN double l1f_rho(int dp) { return (double)(dp / 8 + 4) * 0x1p-24; }

// E_x of an error bound e (l1f_err_up): an integer >= e / s, or -1 for a
// forced row (NaN and inf included)
NGT_L1F_BOUND_FN int32_t l1f_row_err(L1fQuant z, double e) {
  const double v = e / z.s * (1.0 + 0x1p-50);
  if (!(v < (double)kL1fErrCap - 2.0)) return -1;
  return (int32_t)ceil(v) + 1;
}

// T(kd, e_q): an integer >= (kd (1 + rho) + e_q) / s, kL1fAll at the most.
// Monotone in kd and e_q; kd < 0 counts as 0 (no distance is negative).
NGT_L1F_BOUND_FN int32_t l1f_threshold(L1fQuant z, double rho, float kd, double eq) {
  if (!(kd < __builtin_huge_valf()) || !(eq < (double)__builtin_huge_valf())) return kL1fAll;
  const double d = kd > 0.0f ? (double)kd : 0.0;
  const double v = (d * (1.0 + rho) + eq) / z.s * (1.0 + 0x1p-50);
  if (!(v < (double)kL1fAll - 2.0)) return kL1fAll;
  return (int32_t)ceil(v) + 1;
}

// compareL1 on one thread, bit for bit dist_f32<kL1>: eight accumulators, AVX
// lane j taking columns 8i + j in column order, then the fold -- the host
// restatement the bound is tested against; the kernel's form is dist_lane_l1
// (scan_mfma_common.h).  dp: a multiple of 8.
template <typename QP, typename XP>
NGT_L1F_BOUND_FN float l1f_comparator(QP q, XP x, int dp) {
  float l[8];
  for (int j = 0; j < 8; j++) l[j] = 0.0f;
  for (int i = 0; i < dp; i += 8)
    for (int j = 0; j < 8; j++) l[j] = l[j] + fabsf(q[i + j] - x[i + j]);
  return ((l[0] + l[1]) + (l[2] + l[3])) + ((l[4] + l[5]) + (l[6] + l[7]));
}

}  // namespace ngt_amd
