// scan_l1f_bound_host.cpp -- ngt_amd/csrc/scan_l1f_bound.h on the CPU: T against long double arithmetic over
// edge cases and a random walk of (kd, e_q, s), its monotony in kd, E_x s >= e_x, and, for random short vectors
// coded as the scan codes them, that no rejected pair has a comparator distance at or below kd.
// tests/test_scan_l1f_bound_host.py compiles and runs it.
#include <stdio.h>

#include <random>
#include <vector>

#include "../../ngt_amd/csrc/scan_l1f_bound.h"

using namespace ngt_amd;

static long failures = 0;
static void check(bool ok, const char* what, double a, double b) {
  if (!ok && failures++ < 20) printf("FAIL %s at %.17g %.17g\n", what, a, b);
}

static float next_up(float d) { return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, d) + 1u); }

// T against (kd (1 + rho) + e_q) / s in long double, and against the next kd
static void check_threshold(L1fQuant z, double rho, float kd, double eq) {
  const int32_t t = l1f_threshold(z, rho, kd, eq);
  const long double exact = ((long double)kd * (1.0L + (long double)rho) + (long double)eq) / (long double)z.s;
  check(t == kL1fAll || (long double)t >= exact, "T below the exact value", kd, eq);
  check(t >= 0 && t <= kL1fAll, "T out of range", kd, eq);
  check(l1f_threshold(z, rho, next_up(kd), eq) >= t, "T not monotone in kd", kd, eq);
}

// codes, the error bound e (+inf with a non-finite element) and E_x (-1: forced) as the scan computes them
static std::vector<uint8_t> encode(L1fQuant z, const std::vector<float>& v, int dim, double& e, int32_t& ex) {
  std::vector<uint8_t> c(v.size(), 0);
  double sum = 0.0;
  bool bad = false;
  for (int i = 0; i < dim; i++) {
    if (!l1f_finite(v[i])) bad = true;
    else sum += l1f_term(z, v[i], c[i] = (uint8_t)l1f_code(z, v[i]));
  }
  e = bad ? (double)__builtin_huge_valf() : l1f_err_up(z, sum, dim);
  ex = l1f_row_err(z, e);
  return c;
}

int main() {
  std::mt19937_64 rng(12345);
  std::uniform_real_distribution<double> u01(0.0, 1.0);
  long thresholds = 0, pairs = 0, rejected = 0;

  // ---- T: edges, then a random walk over magnitudes -------------------------
  const double rho = l1f_rho(256);
  for (int dp = 16; dp <= 256; dp += 16)  // m = dp / 8 + 3 roundings
    check((long double)l1f_rho(dp) >= powl(1.0L - 0x1p-24L, -(long double)(dp / 8 + 3)) - 1.0L, "rho covers the roundings",
          l1f_rho(dp), dp);
  const float kds[] = {0.0f, -0.0f, 0x1p-149f, 0x1p-126f, 1.0f, 3.0f, 1e10f, 3.0e38f};
  const double eqs[] = {0.0, 0x1p-1074, 1e-30, 0.5, 64.0, 1e20};
  const double ss[] = {0x1p-1074, 1e-300, 0x1p-149, 1e-3, 1.0, 7.8e15, 1e300};
  for (float kd : kds)
    for (double eq : eqs)
      for (double s : ss) check_threshold({0.0, s}, rho, kd, eq), thresholds++;
  const L1fQuant unit = {0.0, 1.0};
  check(l1f_threshold(unit, rho, __builtin_huge_valf(), 0.0) == kL1fAll, "inf kd", 0, 0);
  check(l1f_threshold(unit, rho, __builtin_nanf(""), 0.0) == kL1fAll, "NaN kd", 0, 0);
  check(l1f_threshold(unit, rho, 1.0f, (double)__builtin_huge_valf()) == kL1fAll, "inf e_q", 0, 0);
  check(l1f_threshold(unit, rho, 1.0f, (double)__builtin_nanf("")) == kL1fAll, "NaN e_q", 0, 0);
  check(l1f_threshold(unit, rho, -1.0f, 0.0) == l1f_threshold(unit, rho, 0.0f, 0.0), "negative kd", 0, 0);
  check(l1f_threshold(unit, rho, 0.0f, 0.0) >= 0 && l1f_threshold(unit, rho, 0.0f, 0.0) <= 2, "T(0, 0)", 0, 0);
  check(kL1fSadMax < kL1fErrCap && kL1fSadMax < kL1fAll && kL1fAll + kL1fEmax < kL1fNever && kL1fErrCap <= kL1fEmax,
        "sentinels", 0, 0);
  check(l1f_row_err(unit, (double)__builtin_huge_valf()) == -1 && l1f_row_err(unit, (double)__builtin_nanf("")) == -1 &&
            l1f_row_err(unit, 1e9) == -1 && l1f_row_err(unit, 0.0) >= 0,
        "forced rows", 0, 0);
  for (int it = 0; it < 400000; it++, thresholds++) {
    const double s = std::ldexp(1.0 + u01(rng), (int)(u01(rng) * 80) - 40);
    const float kd = (float)(s * std::ldexp(1.0 + u01(rng), (int)(u01(rng) * 24) - 6));
    const double eq = s * u01(rng) * std::ldexp(1.0, (int)(u01(rng) * 16) - 4);
    check_threshold({u01(rng) - 0.5, s}, l1f_rho(16 * (1 + it % 16)), kd, eq);
    const double e = eq * 3.0;  // E_x s >= e_x
    const int32_t ex = l1f_row_err({0.0, s}, e);
    check(ex == -1 || (long double)ex * (long double)s >= (long double)e, "E_x s below e_x", e, s);
  }

  // ---- the rule on coded vectors: rows in [0, 1) or small integers, an outlier and a non-finite row now and
  // then, queries inside and outside the range; kd every row's distance in turn
  for (int it = 0; it < 3000; it++) {
    const int dp = 16 * (1 + it % 3), dim = dp - (it % 5);
    const int nrows = 24;
    std::vector<std::vector<float>> rows(nrows, std::vector<float>(dp, 0.0f));
    float mn = 0, mx = 0;
    bool any = false;
    for (int r = 0; r < nrows; r++)
      for (int i = 0; i < dim; i++) {
        float v = it % 7 == 0 ? (float)(int)(u01(rng) * 4) : (float)u01(rng);
        if (it % 11 == 0 && r == 3) v *= 1e6f;
        if (it % 13 == 0 && r == 5 && i == 2) v = __builtin_huge_valf();
        rows[r][i] = v;
        if (l1f_finite(v)) {
          mn = any ? std::min(mn, v) : v;
          mx = any ? std::max(mx, v) : v;
          any = true;
        }
      }
    const L1fQuant z = l1f_quant(mn, mx, any);
    std::vector<float> q(dp, 0.0f);
    const double shift = it % 4 == 1 ? 5.0 : it % 4 == 2 ? -5.0 : 0.0;
    for (int i = 0; i < dim; i++) q[i] = it % 7 == 0 ? (float)(int)(u01(rng) * 4) : (float)(u01(rng) + shift);
    double eq, ex_e;
    int32_t ex;
    const std::vector<uint8_t> cq = encode(z, q, dim, eq, ex);
    float eqf = (float)eq;
    if ((double)eqf < eq) eqf = next_up(eqf);
    std::vector<float> dist(nrows);
    for (int r = 0; r < nrows; r++) dist[r] = l1f_comparator(q.data(), rows[r].data(), dp);
    for (int r = 0; r < nrows; r++) {
      const std::vector<uint8_t> cx = encode(z, rows[r], dim, ex_e, ex);
      int32_t sad = 0;
      for (int i = 0; i < dp; i++) sad += std::abs((int)cq[i] - (int)cx[i]);
      check(ex == -1 || (long double)ex * (long double)z.s >= (long double)ex_e, "E_x s below e_x", ex_e, z.s);
      for (int o = 0; o < nrows; o++, pairs++) {
        const float kd = dist[o];
        const int32_t t = l1f_threshold(z, l1f_rho(dp), kd, (double)eqf);
        const bool reject = ex >= 0 && sad > t + ex;
        rejected += reject;
        check(!reject || dist[r] > kd, "a rejected pair at or below kd", dist[r], kd);
      }
    }
  }
  printf("thresholds %ld pairs %ld rejected %ld failures %ld\n", thresholds, pairs, rejected, failures);
  return failures ? 1 : 0;
}
