// scan_l1f.hip -- the exact batch scan of ObjectSpaceRepository::linearSearch
// (lib/NGT/ObjectSpaceRepository.h:466-502) for float rows under L1: a filter
// on the VALU's packed byte-SAD over one-byte codes of rows and queries, and
// the comparator's own float arithmetic for the few pairs it cannot reject.
//
// L1 has no dot-product form, so the matrix cores cannot bound it; v_sad_u8
// can, four dimensions per instruction.  scan_l1f_bound.h proves the rule:
// with S = SAD(c_q, c_x), a pair with S > T_q + E_x has a reference float
// distance strictly above the query's k-th distance.  Everything else is a
// candidate and gets dist_lane_l1, bit for bit dist_f32<kL1>.
//
// Work, as in scan_bytes.hip: a wave is a workgroup.  It owns up to 128
// queries x one contiguous part of the rows and walks it in 64-row tiles,
// lane = row.
//  * Rows: a lane keeps its code row in VGPRs (NC x global_load_dwordx4), the
//    next tile's row in a second set, loaded before the current tile is
//    compared, and with it the row's bias: kL1fEmax - E_x, 0 for a forced
//    row, kL1fNever for removed rows, the dummy row 0 and tile padding.
//  * Queries: the zero-padded code copy comes through the scalar cache
//    straight into the scalar operand of v_sad_u8.
//  * The accumulator starts from the bias: S' = bias + SAD, survivor iff
//    S' <= T_q + kL1fEmax -- the per-row correction costs nothing, a forced
//    row passes every threshold and a removed one none.  The thresholds live
//    in VGPRs, query q in lane q & 63.
//  * Survivors: lane j takes survivor j (ranks through 64 words of LDS) and
//    evaluates the comparator alone, the float row from HBM, the query's
//    float row through the scalar cache: it is wave-uniform and read-only, a
//    (tile, query) with survivors has one or two of them, and staging 4 Dp
//    bytes in LDS per such pair would move more than the recompute reads.
//    Then the radius rule, make_key, insertion by ballot rank into the
//    query's sorted k-list (LDS [128][k]), and T_q from the new k-th distance.
//  * A (tile, query) with more than k survivors (the first tile of a part
//    passes all 64 rows): the k smallest S' first (the bit-by-bit k-th
//    smallest of scan_bytes.hip), T_q from their k real distances, the rest
//    of the mask filtered again.  S' only orders the work: nothing is dropped
//    before a threshold derived from k real distances exists.
// A part with fewer than k accepted rows leaves ~0 in its list; the parts are
// merged by ngt_linear_merge_kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "ngt_device.h"
#include "ngt_kernels.h"
#include "scan_l1f_bound.h"
#include "scan_mfma_common.h"

namespace ngt_amd {

typedef uint32_t lf_u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) uint32_t* lf_const_words;  // read through the scalar cache
typedef const __attribute__((address_space(4))) float* lf_const_floats;

constexpr uint32_t kLfQ = 128;  // queries per wave

// ---- the quantiser's range ---------------------------------------------------
__global__ void __launch_bounds__(256) ngt_scan_l1f_range_kernel(const uint8_t* __restrict__ rows, uint64_t row_bytes,
                                                                 uint64_t nrows, const uint8_t* __restrict__ valid,
                                                                 int dim, uint32_t* __restrict__ mm) {
  uint32_t lo = ~0u, hi = 0u;
  const uint64_t total = nrows * (uint64_t)dim;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
    const uint64_t r = i / (uint32_t)dim;
    const uint32_t c = (uint32_t)(i - r * (uint32_t)dim);
    if (r == 0 || (valid != nullptr && !valid[r])) continue;
    const float v = reinterpret_cast<const float*>(rows + r * row_bytes)[c];
    if (!l1f_finite(v)) continue;
    const uint32_t o = ord_of(v);
    lo = o < lo ? o : lo;
    hi = o > hi ? o : hi;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint32_t l2 = (uint32_t)__shfl_xor((int)lo, o, 64), h2 = (uint32_t)__shfl_xor((int)hi, o, 64);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  if ((threadIdx.x & 63) == 0 && lo <= hi) {
    atomicMin(&mm[0], lo);
    atomicMax(&mm[1], hi);
  }
}

// ---- codes, biases and query bounds -----------------------------------------
// A thread codes one 16-column chunk of one vector; the NC threads of a vector
// are neighbours in a wave and fold their error sums by shuffles.
template <bool QUERY>
__global__ void __launch_bounds__(256) ngt_scan_l1f_encode_kernel(L1fEncodeArgs a, uint32_t nc) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n_pad * nc) return;  // whole waves: n_pad is a multiple of 64
  const uint64_t r = i / nc;
  const uint32_t c = (uint32_t)(i - r * nc);
  const L1fQuant z = {a.lo, a.s};
  const bool live = r < a.n && (QUERY || (r >= 1 && (a.valid == nullptr || a.valid[r])));
  uint32_t w[4] = {0, 0, 0, 0};
  double sum = 0.0;
  int bad = 0;
  if (live && (int)(c * 16) < a.dp) {
    const float4* p = reinterpret_cast<const float4*>(a.src + r * a.stride) + 4 * c;
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const float4 f = p[g];
      const float v[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if ((int)(c * 16) + 4 * g + j >= a.dim) continue;
        if (!l1f_finite(v[j])) {
          bad = 1;
          continue;
        }
        const uint32_t code = l1f_code(z, v[j]);
        sum += l1f_term(z, v[j], code);
        w[g] |= code << (8 * j);
      }
    }
  }
  for (uint32_t o = 1; o < nc; o <<= 1) {
    sum += __shfl_xor(sum, (int)o, 64);
    bad |= __shfl_xor(bad, (int)o, 64);
  }
  lf_u32x4 out = {w[0], w[1], w[2], w[3]};
  reinterpret_cast<lf_u32x4*>(a.codes)[i] = out;
  if (c != 0) return;
  const double e = bad ? (double)__builtin_huge_valf() : l1f_err_up(z, sum, a.dim);
  if constexpr (QUERY) {
    float ef = (float)e;  // rounded up; +inf: everything is a candidate
    if ((double)ef < e) ef = __uint_as_float(__float_as_uint(ef) + 1u);
    a.eq[r] = live ? ef : 0.0f;
    a.tt0[r] = (uint32_t)(l1f_threshold(z, l1f_rho(a.dp), a.kd_init, (double)ef) + kL1fEmax);
  } else {
    const int32_t ex = l1f_row_err(z, e);
    a.bias[r] = !live ? kL1fNever : ex < 0 ? 0 : kL1fEmax - ex;
  }
}

// ---- queries with a NaN element ----------------------------------------------
// Such a query's distance to every row is NaN (the NaN poisons its AVX lane
// and the fold), and no comparison orders NaNs: linearSearch's bounded
// max-heap (push, pop when over k, drain; restated in oracle/ngt_oracle.c)
// then keeps its second to k-th pushes in place and replaces its root with
// every later push.  Over the live rows l_1 < l_2 < ... < l_m in id order
// (radius < 0; with a radius no NaN passes) the result is l_2 .. l_k, l_m
// when m > k and l_2 .. l_m, l_1 otherwise.  The scan below ranks NaN keys by
// id (l_1 .. l_k, the count and the distances are right); this kernel, a wave
// per query after the merge, rewrites the ids of those queries.
__global__ void __launch_bounds__(64) ngt_scan_l1f_nan_kernel(const uint8_t* __restrict__ queries, uint64_t query_bytes,
                                                               int dp, const int32_t* __restrict__ bias,
                                                               uint32_t ntiles, uint32_t k,
                                                               uint32_t* __restrict__ out_ids, uint32_t out_stride) {
  const uint32_t lane = threadIdx.x;
  const float* qf = reinterpret_cast<const float*>(queries + (uint64_t)blockIdx.x * query_bytes);
  bool nan = false;
  for (int i = (int)lane; i < dp; i += 64) nan |= qf[i] != qf[i];
  if (__ballot(nan) == 0) return;
  uint32_t* out = out_ids + (uint64_t)blockIdx.x * out_stride;
  uint32_t count = 0, first = 0, kth = 0;  // rows taken, l_1, the last one taken
  for (uint32_t t = 0; t < ntiles && count < k; t++) {
    const uint32_t id = t * 64 + lane;
    const bool live = bias[id] != kL1fNever;
    const uint64_t m = __ballot(live);
    const uint32_t r = count + mbcnt(m);  // rank in id order, from 0
    const uint64_t take = __ballot(live && r < k);
    if (take == 0) continue;
    if (live && r >= 1 && r < k) out[r - 1] = id;
    if (count == 0) first = t * 64 + (uint32_t)__ffsll((long long)take) - 1;
    kth = t * 64 + 63 - (uint32_t)__builtin_clzll(take);
    count += (uint32_t)__popcll(take);
  }
  if (count == 0) return;
  uint32_t last = kth;
  for (uint32_t t = ntiles; t-- > 0;) {
    const uint64_t m = __ballot(bias[t * 64 + lane] != kL1fNever);
    if (m) {
      last = t * 64 + 63 - (uint32_t)__builtin_clzll(m);
      break;
    }
  }
  if (lane == 0) out[count - 1] = last > kth ? last : first;
}

__device__ __forceinline__ uint64_t lf_readlane(uint64_t v, uint32_t l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l);
  return ((uint64_t)hi << 32) | lo;
}

// ---- the scan ------------------------------------------------------------------
template <int NC>
__global__ void __launch_bounds__(64) ngt_scan_l1f_kernel(L1fScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint64_t* lists = reinterpret_cast<uint64_t*>(smem);          // [128][k] keys ascending, ~0 = empty
  const uint32_t lane = threadIdx.x, k = a.k;
  uint32_t* sel = reinterpret_cast<uint32_t*>(lists + kLfQ * k);  // [64] survivor rank -> lane
  const uint32_t mb = blockIdx.x / a.nparts, part = blockIdx.x % a.nparts;
  const uint32_t q0 = mb * kLfQ;
  const uint32_t nqb = a.nq - q0 < kLfQ ? a.nq - q0 : kLfQ;
  const uint32_t t0 = part * a.tiles_per_part;
  const uint32_t t1 = t0 + a.tiles_per_part < a.ntiles ? t0 + a.tiles_per_part : a.ntiles;
  for (uint32_t i = lane; i < nqb * k; i += 64) lists[i] = ~0ull;
  __syncthreads();
  const L1fQuant z = {a.lo, a.s};
  const double rho = l1f_rho(a.dp);
  // T_q + kL1fEmax and e_q of query h * 64 + lane (the arrays are padded to whole blocks)
  uint32_t tt[2];
  float eqv[2];
#pragma unroll
  for (int h = 0; h < 2; h++) {
    tt[h] = a.tt0[q0 + 64u * h + lane];
    eqv[h] = a.eq[q0 + 64u * h + lane];
  }
  lf_const_words qwords = (lf_const_words)(uintptr_t)(a.qcodes + (uint64_t)q0 * (NC * 4));

  // a lane's code row and bias of tile t (the image is padded to whole tiles)
  auto load_tile = [&](uint32_t t, lf_u32x4 (&dst)[NC], uint32_t& bias) {
    const uint64_t id = (uint64_t)t * 64 + lane;
    const lf_u32x4* p = reinterpret_cast<const lf_u32x4*>(a.codes) + id * NC;
#pragma unroll
    for (int c = 0; c < NC; c++) dst[c] = p[c];
    bias = (uint32_t)a.bias[id];
  };

  // The survivors m of query q in tile t (S: the lanes' S'): recomputed,
  // inserted, and the query's threshold word tq tightened.
  auto process = [&](uint32_t q, uint64_t m, uint32_t S, uint32_t t, uint32_t& tq, float eq) {
    uint64_t* L = lists + q * k;
    uint64_t e = lane < k ? L[lane] : ~0ull;
    lf_const_floats qf = (lf_const_floats)(uintptr_t)(a.queries + (uint64_t)(q0 + q) * a.query_bytes);
    if (a.stats != nullptr && lane == 0) atomicAdd(&a.stats[1], 1ull);

    auto recompute = [&](uint64_t mm) {
      const uint32_t cnt = (uint32_t)__popcll(mm);
      if ((mm >> lane) & 1) sel[mbcnt(mm)] = lane;
      __syncthreads();
      float d = 0.0f;
      uint32_t id = 0;
      if (lane < cnt) {
        id = t * 64 + sel[lane];
        d = dist_lane_l1(qf, reinterpret_cast<const float*>(a.rows + (uint64_t)id * a.row_bytes), a.dp);
      }
      __syncthreads();
      if (a.stats != nullptr && lane == 0) atomicAdd(&a.stats[0], (unsigned long long)cnt);
      // (radius < 0 || d <= radius) of the quad kernel, then the k best (d, id)
      const bool ok = lane < cnt && (a.radius < 0.0 || (double)d <= a.radius);
      const uint64_t key = make_key(d, id);
      uint64_t kth = lf_readlane(e, k - 1);
      uint64_t c = __ballot(ok && key < kth);
      while (c) {
        const uint32_t j = (uint32_t)__ffsll((long long)c) - 1;
        c &= c - 1;
        const uint64_t kj = lf_readlane(key, j);
        if (kj >= kth) continue;
        // kj < kth <= e[k - 1]: the rank is below k, the k-th entry drops out
        const uint32_t pos = (uint32_t)__popcll(__ballot(e < kj));
        const uint32_t ulo = (uint32_t)__shfl_up((int)(uint32_t)e, 1, 64);
        const uint32_t uhi = (uint32_t)__shfl_up((int)(uint32_t)(e >> 32), 1, 64);
        const uint64_t up = ((uint64_t)uhi << 32) | ulo;
        if (lane < k && lane >= pos) e = lane == pos ? kj : up;
        kth = lf_readlane(e, k - 1);
      }
      if (kth != ~0ull) {  // k real distances: the header's rule (NaN: no bound)
        const uint32_t tn = (uint32_t)(l1f_threshold(z, rho, key_dist(kth), (double)eq) + kL1fEmax);
        if (tn < tq) tq = tn;
      }
    };

    uint64_t rest = 0;
    if ((uint32_t)__popcll(m) > k) {
      // the k-th smallest S' of the survivors: the largest T with fewer than
      // k survivors below it (S' <= kL1fAll + kL1fEmax = 2^18)
      uint32_t T = 0;
      for (int b = 18; b >= 0; b--) {
        const uint32_t cand = T | (1u << b);
        if ((uint32_t)__popcll(__ballot(S < cand) & m) < k) T = cand;
      }
      const uint64_t first = m & __ballot(S <= T);
      rest = m & ~first;
      m = first;
    }
    recompute(m);
    if (rest) {
      rest &= __ballot(S <= tq);
      if (rest) recompute(rest);
    }
    if (lane < k) L[lane] = e;
  };

  // the loads of tile t + 1 are in flight while tile t is compared
  lf_u32x4 cur[NC], nxt[NC];
  uint32_t bias_nxt = (uint32_t)kL1fNever;
  if (t0 < t1) load_tile(t0, nxt, bias_nxt);
  for (uint32_t t = t0; t < t1; t++) {
#pragma unroll
    for (int c = 0; c < NC; c++) cur[c] = nxt[c];
    const uint32_t bias = bias_nxt;
    if (t + 1 < t1) load_tile(t + 1, nxt, bias_nxt);
    if (__ballot(bias != (uint32_t)kL1fNever) == 0) continue;
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const uint32_t nh = nqb > 64u * h ? (nqb - 64u * h < 64u ? nqb - 64u * h : 64u) : 0u;
      for (uint32_t ql = 0; ql < nh; ql++) {
        lf_const_words qw = qwords + (64u * h + ql) * (NC * 4);
        uint32_t S = bias;
#pragma unroll
        for (int c = 0; c < NC; c++)
#pragma unroll
          for (int j = 0; j < 4; j++) S = __builtin_amdgcn_sad_u8(cur[c][j], qw[c * 4 + j], S);
        uint32_t tq = (uint32_t)__builtin_amdgcn_readlane((int)tt[h], (int)ql);
        const uint64_t m = __ballot(S <= tq);
        if (m) {
          const float eq = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(eqv[h]), (int)ql));
          process(64u * h + ql, m, S, t, tq, eq);
          if (lane == ql) tt[h] = tq;
        }
      }
    }
  }
  __syncthreads();
  for (uint32_t i = lane; i < nqb * k; i += 64) {
    const uint32_t ql = i / k, rr = i - ql * k;
    a.partial[((uint64_t)(q0 + ql) * a.nparts + part) * k + rr] = lists[i];
  }
}

hipError_t launch_scan_l1f_range(const uint8_t* rows, uint64_t row_bytes, uint64_t nrows, const uint8_t* valid,
                                 int dim, uint32_t* mm, hipStream_t s) {
  const uint64_t total = nrows * (uint64_t)dim;
  const uint64_t blocks = std::max<uint64_t>(1, std::min<uint64_t>((total + 255) / 256, 4096));
  hipLaunchKernelGGL(ngt_scan_l1f_range_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, rows, row_bytes, nrows, valid,
                     dim, mm);
  return hipGetLastError();
}

float scan_l1f_range_value(uint32_t o) {
  const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;  // float_of_ord on the host
  return __builtin_bit_cast(float, u);
}

hipError_t launch_scan_l1f_encode(const L1fEncodeArgs& a, bool query, hipStream_t s) {
  if (a.n_pad % 64 != 0 || a.dp <= 0 || a.dp > 256 || a.dp % 16 != 0 || a.dim > a.dp) return hipErrorNotSupported;
  const uint32_t nc = (uint32_t)scan_bytes_chunks(a.dp);
  const uint64_t blocks = (a.n_pad * nc + 255) / 256;
  if (blocks == 0) return hipSuccess;
  if (query) hipLaunchKernelGGL(ngt_scan_l1f_encode_kernel<true>, dim3((uint32_t)blocks), dim3(256), 0, s, a, nc);
  else hipLaunchKernelGGL(ngt_scan_l1f_encode_kernel<false>, dim3((uint32_t)blocks), dim3(256), 0, s, a, nc);
  return hipGetLastError();
}

hipError_t launch_scan_l1f(const L1fScanArgs& a, hipStream_t s) {
  if (a.k == 0 || a.k > 16 || a.nparts == 0 || a.mblocks == 0 || a.dp > 256 || a.dp % 16 != 0) return hipErrorNotSupported;
  const dim3 grid(a.nparts * a.mblocks), block(64);
  const size_t lds = (size_t)kLfQ * a.k * 8 + 64 * 4;
  switch (scan_bytes_chunks(a.dp)) {
    case 1: hipLaunchKernelGGL(ngt_scan_l1f_kernel<1>, grid, block, lds, s, a); break;
    case 2: hipLaunchKernelGGL(ngt_scan_l1f_kernel<2>, grid, block, lds, s, a); break;
    case 4: hipLaunchKernelGGL(ngt_scan_l1f_kernel<4>, grid, block, lds, s, a); break;
    case 8: hipLaunchKernelGGL(ngt_scan_l1f_kernel<8>, grid, block, lds, s, a); break;
    case 16: hipLaunchKernelGGL(ngt_scan_l1f_kernel<16>, grid, block, lds, s, a); break;
    default: return hipErrorNotSupported;
  }
  return hipGetLastError();
}

hipError_t launch_scan_l1f_nan(const L1fScanArgs& a, uint32_t* out_ids, uint32_t out_stride, hipStream_t s) {
  hipLaunchKernelGGL(ngt_scan_l1f_nan_kernel, dim3(a.nq), dim3(64), 0, s, a.queries, a.query_bytes, a.dp, a.bias, a.ntiles,
                     a.k, out_ids, out_stride);
  return hipGetLastError();
}

}  // namespace ngt_amd
