// scan_l1f_wide.hip -- the exact batch scan of
// ObjectSpaceRepository::linearSearch (lib/NGT/ObjectSpaceRepository.h:466-502)
// for float rows under L1 with lists of up to 128 results: the byte-SAD filter
// of scan_l1f.hip (the rule and its proof: scan_l1f_bound.h) with the lists of
// the other wide scans.
//
// Shared with scan_l1f.hip, unchanged: the rows' image (codes and the bias
// column), the query encode (codes, e_q, the first threshold word), the rule
// "reject iff S' = bias + SAD > T_q + kL1fEmax" with T from l1f_threshold of
// the k-th REAL distance, dist_lane_l1 for whatever the rule cannot reject,
// ngt_scan_l1f_nan_kernel after the merge.
//
// Row side, scan_l1f.hip's: a wave is a workgroup with up to 128 queries x one
// contiguous part of the rows (at most 1024 tiles: a row's offset in the part
// takes 16 bits), 64-row tiles, lane = row, the code row in VGPRs with the
// next tile's loading behind it, the query code words through the scalar cache
// into the scalar operand of v_sad_u8, the accumulator started from the bias,
// T_q + kL1fEmax in VGPRs, query q in lane q & 63.
//
// What differs is what happens to a survivor.  In the byte scans a survivor's
// integer sum is its distance; here it is only a candidate that needs the
// comparator over a 4 Dp-byte float row from HBM.  Nothing in LDS grows with k:
//  * Pending slots: a (tile, query) survivor is appended to the query's 32
//    slots in LDS, 16 bits each, the row's offset in the part (8 KiB a wave).
//    S' is not kept: it only ever ordered work.
//  * A round runs for one query when its slots are full (a tile's up to 64
//    survivors take two), and for every query with pending entries at the
//    part's end.  Lane i takes entry i and evaluates dist_lane_l1, the float
//    row from HBM, the query's float row through the scalar cache -- it is
//    wave-uniform for the whole round, which is why a round serves one query,
//    and the round's up to 32 row reads are in flight together.  Then the
//    radius rule (radius < 0 || (double)d <= radius), make_key, the key
//    against the k-th key.
//  * Lists: the (query, part) list lives in its slot of the partial buffer,
//    sorted keys make_key(distance, id), ~0 beyond its length from the start.
//    A round loads it two keys per lane; list keys and surviving candidates go
//    to their places by ballot rank (candidate: list keys below it + candidates
//    below it; list key: its index + candidates below it), only entries that
//    moved and land below k are stored.  Keys are distinct (ids are), so the
//    places are a permutation.  Agent-scope relaxed atomics, s_waitcnt vmcnt(0)
//    after a round's stores, no barrier: the wave is the list's only reader
//    and writer.  ngt_linear_merge_kernel merges the parts.
//  * When a key moves to the k-th place, T_q is tightened with
//    l1f_threshold(z, rho, key_dist(kth), e_q); a NaN k-th key gives kL1fAll,
//    no bound.  Until the list is full T_q keeps its start value (the largest,
//    or the radius'), so the first ceil(k / 64) tiles of a part go wholly
//    through rounds.  What is left of a tile's mask after a round is filtered
//    again with the new T_q.
//  * Stale thresholds: between rounds the word in the VGPR is up to 31
//    candidates behind the list.  A stale T_q is a larger T_q: it passes more
//    pairs, never fewer, and every T_q ever used comes from k real distances
//    of this query, so the strictness argument of scan_l1f_bound.h is
//    untouched and no new pure rule is needed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "ngt_device.h"
#include "ngt_kernels.h"
#include "scan_l1f_bound.h"
#include "scan_mfma_common.h"

namespace ngt_amd {

typedef uint32_t lw_u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) uint32_t* lw_const_words;  // read through the scalar cache
typedef const __attribute__((address_space(4))) float* lw_const_floats;

constexpr uint32_t kLwQ = 128;  // queries per wave
constexpr uint32_t kLwP = 32;   // pending slots per query

__device__ __forceinline__ uint64_t lw_readlane(uint64_t v, uint32_t l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l);
  return ((uint64_t)hi << 32) | lo;
}

template <int NC>
__global__ void __launch_bounds__(64) ngt_scan_l1f_wide_kernel(L1fScanArgs a) {
  __shared__ uint16_t pend[kLwQ * kLwP];  // a candidate row's offset in the part
  const uint32_t lane = threadIdx.x, k = a.k;
  const uint32_t mb = blockIdx.x / a.nparts, part = blockIdx.x % a.nparts;
  const uint32_t q0 = mb * kLwQ;
  const uint32_t nqb = a.nq - q0 < kLwQ ? a.nq - q0 : kLwQ;
  const uint32_t t0 = part * a.tiles_per_part;
  const uint32_t t1 = t0 + a.tiles_per_part < a.ntiles ? t0 + a.tiles_per_part : a.ntiles;
  const uint32_t row0 = t0 * 64;  // pending rows are offsets from here
  const uint64_t lt = (1ull << lane) - 1;
  const L1fQuant z = {a.lo, a.s};
  const double rho = l1f_rho(a.dp);

  // the list of the wave's query q in this part
  auto list_of = [&](uint32_t q) -> uint64_t* { return a.partial + ((uint64_t)(q0 + q) * a.nparts + part) * k; };

  // empty lists: all ones, which is also what the merge expects beyond a list's length
  for (uint32_t q = 0; q < nqb; q++) {
    uint64_t* L = list_of(q);
    for (uint32_t i = lane; i < k; i += 64) __hip_atomic_store(L + i, ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // of query h * 64 + lane (the arrays are padded to whole blocks): T_q +
  // kL1fEmax, e_q, the pending count
  uint32_t tt[2], cnt[2] = {0, 0};
  float eqv[2];
#pragma unroll
  for (int h = 0; h < 2; h++) {
    tt[h] = a.tt0[q0 + 64u * h + lane];
    eqv[h] = a.eq[q0 + 64u * h + lane];
  }
  lw_const_words qwords = (lw_const_words)(uintptr_t)(a.qcodes + (uint64_t)q0 * (NC * 4));

  // a lane's code row and bias of tile t (the image is padded to whole tiles)
  auto load_tile = [&](uint32_t t, lw_u32x4 (&dst)[NC], uint32_t& bias) {
    const uint64_t id = (uint64_t)t * 64 + lane;
    const lw_u32x4* p = reinterpret_cast<const lw_u32x4*>(a.codes) + id * NC;
#pragma unroll
    for (int c = 0; c < NC; c++) dst[c] = p[c];
    bias = (uint32_t)a.bias[id];
  };

  // A round: the first n pending entries of query q into its list; ttv and
  // eqr are the VGPRs that hold q's threshold word and e_q.
  auto process = [&](uint32_t q, uint32_t n, uint32_t& ttv, float eqr) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the slots' writes, other lanes' included
    uint64_t* L = list_of(q);
    // the list, two keys per lane
    const uint64_t l0 = lane < k ? __hip_atomic_load(L + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ~0ull;
    const uint64_t l1 =
        lane + 64 < k ? __hip_atomic_load(L + lane + 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ~0ull;
    // lane i: the comparator's distance of pending entry i, the radius rule of
    // the quad kernel, the key against the k-th key
    lw_const_floats qf = (lw_const_floats)(uintptr_t)(a.queries + (uint64_t)(q0 + q) * a.query_bytes);
    uint64_t key = ~0ull;
    bool in = false;
    if (lane < n) {
      const uint32_t id = row0 + pend[q * kLwP + lane];
      const float d = dist_lane_l1(qf, reinterpret_cast<const float*>(a.rows + (uint64_t)id * a.row_bytes), a.dp);
      in = a.radius < 0.0 || (double)d <= a.radius;
      key = make_key(d, id);
    }
    if (a.stats != nullptr && lane == 0) {
      atomicAdd(&a.stats[0], (unsigned long long)n);
      atomicAdd(&a.stats[1], 1ull);
    }
    const uint32_t c = (uint32_t)(__popcll(__ballot(l0 != ~0ull)) + __popcll(__ballot(l1 != ~0ull)));
    const uint64_t th = k <= 64 ? lw_readlane(l0, k - 1) : lw_readlane(l1, k - 65);  // ~0 until the list is full
    const bool ok = in && key < th;
    // list keys below each survivor, survivors below each survivor and below each list key
    const uint64_t surv = __ballot(ok);
    if (surv == 0) return;
    uint32_t lb = 0, sb = 0, a0 = 0, a1 = 0;
    for (uint64_t m = surv; m; m &= m - 1) {
      const uint32_t j = (uint32_t)__ffsll((long long)m) - 1;
      const uint64_t sk = lw_readlane(key, j);
      const uint64_t b0 = __ballot(l0 < sk), b1 = __ballot(l1 < sk);
      if (lane == j) lb = (uint32_t)(__popcll(b0) + __popcll(b1));
      sb += sk < key ? 1u : 0u;
      a0 += sk < l0 ? 1u : 0u;
      a1 += sk < l1 ? 1u : 0u;
    }
    // the places are a permutation of 0 .. c + survivors - 1; a list key that
    // no survivor precedes stays where it is, places from k on drop out
    const bool ws = ok && lb + sb < k;
    const bool w0 = lane < c && a0 != 0 && lane + a0 < k;
    const bool w1 = lane + 64 < c && a1 != 0 && lane + 64 + a1 < k;
    if (ws) __hip_atomic_store(L + lb + sb, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (w0) __hip_atomic_store(L + lane + a0, l0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (w1) __hip_atomic_store(L + lane + 64 + a1, l1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // the new k-th key, if a key moved to the last place (an entry that stays
    // there leaves the threshold as it is): k real distances, the header's rule
    const uint64_t bs = __ballot(ws && lb + sb == k - 1);
    const uint64_t bl0 = __ballot(w0 && lane + a0 == k - 1), bl1 = __ballot(w1 && lane + 64 + a1 == k - 1);
    uint64_t kth = ~0ull;
    if (bs) kth = lw_readlane(key, (uint32_t)__ffsll((long long)bs) - 1);
    else if (bl0) kth = lw_readlane(l0, (uint32_t)__ffsll((long long)bl0) - 1);
    else if (bl1) kth = lw_readlane(l1, (uint32_t)__ffsll((long long)bl1) - 1);
    if (kth != ~0ull) {
      const float eq = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(eqr), (int)(q & 63)));
      const uint32_t tn = (uint32_t)(l1f_threshold(z, rho, key_dist(kth), (double)eq) + kL1fEmax);
      if (lane == (q & 63) && tn < ttv) ttv = tn;
    }
    // the round's stores land before a later round loads the list
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  };

  // Survivors m of query q (tile offset toff, S: the lanes' S') into its
  // pending slots.  Full slots are merged at once, and the rest of the mask
  // meets the threshold the round left.
  auto insert = [&](uint32_t q, uint64_t m, uint32_t S, uint32_t toff, uint32_t& ttv, float eqr, uint32_t& cntv) {
    uint32_t n = (uint32_t)__builtin_amdgcn_readlane((int)cntv, (int)(q & 63));
    while (m) {
      const uint32_t slot = n + (uint32_t)__popcll(m & lt);
      const bool mine = ((m >> lane) & 1) != 0 && slot < kLwP;
      if (mine) pend[q * kLwP + slot] = (uint16_t)(toff + lane);
      const uint64_t took = __ballot(mine);
      n += (uint32_t)__popcll(took);
      m &= ~took;
      if (n == kLwP) {
        process(q, kLwP, ttv, eqr);
        n = 0;
        if (m) m &= __ballot(S <= (uint32_t)__builtin_amdgcn_readlane((int)ttv, (int)(q & 63)));
      }
    }
    if (lane == (q & 63)) cntv = n;
  };

  // the loads of tile t + 1 are in flight while tile t is compared
  lw_u32x4 cur[NC], nxt[NC];
  uint32_t bias_nxt = (uint32_t)kL1fNever;
  if (t0 < t1) load_tile(t0, nxt, bias_nxt);
  for (uint32_t t = t0; t < t1; t++) {
#pragma unroll
    for (int c = 0; c < NC; c++) cur[c] = nxt[c];
    const uint32_t bias = bias_nxt;
    if (t + 1 < t1) load_tile(t + 1, nxt, bias_nxt);
    if (__ballot(bias != (uint32_t)kL1fNever) == 0) continue;
    const uint32_t toff = (t - t0) * 64;
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const uint32_t nh = nqb > 64u * h ? (nqb - 64u * h < 64u ? nqb - 64u * h : 64u) : 0u;
      for (uint32_t ql = 0; ql < nh; ql++) {
        lw_const_words qw = qwords + (64u * h + ql) * (NC * 4);
        uint32_t S = bias;
#pragma unroll
        for (int c = 0; c < NC; c++)
#pragma unroll
          for (int j = 0; j < 4; j++) S = __builtin_amdgcn_sad_u8(cur[c][j], qw[c * 4 + j], S);
        const uint32_t tq = (uint32_t)__builtin_amdgcn_readlane((int)tt[h], (int)ql);
        const uint64_t m = __ballot(S <= tq);
        if (m) insert(64u * h + ql, m, S, toff, tt[h], eqv[h], cnt[h]);
      }
    }
  }
  // what is still pending at the part's end; the lists are in place
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const uint32_t nh = nqb > 64u * h ? (nqb - 64u * h < 64u ? nqb - 64u * h : 64u) : 0u;
    for (uint32_t ql = 0; ql < nh; ql++) {
      const uint32_t n = (uint32_t)__builtin_amdgcn_readlane((int)cnt[h], (int)ql);
      if (n) process(64u * h + ql, n, tt[h], eqv[h]);
    }
  }
}

// Waves per SIMD that the kernel's VGPRs allow (compiler
// figures), four at the most: the grid is one resident set.
uint32_t scan_l1f_wide_waves(int dp) { return dp > 128 ? 2 : 4; }

hipError_t launch_scan_l1f_wide(const L1fScanArgs& a, hipStream_t s) {
  if (a.k == 0 || a.k > 128 || a.nparts == 0 || a.mblocks == 0 || a.dp < 16 || a.dp > 256 || a.dp % 16 != 0 ||
      a.tiles_per_part > kL1fWideMaxTiles || (uint64_t)a.nparts * a.tiles_per_part < a.ntiles)
    return hipErrorNotSupported;
  const dim3 grid(a.nparts * a.mblocks), block(64);
  switch (scan_bytes_chunks(a.dp)) {
    case 1: hipLaunchKernelGGL(ngt_scan_l1f_wide_kernel<1>, grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL(ngt_scan_l1f_wide_kernel<2>, grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL(ngt_scan_l1f_wide_kernel<4>, grid, block, 0, s, a); break;
    case 8: hipLaunchKernelGGL(ngt_scan_l1f_wide_kernel<8>, grid, block, 0, s, a); break;
    case 16: hipLaunchKernelGGL(ngt_scan_l1f_wide_kernel<16>, grid, block, 0, s, a); break;
    default: return hipErrorNotSupported;
  }
  return hipGetLastError();
}

}  // namespace ngt_amd
