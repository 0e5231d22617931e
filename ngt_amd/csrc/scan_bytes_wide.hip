// scan_bytes_wide.hip -- the exact batch scan of
// ObjectSpaceRepository::linearSearch (lib/NGT/ObjectSpaceRepository.h:466-502)
// for uint8 rows under L1, Hamming and Jaccard with lists of 1 .. 128 results,
// on the VALU's packed byte-SAD and popcount.
//
// L1 / Hamming: scan_bytes.hip's arithmetic.  S is an integer below 2^24, the
// comparator's distance is exactly (float)S, the rank key is (S, id).
//
// Jaccard (compareJaccardDistance, restated in ngt_device.h): c = popcount(q & x),
// de = popcount(q | x) = |x| + |q| - c, distance (float)(1.0 - (double)c / (double)de).
// A pair costs only c; |x| is the popcount of the lane's row, taken once when
// the row arrives in registers, |q| comes from the prepared queries.
//  * The rule, and its domain de <= 2048 (padded rows of at most 256 bytes):
//    two distinct ratios c/de with denominators up to 2048 differ by at least
//    2^-22, and over all 1,275,587 distinct ratios with 0 <= c <= de <= 2048
//    (float)(1.0 - c/de) is strictly monotone (checked exhaustively on the
//    CPU; at de <= 8192 it is not).  So ranking by (float distance, id) is
//    ranking by (ratio descending, id), and the filter is the integer compare
//    c de_k > c_k de, or equal and id < id_k, against the query's k-th entry
//    (products below 2^23).  The double division is done only for entries
//    that reach a list, to form the output float and its key.
//  * The k-th entry's (c_k, de_k) is not stored: it is found again from its
//    float d_k.  rho' = 1.0 - (double)d_k is within 2^-25 of c_k/de_k, every
//    other ratio is at least 2^-22 - 2^-25 away, so the one de in 1 .. 2048
//    with |rint(rho' de) - rho' de| <= de 2^-24 names it (32 steps of the wave).
//  * de = 0 (an all-zero query against an all-zero live row) is NaN in the
//    comparator: the host does not launch this kernel for a table with such a
//    row.  Removed rows, the dummy row 0 and padding never pass the filter.
//
// Work: a wave is a workgroup, as in scan_bytes.hip.  It owns up to 128
// queries x one contiguous part of the rows (at most 1024 tiles: a row's
// offset in the part takes 16 bits) and walks it in 64-row tiles, lane = row.
//  * Rows: the lane's whole row in VGPRs (NC x global_load_dwordx4), the next
//    tile's row loading behind it.  Queries: the zero-padded copy through the
//    scalar cache into the scalar operand of v_sad_u8 / v_xor_b32 / v_and_b32.
//  * Filter thresholds: query q's k-th entry in lane q & 63 of two VGPR pairs
//    (v_readlane), (S_k << 32 | id_k) or (c_k << 48 | de_k << 32 | id_k); the
//    radius' bound until the list is full.  |q| and the pending counts are
//    kept the same way.
//  * Survivors go to the query's 16 pending slots in LDS, (S or c) << 16 | row
//    offset, Jaccard's de in a second 16-bit array: 8 KiB a wave (12 KiB for
//    Jaccard), whatever k.  A query whose slots are full is merged at once; a
//    tile's up to 64 survivors take several such rounds.  The thresholds are
//    therefore up to 15 entries stale: a stale threshold passes more, never less.
//  * Lists: the (query, part) list lives in its slot of the partial buffer,
//    sorted u64 keys make_key(distance, id), ~0 beyond its length, written
//    with ~0 at the start.  A round loads it two keys per lane, lane c
//    finishes pending entry c (distance, radius rule, key against the k-th
//    key), and list keys and survivors go to their places by ballot rank
//    (agent-scope relaxed atomics, s_waitcnt vmcnt(0) after a round's stores;
//    the wave is the list's only reader and writer).  Keys are distinct (ids
//    are), so the places are a permutation.  ngt_linear_merge_kernel merges
//    the parts.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "ngt_device.h"
#include "ngt_kernels.h"

namespace ngt_amd {

typedef uint32_t bw_u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) uint32_t* bw_const_words;  // read through the scalar cache

constexpr uint32_t kBwQ = 128;  // queries per wave
constexpr uint32_t kBwP = 16;   // pending slots per query

// |q| of the zero-padded queries: [mblocks * 128]
__global__ void __launch_bounds__(256) ngt_scan_bytes_wide_qpop_kernel(const uint32_t* __restrict__ qpad,
                                                                       uint32_t qwords, uint32_t n,
                                                                       uint32_t* __restrict__ out) {
  const uint32_t q = blockIdx.x * 256 + threadIdx.x;
  if (q >= n) return;
  uint32_t s = 0;
  for (uint32_t w = 0; w < qwords; w++) s += __popc(qpad[(uint64_t)q * qwords + w]);
  out[q] = s;
}

// *flag |= 1 if a live row (valid, not the dummy row 0) is all zero
__global__ void __launch_bounds__(256) ngt_scan_bytes_wide_zero_kernel(const uint8_t* __restrict__ rows,
                                                                       uint64_t row_bytes, uint64_t nrows,
                                                                       const uint8_t* __restrict__ valid, int dp,
                                                                       uint32_t* flag) {
  for (uint64_t id = 1 + (uint64_t)blockIdx.x * 256 + threadIdx.x; id < nrows; id += (uint64_t)gridDim.x * 256) {
    if (valid != nullptr && valid[id] == 0) continue;
    const bw_u32x4* p = reinterpret_cast<const bw_u32x4*>(rows + id * row_bytes);
    uint32_t o = 0;
    for (int c = 0; c < (dp >> 4); c++) {
      const bw_u32x4 v = p[c];
      o |= v[0] | v[1] | v[2] | v[3];
    }
    if (o == 0) atomicOr(flag, 1u);
  }
}

__device__ __forceinline__ uint64_t bw_readlane(uint64_t v, uint32_t l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l);
  return ((uint64_t)hi << 32) | lo;
}

// (c << 16 | de) of the one ratio c/de, de <= 2048, whose Jaccard distance is
// d (the rule at the top of the file); the whole wave calls it.
__device__ __forceinline__ uint32_t bw_ratio_of(float d, uint32_t lane) {
  const double rho = 1.0 - (double)d;
  uint32_t found = 0;
  uint64_t b = 0;
  for (uint32_t i = 0; i < 32 && b == 0; i++) {
    const uint32_t de = 64 * i + lane + 1;
    const double x = rho * (double)de, c = __builtin_rint(x);
    if (__builtin_fabs(c - x) <= (double)de * 0x1p-24) found = ((uint32_t)c << 16) | de;
    b = __ballot(found != 0);
  }
  // no match cannot happen for a distance of the domain; (0, 1) passes every pair
  return b ? (uint32_t)__builtin_amdgcn_readlane((int)found, __ffsll((long long)b) - 1) : 1u;
}

template <int M, int NC>
__global__ void __launch_bounds__(64) ngt_scan_bytes_wide_kernel(BytesWideScanArgs a) {
  constexpr bool kJ = M == kJaccard;
  __shared__ uint32_t pend[kBwQ * kBwP];             // (S or c) << 16 | row offset in the part
  __shared__ uint16_t pde[kJ ? kBwQ * kBwP : 1];     // Jaccard: de
  const uint32_t lane = threadIdx.x, k = a.k;
  const uint32_t mb = blockIdx.x / a.nparts, part = blockIdx.x % a.nparts;
  const uint32_t q0 = mb * kBwQ;
  const uint32_t nqb = a.nq - q0 < kBwQ ? a.nq - q0 : kBwQ;
  const uint32_t t0 = part * a.tiles_per_part;
  const uint32_t t1 = t0 + a.tiles_per_part < a.ntiles ? t0 + a.tiles_per_part : a.ntiles;
  const uint32_t row0 = t0 * 64;  // pending rows are offsets from here
  const uint64_t lt = (1ull << lane) - 1;

  // the list of the wave's query q in this part
  auto list_of = [&](uint32_t q) -> uint64_t* { return a.partial + ((uint64_t)(q0 + q) * a.nparts + part) * k; };

  // empty lists: all ones, which is also what the merge expects beyond a list's length
  for (uint32_t q = 0; q < nqb; q++) {
    uint64_t* L = list_of(q);
    for (uint32_t i = lane; i < k; i += 64) __hip_atomic_store(L + i, ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // of query h * 64 + lane: the filter threshold, the pending count, |q|
  uint64_t thr[2] = {a.thr_init, a.thr_init};
  uint32_t cnt[2] = {0, 0};
  uint32_t qp[2] = {0, 0};
  if constexpr (kJ) {
    qp[0] = a.qpop[q0 + lane];
    qp[1] = a.qpop[q0 + 64 + lane];
  }
  bw_const_words qwords = (bw_const_words)(uintptr_t)(a.qpad + (uint64_t)q0 * (NC * 4));

  // a lane's row of tile t and its byte of the valid column; rows past the
  // table reload the last one
  auto load_tile = [&](uint32_t t, bw_u32x4 (&dst)[NC], uint32_t& vb) {
    const uint64_t id = (uint64_t)t * 64 + lane;
    const uint64_t rid = id < a.nrows ? id : a.nrows - 1;
    const uint8_t* p = a.rows + rid * a.row_bytes;
#pragma unroll
    for (int c = 0; c < NC; c++) {
      bw_u32x4 v = {0, 0, 0, 0};
      if (c * 16 < a.dp) v = *reinterpret_cast<const bw_u32x4*>(p + 16 * c);
      dst[c] = v;
    }
    vb = 1;
    if (a.valid != nullptr) vb = a.valid[rid];
  };

  // A round: the first n pending entries of query q into its list; thrv is
  // the VGPR pair that holds q's filter threshold.
  auto process = [&](uint32_t q, uint32_t n, uint64_t& thrv) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the slots' writes, other lanes' included
    uint64_t* L = list_of(q);
    // the list, two keys per lane
    const uint64_t l0 = lane < k ? __hip_atomic_load(L + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ~0ull;
    const uint64_t l1 =
        lane + 64 < k ? __hip_atomic_load(L + lane + 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ~0ull;
    const uint32_t c = (uint32_t)(__popcll(__ballot(l0 != ~0ull)) + __popcll(__ballot(l1 != ~0ull)));
    const uint64_t th = k <= 64 ? bw_readlane(l0, k - 1) : bw_readlane(l1, k - 65);  // ~0 until the list is full
    // lane i: the comparator's distance of pending entry i, the radius rule
    // (L1 / Hamming: the filter's start threshold was the radius, exactly),
    // the key against the k-th key
    uint64_t key = ~0ull;
    bool ok = false;
    if (lane < n) {
      const uint32_t w = pend[q * kBwP + lane];
      const uint32_t id = row0 + (w & 0xffffu), v = w >> 16;
      float d;
      bool in = true;
      if constexpr (kJ) {
        d = (float)(1.0 - (double)v / (double)pde[q * kBwP + lane]);
        in = a.radius < 0.0 || (double)d <= a.radius;
      } else {
        d = (float)v;
      }
      if (in) {
        key = make_key(d, id);
        ok = key < th;
      }
    }
    // list keys below each survivor, survivors below each survivor and below each list key
    const uint64_t surv = __ballot(ok);
    uint32_t lb = 0, sb = 0, a0 = 0, a1 = 0;
    for (uint64_t m = surv; m; m &= m - 1) {
      const uint32_t j = (uint32_t)__ffsll((long long)m) - 1;
      const uint64_t sk = bw_readlane(key, j);
      const uint64_t b0 = __ballot(l0 < sk), b1 = __ballot(l1 < sk);
      if (lane == j) lb = (uint32_t)(__popcll(b0) + __popcll(b1));
      sb += sk < key ? 1u : 0u;
      a0 += sk < l0 ? 1u : 0u;
      a1 += sk < l1 ? 1u : 0u;
    }
    if (surv == 0) return;
    // the places are a permutation of 0 .. c + survivors - 1; a list key that
    // no survivor precedes stays where it is, places from k on drop out
    const bool ws = ok && lb + sb < k;
    const bool w0 = lane < c && a0 != 0 && lane + a0 < k;
    const bool w1 = lane + 64 < c && a1 != 0 && lane + 64 + a1 < k;
    if (ws) __hip_atomic_store(L + lb + sb, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (w0) __hip_atomic_store(L + lane + a0, l0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (w1) __hip_atomic_store(L + lane + 64 + a1, l1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // the new k-th key, if a key moved to the last place (an entry that stays
    // there leaves the threshold as it is)
    const uint64_t bs = __ballot(ws && lb + sb == k - 1);
    const uint64_t bl0 = __ballot(w0 && lane + a0 == k - 1), bl1 = __ballot(w1 && lane + 64 + a1 == k - 1);
    uint64_t kth = ~0ull;
    if (bs) kth = bw_readlane(key, (uint32_t)__ffsll((long long)bs) - 1);
    else if (bl0) kth = bw_readlane(l0, (uint32_t)__ffsll((long long)bl0) - 1);
    else if (bl1) kth = bw_readlane(l1, (uint32_t)__ffsll((long long)bl1) - 1);
    if (kth != ~0ull) {
      uint64_t f;
      if constexpr (kJ) f = ((uint64_t)bw_ratio_of(key_dist(kth), lane) << 32) | (uint32_t)kth;
      else f = ((uint64_t)(uint32_t)key_dist(kth) << 32) | (uint32_t)kth;
      if (lane == (q & 63)) thrv = f;
    }
    // the round's stores land before a later round loads the list
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  };

  // Survivors m of query q (tile offset toff) into its pending slots; v and de
  // are the lanes' values.  Full slots are merged at once.
  auto insert = [&](uint32_t q, uint64_t m, uint32_t v, uint32_t de, uint32_t toff, uint64_t& thrv, uint32_t& cntv) {
    uint32_t n = (uint32_t)__builtin_amdgcn_readlane((int)cntv, (int)(q & 63));
    while (m) {
      const uint32_t slot = n + (uint32_t)__popcll(m & lt);
      const bool mine = ((m >> lane) & 1) != 0 && slot < kBwP;
      if (mine) {
        pend[q * kBwP + slot] = (v << 16) | (toff + lane);
        if constexpr (kJ) pde[q * kBwP + slot] = (uint16_t)de;
      }
      const uint64_t took = __ballot(mine);
      n += (uint32_t)__popcll(took);
      m &= ~took;
      if (n == kBwP) {
        process(q, kBwP, thrv);
        n = 0;
      }
    }
    if (lane == (q & 63)) cntv = n;
  };

  // the loads of tile t + 1 are in flight while tile t is compared
  bw_u32x4 cur[NC], nxt[NC];
  uint32_t vb_nxt = 0;
  if (t0 < t1) load_tile(t0, nxt, vb_nxt);
  for (uint32_t t = t0; t < t1; t++) {
#pragma unroll
    for (int c = 0; c < NC; c++) cur[c] = nxt[c];
    // the lane's id, ~0 for removed rows, the dummy row 0 and padding
    const uint64_t id = (uint64_t)t * 64 + lane;
    const uint32_t id_cur = vb_nxt != 0 && id >= 1 && id < a.nrows ? (uint32_t)id : ~0u;
    if (t + 1 < t1) load_tile(t + 1, nxt, vb_nxt);
    const uint64_t livem = __ballot(id_cur != ~0u);
    if (livem == 0) continue;
    uint32_t xp = 0;  // Jaccard: |x|
    if constexpr (kJ) {
#pragma unroll
      for (int c = 0; c < NC; c++)
#pragma unroll
        for (int j = 0; j < 4; j++) xp += __popc(cur[c][j]);
    }
    const uint32_t toff = (t - t0) * 64;
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const uint32_t nh = nqb > 64u * h ? (nqb - 64u * h < 64u ? nqb - 64u * h : 64u) : 0u;
      for (uint32_t ql = 0; ql < nh; ql++) {
        const uint32_t q = 64u * h + ql;
        bw_const_words qw = qwords + q * (NC * 4);
        uint32_t S = 0;
#pragma unroll
        for (int c = 0; c < NC; c++)
#pragma unroll
          for (int j = 0; j < 4; j++) {
            if constexpr (M == kL1) S = __builtin_amdgcn_sad_u8(cur[c][j], qw[c * 4 + j], S);
            else if constexpr (M == kHamming) S += __popc(cur[c][j] ^ qw[c * 4 + j]);
            else S += __popc(cur[c][j] & qw[c * 4 + j]);
          }
        const uint64_t tq = bw_readlane(thr[h], ql);
        uint32_t de = 0;
        bool pass;
        if constexpr (kJ) {
          de = xp + (uint32_t)__builtin_amdgcn_readlane((int)qp[h], (int)ql) - S;
          const uint32_t A = __umul24(S, (uint32_t)(tq >> 32) & 0xffffu), B = __umul24((uint32_t)(tq >> 48), de);
          pass = A > B || (A == B && id_cur < (uint32_t)tq);
        } else {
          pass = (((uint64_t)S << 32) | id_cur) < tq;
        }
        const uint64_t m = __ballot(pass) & livem;
        if (m) insert(q, m, S, de, toff, thr[h], cnt[h]);
      }
    }
  }
  // what is still pending at the part's end; the lists are in place
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const uint32_t nh = nqb > 64u * h ? (nqb - 64u * h < 64u ? nqb - 64u * h : 64u) : 0u;
    for (uint32_t ql = 0; ql < nh; ql++) {
      const uint32_t n = (uint32_t)__builtin_amdgcn_readlane((int)cnt[h], (int)ql);
      if (n) process(64u * h + ql, n, thr[h]);
    }
  }
}

hipError_t launch_scan_bytes_wide_qpop(const uint32_t* qpad, int dp, uint32_t mblocks, uint32_t* qpop, hipStream_t s) {
  const uint32_t n = mblocks * kBwQ;
  hipLaunchKernelGGL(ngt_scan_bytes_wide_qpop_kernel, dim3((n + 255) / 256), dim3(256), 0, s, qpad,
                     (uint32_t)scan_bytes_chunks(dp) * 4, n, qpop);
  return hipGetLastError();
}

hipError_t launch_scan_bytes_wide_zero(const uint8_t* rows, uint64_t row_bytes, uint64_t nrows, const uint8_t* valid,
                                       int dp, uint32_t* flag, hipStream_t s) {
  const uint64_t blocks = std::min<uint64_t>((nrows + 255) / 256, 65536);
  hipLaunchKernelGGL(ngt_scan_bytes_wide_zero_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, rows, row_bytes, nrows,
                     valid, dp, flag);
  return hipGetLastError();
}

template <int M>
static hipError_t launch_scan_bytes_wide_metric(const BytesWideScanArgs& a, hipStream_t s) {
  const dim3 grid(a.nparts * a.mblocks), block(64);
  switch (scan_bytes_chunks(a.dp)) {
    case 1: hipLaunchKernelGGL((ngt_scan_bytes_wide_kernel<M, 1>), grid, block, 0, s, a); break;
    case 2: hipLaunchKernelGGL((ngt_scan_bytes_wide_kernel<M, 2>), grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL((ngt_scan_bytes_wide_kernel<M, 4>), grid, block, 0, s, a); break;
    case 8: hipLaunchKernelGGL((ngt_scan_bytes_wide_kernel<M, 8>), grid, block, 0, s, a); break;
    case 16: hipLaunchKernelGGL((ngt_scan_bytes_wide_kernel<M, 16>), grid, block, 0, s, a); break;
    default: return hipErrorNotSupported;
  }
  return hipGetLastError();
}

hipError_t launch_scan_bytes_wide(const BytesWideScanArgs& a, int metric, hipStream_t s) {
  if (a.k == 0 || a.k > 128 || a.nparts == 0 || a.mblocks == 0 || a.dp < 16 || a.dp > 256 || a.dp % 16 ||
      a.tiles_per_part > kBytesWideMaxTiles || (uint64_t)a.nparts * a.tiles_per_part < a.ntiles)
    return hipErrorNotSupported;
  if (metric == kL1) return launch_scan_bytes_wide_metric<kL1>(a, s);
  if (metric == kHamming) return launch_scan_bytes_wide_metric<kHamming>(a, s);
  if (metric == kJaccard && a.qpop != nullptr) return launch_scan_bytes_wide_metric<kJaccard>(a, s);
  return hipErrorNotSupported;
}

}  // namespace ngt_amd
