// scan_bytes_common.h -- what the uint8 L1 / Hamming scans with k-lists in LDS
// share (scan_bytes.hip, scan_bytes_long.hip): the register types, the 64-bit
// v_readlane and the insertion of a (tile, query)'s survivors into the query's
// sorted list.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ngt_device.h"

namespace ngt_amd {

typedef uint32_t bs_u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) uint32_t* bs_const_words;  // read through the scalar cache

__device__ __forceinline__ uint64_t bs_readlane(uint64_t v, uint32_t l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, (int)l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), (int)l);
  return ((uint64_t)hi << 32) | lo;
}

// Survivors m of query q into its list lists[q * k .. q * k + k - 1] in LDS,
// (S << 32 | id) ascending, ~0 = empty; S and key are the lanes' values, t the
// query's k-th key, thrv the VGPR pair that holds it in lane q & 63.  No S is
// above kMaxS.
template <uint32_t kMaxS>
__device__ __forceinline__ void bs_insert(uint64_t* lists, uint32_t k, uint32_t lane, uint32_t q, uint64_t m,
                                          uint32_t S, uint64_t key, uint64_t t, uint64_t& thrv) {
  if ((uint32_t)__popcll(m) > k) {
    // T = the k-th smallest S of the survivors: the largest T with fewer
    // than k survivors below it
    uint32_t T = 0;
    for (int b = 31 - __builtin_clz(kMaxS); b >= 0; b--) {
      const uint32_t cand = T | (1u << b);
      if ((uint32_t)__popcll(__ballot(S < cand) & m) < k) T = cand;
    }
    m &= __ballot(S <= T);
  }
  uint64_t* L = lists + q * k;
  uint64_t e = lane < k ? L[lane] : ~0ull;
  while (m) {
    const uint32_t j = (uint32_t)__ffsll((long long)m) - 1;
    m &= m - 1;
    const uint64_t kj = bs_readlane(key, j);
    if (kj >= t) continue;
    // kj < t <= e[k - 1]: the rank is below k, the k-th entry drops out
    const uint32_t pos = (uint32_t)__popcll(__ballot(e < kj));
    const uint32_t ulo = (uint32_t)__shfl_up((int)(uint32_t)e, 1, 64);
    const uint32_t uhi = (uint32_t)__shfl_up((int)(uint32_t)(e >> 32), 1, 64);
    const uint64_t up = ((uint64_t)uhi << 32) | ulo;
    if (lane < k && lane >= pos) e = lane == pos ? kj : up;
    const uint64_t kth = bs_readlane(e, k - 1);
    if (kth < t) t = kth;
  }
  if (lane < k) L[lane] = e;
  if (lane == (q & 63)) thrv = t;
}

// The part's lists go out as make_key((float)S, id), ~0 for an empty place:
// partial[(q0 + ql) * nparts + part][k].
__device__ __forceinline__ void bs_store_lists(const uint64_t* lists, uint32_t nqb, uint32_t k, uint32_t lane,
                                               uint32_t q0, uint32_t nparts, uint32_t part, uint64_t* partial) {
  for (uint32_t i = lane; i < nqb * k; i += 64) {
    const uint32_t ql = i / k, rr = i - ql * k;
    const uint64_t e = lists[i];
    partial[((uint64_t)(q0 + ql) * nparts + part) * k + rr] =
        e == ~0ull ? ~0ull : make_key((float)(uint32_t)(e >> 32), (uint32_t)e);
  }
}

}  // namespace ngt_amd
