// unchecked_set.h -- the reference's "unchecked" priority set
// (lib/NGT/Graph.cpp:398-495) as one wave keeps it, in three levels:
//
//   head   sorted, in the wave's registers: lane i holds the i-th smallest
//          key, hn <= 64 keys, all below the bound B.  A pop is a lane shift
//          and never scans anything; the next nodes to expand are its first
//          lanes.
//   tail   unsorted, in LDS: ntail keys k with B <= k < T.  It takes what a
//          full head pushes out without sorting anything.
//   spill  unsorted, in HBM: nspill keys >= T.  A graph over 12.5M objects
//          keeps ~40k unchecked keys per query; LDS cannot hold them.
//
// Invariant: every head key < B <= every tail key < T <= every spill key, so
// the smallest keys are in the head while it is not empty.  A full head sends
// its largest key to the tail (B drops); an empty head takes the smallest
// tail keys (threshold selection + bitonic sort, B rises).  A full tail first
// drops the keys beyond the exploration radius -- they can never be popped
// (Graph.cpp:433-435) and the radius only shrinks -- and, if still over half
// full, moves its larger keys to the spill (T drops); an empty tail takes the
// smallest spill keys within the radius (T rises).  Exact throughout: what
// pop() returns is the minimum of the keys inserted and not yet popped, as
// long as that minimum lies within the radius.
//
// Users: the latency kernel (search_lat.hip, UncheckedSet<true, false>: each
// head lane carries the tag of its speculation slot) and the NGTQG kernel
// (qg_kernels.hip, UncheckedSet<false, true>).  The lookahead kernel
// (search_la.hip) uses SortedHead, partition_keys and lat_select with
// tail and spill policies of its own.
//
// One difference between the users is kept as it was found, not decided
// here.  TRIM: with it a full spill first drops its keys beyond the
// exploration radius and reports the capacity error only if it is still full;
// without it (the latency kernel) a full spill is an error at once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "search_common.h"

namespace ngt_amd {

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
  return ((uint64_t)hi << 32) | lo;
}
// whole-wave lane shifts by one on the DPP path (gfx9 wave_shr:1 /
// wave_shl:1: one VALU op instead of an LDS-crossbar ds_bpermute): up1 gives
// lane i the value of lane i-1, down1 the value of lane i+1; the lane with
// no source keeps its own value (the callers overwrite or mask it)
__device__ __forceinline__ uint32_t wave_up1(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x138, 0xf, 0xf, false);
}
__device__ __forceinline__ uint32_t wave_down1(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x130, 0xf, 0xf, false);
}
__device__ __forceinline__ uint64_t wave_up1_u64(uint64_t v) {
  return ((uint64_t)wave_up1((uint32_t)(v >> 32)) << 32) | wave_up1((uint32_t)v);
}
__device__ __forceinline__ uint64_t wave_down1_u64(uint64_t v) {
  return ((uint64_t)wave_down1((uint32_t)(v >> 32)) << 32) | wave_down1((uint32_t)v);
}
__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, int l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
  return ((uint64_t)hi << 32) | lo;
}
// a wave-uniform u64 in SGPRs (the reductions leave it in every lane)
__device__ __forceinline__ uint64_t uniform_u64_lat(uint64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}
// A threshold t over the keys of arr[0..n) that are <= lim (wave-uniform
// arguments): at most M keys lie below t, at least one does, and M/2 or more
// when the keys allow.  Histogram passes over 64 power-of-two bins of the key
// range (64 LDS counters in hist), refining the first bin that overflows.
// Returns 0 when no key is <= lim.  Not inlined: it runs a few times per
// query and would otherwise share the commit loop's registers.
__device__ __noinline__ uint64_t lat_select(const uint64_t* arr, uint32_t n, uint32_t M, uint64_t lim, uint32_t* hist) {
  const int lane = lane_id();
  uint64_t lo = ~0ull, hi = 0;
  for (uint32_t i = lane; i < n; i += 64) {
    const uint64_t v = arr[i];
    if (v <= lim) {
      lo = v < lo ? v : lo;
      hi = v > hi ? v : hi;
    }
  }
  lo = uniform_u64_lat(wave_min_u64(lo));
  hi = uniform_u64_lat(~wave_min_u64(~hi));
  if (lo > hi) return 0ull;
  uint32_t base = 0;
  for (int it = 0; it < 16; it++) {
    const uint64_t span = hi - lo;
    const int bits = span ? 64 - __clzll((long long)span) : 0;
    const int shift = bits > 6 ? bits - 6 : 0;
    // hist is LDS reached through a generic pointer: flat accesses may
    // complete out of order, so each phase drains before the next
    hist[lane] = 0u;
    __threadfence_block();
    for (uint32_t i = lane; i < n; i += 64) {
      const uint64_t v = arr[i];
      if (v >= lo && v <= hi && v <= lim) atomicAdd(hist + (uint32_t)((v - lo) >> shift), 1u);
    }
    __threadfence_block();
    uint32_t incl = hist[lane];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t u = (uint32_t)__shfl_up((int)incl, o, 64);
      if (lane >= o) incl += u;
    }
    const uint32_t b = (uint32_t)__popcll(ballot64(base + incl <= M));  // bins [0, b) fit
    if (b == 64u) return hi + 1;
    const uint32_t below = base + (b ? (uint32_t)__builtin_amdgcn_readlane((int)incl, (int)b - 1) : 0u);
    if ((below >= M / 2 && below > 0) || shift == 0) return lo + ((uint64_t)b << shift);
    base = below;
    lo = lo + ((uint64_t)b << shift);
    const uint64_t top = lo + ((1ull << shift) - 1ull);
    hi = top < hi ? top : hi;
  }
  return lo + 1;  // never expected: the minimum alone
}

// bitonic sort of one value per lane across the 64 lanes, ascending
__device__ __forceinline__ uint64_t bitonic_sort64(uint64_t v) {
  const int lane = lane_id();
#pragma unroll
  for (int kk = 2; kk <= 64; kk <<= 1) {
#pragma unroll
    for (int j = kk >> 1; j > 0; j >>= 1) {
      const uint64_t o = shfl_xor_u64(v, j);
      const bool up = ((lane & kk) == 0);
      const bool lower = (lane & j) == 0;
      const uint64_t mn = o < v ? o : v, mx = o < v ? v : o;
      v = (lower == up) ? mn : mx;
    }
  }
  return v;
}

// Compacts in place, in order, the keys of arr[0..n) that keep(key) holds
// for, and returns their number.  The whole wave calls other(key, rest) once
// per 64 keys, `rest` marking the lanes whose key is not kept: it moves them
// elsewhere or drops them.
template <class Keep, class Other>
__device__ __forceinline__ uint32_t partition_keys(uint64_t* arr, uint32_t n, Keep keep, Other other) {
  const int lane = lane_id();
  uint32_t out = 0;
  for (uint32_t b0 = 0; b0 < n; b0 += 64) {
    const uint32_t i = b0 + (uint32_t)lane;
    const uint64_t key = i < n ? arr[i] : ~0ull;
    const bool kp = i < n && keep(key);
    const uint64_t km = ballot64(kp);
    __builtin_amdgcn_wave_barrier();
    other(key, i < n && !kp);
    if (kp) arr[out + mbcnt(km)] = key;
    __builtin_amdgcn_wave_barrier();
    out += (uint32_t)__popcll(km);
  }
  return out;
}

constexpr uint32_t kNoTag = 0xffu;  // a head entry without a tag

template <bool TAGGED>
struct HeadTags {
  uint32_t ht = kNoTag;  // lane i: the tag of the i-th smallest key
  // bit t: tag t's key left the head for the tail with its tag still on (the
  // caller, who hands the tags out, takes it from here and clears the bit)
  uint64_t orphan = 0ull;
};
template <>
struct HeadTags<false> {};

// hn <= 64 keys sorted across the lanes of one wave: lane i holds the i-th
// smallest in hk, the lanes from hn on hold ~0.
template <bool TAGGED>
struct SortedHead : HeadTags<TAGGED> {
  uint64_t hk = ~0ull;
  uint32_t hn = 0;

  // the number of head keys below `key`: the lane it belongs in
  __device__ __forceinline__ uint32_t rank(uint64_t key) const {
    return (uint32_t)__popcll(ballot64((uint32_t)lane_id() < hn && hk < key));
  }
  // key enters at lane pos = rank(key) < 64, untagged; the keys from there
  // on move up a lane, and a full head's last key falls out (read it first)
  __device__ __forceinline__ void insert_at(uint32_t pos, uint64_t key) {
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t uk = wave_up1_u64(hk);
    const bool mv = lane > pos && (hn == 64u || lane <= hn);
    if (mv) hk = uk;
    if (lane == pos) hk = key;
    if constexpr (TAGGED) {
      const uint32_t ut = wave_up1(this->ht);
      if (mv) this->ht = ut;
      if (lane == pos) this->ht = kNoTag;
    }
    if (hn < 64u) hn++;
  }
  // the first key leaves (hn > 0)
  __device__ __forceinline__ void pop_first() {
    const uint32_t lane = (uint32_t)lane_id();
    const uint64_t dk = wave_down1_u64(hk);
    hk = lane + 1 < hn ? dk : ~0ull;
    if constexpr (TAGGED) {
      const uint32_t dt = wave_down1(this->ht);
      this->ht = lane + 1 < hn ? dt : kNoTag;
    }
    hn--;
  }
};

template <bool TRIM>
struct TrimCount {
  uint32_t ntrim = 0;  // spill trims
};
template <>
struct TrimCount<false> {};

template <bool TAGGED, bool TRIM>
struct UncheckedSet : SortedHead<TAGGED>, TrimCount<TRIM> {
  using SortedHead<TAGGED>::hk;
  using SortedHead<TAGGED>::hn;
  uint32_t ntail = 0, nspill = 0;
  uint64_t B = ~0ull, T = ~0ull;
  uint32_t maxq = 0;  // the largest hn + ntail + nspill an insert left
  // pending error bits: 1 the spill is full (keys were lost), 32 / 64 / 128
  // a threshold selection moved no key or too many (never expected)
  uint32_t err = 0;

  uint64_t* const tail;
  const uint32_t tail_cap;
  uint64_t* const spill;
  const uint32_t spill_cap;
  uint32_t* const hist;    // 64 counters for lat_select
  uint64_t* const stage;   // 64 keys on their way into the head
  const float& expr;       // the exploration radius now: it shrinks during a query

  __device__ __forceinline__ UncheckedSet(uint64_t* tail_, uint32_t tail_cap_, uint64_t* spill_, uint32_t spill_cap_,
                                          uint32_t* hist_, uint64_t* stage_, const float& expr_)
      : tail(tail_), tail_cap(tail_cap_), spill(spill_), spill_cap(spill_cap_), hist(hist_), stage(stage_),
        expr(expr_) {}

  // the largest key within the exploration radius
  __device__ __forceinline__ uint64_t radius_key() const { return ((uint64_t)ord_of(expr) << 32) | 0xffffffffull; }

  // TRIM: a full spill drops its keys beyond the exploration radius
  __device__ __forceinline__ void spill_trim() {
    if constexpr (TRIM) {
      const uint64_t lim = radius_key();
      nspill = partition_keys(spill, nspill, [&](uint64_t key) { return key <= lim; }, [](uint64_t, bool) {});
      this->ntrim++;
    }
  }
  __device__ __forceinline__ void spill_push(uint64_t key) {
    if (nspill >= spill_cap) spill_trim();
    if (nspill >= spill_cap) {
      err |= 1u;
    } else {
      if (lane_id() == 0) spill[nspill] = key;
      nspill++;
    }
  }
  // the tail is full: drop the keys beyond the exploration radius; if it is
  // still over half full, move the keys from a threshold up to the spill
  // (the NGTQG kernel sits at its VGPR cap and this spelling of the capacity
  // test is one that adds no scratch to it: re-check the compiler's resource
  // report of qg_kernels.hip after touching it)
  __device__ __forceinline__ void tail_room() {
    ntail = compact(tail, ntail, expr);
    const uint32_t keep = tail_cap / 2;
    if (ntail <= keep) return;
    const uint64_t l = lat_select(tail, ntail, keep, ~0ull, hist);
    ntail = partition_keys(tail, ntail, [&](uint64_t key) { return key < l; },
                           [&](uint64_t key, bool mv) {
                             const uint64_t mm = ballot64(mv);
                             const uint32_t nm = (uint32_t)__popcll(mm);
                             if (nspill + nm > spill_cap) spill_trim();
                             if (nspill + nm > spill_cap) {
                               err |= 1u;
                             } else if (mv) {
                               spill[nspill + mbcnt(mm)] = key;
                             }
                             if (nspill + nm <= spill_cap) nspill += nm;
                           });
    if (ntail == 0u || ntail > keep) err |= 32u;  // selection check
    T = l;
  }
  __device__ __forceinline__ void tail_push(uint64_t key) {
    if (key < T && ntail >= tail_cap) tail_room();
    if (key >= T) {
      spill_push(key);
    } else {
      if (lane_id() == 0) tail[ntail] = key;
      ntail++;
    }
    __builtin_amdgcn_wave_barrier();
  }
  __device__ __forceinline__ void count() {
    const uint32_t q = hn + ntail + nspill;
    if (q > maxq) maxq = q;
  }
  __device__ __forceinline__ void insert(uint64_t key) {
    if (key < B) {
      const uint32_t pos = this->rank(key);
      if (pos == 64u) {
        // beyond a full head: straight to the tail
        B = key;
        tail_push(key);
      } else if (hn == 64u) {
        // the head is full: its largest key moves to the tail
        const uint64_t e = readlane_u64(hk, 63);
        if constexpr (TAGGED) {
          const uint32_t tag = (uint32_t)__builtin_amdgcn_readlane((int)this->ht, 63);
          if (tag != kNoTag) this->orphan |= 1ull << tag;
        }
        this->insert_at(pos, key);
        B = e;
        tail_push(e);
      } else {
        this->insert_at(pos, key);
      }
    } else {
      tail_push(key);
    }
    count();
  }
  // an empty tail takes the smallest spill keys within the exploration
  // radius; the ones beyond it are dropped
  __device__ __forceinline__ void refill_tail() {
    const uint32_t want = tail_cap / 2;
    const uint64_t lim = radius_key();
    const uint64_t l = lat_select(spill, nspill, want, lim, hist);
    if (l == 0ull) {  // nothing within the radius: the search ends
      nspill = 0;
      T = ~0ull;
      return;
    }
    nspill = partition_keys(spill, nspill, [&](uint64_t key) { return key <= lim && key >= l; },
                            [&](uint64_t key, bool rest) {
                              const bool mv = rest && key <= lim && key < l;
                              const uint64_t mm = ballot64(mv);
                              if (mv) tail[ntail + mbcnt(mm)] = key;
                              ntail += (uint32_t)__popcll(mm);
                            });
    T = nspill ? l : ~0ull;
    if (ntail == 0u || ntail > want) err |= 64u;  // selection check
  }
  // an empty head takes the (at most 64, at least 32 when there are) smallest
  // tail keys, the tail the smallest spill keys first when it has none
  __device__ __forceinline__ void refill_head() {
    if (ntail == 0 && nspill != 0) refill_tail();
    if (ntail == 0) return;
    const uint64_t t = lat_select(tail, ntail, 64u, ~0ull, hist);
    uint32_t got = 0;
    ntail = partition_keys(tail, ntail, [&](uint64_t key) { return key >= t; },
                           [&](uint64_t key, bool mv) {
                             const uint64_t mm = ballot64(mv);
                             if (mv) stage[got + mbcnt(mm)] = key;
                             got += (uint32_t)__popcll(mm);
                           });
    if (got == 0u || got > 64u) err |= 128u;  // selection check
    hk = bitonic_sort64((uint32_t)lane_id() < got ? stage[lane_id()] : ~0ull);
    if constexpr (TAGGED) this->ht = kNoTag;
    hn = got;
    B = (ntail + nspill) ? readlane_u64(hk, (int)got - 1) + 1 : ~0ull;
    __builtin_amdgcn_wave_barrier();
  }
  // the smallest key (and its tag) leaves; false when the set is empty or
  // every key left lies beyond the exploration radius
  __device__ __forceinline__ bool pop(uint64_t& key) {
    if (hn == 0) refill_head();
    if (hn == 0) return false;
    key = readlane_u64(hk, 0);
    this->pop_first();
    return true;
  }
  __device__ __forceinline__ bool pop(uint64_t& key, uint32_t& tag) {
    static_assert(TAGGED, "only a tagged head has tags");
    if (hn == 0) refill_head();
    if (hn == 0) return false;
    key = readlane_u64(hk, 0);
    tag = (uint32_t)__builtin_amdgcn_readlane((int)this->ht, 0);
    this->pop_first();
    return true;
  }
};

}  // namespace ngt_amd
