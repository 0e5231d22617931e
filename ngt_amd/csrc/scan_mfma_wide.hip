// scan_mfma_wide.hip -- the matrix-core filtered exact scan (scan_mfma.hip)
// for lists of 17 .. 128 results: float L2, Cosine, Angle and the normalized
// metrics (the latter four: 3-pass filter, thresholds from scan_dot_bound.h),
// >= 32 queries.
//
// The filter is scan_mfma.hip's: the same fragment-ordered bf16 hi + lo row
// image and query operands, the same extra k-step, the same H_q, kappa, rho
// and margins, the same 4-deep LDS-DMA ring with counted vmcnt waits, the
// same wave tile (128 rows x 64 queries; a workgroup = 4 waves x 128 queries
// x one part of the rows in 256-row tiles).  What follows the filter is
// its own:
//
//  * A (query, part) list lives where it ends up: its slot of the partial
//    buffer ([query][part][k] u64 keys, sorted, ~0 beyond its length), read
//    and written through the L2.  LDS keeps per query the k-th key, the list
//    length, the pending count and H -- nothing that grows with k.
//  * Query q belongs to wave q & 3 of the workgroup: that wave alone reads
//    and writes q's list, and it drains its vector-memory counter
//    (s_waitcnt vmcnt(0)) after the writes of a round, so the next round's
//    loads (agent scope: served by the L2, not the CU's vector cache) see
//    them.  No other ordering is relied on.
//  * 64 pending slots per query (row offsets only).  In a round the owning
//    wave takes one query at a time: lane c evaluates pending candidate c with
//    the comparator (dist_lane), applies the radius rule, forms the key and
//    drops it unless it is below the k-th key and not in the list already;
//    the survivors are then merged by rank -- the wave holds the list two
//    keys per lane, every survivor is broadcast once (readlane) and compared
//    by every lane, position = (list keys below, by ballot) + (survivors
//    below) for a survivor, index + (survivors below) for a list key; what
//    lands below k is written back.  No thread walks a list.
//  * The first tile's bootstrap takes the k-th largest of the query's 256
//    filter values (in the accumulators of two waves) bit by bit over the
//    float's ordered bit pattern with per-query LDS counters, 32 steps once
//    per part.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ngt_device.h"
#include "ngt_kernels.h"
#include "scan_mfma_common.h"
#include "unchecked_set.h"

namespace ngt_amd {

constexpr int kWdPend = 64;  // pending candidates per query between rounds: one per lane
constexpr int kWdTrig = 16;  // a query within this many of its slots asks for a round

template <int M, int P>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
ngt_scan_mfma_wide_kernel(MfmaScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const uint32_t k = a.k;
  uint8_t* stage = smem;                                                    // [4][24 KiB] ring
  uint32_t* pend = reinterpret_cast<uint32_t*>(smem + kMxNst * kMxStage);  // [128][64] pending rows
  uint64_t* thr = reinterpret_cast<uint64_t*>(pend + kMxQ * kWdPend);      // [128] k-th key or ~0
  float* H = reinterpret_cast<float*>(thr + kMxQ);                         // [128]
  float* HB = H + kMxQ;                                                     // [128]
  float* HM = HB + kMxQ;                                                    // [128]
  uint32_t* cnt = reinterpret_cast<uint32_t*>(HM + kMxQ);                  // [128] list lengths
  uint32_t* pc = cnt + kMxQ;                                                // [128] pending counts
  uint32_t* bits = pc + kMxQ;                                               // [128][8]
  uint32_t* bcnt = bits + kMxQ * kMxW;                                      // [3][128] bootstrap counters
  uint32_t* flags = bcnt + 3 * kMxQ;                                        // [4]

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w & 1, wq = w >> 1;
  const uint32_t slot = a.xcd ? blockIdx.x >> 3 : blockIdx.x;
  const uint32_t mb = a.mb0 + slot % a.mblocks;
  const uint32_t part = a.xcd ? (slot / a.mblocks) * 8 + (blockIdx.x & 7) : slot / a.mblocks;
  const uint32_t q0 = mb * kMxQ;
  const uint32_t t0 = part * a.tiles_per_part;
  uint32_t t1 = t0 + a.tiles_per_part;
  if (t1 > a.ntiles) t1 = a.ntiles;
  const uint32_t ks = a.ks;
  const uint64_t row0 = (uint64_t)t0 * kMxR;  // pending rows are offsets from here
  // the dot family's finish and threshold rule (scan_dot_bound.h)
  [[maybe_unused]] const int fin = M == kAngle ? (int)kAngle : a.fin;

  // the list of the workgroup's query ql in this part
  auto list_of = [&](uint32_t ql) -> uint64_t* {
    return a.partial + ((uint64_t)(q0 + ql - a.mb0 * kMxQ) * a.nparts + part) * k;
  };

  for (int i = tid; i < kMxQ; i += 256) {
    thr[i] = ~0ull;
    cnt[i] = 0;
    pc[i] = 0;
    HB[i] = a.hb[q0 + i];
    HM[i] = a.hm[q0 + i];
    if constexpr (kIsDotFamily<M>) H[i] = scan_dot_h(fin, HB[i], a.t_init);
    else H[i] = HB[i] - a.scale * a.t_init;
  }
  for (int i = tid; i < kMxQ * kMxW; i += 256) bits[i] = 0;
  for (int i = tid; i < 3 * kMxQ; i += 256) bcnt[i] = 0;
  if (tid < 4) flags[tid] = 0;
  // empty lists: all ones, which is also what the merge expects beyond a
  // list's length (entries are only ever written below the length)
  for (uint32_t ql = w; ql < (uint32_t)kMxQ && q0 + ql < a.nq; ql += 4) {
    uint64_t* L = list_of(ql);
    for (uint32_t i = lane; i < k; i += 64)
      __hip_atomic_store(L + i, ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");

  // A round: every query with pending candidates, by its wave; then the new
  // filter thresholds.  Called by the whole workgroup.
  auto process = [&]() {
    const uint32_t mine = (uint32_t)w + 4u * (uint32_t)(lane & 31);
    uint64_t todo = ballot64(lane < 32 && q0 + mine < a.nq && pc[mine] != 0);
    while (todo) {
      const uint32_t q = (uint32_t)w + 4u * (uint32_t)(__ffsll((long long)todo) - 1);
      todo &= todo - 1;
      const uint32_t n = min(pc[q], (uint32_t)kWdPend);
      const uint32_t c = cnt[q];
      const uint64_t th = thr[q];
      uint64_t* L = list_of(q);
      // the list, two keys per lane
      const uint64_t l0 = (uint32_t)lane < c
                              ? __hip_atomic_load(L + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                              : ~0ull;
      const uint64_t l1 = (uint32_t)lane + 64 < c
                              ? __hip_atomic_load(L + lane + 64, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                              : ~0ull;
      // lane c: the comparator's distance of pending candidate c, the radius
      // rule, the key against the k-th key
      uint64_t key = ~0ull;
      bool ok = false;
      if ((uint32_t)lane < n) {
        const uint64_t row = row0 + pend[q * kWdPend + lane];
        const float d = dist_lane<M>(reinterpret_cast<const float*>(a.queries + (uint64_t)(q0 + q) * a.query_bytes),
                                     reinterpret_cast<const float*>(a.rows + row * a.row_bytes), a.dp, fin);
        if (a.radius < 0.0 || (double)d <= a.radius) {
          key = make_key(d, (uint32_t)row);
          ok = key < th;
        }
      }
      // list keys below each candidate; a candidate that is in the list
      // already (a pair seen again on the bitmap path) drops out
      uint32_t lb = 0;
      bool dup = false;
      for (uint64_t m = ballot64(ok); m; m &= m - 1) {
        const int j = __ffsll((long long)m) - 1;
        const uint64_t sk = readlane_u64(key, j);
        const uint64_t b0 = ballot64(l0 < sk), b1 = ballot64(l1 < sk), be = ballot64(l0 == sk || l1 == sk);
        if (lane == j) {
          lb = (uint32_t)(__popcll(b0) + __popcll(b1));
          dup = be != 0;
        }
      }
      ok = ok && !dup;
      // survivors below each survivor and below each list key
      const uint64_t surv = ballot64(ok);
      uint32_t sb = 0, a0 = 0, a1 = 0;
      for (uint64_t m = surv; m; m &= m - 1) {
        const uint64_t sk = readlane_u64(key, __ffsll((long long)m) - 1);
        sb += sk < key ? 1u : 0u;
        a0 += sk < l0 ? 1u : 0u;
        a1 += sk < l1 ? 1u : 0u;
      }
      if (surv) {
        // positions are a permutation of 0 .. c + m - 1 (keys are distinct);
        // a list key that no survivor precedes stays where it is
        if (ok && lb + sb < k) {
          __hip_atomic_store(L + lb + sb, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (lb + sb == k - 1) thr[q] = key;
        }
        if ((uint32_t)lane < c && a0 && lane + a0 < k) {
          __hip_atomic_store(L + lane + a0, l0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (lane + a0 == k - 1) thr[q] = l0;
        }
        if ((uint32_t)lane + 64 < c && a1 && lane + 64 + a1 < k) {
          __hip_atomic_store(L + lane + 64 + a1, l1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (lane + 64 + a1 == k - 1) thr[q] = l1;
        }
      }
      if (lane == 0) {
        cnt[q] = min(c + (uint32_t)__popcll(surv), k);
        pc[q] = 0;
        if (a.stats) atomicAdd(&a.stats[0], (unsigned long long)n);
      }
    }
    // this wave's list writes land before any later round loads them
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    lds_barrier();
    if (tid < kMxQ && q0 + tid < a.nq) {
      // every part's k-th key bounds the query's global k-th key: publish
      // this part's, take the smallest over the parts for the filter
      const uint64_t th = thr[tid];
      const uint64_t g = __hip_atomic_fetch_min(a.gthr + q0 + tid, (unsigned long long)th, __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_AGENT);
      const uint64_t best = g < th ? g : th;
      if (best != ~0ull) {
        const float kd = key_dist(best);
        if constexpr (kIsDotFamily<M>) {
          H[tid] = fmaxf(H[tid], scan_dot_h(fin, HB[tid], fminf(a.t_init, kd)));
        } else {
          const float tv = M == kL2 ? fminf(a.t_init, scan_sq_bound(kd)) : fminf(a.t_init, kd);
          H[tid] = fmaxf(H[tid], HB[tid] - a.scale * tv);
        }
      }
    }
    if (a.stats && tid == 0) atomicAdd(&a.stats[1], 1ull);
    lds_barrier();
  };

  // staging ring, as in ngt_scan_mfma_kernel: k-step g of the part goes to
  // slot g % 4 by LDS-DMA; wave w moves blocks w, 4 + w, ... of the 24 1-KiB
  // blocks of a k-step
  typedef __attribute__((address_space(3))) void* lds_ptr;
  const uint32_t G = (t1 > t0 ? t1 - t0 : 0) * ks;
  auto issue = [&](uint32_t g) {
    uint8_t* base = stage + (g % kMxNst) * kMxStage + w * 1024;
    const uint32_t gg = g < G ? g : G - 1;  // past the end: a harmless reload
    const uint32_t rt = t0 + gg / ks, s = gg - (gg / ks) * ks;
    const size_t ro0 = (((size_t)rt * 8 + w) * ks + s) * 512 + (size_t)lane * 8;
    const size_t ro1 = ro0 + (size_t)4 * ks * 512;
    const size_t qo = (((size_t)mb * 4 + w) * ks + s) * 512 + (size_t)lane * 8;
    __builtin_amdgcn_global_load_lds((const void*)(a.rh + ro0), (lds_ptr)(base), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((const void*)(a.rh + ro1), (lds_ptr)(base + 4096), 16, 0, 0);
    __builtin_amdgcn_global_load_lds((const void*)(a.qh + qo), (lds_ptr)(base + 16384), 16, 0, 0);
    if (P == 3) {  // the lo parts
      __builtin_amdgcn_global_load_lds((const void*)(a.rl + ro0), (lds_ptr)(base + 8192), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((const void*)(a.rl + ro1), (lds_ptr)(base + 12288), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((const void*)(a.ql + qo), (lds_ptr)(base + 20480), 16, 0, 0);
    }
  };

  f32x16 acc[4][2];
#pragma unroll
  for (int mt = 0; mt < 4; mt++)
#pragma unroll
    for (int nt = 0; nt < 2; nt++) acc[mt][nt] = (f32x16){};

  __syncthreads();
  if (G) {
    issue(0);
    issue(1);
    issue(2);
  }
  const int ql0 = wq * 64 + (lane & 31);  // this lane's query in n-tile 0
  const int rsh = 4 * (lane >> 5);
  for (uint32_t g = 0; g < G; g++) {
    const uint32_t rt = t0 + g / ks, s = g - (g / ks) * ks;
    // k-step g has landed once at most k-steps g+1, g+2 (2P loads each) are
    // outstanding; the barrier publishes every wave's blocks and retires the
    // reads of slot (g + 3) % 4, which is refilled right after
    if (P == 3) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    lds_barrier();
    issue(g + 3);
    // hi x hi + hi x lo + lo x hi (the norm column's lo parts are 0)
    {
      const uint8_t* sb = stage + (g % kMxNst) * kMxStage + lane * 16;
      bf16x8 ah[4], al[4], bh[2], bl[2];
#pragma unroll
      for (int mt = 0; mt < 4; mt++) {
        ah[mt] = *reinterpret_cast<const bf16x8*>(sb + (wr * 4 + mt) * 1024);
        if (P == 3) al[mt] = *reinterpret_cast<const bf16x8*>(sb + 8192 + (wr * 4 + mt) * 1024);
      }
#pragma unroll
      for (int nt = 0; nt < 2; nt++) {
        bh[nt] = *reinterpret_cast<const bf16x8*>(sb + 16384 + (wq * 2 + nt) * 1024);
        if (P == 3) bl[nt] = *reinterpret_cast<const bf16x8*>(sb + 20480 + (wq * 2 + nt) * 1024);
      }
#pragma unroll
      for (int mt = 0; mt < 4; mt++)
#pragma unroll
        for (int nt = 0; nt < 2; nt++) {
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mt], bh[nt], acc[mt][nt], 0, 0, 0);
          if (P == 3) {
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mt], bl[nt], acc[mt][nt], 0, 0, 0);
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[mt], bh[nt], acc[mt][nt], 0, 0, 0);
          }
        }
    }
    if (s + 1 < ks) continue;

    if (a.dbg & 1) {
#pragma unroll
      for (int mt = 0; mt < 4; mt++)
#pragma unroll
        for (int nt = 0; nt < 2; nt++) acc[mt][nt] = (f32x16){};
      continue;
    }
    if (rt == t0 && !(a.dbg & 4)) {
      // bootstrap: the k-th largest finite filter value of the tile's 256
      // distinct rows bounds the k-th distance from above; rows more than the
      // margin HM below it cannot make the top k.  A query's
      // values sit in four threads (two waves x two lane halves); the largest
      // ordered bit pattern pv with k or more values at or above it is found
      // bit by bit.  NaN (removed rows) never compares, +inf (forced rows) is
      // counted out, and a pivot in the patterns below -inf is a NaN that
      // nothing reaches, so fewer than k finite values leave pv = 0.  -0.0
      // counts at a +0.0 pivot although its pattern is one lower: the two
      // pivots then count alike, and H comes out the same value either way.
      uint32_t pv[2] = {0u, 0u}, ninf[2] = {0u, 0u};
#pragma unroll
      for (int nt = 0; nt < 2; nt++)
#pragma unroll
        for (int mt = 0; mt < 4; mt++)
#pragma unroll
          for (int e = 0; e < 16; e++) ninf[nt] += acc[mt][nt][e] == __builtin_huge_valf() ? 1u : 0u;
      for (int step = 0; step < 32; step++) {
        uint32_t* bc = bcnt + (step % 3) * kMxQ;
        const uint32_t bit = 0x80000000u >> step;
#pragma unroll
        for (int nt = 0; nt < 2; nt++) {
          const float pivot = float_of_ord(pv[nt] | bit);
          uint32_t ge = 0;
#pragma unroll
          for (int mt = 0; mt < 4; mt++)
#pragma unroll
            for (int e = 0; e < 16; e++) ge += acc[mt][nt][e] >= pivot ? 1u : 0u;
          if (ge > ninf[nt]) atomicAdd(&bc[ql0 + nt * 32], ge - ninf[nt]);
        }
        lds_barrier();
#pragma unroll
        for (int nt = 0; nt < 2; nt++)
          if (bc[ql0 + nt * 32] >= k) pv[nt] |= bit;
        // the counters of the step before: read by all before this barrier,
        // used again two barriers from now
        if (tid < kMxQ) bcnt[((step + 2) % 3) * kMxQ + tid] = 0;
      }
      // the four threads of a query write the same value
#pragma unroll
      for (int nt = 0; nt < 2; nt++) {
        const int q = ql0 + nt * 32;
        if (pv[nt] && q0 + q < a.nq) {
          float hb;
          if constexpr (kIsDotFamily<M>) hb = scan_dot_boot(fin, HB[q], HM[q], float_of_ord(pv[nt]));
          else hb = float_of_ord(pv[nt]) - HM[q];
          if (hb > H[q]) H[q] = hb;
        }
      }
      lds_barrier();
    }

    // ---- filter: lane holds queries ql0 + 32 nt x 64 rows of the tile.
    // Fast path: a 16-value block whose maximum is below the threshold is
    // done in 8 VALU operations; passing values go straight into the query's
    // pending slots (LDS atomics).  A full slot array falls back to the
    // candidate bitmap below.
    float hq[2];
#pragma unroll
    for (int nt = 0; nt < 2; nt++) hq[nt] = H[ql0 + nt * 32];
    const uint32_t rbase = (rt - t0) * kMxR + wr * 128 + rsh;
#pragma unroll
    for (int mt = 0; mt < 4; mt++)
#pragma unroll
      for (int nt = 0; nt < 2; nt++) {
        float mx = acc[mt][nt][0];
#pragma unroll
        for (int e = 1; e < 16; e++) mx = fmaxf(mx, acc[mt][nt][e]);
        const bool hit = mx >= hq[nt];
        if (__ballot(hit)) {
          if (hit) {
            const uint32_t q = ql0 + nt * 32;
#pragma unroll
            for (int e = 0; e < 16; e++)
              if (acc[mt][nt][e] >= hq[nt]) {
                const uint32_t n = atomicAdd(&pc[q], 1u);
                if (n < (uint32_t)kWdPend) pend[q * kWdPend + n] = rbase + mt * 32 + (e & 3) + 8 * (e >> 2);
                if (n + kWdTrig >= (uint32_t)kWdPend) flags[1] = 1;  // process after this tile
                if (n >= (uint32_t)kWdPend) flags[2] = 1;            // overflow: bitmap path
              }
          }
        }
      }
    lds_barrier();
    const uint32_t now = flags[1], over = flags[2];
    lds_barrier();
    if (tid == 0) flags[1] = flags[2] = 0;
    if (a.stats && tid == 0 && now) atomicAdd(&a.stats[2], 1ull);
    if (now && !(a.dbg & 2)) {
      if (tid < kMxQ && pc[tid] > (uint32_t)kWdPend) pc[tid] = kWdPend;
      lds_barrier();
      process();
      if (over) {
        // some passing pairs found no slot: redo the tile through the
        // candidate bitmap with the tightened thresholds (pairs already
        // processed are skipped at insertion, every round takes new bits)
#pragma unroll
        for (int nt = 0; nt < 2; nt++) hq[nt] = H[ql0 + nt * 32];
#pragma unroll
        for (int mt = 0; mt < 4; mt++)
#pragma unroll
          for (int nt = 0; nt < 2; nt++) {
            uint32_t mask = 0;
#pragma unroll
            for (int e = 0; e < 16; e++)
              mask |= (acc[mt][nt][e] >= hq[nt] ? 1u : 0u) << ((e & 3) + 8 * (e >> 2) + rsh);
            if (mask) atomicOr(&bits[(ql0 + nt * 32) * kMxW + wr * 4 + mt], mask);
          }
        lds_barrier();
        for (;;) {
          if (tid < kMxQ) {
            uint32_t n = 0;
            bool rest = false;
#pragma unroll
            for (int wd = 0; wd < kMxW; wd++) {
              uint32_t b = bits[tid * kMxW + wd];
              while (b && n < (uint32_t)kWdPend) {
                pend[tid * kWdPend + n++] = (uint32_t)((rt - t0) * kMxR) + wd * 32 + (__ffs(b) - 1);
                b &= b - 1;
              }
              bits[tid * kMxW + wd] = b;
              rest = rest || b != 0;
            }
            pc[tid] = n;
            if (rest) flags[2] = 1;
          }
          lds_barrier();
          const uint32_t more = flags[2];
          lds_barrier();
          if (tid == 0) flags[2] = 0;
          process();
          if (!more) break;
          // drop the bits the tightened thresholds now exclude
#pragma unroll
          for (int nt = 0; nt < 2; nt++) hq[nt] = H[ql0 + nt * 32];
#pragma unroll
          for (int mt = 0; mt < 4; mt++)
#pragma unroll
            for (int nt = 0; nt < 2; nt++) {
              uint32_t fail = 0;
#pragma unroll
              for (int e = 0; e < 16; e++)
                fail |= (acc[mt][nt][e] >= hq[nt] ? 0u : 1u) << ((e & 3) + 8 * (e >> 2) + rsh);
              if (fail) atomicAnd(&bits[(ql0 + nt * 32) * kMxW + wr * 4 + mt], ~fail);
            }
          lds_barrier();
        }
      }
    }
#pragma unroll
    for (int mt = 0; mt < 4; mt++)
#pragma unroll
      for (int nt = 0; nt < 2; nt++) acc[mt][nt] = (f32x16){};
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  process();  // what is still pending at the part's end; the lists are in place
}

size_t scan_mfma_wide_lds_bytes() {
  return kMxNst * kMxStage + (size_t)kMxQ * kWdPend * 4 + kMxQ * 8 + kMxQ * 4 * 5 + kMxQ * kMxW * 4 + 3 * kMxQ * 4 + 16;
}

template <int M, int P>
static void launch_scan_mfma_wide_t(const MfmaScanArgs& a, uint32_t grid, hipStream_t s) {
  static bool attr = [] {
    (void)hipFuncSetAttribute((const void*)ngt_scan_mfma_wide_kernel<M, P>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    return true;
  }();
  (void)attr;
  hipLaunchKernelGGL((ngt_scan_mfma_wide_kernel<M, P>), dim3(grid), dim3(256), scan_mfma_wide_lds_bytes(), s, a);
}

hipError_t launch_scan_mfma_wide(const MfmaScanArgs& a, int metric, int passes, hipStream_t s) {
  if (a.k < 17 || a.k > 128) return hipErrorNotSupported;
  const uint32_t grid = a.nparts * a.mblocks;
  if (metric == kL2 && passes == 3) launch_scan_mfma_wide_t<kL2, 3>(a, grid, s);
  else if (metric == kL2 && passes == 1) launch_scan_mfma_wide_t<kL2, 1>(a, grid, s);
  else if (metric == kCosine && passes == 3) launch_scan_mfma_wide_t<kCosine, 3>(a, grid, s);
  else if (metric == kCosine && passes == 1) launch_scan_mfma_wide_t<kCosine, 1>(a, grid, s);
  else if (metric == kAngle && passes == 3) launch_scan_mfma_wide_t<kAngle, 3>(a, grid, s);
  else if ((metric == kNormalizedAngle || metric == kNormalizedCosine || metric == kNormalizedL2) && passes == 3)
    launch_scan_mfma_wide_t<kScanDot, 3>(a, grid, s);
  else return hipErrorNotSupported;
  return hipGetLastError();
}

}  // namespace ngt_amd
