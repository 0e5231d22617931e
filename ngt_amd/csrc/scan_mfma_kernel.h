// scan_mfma_kernel.h -- ngt_scan_mfma_kernel (see scan_mfma.hip) and its launch,
// for the translation units that instantiate it: scan_mfma.hip (L2, Cosine)
// and scan_mfma_dot.hip (the dot family, compiled without packed fp32
// operations).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ngt_device.h"
#include "ngt_kernels.h"
#include "scan_mfma_common.h"
#include "search_common.h"

namespace ngt_amd {

constexpr int kMxPend = 16;  // pending candidates per query between processing rounds

// ---------------------------------------------------------------------------
// The scan.
// ---------------------------------------------------------------------------
template <int M, int P>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
ngt_scan_mfma_kernel(MfmaScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const uint32_t k = a.k;
  uint8_t* stage = smem;                                              // [4][24 KiB] ring
  uint64_t* lists = reinterpret_cast<uint64_t*>(smem + kMxNst * kMxStage);  // [256][k]
  uint64_t* thr = lists + (size_t)kMxQ * k;                            // [256] k-th key or ~0
  uint32_t* pend = reinterpret_cast<uint32_t*>(thr + kMxQ);           // [128][16] pending rows
  float* boot = reinterpret_cast<float*>(pend);                        // [128][16] (first tile, before any pending)
  float* pdist = reinterpret_cast<float*>(pend + kMxQ * kMxPend);      // [128][16] their distances
  float* H = pdist + kMxQ * kMxPend;                                   // [128]
  float* HB = H + kMxQ;                                                // [256]
  float* HM = HB + kMxQ;                                               // [256]
  uint32_t* cnt = reinterpret_cast<uint32_t*>(HM + kMxQ);             // [256] list sizes
  uint32_t* pc = cnt + kMxQ;                                           // [256] pending counts
  uint32_t* bits = pc + kMxQ;                                          // [256][4]
  uint32_t* flags = bits + kMxQ * kMxW;                                // [4]

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w & 1, wq = w >> 1;
  // the launch covers query blocks mb0 .. mb0 + mblocks - 1; its parts are
  // a multiple of 8 and part p runs on XCD p % 8 (blockIdx % 8 picks the
  // XCD), so the workgroups streaming one part share that XCD's L2
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
  if (tid < 4) flags[tid] = 0;

  // The comparator's distances of every pending (query, row), then their
  // insertion into the k-lists (one thread per query) and the new filter
  // thresholds.  Called by the whole workgroup.
  auto process = [&]() {
    {  // the comparator's distances: two threads per query
      const uint32_t q = tid & (kMxQ - 1);
      const uint32_t n = min(pc[q], (uint32_t)kMxPend);
      if (n) {
        const float* qp = reinterpret_cast<const float*>(a.queries + (uint64_t)(q0 + q) * a.query_bytes);
        for (uint32_t ci = tid >> 7; ci < n; ci += 2) {
          const uint64_t row = row0 + pend[q * kMxPend + ci];
          pdist[q * kMxPend + ci] =
              dist_lane<M>(qp, reinterpret_cast<const float*>(a.rows + row * a.row_bytes), a.dp, fin);
        }
      }
    }
    lds_barrier();
    if (tid < kMxQ && pc[tid]) {
      const uint32_t n = min(pc[tid], (uint32_t)kMxPend);
      uint32_t c = cnt[tid];
      uint64_t* L = lists + (size_t)tid * k;
      uint64_t th = thr[tid];
      for (uint32_t ci = 0; ci < n; ci++) {
        const float d = pdist[tid * kMxPend + ci];
        if (!(a.radius < 0.0 || (double)d <= a.radius)) continue;
        const uint64_t key = make_key(d, (uint32_t)(row0 + pend[tid * kMxPend + ci]));
        if (key >= th) continue;
        bool dup = false;  // a pair seen again on the bitmap path
        for (uint32_t j = 0; j < c; j++) dup = dup || L[j] == key;
        if (dup) continue;
        uint32_t p = c < k ? c : k - 1;  // the k-th entry drops out when full
        while (p > 0 && L[p - 1] > key) {
          L[p] = L[p - 1];
          p--;
        }
        L[p] = key;
        if (c < k) c++;
        if (c >= k) th = L[k - 1];
      }
      if (a.stats) atomicAdd(&a.stats[0], (unsigned long long)n);
      pc[tid] = 0;
      thr[tid] = th;
      cnt[tid] = c;
    }
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

  // staging ring: k-step g of the part (tile t0 + g / ks, k-step g % ks)
  // goes to slot g % 4 by LDS-DMA; wave w moves blocks w, 4 + w, ... of the
  // 24 1-KiB blocks (rows hi, rows lo: 8 tiles each; queries hi, lo: 4
  // tiles each), so the image is the fragment order of the HBM arrays
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
    if (rt == t0) {
      // bootstrap: the k-th largest of 16 filter values of distinct rows
      // (each lane's 4 largest finite ones of its 32) bounds the k-th
      // distance from above; rows more than the margin HM below it cannot
      // make the top k
#pragma unroll
      for (int nt = 0; nt < 2; nt++) {
        float t4[4] = {-__builtin_huge_valf(), -__builtin_huge_valf(), -__builtin_huge_valf(),
                       -__builtin_huge_valf()};
#pragma unroll
        for (int mt = 0; mt < 4; mt++)
#pragma unroll
          for (int e = 0; e < 16; e++) {
            float v = acc[mt][nt][e];
            if (!(v < __builtin_huge_valf())) v = -__builtin_huge_valf();  // NaN, +inf
#pragma unroll
            for (int j = 0; j < 4; j++) {
              const float hi = fmaxf(t4[j], v), lo = fminf(t4[j], v);
              t4[j] = hi;
              v = lo;
            }
          }
        float* bp = boot + (ql0 + nt * 32) * 16 + (wr * 2 + (lane >> 5)) * 4;
#pragma unroll
        for (int j = 0; j < 4; j++) bp[j] = t4[j];
      }
      lds_barrier();
      if (tid < kMxQ && q0 + tid < a.nq) {
        float v[16];
#pragma unroll
        for (int j = 0; j < 16; j++) v[j] = boot[tid * 16 + j];
        // k-th largest: k - 1 passes of removing the maximum
        float kth = -__builtin_huge_valf();
        for (uint32_t r = 0; r < k; r++) {
          float mx = -__builtin_huge_valf();
          int at = 0;
#pragma unroll
          for (int j = 0; j < 16; j++)
            if (v[j] > mx) {
              mx = v[j];
              at = j;
            }
          kth = mx;
#pragma unroll
          for (int j = 0; j < 16; j++)
            if (j == at) v[j] = -__builtin_huge_valf();
        }
        float hb;
        if constexpr (kIsDotFamily<M>) hb = scan_dot_boot(fin, HB[tid], HM[tid], kth);
        else hb = kth - HM[tid];
        if (hb > H[tid]) H[tid] = hb;
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
                if (n < (uint32_t)kMxPend) pend[q * kMxPend + n] = rbase + mt * 32 + (e & 3) + 8 * (e >> 2);
                if (n + 4 >= (uint32_t)kMxPend) flags[1] = 1;  // process after this tile
                if (n >= (uint32_t)kMxPend) flags[2] = 1;      // overflow: bitmap path
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
      if (tid < kMxQ && pc[tid] > (uint32_t)kMxPend) pc[tid] = kMxPend;
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
              while (b && n < (uint32_t)kMxPend) {
                pend[tid * kMxPend + n++] = (uint32_t)((rt - t0) * kMxR) + wd * 32 + (__ffs(b) - 1);
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
  process();  // what is still pending at the part's end
  for (uint32_t i = tid; i < (uint32_t)kMxQ * k; i += 256) {
    const uint32_t ql = i / k, r = i - ql * k;
    const uint32_t qi = q0 + ql;
    if (qi < a.nq)
      a.partial[((uint64_t)(qi - a.mb0 * kMxQ) * a.nparts + part) * k + r] = r < cnt[ql] ? lists[i] : ~0ull;
  }
}

template <int M, int P>
static void launch_scan_mfma_t(const MfmaScanArgs& a, size_t lds, uint32_t grid, hipStream_t s) {
  static bool attr = [] {
    (void)hipFuncSetAttribute((const void*)ngt_scan_mfma_kernel<M, P>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    return true;
  }();
  (void)attr;
  hipLaunchKernelGGL((ngt_scan_mfma_kernel<M, P>), dim3(grid), dim3(256), lds, s, a);
}

}  // namespace ngt_amd
