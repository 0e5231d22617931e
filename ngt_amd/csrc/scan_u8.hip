// scan_u8.hip -- the exact batch scan of ObjectSpaceRepository::linearSearch
// (lib/NGT/ObjectSpaceRepository.h:466-502) for uint8 rows under L2, on the
// int8 matrix cores.
//
// S = sum (q_i - x_i)^2 over the padded row is an integer.  Both operands are
// shifted by 128 (b ^ 0x80 read as int8), which leaves every difference as it
// was, and S = |q'|^2 + |x'|^2 - 2 q'.x' with q'.x' an exact i32 sum of
// v_mfma_i32_32x32x32_i8 (|q'.x'| <= Dp 2^14, no overflow for Dp <= 1024).
// Integer sums do not depend on the order, so the only thing the fragment
// layout has to respect is that A and B map lanes to bytes the same way: lane
// l of a k-step holds bytes 32 s + 16 (l >> 5) .. + 15 of object l & 31.
//
// While S < 2^24 the reference's distance is exactly (float)sqrt((double)S)
// (scan_u8_bound.h); a survivor with S >= 2^24 (possible for Dp > 256) gets
// the comparator's four float lanes and folds (u8_l2_lane = dist_u8<kL2>).
// Results are ranked by (float distance, id): distinct S round to the same
// float from S ~ 4.2e6 on, so a pair is dropped only when S is above the
// query's integer threshold -- u8_sum_threshold of its k-th distance -- and
// ties at the k-th distance are decided by the keys at insertion.
//
// Work: a workgroup (4 waves, one per SIMD) owns 128 queries x one contiguous
// part of the rows and walks it in 256-row tiles; wave (wr, wq) computes 128
// rows x 64 queries (4 x 2 MFMA tiles, 128 i32 accumulators).
//  * Queries: shifted, in fragment order in LDS for the whole part
//    ([32-query tile][k-step][lane][16 bytes], conflict-free b128 reads).
//  * Rows: straight from the stored rows, which are fragment-shaped as they
//    are (16 contiguous bytes per lane and k-step).  A lane loads a 128-byte
//    chunk of its four rows (4 k-steps x 4 row tiles x 16 bytes) one chunk
//    ahead of the MFMAs that use it and shifts it in registers; the two
//    halves of the wave read the two halves of each row's cache line.
//  * Removed and padding rows carry kU8SumNever in the norm column: their S
//    is above every threshold.  Rows past the table are clamped to the last
//    row for the loads.
//  * Epilogue per tile: S = nq + nx - 2 acc against the query's threshold;
//    survivors go into the query's pending slots as (row, S) (LDS atomics),
//    one thread per query inserts them into the sorted k-list.  A tile with
//    more survivors than slots (the first of a part, tables of duplicates)
//    is redone through a 256-bit candidate bitmap, lowest ids first.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "ngt_device.h"
#include "ngt_kernels.h"
#include "scan_u8_bound.h"
#include "scan_u8_lane.h"

namespace ngt_amd {

typedef int u8s_i32x4 __attribute__((ext_vector_type(4)));
typedef int u8s_i32x16 __attribute__((ext_vector_type(16)));

constexpr int kU8Q = 128;         // queries per workgroup
constexpr int kU8R = 256;         // rows per tile
constexpr int kU8W = kU8R / 32;   // candidate bitmap words per query
constexpr int kU8Chunk = 128;     // bytes of a row per pipeline stage (4 k-steps)
constexpr int kU8Shift = (int)0x80808080u;

// |x'|^2 of every row, kU8SumNever for removed rows and the padding of the
// last tile: one thread per row.
__global__ void __launch_bounds__(256) ngt_scan_u8_norms_kernel(const uint8_t* __restrict__ rows, uint64_t row_bytes,
                                                                uint64_t nrows, const uint8_t* __restrict__ valid,
                                                                int dp, int32_t* __restrict__ nx, uint64_t npad) {
  for (uint64_t id = (uint64_t)blockIdx.x * 256 + threadIdx.x; id < npad; id += (uint64_t)gridDim.x * 256) {
    int32_t s = kU8SumNever;
    if (id < nrows && (valid == nullptr || valid[id])) {
      const uint32_t* xw = reinterpret_cast<const uint32_t*>(rows + id * row_bytes);
      s = 0;
      for (int i = 0; i < (dp >> 2); i++) {
        const uint32_t v = xw[i];
#pragma unroll
        for (int c = 0; c < 4; c++) {
          const int d = (int)((v >> (8 * c)) & 0xff) - 128;
          s += d * d;
        }
      }
    }
    nx[id] = s;
  }
}

__device__ __forceinline__ void u8_lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
ngt_scan_u8_kernel(U8ScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const uint32_t k = a.k, kp = a.pend;
  const uint32_t nch = ((uint32_t)a.dp + kU8Chunk - 1) / kU8Chunk;  // chunks per row
  const uint32_t ks = nch * 4;                                      // k-steps per row, zero-filled past dp
  uint8_t* qfrag = smem;                                            // [4][ks][64][16]
  uint64_t* lists = reinterpret_cast<uint64_t*>(smem + (size_t)4 * ks * 1024);  // [128][k]
  uint32_t* pend = reinterpret_cast<uint32_t*>(lists + (size_t)kU8Q * k);      // [128][kp] pending rows
  int32_t* psum = reinterpret_cast<int32_t*>(pend + kU8Q * kp);                // [128][kp] their S, -1: recompute
  int32_t* H = psum + kU8Q * kp;                                               // [128] thresholds
  int32_t* NQ = H + kU8Q;                                                      // [128] |q'|^2
  uint32_t* cnt = reinterpret_cast<uint32_t*>(NQ + kU8Q);                      // [128] list sizes
  uint32_t* pc = cnt + kU8Q;                                                   // [128] pending counts
  uint32_t* bits = pc + kU8Q;                                                  // [128][8]
  int32_t* nxs = reinterpret_cast<int32_t*>(bits + kU8Q * kU8W);               // [256] the tile's norm column
  uint32_t* flags = reinterpret_cast<uint32_t*>(nxs + kU8R);                   // [4]

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w & 1, wq = w >> 1;
  const int r = lane & 31, h = lane >> 5;
  const uint32_t mb = blockIdx.x % a.mblocks, part = blockIdx.x / a.mblocks;
  const uint32_t q0 = mb * kU8Q;
  const uint32_t t0 = part * a.tiles_per_part;
  uint32_t t1 = t0 + a.tiles_per_part;
  if (t1 > a.ntiles) t1 = a.ntiles;
  const uint64_t row0 = (uint64_t)t0 * kU8R;  // pending rows are offsets from here

  // ---- the queries: shifted fragments, norms, start thresholds
  for (uint32_t i = tid; i < 4 * ks * 64; i += 256) {
    const uint32_t l = i & 63, s = (i >> 6) % ks, qt = (i >> 6) / ks;
    const uint32_t q = q0 + qt * 32 + (l & 31), kofs = 32 * s + 16 * (l >> 5);
    u8s_i32x4 v = {0, 0, 0, 0};
    if (q < a.nq && kofs < (uint32_t)a.dp)
      v = *reinterpret_cast<const u8s_i32x4*>(a.queries + (uint64_t)q * a.query_bytes + kofs) ^ kU8Shift;
    *reinterpret_cast<u8s_i32x4*>(qfrag + (size_t)i * 16) = v;
  }
  if (tid < kU8Q) {
    int32_t s = 0;
    const bool ok = q0 + tid < a.nq;
    if (ok) {
      const uint32_t* qw = reinterpret_cast<const uint32_t*>(a.queries + (uint64_t)(q0 + tid) * a.query_bytes);
      for (int i = 0; i < (a.dp >> 2); i++) {
        const uint32_t v = qw[i];
#pragma unroll
        for (int c = 0; c < 4; c++) {
          const int d = (int)((v >> (8 * c)) & 0xff) - 128;
          s += d * d;
        }
      }
    }
    NQ[tid] = s;
    H[tid] = ok ? a.s_init : -1;
    cnt[tid] = 0;
    pc[tid] = 0;
  }
  for (int i = tid; i < kU8Q * kU8W; i += 256) bits[i] = 0;
  if (tid < 4) flags[tid] = 0;

  // The pending (query, row, S) triples into the k-lists, one thread per
  // query, then the query's new threshold.  Called by the whole workgroup.
  auto process = [&]() {
    if (tid < kU8Q && pc[tid]) {
      const uint32_t n = min(pc[tid], kp);
      uint32_t c = cnt[tid];
      uint64_t* L = lists + (size_t)tid * k;
      uint64_t th = c >= k ? L[k - 1] : ~0ull;
      const uint8_t* qp = a.queries + (uint64_t)(q0 + tid) * a.query_bytes;
      for (uint32_t ci = 0; ci < n; ci++) {
        const uint64_t row = row0 + pend[tid * kp + ci];
        const int32_t S = psum[tid * kp + ci];
        const float d = S >= 0 && S < kU8ExactSums ? u8_sum_distance(S)
                                                    : u8_l2_lane(qp, a.rows + row * a.row_bytes, a.dp);
        if (!(a.radius < 0.0 || (double)d <= a.radius)) continue;
        const uint64_t key = make_key(d, (uint32_t)row);
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
      pc[tid] = 0;
      cnt[tid] = c;
      if (c >= k) H[tid] = min(H[tid], u8_sum_threshold(key_dist(th)));
    }
    u8_lds_barrier();
  };

  // ---- the rows: chunk g of the part is bytes 128 (g % nch) .. + 127 of the
  // rows of tile t0 + g / nch; a lane holds 16 bytes of row r of each of its
  // wave's four row tiles for each of the chunk's four k-steps
  const uint32_t G = (t1 > t0 ? t1 - t0 : 0) * nch;
  u8s_i32x4 cur[4][4], nxt[4][4];  // [k-step][row tile]
  int32_t nx_cur = kU8SumNever, nx_nxt = kU8SumNever;
  auto load_chunk = [&](uint32_t g, u8s_i32x4 (&dst)[4][4], int32_t& nxv) {
    const uint32_t gg = g < G ? g : G - 1;  // past the end: a harmless reload
    const uint32_t t = t0 + gg / nch, c = gg % nch;
    if (c == 0) nxv = a.nx[(uint64_t)t * kU8R + tid];
#pragma unroll
    for (int mt = 0; mt < 4; mt++) {
      uint64_t rid = (uint64_t)t * kU8R + wr * 128 + mt * 32 + r;
      if (rid >= a.nrows) rid = a.nrows - 1;
      const uint8_t* p = a.rows + rid * a.row_bytes + c * kU8Chunk + 16 * h;
#pragma unroll
      for (int s = 0; s < 4; s++) {
        // bytes past dp: the shift's own pattern, 0 once shifted
        u8s_i32x4 v = {kU8Shift, kU8Shift, kU8Shift, kU8Shift};
        if (c * kU8Chunk + 32 * s + 16 * h < (uint32_t)a.dp) v = *reinterpret_cast<const u8s_i32x4*>(p + 32 * s);
        dst[s][mt] = v;
      }
    }
  };

  u8s_i32x16 acc[4][2];
#pragma unroll
  for (int mt = 0; mt < 4; mt++)
#pragma unroll
    for (int nt = 0; nt < 2; nt++) acc[mt][nt] = (u8s_i32x16){};

  __syncthreads();
  if (G) load_chunk(0, cur, nx_cur);
  const int ql0 = wq * 64 + r;  // this lane's query in n-tile 0
  const int rsh = 4 * h;
  for (uint32_t g = 0; g < G; g++) {
    const uint32_t rt = t0 + g / nch, c = g % nch;
    load_chunk(g + 1, nxt, nx_nxt);
#pragma unroll
    for (int s = 0; s < 4; s++) {
      if (c * kU8Chunk + 32 * s < (uint32_t)a.dp) {
        const uint8_t* qb = qfrag + ((size_t)(c * 4 + s) * 64 + lane) * 16;
        u8s_i32x4 b[2];
#pragma unroll
        for (int nt = 0; nt < 2; nt++)
          b[nt] = *reinterpret_cast<const u8s_i32x4*>(qb + (size_t)(wq * 2 + nt) * ks * 1024);
#pragma unroll
        for (int mt = 0; mt < 4; mt++) {
          const u8s_i32x4 av = cur[s][mt] ^ kU8Shift;
#pragma unroll
          for (int nt = 0; nt < 2; nt++)
            acc[mt][nt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, b[nt], acc[mt][nt], 0, 0, 0);
        }
      }
    }
    const int32_t nx_tile = nx_cur;
#pragma unroll
    for (int s = 0; s < 4; s++)
#pragma unroll
      for (int mt = 0; mt < 4; mt++) cur[s][mt] = nxt[s][mt];
    if (c + 1 == nch) nx_cur = nx_nxt;
    if (c + 1 < nch) continue;

    // ---- filter: the lane holds queries ql0 + 32 nt x 64 rows of the tile.
    // A 16-value block whose smallest S is above the threshold is done in a
    // few VALU operations; passing values go into the query's pending slots.
    nxs[tid] = nx_tile;
    u8_lds_barrier();
    int32_t hq[2], nqv[2];
#pragma unroll
    for (int nt = 0; nt < 2; nt++) {
      hq[nt] = H[ql0 + nt * 32];
      nqv[nt] = NQ[ql0 + nt * 32];
    }
    const uint32_t rbase = (rt - t0) * kU8R + wr * 128 + rsh;
    // S of accumulator e of block (mt, nt): row (e & 3) + 8 (e >> 2) + rsh of row tile mt
    auto sum_of = [&](int mt, int nt, int e) -> int32_t {
      return nqv[nt] + nxs[wr * 128 + mt * 32 + (e & 3) + 8 * (e >> 2) + rsh] - 2 * acc[mt][nt][e];
    };
#pragma unroll
    for (int mt = 0; mt < 4; mt++)
#pragma unroll
      for (int nt = 0; nt < 2; nt++) {
        int32_t mn = sum_of(mt, nt, 0);
#pragma unroll
        for (int e = 1; e < 16; e++) mn = min(mn, sum_of(mt, nt, e));
        const bool hit = mn <= hq[nt];
        if (__ballot(hit)) {
          if (hit) {
            const uint32_t q = ql0 + nt * 32;
#pragma unroll
            for (int e = 0; e < 16; e++) {
              const int32_t S = sum_of(mt, nt, e);
              if (S <= hq[nt]) {
                const uint32_t n = atomicAdd(&pc[q], 1u);
                if (n < kp) {
                  pend[q * kp + n] = rbase + mt * 32 + (e & 3) + 8 * (e >> 2);
                  psum[q * kp + n] = S;
                }
                if (n + 4 >= kp) flags[1] = 1;  // process after this tile
                if (n >= kp) flags[2] = 1;      // overflow: bitmap path
              }
            }
          }
        }
      }
    u8_lds_barrier();
    const uint32_t now = flags[1], over = flags[2];
    u8_lds_barrier();
    if (tid == 0) flags[1] = flags[2] = 0;
    if (now) {
      if (tid < kU8Q && pc[tid] > kp) pc[tid] = kp;
      u8_lds_barrier();
      process();
      if (over) {
        // some passing pairs found no slot: redo the tile through the
        // candidate bitmap with the tightened thresholds (pairs already
        // inserted are skipped at insertion, every round takes new bits,
        // lowest ids first; their distances come from the stored bytes)
#pragma unroll
        for (int nt = 0; nt < 2; nt++) hq[nt] = H[ql0 + nt * 32];
#pragma unroll
        for (int mt = 0; mt < 4; mt++)
#pragma unroll
          for (int nt = 0; nt < 2; nt++) {
            uint32_t mask = 0;
#pragma unroll
            for (int e = 0; e < 16; e++)
              mask |= (sum_of(mt, nt, e) <= hq[nt] ? 1u : 0u) << ((e & 3) + 8 * (e >> 2) + rsh);
            if (mask) atomicOr(&bits[(ql0 + nt * 32) * kU8W + wr * 4 + mt], mask);
          }
        u8_lds_barrier();
        for (;;) {
          if (tid < kU8Q) {
            uint32_t n = 0;
            bool rest = false;
#pragma unroll
            for (int wd = 0; wd < kU8W; wd++) {
              uint32_t b = bits[tid * kU8W + wd];
              while (b && n < kp) {
                pend[tid * kp + n] = (uint32_t)((rt - t0) * kU8R) + wd * 32 + (__ffs(b) - 1);
                psum[tid * kp + n] = -1;
                n++;
                b &= b - 1;
              }
              bits[tid * kU8W + wd] = b;
              rest = rest || b != 0;
            }
            pc[tid] = n;
            if (rest) flags[2] = 1;
          }
          u8_lds_barrier();
          const uint32_t more = flags[2];
          u8_lds_barrier();
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
                fail |= (sum_of(mt, nt, e) <= hq[nt] ? 0u : 1u) << ((e & 3) + 8 * (e >> 2) + rsh);
              if (fail) atomicAnd(&bits[(ql0 + nt * 32) * kU8W + wr * 4 + mt], ~fail);
            }
          u8_lds_barrier();
        }
      }
    }
#pragma unroll
    for (int mt = 0; mt < 4; mt++)
#pragma unroll
      for (int nt = 0; nt < 2; nt++) acc[mt][nt] = (u8s_i32x16){};
  }
  __syncthreads();
  process();  // what is still pending at the part's end
  for (uint32_t i = tid; i < (uint32_t)kU8Q * k; i += 256) {
    const uint32_t ql = i / k, rr = i - ql * k;
    const uint32_t qi = q0 + ql;
    if (qi < a.nq) a.partial[((uint64_t)qi * a.nparts + part) * k + rr] = rr < cnt[ql] ? lists[i] : ~0ull;
  }
}

size_t scan_u8_lds_bytes(uint32_t k, int dp, uint32_t pend) {
  const size_t ks = (size_t)((dp + kU8Chunk - 1) / kU8Chunk) * 4;
  return 4 * ks * 1024 + (size_t)kU8Q * k * 8 + (size_t)kU8Q * pend * 8 + kU8Q * 4 * 4 + kU8Q * kU8W * 4 +
         kU8R * 4 + 16;
}

hipError_t launch_scan_u8_norms(const uint8_t* rows, uint64_t row_bytes, uint64_t nrows, const uint8_t* valid, int dp,
                                int32_t* nx, uint64_t npad, hipStream_t s) {
  if (npad == 0) return hipSuccess;
  const uint64_t blocks = std::min<uint64_t>((npad + 255) / 256, 65536);
  hipLaunchKernelGGL(ngt_scan_u8_norms_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, rows, row_bytes, nrows, valid,
                     dp, nx, npad);
  return hipGetLastError();
}

hipError_t launch_scan_u8(const U8ScanArgs& a, hipStream_t s) {
  static bool attr = [] {
    (void)hipFuncSetAttribute((const void*)ngt_scan_u8_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    return true;
  }();
  (void)attr;
  const size_t lds = scan_u8_lds_bytes(a.k, a.dp, a.pend);
  if (lds > 160 * 1024) return hipErrorNotSupported;
  hipLaunchKernelGGL(ngt_scan_u8_kernel, dim3(a.nparts * a.mblocks), dim3(256), lds, s, a);
  return hipGetLastError();
}

}  // namespace ngt_amd
