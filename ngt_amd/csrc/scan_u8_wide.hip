// scan_u8_wide.hip -- the exact batch scan of
// ObjectSpaceRepository::linearSearch (lib/NGT/ObjectSpaceRepository.h:466-502)
// for uint8 rows under L2 with lists of 17 .. 128 results, on the int8 matrix
// cores.
//
// The arithmetic is scan_u8.hip's: S = sum (q_i - x_i)^2 over the padded row
// is one exact integer, S = |q'|^2 + |x'|^2 - 2 q'.x' with both operands
// shifted by 128 and q'.x' an exact i32 sum of v_mfma_i32_32x32x32_i8.  While
// S < 2^24 the reference's distance is (float)sqrt((double)S); a survivor
// with S >= 2^24 gets the comparator on one lane (u8_l2_lane = dist_u8<kL2>).
// The filter is an integer compare against u8_sum_threshold of the query's
// k-th distance (scan_u8_bound.h): no float margin.  Results are ranked by
// (float distance, id), never by S -- distinct sums share a float distance
// from S ~ 4.2e6 on -- and ties at the k-th distance pass the filter and are
// decided by the keys.
//
// Work, as in scan_u8.hip: a workgroup (4 waves, one per SIMD) owns 128
// queries x one contiguous part of the rows and walks it in 256-row tiles;
// wave (wr, wq) computes 128 rows x 64 queries (4 x 2 MFMA tiles).  Shifted
// queries sit in LDS in fragment order for the whole part; rows come straight
// from the stored bytes, a 128-byte chunk ahead of the MFMAs.  The per-row
// state is scan_u8.hip's norm column (|x'|^2, kU8SumNever for removed rows,
// the dummy row 0 and the padding of the last tile).
//
// Its own:
//  * Epilogue: the tile's norm column goes through LDS negated, and a value is
//    m = 2 acc - |x'|^2 (one shift-add), which passes iff m >= |q'|^2 - H_q;
//    a 16-value block is reduced by its maximum before any branch, and
//    S = |q'|^2 - m only for the values that pass.
//  * Lists as in scan_u8cos.hip, nothing in LDS grows with k: a (query, part)
//    list lives in its slot of the partial buffer (sorted u64 keys, ~0 beyond
//    its length); query q belongs to wave q & 3, which holds the list two keys
//    per lane and merges a round's candidates by ballot rank.  Pending slots
//    hold (row offset, S): lane c finishes candidate c, applies the radius
//    rule and compares the key against the k-th key.  One thread per query
//    recomputes the integer threshold only when that query's k-th key changed.
//  * The number of pending slots per query (64, 32 or 16) is the host's, from
//    the LDS the queries leave.  A tile with more passing values than slots --
//    the first of a part, tables of duplicates -- is redone from the
//    accumulators in windows of as many rows as there are slots, lowest rows
//    first, a round and a threshold refresh after each window: a window cannot
//    overflow, and pairs already in the list drop out by their key.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ngt_device.h"
#include "ngt_kernels.h"
#include "scan_mfma_common.h"
#include "scan_u8_bound.h"
#include "scan_u8_lane.h"
#include "unchecked_set.h"

namespace ngt_amd {

typedef int u8w_i32x4 __attribute__((ext_vector_type(4)));
typedef int u8w_i32x16 __attribute__((ext_vector_type(16)));

constexpr int kU8wQ = 128;      // queries per workgroup
constexpr int kU8wR = 256;      // rows per tile
constexpr int kU8wChunk = 128;  // bytes of a row per pipeline stage (4 k-steps)
constexpr int kU8wShift = (int)0x80808080u;

__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
ngt_scan_u8_wide_kernel(U8ScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const uint32_t k = a.k, kp = a.pend;
  const uint32_t nch = ((uint32_t)a.dp + kU8wChunk - 1) / kU8wChunk;  // chunks per row
  const uint32_t ks = nch * 4;                                        // k-steps per row, zero-filled past dp
  uint8_t* qfrag = smem;                                              // [4][ks][64][16]
  uint32_t* pend = reinterpret_cast<uint32_t*>(smem + (size_t)4 * ks * 1024);  // [128][kp] pending row offsets
  int32_t* psum = reinterpret_cast<int32_t*>(pend + kU8wQ * kp);               // [128][kp] their S
  uint64_t* thr = reinterpret_cast<uint64_t*>(psum + kU8wQ * kp);              // [128] k-th key or ~0
  int32_t* H = reinterpret_cast<int32_t*>(thr + kU8wQ);                        // [128] thresholds on S
  int32_t* NQ = H + kU8wQ;                                                     // [128] |q'|^2
  uint32_t* cnt = reinterpret_cast<uint32_t*>(NQ + kU8wQ);                     // [128] list lengths
  uint32_t* pc = cnt + kU8wQ;                                                  // [128] pending counts
  int32_t* nxs = reinterpret_cast<int32_t*>(pc + kU8wQ);                       // [256] the tile's -|x'|^2
  uint32_t* flags = reinterpret_cast<uint32_t*>(nxs + kU8wR);                  // [4]

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w & 1, wq = w >> 1;
  const int r = lane & 31, h = lane >> 5;
  const uint32_t mb = blockIdx.x % a.mblocks, part = blockIdx.x / a.mblocks;
  const uint32_t q0 = mb * kU8wQ;
  const uint32_t t0 = part * a.tiles_per_part;
  uint32_t t1 = t0 + a.tiles_per_part;
  if (t1 > a.ntiles) t1 = a.ntiles;
  const uint64_t row0 = (uint64_t)t0 * kU8wR;  // pending rows are offsets from here

  // the list of the workgroup's query ql in this part
  auto list_of = [&](uint32_t ql) -> uint64_t* { return a.partial + ((uint64_t)(q0 + ql) * a.nparts + part) * k; };

  // ---- the queries: shifted fragments, norms, start thresholds
  for (uint32_t i = tid; i < 4 * ks * 64; i += 256) {
    const uint32_t l = i & 63, s = (i >> 6) % ks, qt = (i >> 6) / ks;
    const uint32_t q = q0 + qt * 32 + (l & 31), kofs = 32 * s + 16 * (l >> 5);
    u8w_i32x4 v = {0, 0, 0, 0};  // past dp and past the batch: 0, adds nothing to q'.x'
    if (q < a.nq && kofs < (uint32_t)a.dp)
      v = *reinterpret_cast<const u8w_i32x4*>(a.queries + (uint64_t)q * a.query_bytes + kofs) ^ kU8wShift;
    *reinterpret_cast<u8w_i32x4*>(qfrag + (size_t)i * 16) = v;
  }
  if (tid < kU8wQ) {
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
    H[tid] = ok ? a.s_init : -1;  // a query past the batch: no S >= 0 passes
    thr[tid] = ~0ull;
    cnt[tid] = 0;
    pc[tid] = 0;
  }
  if (tid < 4) flags[tid] = 0;
  // empty lists: all ones, which is also what the merge expects beyond a
  // list's length (entries are only ever written below the length)
  for (uint32_t ql = w; ql < (uint32_t)kU8wQ && q0 + ql < a.nq; ql += 4) {
    uint64_t* L = list_of(ql);
    for (uint32_t i = lane; i < k; i += 64)
      __hip_atomic_store(L + i, ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  uint64_t seen = ~0ull;  // tid < 128: the k-th key H[tid] was last derived from

  // A round: every query with pending candidates, by its wave; then the new
  // filter thresholds.  Called by the whole workgroup.
  auto process = [&]() {
    const uint32_t mine = (uint32_t)w + 4u * (uint32_t)(lane & 31);
    uint64_t todo = ballot64(lane < 32 && q0 + mine < a.nq && pc[mine] != 0);
    while (todo) {
      const uint32_t q = (uint32_t)w + 4u * (uint32_t)(__ffsll((long long)todo) - 1);
      todo &= todo - 1;
      const uint32_t n = min(pc[q], kp);
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
      // lane c: the reference's distance of pending candidate c from its sum
      // (or from the stored bytes), the radius rule, the key against the k-th key
      uint64_t key = ~0ull;
      bool ok = false;
      if ((uint32_t)lane < n) {
        const uint64_t row = row0 + pend[q * kp + lane];
        const int32_t S = psum[q * kp + lane];
        const float d = S < kU8ExactSums ? u8_sum_distance(S)
                                         : u8_l2_lane(a.queries + (uint64_t)(q0 + q) * a.query_bytes,
                                                      a.rows + row * a.row_bytes, a.dp);
        if (a.radius < 0.0 || (double)d <= a.radius) {
          key = make_key(d, (uint32_t)row);
          ok = key < th;
        }
      }
      // list keys below each candidate; a candidate that is in the list
      // already (a pair seen again when a tile is redone) drops out
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
      }
    }
    // this wave's list writes land before any later round loads them
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    lds_barrier();
    if (tid < kU8wQ && q0 + tid < a.nq) {
      const uint64_t th = thr[tid];
      if (th != seen) {
        seen = th;
        H[tid] = min(H[tid], u8_sum_threshold(key_dist(th)));
      }
    }
    lds_barrier();
  };

  // ---- the rows: chunk g of the part is bytes 128 (g % nch) .. + 127 of the
  // rows of tile t0 + g / nch; a lane holds 16 bytes of row r of each of its
  // wave's four row tiles for each of the chunk's four k-steps
  const uint32_t G = (t1 > t0 ? t1 - t0 : 0) * nch;
  u8w_i32x4 cur[4][4], nxt[4][4];  // [k-step][row tile]
  int32_t nx_cur = kU8SumNever, nx_nxt = kU8SumNever;
  auto load_chunk = [&](uint32_t g, u8w_i32x4 (&dst)[4][4], int32_t& nxv) {
    const uint32_t gg = g < G ? g : G - 1;  // past the end: a harmless reload
    const uint32_t t = t0 + gg / nch, c = gg % nch;
    if (c == 0) nxv = a.nx[(uint64_t)t * kU8wR + tid];
#pragma unroll
    for (int mt = 0; mt < 4; mt++) {
      uint64_t rid = (uint64_t)t * kU8wR + wr * 128 + mt * 32 + r;
      if (rid >= a.nrows) rid = a.nrows - 1;
      const uint8_t* p = a.rows + rid * a.row_bytes + c * kU8wChunk + 16 * h;
#pragma unroll
      for (int s = 0; s < 4; s++) {
        // bytes past dp: the shift's own pattern, 0 once shifted
        u8w_i32x4 v = {kU8wShift, kU8wShift, kU8wShift, kU8wShift};
        if (c * kU8wChunk + 32 * s + 16 * h < (uint32_t)a.dp) v = *reinterpret_cast<const u8w_i32x4*>(p + 32 * s);
        dst[s][mt] = v;
      }
    }
  };

  u8w_i32x16 acc[4][2];
  auto reset_acc = [&]() {
#pragma unroll
    for (int mt = 0; mt < 4; mt++)
#pragma unroll
      for (int nt = 0; nt < 2; nt++) acc[mt][nt] = (u8w_i32x16){};
  };
  reset_acc();

  __syncthreads();
  if (G) load_chunk(0, cur, nx_cur);
  const int ql0 = wq * 64 + r;  // this lane's query in n-tile 0
  const int rsh = 4 * h;
  for (uint32_t g = 0; g < G; g++) {
    const uint32_t rt = t0 + g / nch, c = g % nch;
    load_chunk(g + 1, nxt, nx_nxt);
#pragma unroll
    for (int s = 0; s < 4; s++) {
      if (c * kU8wChunk + 32 * s < (uint32_t)a.dp) {
        const uint8_t* qb = qfrag + ((size_t)(c * 4 + s) * 64 + lane) * 16;
        u8w_i32x4 b[2];
#pragma unroll
        for (int nt = 0; nt < 2; nt++)
          b[nt] = *reinterpret_cast<const u8w_i32x4*>(qb + (size_t)(wq * 2 + nt) * ks * 1024);
#pragma unroll
        for (int mt = 0; mt < 4; mt++) {
          const u8w_i32x4 av = cur[s][mt] ^ kU8wShift;
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
    // Accumulator e of block (mt, nt) is row (e & 3) + 8 (e >> 2) + rsh of row
    // tile mt.  S = nq + nx - 2 acc <= H  iff  m = 2 acc - nx >= nq - H: a
    // 16-value block whose largest m is below that is done without a branch;
    // passing values go into the query's pending slots as (row offset, S).
    nxs[tid] = -nx_tile;
    lds_barrier();
    int32_t nqv[2], lim[2];
#pragma unroll
    for (int nt = 0; nt < 2; nt++) {
      nqv[nt] = NQ[ql0 + nt * 32];
      lim[nt] = nqv[nt] - H[ql0 + nt * 32];
    }
    const uint32_t tbase = (rt - t0) * kU8wR;
    const int lrow = wr * 128 + rsh;  // + mt * 32 + (e & 3) + 8 (e >> 2): the row in the tile
#pragma unroll
    for (int mt = 0; mt < 4; mt++) {
      int32_t nnx[16];
#pragma unroll
      for (int e = 0; e < 16; e++) nnx[e] = nxs[lrow + mt * 32 + (e & 3) + 8 * (e >> 2)];
#pragma unroll
      for (int nt = 0; nt < 2; nt++) {
        auto value = [&](int e) -> int32_t { return 2 * acc[mt][nt][e] + nnx[e]; };
        int32_t mx = value(0);
#pragma unroll
        for (int e = 1; e < 16; e++) mx = max(mx, value(e));
        const bool hit = mx >= lim[nt];
        if (__ballot(hit)) {
          if (hit) {
            const uint32_t q = ql0 + nt * 32;
#pragma unroll
            for (int e = 0; e < 16; e++)
              if (value(e) >= lim[nt]) {
                const uint32_t n = atomicAdd(&pc[q], 1u);
                if (n < kp) {
                  pend[q * kp + n] = tbase + lrow + mt * 32 + (e & 3) + 8 * (e >> 2);
                  psum[q * kp + n] = nqv[nt] - value(e);
                }
                if (n + (kp >> 2) >= kp) flags[1] = 1;  // process after this tile
                if (n >= kp) flags[2] = 1;              // overflow: redo in windows
              }
          }
        }
      }
    }
    lds_barrier();
    const uint32_t now = flags[1], over = flags[2];
    lds_barrier();
    if (tid == 0) flags[1] = flags[2] = 0;
    if (now) {
      if (tid < kU8wQ && pc[tid] > kp) pc[tid] = kp;
      lds_barrier();
      process();
      if (over) {
        // some passing pairs found no slot: the tile again from the
        // accumulators, kp rows at a time, lowest rows first, with the
        // thresholds of the round before.  A window holds at most kp rows, so
        // every passing pair has a slot.
        for (uint32_t lo = 0; lo < (uint32_t)kU8wR; lo += kp) {
#pragma unroll
          for (int nt = 0; nt < 2; nt++) lim[nt] = nqv[nt] - H[ql0 + nt * 32];
#pragma unroll
          for (int mt = 0; mt < 4; mt++) {
            const uint32_t tl = wr * 128 + mt * 32;  // the row tile's rows: wave-uniform test
            if (tl < lo + kp && tl + 32 > lo) {
#pragma unroll
              for (int e = 0; e < 16; e++) {
                const uint32_t row = lrow + mt * 32 + (e & 3) + 8 * (e >> 2);
                if (row >= lo && row < lo + kp) {
                  const int32_t nne = nxs[row];
#pragma unroll
                  for (int nt = 0; nt < 2; nt++) {
                    const int32_t m = 2 * acc[mt][nt][e] + nne;
                    if (m >= lim[nt]) {
                      const uint32_t q = ql0 + nt * 32;
                      const uint32_t n = atomicAdd(&pc[q], 1u);
                      if (n < kp) {  // always
                        pend[q * kp + n] = tbase + row;
                        psum[q * kp + n] = nqv[nt] - m;
                      }
                    }
                  }
                }
              }
            }
          }
          lds_barrier();
          process();
        }
      }
    }
    reset_acc();
  }
  __syncthreads();
  process();  // what is still pending at the part's end; the lists are in place
}

size_t scan_u8_wide_lds_bytes(int dp, uint32_t pend) {
  const size_t ks = (size_t)((dp + kU8wChunk - 1) / kU8wChunk) * 4;
  return 4 * ks * 1024 + (size_t)kU8wQ * pend * 8 + kU8wQ * 8 + kU8wQ * 4 * 4 + kU8wR * 4 + 16;
}

// pending slots per query: the most of 64, 32, 16 that fit beside the queries; 0: none does
uint32_t scan_u8_wide_pend(int dp) {
  for (uint32_t p = 64; p >= 16; p >>= 1)
    if (scan_u8_wide_lds_bytes(dp, p) <= 160 * 1024) return p;
  return 0;
}

hipError_t launch_scan_u8_wide(const U8ScanArgs& a, hipStream_t s) {
  static bool attr = [] {
    (void)hipFuncSetAttribute((const void*)ngt_scan_u8_wide_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    return true;
  }();
  (void)attr;
  if (a.k < 17 || a.k > 128 || a.dp < 16 || a.dp > 1024 || a.dp % 16) return hipErrorNotSupported;
  if (a.pend != 16 && a.pend != 32 && a.pend != 64) return hipErrorNotSupported;
  const size_t lds = scan_u8_wide_lds_bytes(a.dp, a.pend);
  if (lds > 160 * 1024) return hipErrorNotSupported;
  hipLaunchKernelGGL(ngt_scan_u8_wide_kernel, dim3(a.nparts * a.mblocks), dim3(256), lds, s, a);
  return hipGetLastError();
}

}  // namespace ngt_amd
