// scan_u8cos.hip -- the exact batch scan of ObjectSpaceRepository::linearSearch
// (lib/NGT/ObjectSpaceRepository.h:466-502) for uint8 rows under Cosine and
// Angle, on the int8 matrix cores, lists of 1 .. 128 results.
//
// The comparator's distance is a function of three exact integers,
//   c = (double)s / sqrt((double)na * (double)nb),  s = q.x, na = |q|^2, nb = |x|^2
// (dist_u8<kCosine> / dist_u8<kAngle>, ngt_device.h), so a pair that survives
// the filter is finished bit for bit from (s, na, nb): no row is read again.
//
// s: both operands are shifted by 128 (b ^ 0x80 read as int8) and
// v_mfma_i32_32x32x32_i8 sums q'.x' exactly; over the Dp stored bytes
//   s = q'.x' + (128 sum q - 16384 Dp) + 128 sum x.
// The query's term sits in a register of the lanes that hold its accumulators,
// the row's term is the row's correction column, and one three-operand add
// (v_add3_u32) rebuilds s; accumulators that start from the query's term
// instead cost the kernel 368 bytes of scratch per lane.  Fragment bytes past Dp are 0 after the shift on the
// query's side, so they add nothing, and Dp in the correction is the stored
// row's.  s <= 255^2 1024 < 2^27 and every partial sum stays below 2^27 in
// magnitude: exact in i32.
//
// Filter (scan_u8cos_bound.h): the pair is dropped iff
//   fmaf(-H_q, rx, (float)s) < 0,  rx = (float)sqrt(nb),
// H_q from the query's k-th distance (or the radius) with a proven margin;
// a dropped pair's distance is strictly above the k-th, so ties at the k-th
// distance survive and are decided by the keys (float distance, id) --
// distinct c share a float distance.  Removed rows, the dummy row 0 and the
// padding of the last tile carry rx = NaN: no threshold passes them.
//
// Work, as in scan_u8.hip: a workgroup (4 waves, one per SIMD) owns 128
// queries x one contiguous part of the rows and walks it in 256-row tiles;
// wave (wr, wq) computes 128 rows x 64 queries (4 x 2 MFMA tiles).  Shifted
// queries sit in LDS in fragment order for the whole part; rows come straight
// from the stored bytes, a 128-byte chunk ahead of the MFMAs.
//
// Its own:
//  * Epilogue per value, as every row has its own rx: the tile's rx and
//    correction columns go through LDS, a lane takes the 16 rows of a block
//    into registers once for its two queries, and a value costs the add, a
//    conversion, one fused multiply-add and a max; a 16-value block is reduced
//    before any branch.
//  * One survivor design for k = 1 .. 128, nothing in LDS grows with k.  A
//    (query, part) list lives in its slot of the partial buffer (sorted u64
//    keys, ~0 beyond its length); query q belongs to wave q & 3, which merges
//    by ballot rank as scan_mfma_wide.hip does.  Pending slots hold (row
//    offset, s): in a round lane c finishes candidate c from (s, na, nb[row]).
//  * The number of pending slots per query (64, 32 or 16) is the host's, from
//    the LDS the queries leave.  A tile with more survivors than slots -- the
//    first of a part, tables of duplicates -- is redone in windows of as many
//    rows as there are slots, lowest rows first, the thresholds refreshed
//    after each window: a window cannot overflow, and its candidates carry
//    their s like any other.  Pairs already in the list drop out by their key.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "ngt_device.h"
#include "ngt_kernels.h"
#include "scan_mfma_common.h"
#include "scan_u8cos_bound.h"
#include "unchecked_set.h"

namespace ngt_amd {

typedef int u8c_i32x4 __attribute__((ext_vector_type(4)));
typedef int u8c_i32x16 __attribute__((ext_vector_type(16)));

constexpr int kU8cQ = 128;         // queries per workgroup
constexpr int kU8cR = 256;         // rows per tile
constexpr int kU8cChunk = 128;     // bytes of a row per pipeline stage (4 k-steps)
constexpr int kU8cShift = (int)0x80808080u;

// sum x and sum x^2 over the dp stored bytes (dp a multiple of 4)
__device__ __forceinline__ void u8c_sums(const uint8_t* __restrict__ p, int dp, uint32_t& sum, uint32_t& sq) {
  const uint32_t* w = reinterpret_cast<const uint32_t*>(p);
  sum = 0;
  sq = 0;
  for (int i = 0; i < (dp >> 2); i++) {
    const uint32_t v = w[i];
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const uint32_t b = (v >> (8 * c)) & 0xff;
      sum += b;
      sq += b * b;
    }
  }
}

// The per-row state: correction 128 sum x, nb = |x|^2, rx = (float)sqrt(nb);
// NaN in rx for removed rows, the dummy row 0 and the padding of the last tile.
__global__ void __launch_bounds__(256) ngt_scan_u8cos_rows_kernel(const uint8_t* __restrict__ rows, uint64_t row_bytes,
                                                                  uint64_t nrows, const uint8_t* __restrict__ valid,
                                                                  int dp, int32_t* __restrict__ cx,
                                                                  uint32_t* __restrict__ nb, float* __restrict__ rx,
                                                                  uint64_t npad) {
  for (uint64_t id = (uint64_t)blockIdx.x * 256 + threadIdx.x; id < npad; id += (uint64_t)gridDim.x * 256) {
    uint32_t sum = 0, sq = 0;
    float r = __builtin_nanf("");
    if (id > 0 && id < nrows && (valid == nullptr || valid[id])) {
      u8c_sums(rows + id * row_bytes, dp, sum, sq);
      r = u8cos_rx(sq);
    }
    cx[id] = (int32_t)(128u * sum);
    nb[id] = sq;
    rx[id] = r;
  }
}

template <int M>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 1)))
ngt_scan_u8cos_kernel(U8CosScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const uint32_t k = a.k, kp = a.pend;
  const uint32_t nch = ((uint32_t)a.dp + kU8cChunk - 1) / kU8cChunk;  // chunks per row
  const uint32_t ks = nch * 4;                                        // k-steps per row, zero-filled past dp
  uint8_t* qfrag = smem;                                              // [4][ks][64][16]
  uint32_t* pend = reinterpret_cast<uint32_t*>(smem + (size_t)4 * ks * 1024);  // [128][kp] pending row offsets
  int32_t* psum = reinterpret_cast<int32_t*>(pend + kU8cQ * kp);               // [128][kp] their s
  uint64_t* thr = reinterpret_cast<uint64_t*>(psum + kU8cQ * kp);              // [128] k-th key or ~0
  float* H = reinterpret_cast<float*>(thr + kU8cQ);                            // [128] thresholds
  uint32_t* NA = reinterpret_cast<uint32_t*>(H + kU8cQ);                       // [128] |q|^2
  uint32_t* cnt = NA + kU8cQ;                                                  // [128] list lengths
  uint32_t* pc = cnt + kU8cQ;                                                  // [128] pending counts
  int32_t* cxs = reinterpret_cast<int32_t*>(pc + kU8cQ);                       // [256] the tile's corrections
  float* rxs = reinterpret_cast<float*>(cxs + kU8cR);                          // [256] the tile's rx
  uint32_t* flags = reinterpret_cast<uint32_t*>(rxs + kU8cR);                  // [4]

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int wr = w & 1, wq = w >> 1;
  const int r = lane & 31, h = lane >> 5;
  const uint32_t mb = blockIdx.x % a.mblocks, part = blockIdx.x / a.mblocks;
  const uint32_t q0 = mb * kU8cQ;
  const uint32_t t0 = part * a.tiles_per_part;
  uint32_t t1 = t0 + a.tiles_per_part;
  if (t1 > a.ntiles) t1 = a.ntiles;
  const uint64_t row0 = (uint64_t)t0 * kU8cR;  // pending rows are offsets from here

  // the list of the workgroup's query ql in this part
  auto list_of = [&](uint32_t ql) -> uint64_t* { return a.partial + ((uint64_t)(q0 + ql) * a.nparts + part) * k; };

  // ---- the queries: shifted fragments, sums, start thresholds
  for (uint32_t i = tid; i < 4 * ks * 64; i += 256) {
    const uint32_t l = i & 63, s = (i >> 6) % ks, qt = (i >> 6) / ks;
    const uint32_t q = q0 + qt * 32 + (l & 31), kofs = 32 * s + 16 * (l >> 5);
    u8c_i32x4 v = {0, 0, 0, 0};  // past dp and past the batch: 0, adds nothing to q'.x'
    if (q < a.nq && kofs < (uint32_t)a.dp)
      v = *reinterpret_cast<const u8c_i32x4*>(a.queries + (uint64_t)q * a.query_bytes + kofs) ^ kU8cShift;
    *reinterpret_cast<u8c_i32x4*>(qfrag + (size_t)i * 16) = v;
  }
  // the query's term of s, kept by the four threads that hold its accumulators
  const int ql0 = wq * 64 + r;  // this lane's query in n-tile 0
  int32_t cq[2] = {0, 0};
#pragma unroll
  for (int nt = 0; nt < 2; nt++)
    if (q0 + ql0 + nt * 32 < a.nq) {
      uint32_t sum, sq;
      u8c_sums(a.queries + (uint64_t)(q0 + ql0 + nt * 32) * a.query_bytes, a.dp, sum, sq);
      cq[nt] = (int32_t)(128u * sum) - 16384 * a.dp;
      if (wr == 0 && h == 0) NA[ql0 + nt * 32] = sq;
    } else if (wr == 0 && h == 0) {
      NA[ql0 + nt * 32] = 0;
    }
  if (tid < kU8cQ) {
    thr[tid] = ~0ull;
    cnt[tid] = 0;
    pc[tid] = 0;
  }
  if (tid < 4) flags[tid] = 0;
  // empty lists: all ones, which is also what the merge expects beyond a
  // list's length (entries are only ever written below the length)
  for (uint32_t ql = w; ql < (uint32_t)kU8cQ && q0 + ql < a.nq; ql += 4) {
    uint64_t* L = list_of(ql);
    for (uint32_t i = lane; i < k; i += 64)
      __hip_atomic_store(L + i, ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  // a query past the batch: +inf drops every pair (rx = 0 gives NaN, which passes nothing either)
  if (tid < kU8cQ) H[tid] = q0 + tid < a.nq ? u8cos_h(M, a.kd_init, NA[tid]) : __builtin_huge_valf();
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
      // lane c: the comparator's distance of pending candidate c from its
      // integers, the radius rule, the key against the k-th key
      uint64_t key = ~0ull;
      bool ok = false;
      if ((uint32_t)lane < n) {
        const uint64_t row = row0 + pend[q * kp + lane];
        const float d = u8cos_distance(M, (uint32_t)psum[q * kp + lane], NA[q], a.nb[row]);
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
    if (tid < kU8cQ && q0 + tid < a.nq) {
      const uint64_t th = thr[tid];
      if (th != seen) {
        seen = th;
        // a NaN k-th distance (rows or a query of zeros) bounds nothing: fminf keeps the radius
        H[tid] = fmaxf(H[tid], u8cos_h(M, fminf(a.kd_init, key_dist(th)), NA[tid]));
      }
    }
    lds_barrier();
  };

  // ---- the rows: chunk g of the part is bytes 128 (g % nch) .. + 127 of the
  // rows of tile t0 + g / nch; a lane holds 16 bytes of row r of each of its
  // wave's four row tiles for each of the chunk's four k-steps
  const uint32_t G = (t1 > t0 ? t1 - t0 : 0) * nch;
  u8c_i32x4 cur[4][4], nxt[4][4];  // [k-step][row tile]
  int32_t cx_cur = 0, cx_nxt = 0;
  float rx_cur = __builtin_nanf(""), rx_nxt = __builtin_nanf("");
  auto load_chunk = [&](uint32_t g, u8c_i32x4 (&dst)[4][4], int32_t& cxv, float& rxv) {
    const uint32_t gg = g < G ? g : G - 1;  // past the end: a harmless reload
    const uint32_t t = t0 + gg / nch, c = gg % nch;
    if (c == 0) {
      cxv = a.cx[(uint64_t)t * kU8cR + tid];
      rxv = a.rx[(uint64_t)t * kU8cR + tid];
    }
#pragma unroll
    for (int mt = 0; mt < 4; mt++) {
      uint64_t rid = (uint64_t)t * kU8cR + wr * 128 + mt * 32 + r;
      if (rid >= a.nrows) rid = a.nrows - 1;
      const uint8_t* p = a.rows + rid * a.row_bytes + c * kU8cChunk + 16 * h;
#pragma unroll
      for (int s = 0; s < 4; s++) {
        // bytes past dp: the shift's own pattern, 0 once shifted (the query's are 0 too)
        u8c_i32x4 v = {kU8cShift, kU8cShift, kU8cShift, kU8cShift};
        if (c * kU8cChunk + 32 * s + 16 * h < (uint32_t)a.dp) v = *reinterpret_cast<const u8c_i32x4*>(p + 32 * s);
        dst[s][mt] = v;
      }
    }
  };

  u8c_i32x16 acc[4][2];
  auto reset_acc = [&]() {
#pragma unroll
    for (int mt = 0; mt < 4; mt++)
#pragma unroll
      for (int nt = 0; nt < 2; nt++) acc[mt][nt] = (u8c_i32x16){};
  };
  reset_acc();

  __syncthreads();
  if (G) load_chunk(0, cur, cx_cur, rx_cur);
  const int rsh = 4 * h;
  for (uint32_t g = 0; g < G; g++) {
    const uint32_t rt = t0 + g / nch, c = g % nch;
    load_chunk(g + 1, nxt, cx_nxt, rx_nxt);
#pragma unroll
    for (int s = 0; s < 4; s++) {
      if (c * kU8cChunk + 32 * s < (uint32_t)a.dp) {
        const uint8_t* qb = qfrag + ((size_t)(c * 4 + s) * 64 + lane) * 16;
        u8c_i32x4 b[2];
#pragma unroll
        for (int nt = 0; nt < 2; nt++)
          b[nt] = *reinterpret_cast<const u8c_i32x4*>(qb + (size_t)(wq * 2 + nt) * ks * 1024);
#pragma unroll
        for (int mt = 0; mt < 4; mt++) {
          const u8c_i32x4 av = cur[s][mt] ^ kU8cShift;
#pragma unroll
          for (int nt = 0; nt < 2; nt++)
            acc[mt][nt] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av, b[nt], acc[mt][nt], 0, 0, 0);
        }
      }
    }
    const int32_t cx_tile = cx_cur;
    const float rx_tile = rx_cur;
#pragma unroll
    for (int s = 0; s < 4; s++)
#pragma unroll
      for (int mt = 0; mt < 4; mt++) cur[s][mt] = nxt[s][mt];
    if (c + 1 == nch) {
      cx_cur = cx_nxt;
      rx_cur = rx_nxt;
    }
    if (c + 1 < nch) continue;

    // ---- filter: the lane holds queries ql0 + 32 nt x 64 rows of the tile.
    // Accumulator e of block (mt, nt) is row (e & 3) + 8 (e >> 2) + rsh of row
    // tile mt.  A 16-value block whose largest filter value is below zero is
    // done without a branch; passing values go into the query's pending slots
    // as (row offset, s).
    cxs[tid] = cx_tile;
    rxs[tid] = rx_tile;
    lds_barrier();
    float nh[2];
#pragma unroll
    for (int nt = 0; nt < 2; nt++) nh[nt] = -H[ql0 + nt * 32];
    const uint32_t tbase = (rt - t0) * kU8cR;
    const int lrow = wr * 128 + rsh;  // + mt * 32 + (e & 3) + 8 (e >> 2): the row in the tile
#pragma unroll
    for (int mt = 0; mt < 4; mt++) {
      int32_t cxv[16];
      float rxv[16];
#pragma unroll
      for (int e = 0; e < 16; e++) {
        cxv[e] = cxs[lrow + mt * 32 + (e & 3) + 8 * (e >> 2)];
        rxv[e] = rxs[lrow + mt * 32 + (e & 3) + 8 * (e >> 2)];
      }
#pragma unroll
      for (int nt = 0; nt < 2; nt++) {
        auto value = [&](int e) { return __builtin_fmaf(nh[nt], rxv[e], (float)(acc[mt][nt][e] + cxv[e] + cq[nt])); };
        float mx = value(0);
#pragma unroll
        for (int e = 1; e < 16; e++) mx = fmaxf(mx, value(e));
        const bool hit = mx >= 0.0f;
        if (__ballot(hit)) {
          if (hit) {
            const uint32_t q = ql0 + nt * 32;
#pragma unroll
            for (int e = 0; e < 16; e++)
              if (value(e) >= 0.0f) {
                const uint32_t n = atomicAdd(&pc[q], 1u);
                if (n < kp) {
                  pend[q * kp + n] = tbase + lrow + mt * 32 + (e & 3) + 8 * (e >> 2);
                  psum[q * kp + n] = acc[mt][nt][e] + cxv[e] + cq[nt];
                }
                if (n + (kp >> 2) >= kp) flags[1] = 1;  // process after this tile
                if (n >= kp) flags[2] = 1;              // overflow: redo in windows
              }
          }
        }
        // one block at a time: the scheduler would otherwise convert every
        // accumulator of the tile at once and run out of registers
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    lds_barrier();
    const uint32_t now = flags[1], over = flags[2];
    lds_barrier();
    if (tid == 0) flags[1] = flags[2] = 0;
    if (now) {
      if (tid < kU8cQ && pc[tid] > kp) pc[tid] = kp;
      lds_barrier();
      process();
      if (over) {
        // some passing pairs found no slot: the tile again, kp rows at a
        // time, lowest rows first, with the thresholds of the round before.
        // A window holds at most kp rows, so every passing pair has a slot.
        for (uint32_t lo = 0; lo < (uint32_t)kU8cR; lo += kp) {
#pragma unroll
          for (int nt = 0; nt < 2; nt++) nh[nt] = -H[ql0 + nt * 32];
#pragma unroll
          for (int mt = 0; mt < 4; mt++) {
            const uint32_t tl = wr * 128 + mt * 32;  // the row tile's rows: wave-uniform test
            if (tl < lo + kp && tl + 32 > lo) {
#pragma unroll
              for (int e = 0; e < 16; e++) {
                const uint32_t row = lrow + mt * 32 + (e & 3) + 8 * (e >> 2);
                if (row >= lo && row < lo + kp) {
                  const int32_t cxe = cxs[row];
                  const float rxe = rxs[row];
#pragma unroll
                  for (int nt = 0; nt < 2; nt++) {
                    const int32_t s = acc[mt][nt][e] + cxe + cq[nt];
                    if (__builtin_fmaf(nh[nt], rxe, (float)s) >= 0.0f) {
                      const uint32_t q = ql0 + nt * 32;
                      const uint32_t n = atomicAdd(&pc[q], 1u);
                      if (n < kp) {  // always
                        pend[q * kp + n] = tbase + row;
                        psum[q * kp + n] = s;
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

// pending slots per query: the most of 64, 32, 16 that fit beside the queries; 0: none does
uint32_t scan_u8cos_pend(int dp) {
  for (uint32_t p = 64; p >= 16; p >>= 1)
    if (scan_u8cos_lds_bytes(dp, p) <= 160 * 1024) return p;
  return 0;
}

size_t scan_u8cos_lds_bytes(int dp, uint32_t pend) {
  const size_t ks = (size_t)((dp + kU8cChunk - 1) / kU8cChunk) * 4;
  return 4 * ks * 1024 + (size_t)kU8cQ * pend * 8 + kU8cQ * 8 + kU8cQ * 4 * 4 + kU8cR * 4 * 2 + 16;
}

hipError_t launch_scan_u8cos_rows(const uint8_t* rows, uint64_t row_bytes, uint64_t nrows, const uint8_t* valid, int dp,
                                  int32_t* cx, uint32_t* nb, float* rx, uint64_t npad, hipStream_t s) {
  if (npad == 0) return hipSuccess;
  const uint64_t blocks = std::min<uint64_t>((npad + 255) / 256, 65536);
  hipLaunchKernelGGL(ngt_scan_u8cos_rows_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, rows, row_bytes, nrows, valid,
                     dp, cx, nb, rx, npad);
  return hipGetLastError();
}

template <int M>
static void launch_scan_u8cos_t(const U8CosScanArgs& a, size_t lds, hipStream_t s) {
  static bool attr = [] {
    (void)hipFuncSetAttribute((const void*)ngt_scan_u8cos_kernel<M>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    return true;
  }();
  (void)attr;
  hipLaunchKernelGGL((ngt_scan_u8cos_kernel<M>), dim3(a.nparts * a.mblocks), dim3(256), lds, s, a);
}

hipError_t launch_scan_u8cos(const U8CosScanArgs& a, int metric, hipStream_t s) {
  if (a.k < 1 || a.k > 128 || a.dp > kU8cMaxDp || a.dp % 16) return hipErrorNotSupported;
  if (a.pend != 16 && a.pend != 32 && a.pend != 64) return hipErrorNotSupported;
  const size_t lds = scan_u8cos_lds_bytes(a.dp, a.pend);
  if (lds > 160 * 1024) return hipErrorNotSupported;
  if (metric == kCosine) launch_scan_u8cos_t<kCosine>(a, lds, s);
  else if (metric == kAngle) launch_scan_u8cos_t<kAngle>(a, lds, s);
  else return hipErrorNotSupported;
  return hipGetLastError();
}

}  // namespace ngt_amd
