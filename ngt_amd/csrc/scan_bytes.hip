// scan_bytes.hip -- the exact batch scan of ObjectSpaceRepository::linearSearch
// (lib/NGT/ObjectSpaceRepository.h:466-502) for uint8 rows under L1 and
// Hamming, on the VALU's packed byte-SAD and popcount.
//
// S = sum |q_i - x_i| (L1) or popcount(q ^ x) (Hamming) over the padded row is
// an integer, S <= 255 Dp = 65,280 at Dp = 256, and the comparator's distance
// is exactly (float)S (dist_u8<kL1>, dist_u8<kHamming>: every partial sum is
// an integer below 2^24).  S -> (float)S is strictly monotone, so ranking by
// the key (S << 32 | id) is ranking by (float distance, id): no error bound,
// no recompute, and a tie at the k-th place is decided inside the filter.
//
// Work: a wave is a workgroup.  It owns up to 128 queries x one contiguous part
// of the rows and walks the part in 64-row tiles, lane = row.
//  * Rows: a lane keeps its whole row in VGPRs (NC x global_load_dwordx4, NC
//    the row's 16-byte chunks rounded up to 1, 2, 4, 8 or 16), the next tile's
//    row in a second set, loaded before the current tile is compared.  Chunks
//    past Dp are zero.
//  * Queries: a zero-padded copy [query][NC x 16 bytes] written by the prep
//    kernel before the launch and read-only in it, so the wave-uniform query
//    words come through the scalar cache straight into the scalar operand of
//    v_sad_u8 / v_xor_b32: no LDS traffic, no VGPRs, nothing to reorder.
//  * One pair ends in one accumulator; (S, id) against the query's k-th key
//    gives the survivor mask, zero for almost every (tile, query).  The k-th
//    keys live in VGPRs, query q in lane q & 63 (v_readlane).
//  * Survivors: the query's sorted k-list comes from LDS into lanes 0 .. k-1,
//    takes each survivor by ballot rank and a one-lane shift, and goes back.
//    A (tile, query) with more than k survivors (the first tile of a part)
//    first finds the k-th smallest S of the tile bit by bit with ballots and
//    keeps only the survivors up to it.
//  * Removed rows, the dummy row 0 and the padding of the last tile are masked
//    out of every survivor mask.  A part with fewer than k live rows leaves
//    ~0 in its list; the parts are merged by ngt_linear_merge_kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "ngt_device.h"
#include "ngt_kernels.h"
#include "scan_bytes_common.h"

namespace ngt_amd {

constexpr uint32_t kBsQ = 128;  // queries per wave

// The zero-padded query copy: [mblocks * 128][qwords] words.
__global__ void __launch_bounds__(256) ngt_scan_bytes_prep_kernel(const uint8_t* __restrict__ queries,
                                                                  uint64_t query_bytes, uint32_t nq, int dp,
                                                                  uint32_t qwords, uint32_t* __restrict__ out,
                                                                  uint64_t total) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
    const uint64_t q = i / qwords;
    const uint32_t w = (uint32_t)(i - q * qwords);
    uint32_t v = 0;
    if (q < nq && w * 4 < (uint32_t)dp) v = reinterpret_cast<const uint32_t*>(queries + q * query_bytes)[w];
    out[i] = v;
  }
}

template <int M, int NC>
__global__ void __launch_bounds__(64) ngt_scan_bytes_kernel(BytesScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint64_t* lists = reinterpret_cast<uint64_t*>(smem);  // [128][k], (S << 32 | id) ascending, ~0 = empty
  const uint32_t lane = threadIdx.x, k = a.k;
  const uint32_t mb = blockIdx.x / a.nparts, part = blockIdx.x % a.nparts;
  const uint32_t q0 = mb * kBsQ;
  const uint32_t nqb = a.nq - q0 < kBsQ ? a.nq - q0 : kBsQ;
  const uint32_t t0 = part * a.tiles_per_part;
  const uint32_t t1 = t0 + a.tiles_per_part < a.ntiles ? t0 + a.tiles_per_part : a.ntiles;
  for (uint32_t i = lane; i < nqb * k; i += 64) lists[i] = ~0ull;
  __syncthreads();
  // the k-th key of query h * 64 + lane: the radius' key until the list is full
  uint64_t thr[2] = {a.key_init, a.key_init};
  bs_const_words qwords = (bs_const_words)(uintptr_t)(a.qpad + (uint64_t)q0 * (NC * 4));

  // a lane's row of tile t and its byte of the valid column; rows past the
  // table reload the last one
  auto load_tile = [&](uint32_t t, bs_u32x4 (&dst)[NC], uint32_t& vb) {
    const uint64_t id = (uint64_t)t * 64 + lane;
    const uint64_t rid = id < a.nrows ? id : a.nrows - 1;
    const uint8_t* p = a.rows + rid * a.row_bytes;
#pragma unroll
    for (int c = 0; c < NC; c++) {
      bs_u32x4 v = {0, 0, 0, 0};
      if (c * 16 < a.dp) v = *reinterpret_cast<const bs_u32x4*>(p + 16 * c);
      dst[c] = v;
    }
    vb = 1;
    if (a.valid != nullptr) vb = a.valid[rid];
  };

  // the loads of tile t + 1 are in flight while tile t is compared
  bs_u32x4 cur[NC], nxt[NC];
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
    if (livem) {
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const uint32_t nh = nqb > 64u * h ? (nqb - 64u * h < 64u ? nqb - 64u * h : 64u) : 0u;
        for (uint32_t ql = 0; ql < nh; ql++) {
          const uint32_t q = 64u * h + ql;
          bs_const_words qw = qwords + q * (NC * 4);
          uint32_t S = 0;
#pragma unroll
          for (int c = 0; c < NC; c++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
              if constexpr (M == kL1) S = __builtin_amdgcn_sad_u8(cur[c][j], qw[c * 4 + j], S);
              else S += __popc(cur[c][j] ^ qw[c * 4 + j]);
            }
          const uint64_t key = ((uint64_t)S << 32) | id_cur;
          const uint64_t tq = bs_readlane(thr[h], ql);
          const uint64_t m = __ballot(key < tq) & livem;
          if (m) bs_insert<NC * 16 * 255>(lists, k, lane, q, m, S, key, tq, thr[h]);
        }
      }
    }
  }
  __syncthreads();
  bs_store_lists(lists, nqb, k, lane, q0, a.nparts, part, a.partial);
}

int scan_bytes_chunks(int dp) {
  int nc = 1;
  while (nc * 16 < dp) nc *= 2;
  return nc;
}

hipError_t launch_scan_bytes_prep(const uint8_t* queries, uint64_t query_bytes, uint32_t nq, int dp, uint32_t* qpad,
                                  uint32_t mblocks, hipStream_t s) {
  const uint32_t qwords = (uint32_t)scan_bytes_chunks(dp) * 4;
  const uint64_t total = (uint64_t)mblocks * kBsQ * qwords;
  const uint64_t blocks = std::min<uint64_t>((total + 255) / 256, 65536);
  hipLaunchKernelGGL(ngt_scan_bytes_prep_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, queries, query_bytes, nq, dp,
                     qwords, qpad, total);
  return hipGetLastError();
}

template <int M>
static hipError_t launch_scan_bytes_metric(const BytesScanArgs& a, hipStream_t s) {
  const dim3 grid(a.nparts * a.mblocks), block(64);
  const size_t lds = (size_t)kBsQ * a.k * 8;
  switch (scan_bytes_chunks(a.dp)) {
    case 1: hipLaunchKernelGGL((ngt_scan_bytes_kernel<M, 1>), grid, block, lds, s, a); break;
    case 2: hipLaunchKernelGGL((ngt_scan_bytes_kernel<M, 2>), grid, block, lds, s, a); break;
    case 4: hipLaunchKernelGGL((ngt_scan_bytes_kernel<M, 4>), grid, block, lds, s, a); break;
    case 8: hipLaunchKernelGGL((ngt_scan_bytes_kernel<M, 8>), grid, block, lds, s, a); break;
    case 16: hipLaunchKernelGGL((ngt_scan_bytes_kernel<M, 16>), grid, block, lds, s, a); break;
    default: return hipErrorNotSupported;
  }
  return hipGetLastError();
}

hipError_t launch_scan_bytes(const BytesScanArgs& a, int metric, hipStream_t s) {
  if (a.k == 0 || a.k > 16 || a.nparts == 0 || a.mblocks == 0) return hipErrorNotSupported;
  if (metric == kL1) return launch_scan_bytes_metric<kL1>(a, s);
  if (metric == kHamming) return launch_scan_bytes_metric<kHamming>(a, s);
  return hipErrorNotSupported;
}

}  // namespace ngt_amd
