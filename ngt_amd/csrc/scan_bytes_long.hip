// scan_bytes_long.hip -- the exact batch scan of
// ObjectSpaceRepository::linearSearch (lib/NGT/ObjectSpaceRepository.h:466-502)
// for uint8 rows of 272 .. 1024 padded bytes under L1 and Hamming, lists of
// 1 .. 16 results, on the VALU's packed byte-SAD and popcount.
//
// scan_bytes.hip's arithmetic: S = sum |q_i - x_i| or popcount(q ^ x) is an
// integer, S <= 255 * 1024 = 261,120 < 2^24, the comparator's distance is
// exactly (float)S and the key (S << 32 | id) ranks by (float distance, id).
// What differs is the row side: a row of up to 1024 bytes does not fit a
// lane's registers twice over, so the row is walked in pieces and the sums of
// the lane's row against every query of the wave are kept instead.
//
// Work: a wave is a workgroup.  It owns QB = 64 queries x one contiguous
// part of the rows and walks the part in 64-row tiles, lane = row.
//  * Row pieces: 64 bytes of the lane's row (4 x global_load_dwordx4, 16
//    VGPRs); the next piece -- of this tile, or the first of the next tile --
//    loads into a second set before the current one is used.  A 16-byte chunk
//    at or beyond Dp is never read: it is zero in the registers.
//  * Accumulators: acc[q], one VGPR per query of the wave, live across the
//    pieces of a tile.  The query loop is unrolled inside the piece loop, so
//    every acc[q] has a fixed register.
//  * Queries: the prep kernel writes a zero-padded copy in the order the loop
//    reads it, [query block][piece][query][16 words].  The words of (piece,
//    query) are wave-uniform and come through the scalar cache
//    (s_load_dwordx16 at base + 64 q) as the scalar operand of v_sad_u8 /
//    v_xor_b32.  A wave's query block (Dp x 64 bytes) is larger than the
//    scalar cache, so the words of two queries are asked for a batch ahead,
//    while the batch before them is summed.
//  * End of a tile: the sums go through LDS 32 queries at a time (lane-private
//    words, 8 KiB), which frees the fixed registers for a rolled loop over the
//    queries: S, the key, the query's k-th key from a VGPR pair (v_readlane),
//    the survivor mask.  Survivors, lists and output are scan_bytes.hip's
//    (scan_bytes_common.h), the first-tile selection with a top bit that
//    covers 261,120.
//  * Removed rows, the dummy row 0 and the padding of the last tile are masked
//    out of every survivor mask; a part with fewer than k live rows leaves ~0
//    in its list; the parts are merged by ngt_linear_merge_kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "ngt_device.h"
#include "ngt_kernels.h"
#include "scan_bytes_common.h"

namespace ngt_amd {

constexpr uint32_t kBlG = 32;  // queries whose sums go through LDS together
constexpr int kBlB = 2;        // queries whose words are loaded together, one such batch ahead

// The zero-padded query copy: [mblocks][pieces][qb][16] words.
__global__ void __launch_bounds__(256) ngt_scan_bytes_long_prep_kernel(const uint8_t* __restrict__ queries,
                                                                       uint64_t query_bytes, uint32_t nq, int dp,
                                                                       uint32_t qb, uint32_t pieces,
                                                                       uint32_t* __restrict__ out, uint64_t total) {
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
    const uint32_t w16 = (uint32_t)(i & 15);
    const uint64_t r = i >> 4;
    const uint32_t ql = (uint32_t)(r % qb);
    const uint64_t r2 = r / qb;
    const uint32_t pc = (uint32_t)(r2 % pieces);
    const uint64_t q = (r2 / pieces) * qb + ql;
    const uint32_t w = pc * 16 + w16;
    uint32_t v = 0;
    if (q < nq && w * 4 < (uint32_t)dp) v = reinterpret_cast<const uint32_t*>(queries + q * query_bytes)[w];
    out[i] = v;
  }
}

template <int M, int QB>
__global__ void __launch_bounds__(64) ngt_scan_bytes_long_kernel(BytesScanArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const uint32_t lane = threadIdx.x, k = a.k;
  uint64_t* lists = reinterpret_cast<uint64_t*>(smem);               // [QB][k], (S << 32 | id) ascending, ~0 = empty
  uint32_t* stage = reinterpret_cast<uint32_t*>(lists + QB * k);     // [kBlG][64] sums, lane-private
  const uint32_t mb = blockIdx.x / a.nparts, part = blockIdx.x % a.nparts;
  const uint32_t q0 = mb * QB;
  const uint32_t nqb = a.nq - q0 < (uint32_t)QB ? a.nq - q0 : (uint32_t)QB;
  const uint32_t t0 = part * a.tiles_per_part;
  const uint32_t t1 = t0 + a.tiles_per_part < a.ntiles ? t0 + a.tiles_per_part : a.ntiles;
  const uint32_t nchunks = (uint32_t)a.dp >> 4, pieces = (nchunks + 3) >> 2;
  for (uint32_t i = lane; i < nqb * k; i += 64) lists[i] = ~0ull;
  __syncthreads();
  // the k-th key of query h * 64 + lane: the radius' key until the list is full
  uint64_t thr[QB / 64];
#pragma unroll
  for (int h = 0; h < QB / 64; h++) thr[h] = a.key_init;
  bs_const_words qblock = (bs_const_words)(uintptr_t)(a.qpad + (uint64_t)mb * pieces * (QB * 16));

  // the lane's row of tile t and its byte of the valid column; rows past the
  // table reload the last one
  auto row_of = [&](uint32_t t, uint32_t& vb) -> const uint8_t* {
    const uint64_t id = (uint64_t)t * 64 + lane;
    const uint64_t rid = id < a.nrows ? id : a.nrows - 1;
    vb = 1;
    if (a.valid != nullptr) vb = a.valid[rid];
    return a.rows + rid * a.row_bytes;
  };
  // piece pc of the row at p; chunks at or beyond Dp are not read
  auto load_piece = [&](const uint8_t* p, uint32_t pc, bs_u32x4 (&dst)[4]) {
#pragma unroll
    for (int c = 0; c < 4; c++) {
      bs_u32x4 v = {0, 0, 0, 0};
      if (pc * 4 + c < nchunks) v = *reinterpret_cast<const bs_u32x4*>(p + 64 * pc + 16 * c);
      dst[c] = v;
    }
  };

  uint32_t acc[QB];
#pragma unroll
  for (int q = 0; q < QB; q++) acc[q] = 0;

  // the loads of the next piece are in flight while this one is compared
  bs_u32x4 cur[4], nxt[4];
  uint32_t vb_nxt = 0;
  const uint8_t* row = nullptr;
  if (t0 < t1) {
    row = row_of(t0, vb_nxt);
    load_piece(row, 0, nxt);
  }
  // the query words of two batches, wave-uniform: the one being summed and
  // the one in flight
  static_assert(kBlB == 2 && QB / kBlB % 2 == 0, "the wait below names two queries; a piece ends in w1");
  uint32_t w0[kBlB * 16], w1[kBlB * 16];
#pragma unroll
  for (int i = 0; i < kBlB * 16; i++) w0[i] = qblock[i];
  for (uint32_t t = t0; t < t1; t++) {
    // the lane's id, ~0 for removed rows, the dummy row 0 and padding
    const uint64_t id = (uint64_t)t * 64 + lane;
    const uint32_t id_cur = vb_nxt != 0 && id >= 1 && id < a.nrows ? (uint32_t)id : ~0u;
    const uint64_t livem = __ballot(id_cur != ~0u);
    for (uint32_t pc = 0; pc < pieces; pc++) {
#pragma unroll
      for (int c = 0; c < 4; c++) cur[c] = nxt[c];
      if (pc + 1 < pieces) {
        load_piece(row, pc + 1, nxt);
      } else if (t + 1 < t1) {
        row = row_of(t + 1, vb_nxt);
        load_piece(row, 0, nxt);
      }
      // the words of the next kBlB queries -- of the next piece after the
      // last ones -- are asked for before this batch is summed
      bs_const_words qw = qblock + pc * (QB * 16);
      bs_const_words qw_next = qblock + (pc + 1 < pieces ? pc + 1 : 0) * (QB * 16);
#pragma unroll
      for (int b = 0; b < QB / kBlB; b++) {
        uint32_t (&w)[kBlB * 16] = b & 1 ? w1 : w0;
        uint32_t (&wn)[kBlB * 16] = b & 1 ? w0 : w1;
        // scalar loads return in any order, so a wait is for all of them: this
        // batch's words are waited for here, before the next loads are issued
        asm volatile("" ::"s"(w[0]), "s"(w[16]));
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < kBlB * 16; i++) wn[i] = b + 1 < QB / kBlB ? qw[(b + 1) * kBlB * 16 + i] : qw_next[i];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < kBlB; i++) {
          uint32_t S = acc[b * kBlB + i];
#pragma unroll
          for (int j = 0; j < 16; j++) {
            if constexpr (M == kL1) S = __builtin_amdgcn_sad_u8(cur[j >> 2][j & 3], w[i * 16 + j], S);
            else S += __popc(cur[j >> 2][j & 3] ^ w[i * 16 + j]);
          }
          acc[b * kBlB + i] = S;
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    // the tile's sums against the k-th keys, kBlG queries at a time
#pragma unroll
    for (int g = 0; g < QB / (int)kBlG; g++) {
#pragma unroll
      for (int i = 0; i < (int)kBlG; i++) {
        stage[i * 64 + lane] = acc[g * kBlG + i];
        acc[g * kBlG + i] = 0;
      }
      const uint32_t ng = nqb > kBlG * g ? (nqb - kBlG * g < kBlG ? nqb - kBlG * g : kBlG) : 0u;
      uint64_t& thrv = thr[g * kBlG / 64];
      for (uint32_t i = 0; i < ng; i++) {
        const uint32_t q = kBlG * g + i;
        const uint32_t S = stage[i * 64 + lane];
        const uint64_t key = ((uint64_t)S << 32) | id_cur;
        const uint64_t tq = bs_readlane(thrv, q & 63);
        const uint64_t m = __ballot(key < tq) & livem;
        if (m) bs_insert<1024 * 255>(lists, k, lane, q, m, S, key, tq, thrv);
      }
    }
  }
  __syncthreads();
  bs_store_lists(lists, nqb, k, lane, q0, a.nparts, part, a.partial);
}

uint32_t scan_bytes_long_pieces(int dp) { return ((uint32_t)dp + 63) / 64; }

size_t scan_bytes_long_lds_bytes(uint32_t k) { return (size_t)kBytesLongQ * k * 8 + kBlG * 64 * 4; }

hipError_t launch_scan_bytes_long_prep(const uint8_t* queries, uint64_t query_bytes, uint32_t nq, int dp,
                                       uint32_t* qpad, uint32_t mblocks, hipStream_t s) {
  const uint32_t pieces = scan_bytes_long_pieces(dp);
  const uint32_t qb = kBytesLongQ;
  const uint64_t total = (uint64_t)mblocks * pieces * qb * 16;
  const uint64_t blocks = std::min<uint64_t>((total + 255) / 256, 65536);
  hipLaunchKernelGGL(ngt_scan_bytes_long_prep_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, queries, query_bytes, nq,
                     dp, qb, pieces, qpad, total);
  return hipGetLastError();
}

template <int M>
static hipError_t launch_scan_bytes_long_metric(const BytesScanArgs& a, hipStream_t s) {
  const dim3 grid(a.nparts * a.mblocks), block(64);
  const size_t lds = scan_bytes_long_lds_bytes(a.k);
  hipLaunchKernelGGL((ngt_scan_bytes_long_kernel<M, (int)kBytesLongQ>), grid, block, lds, s, a);
  return hipGetLastError();
}

hipError_t launch_scan_bytes_long(const BytesScanArgs& a, int metric, hipStream_t s) {
  const uint32_t qb = kBytesLongQ;
  if (a.k == 0 || a.k > 16 || a.nparts == 0 || a.mblocks == 0 || a.dp <= 256 || a.dp > 1024 || a.dp % 16 ||
      a.mblocks != (a.nq + qb - 1) / qb || a.nrows < 2 ||
      (uint64_t)a.nparts * a.tiles_per_part < a.ntiles || (uint64_t)a.ntiles * 64 < a.nrows ||
      a.row_bytes < (uint64_t)a.dp || a.row_bytes % 16 || (uintptr_t)a.rows % 16)
    return hipErrorNotSupported;
  if (metric == kL1) return launch_scan_bytes_long_metric<kL1>(a, s);
  if (metric == kHamming) return launch_scan_bytes_long_metric<kHamming>(a, s);
  return hipErrorNotSupported;
}

}  // namespace ngt_amd
