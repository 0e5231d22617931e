// remove_kernels.hip -- gfx950 kernels of object removal: the relink chain of
// NeighborhoodGraph::removeEdgesReliably (lib/NGT/Graph.cpp:739-845).
//
// The removed node's neighbours are joined to one another so the graph stays
// connected: for i = 0 .. d-2 the neighbour at position i of the current order
// is linked with the nearest of the later positions (the first strict minimum
// of comparator(object[i], object[j]), j > i), which then moves to position
// i + 1.  The chain is sequential by definition -- each step's order depends on
// the previous swap -- so one workgroup runs it; the distances of one step are
// independent and spread over the workgroup's quads.
//
//  * ngt_relink_fast_kernel   : up to kFastCap rows gathered into LDS, the whole
//    chain in one launch, one quad per (i, j) comparator.
//  * ngt_relink_matrix_kernel : hubs.  The full d x d matrix comparator(row a,
//    row b) by the whole grid, argument order as the chain uses it (symmetry of
//    the float result is not assumed);
//    ngt_relink_chain_kernel  : the chain over that matrix, one workgroup.
// Both keep the current order in LDS and pick the minimum as a packed
// (distance, current position) key, so equal distances resolve to the lowest
// position exactly as the reference's `d < mind` scan does.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "ngt_device.h"
#include "ngt_kernels.h"
#include "remove_kernels.h"
#include "search_common.h"
#include "stored_dispatch.h"

namespace ngt_amd {
namespace removal {

namespace {

constexpr int kChainThreads = 256;
constexpr int kChainWaves = kChainThreads / 64;
constexpr int kMatrixChainThreads = 1024;
constexpr int kMatrixChainWaves = kMatrixChainThreads / 64;

// The workgroup's minimum of the per-thread keys `best` (~0 = none) decides
// link i: thread 0 records it and moves the chosen position next to i.
template <int WAVES>
__device__ __forceinline__ void commit_link(const RelinkArgs& a, uint32_t i, uint64_t best, uint64_t* wmin,
                                            uint32_t* order) {
  best = wave_min_u64(best);
  if (lane_id() == 0) wmin[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t m = wmin[0];
    for (int w = 1; w < WAVES; w++) m = min_u64(m, wmin[w]);
    uint32_t minj = (uint32_t)m;
    if (minj <= i || minj >= a.d) minj = i + 1;  // no candidate can win only on a malformed key
    a.link_a[i] = a.ids[order[i]];
    a.link_b[i] = a.ids[order[minj]];
    a.link_dist[i] = float_of_ord((uint32_t)(m >> 32));
    const uint32_t t = order[i + 1];
    order[i + 1] = order[minj];
    order[minj] = t;
  }
  __syncthreads();
}

template <int M, typename T>
__global__ void __launch_bounds__(kChainThreads) ngt_relink_fast_kernel(RelinkArgs a) {
  extern __shared__ uint4 smem[];
  uint8_t* lrows = reinterpret_cast<uint8_t*>(smem);
  uint64_t* wmin = reinterpret_cast<uint64_t*>(lrows + (uint64_t)a.d * a.row_bytes);
  uint32_t* order = reinterpret_cast<uint32_t*>(wmin + kChainWaves);
  const uint32_t per = (uint32_t)(a.row_bytes >> 4);
  for (uint32_t t = threadIdx.x; t < a.d * per; t += kChainThreads) {
    const uint32_t r = t / per, c = t - r * per;
    smem[t] = reinterpret_cast<const uint4*>(a.rows + (uint64_t)a.ids[r] * a.row_bytes)[c];
  }
  for (uint32_t t = threadIdx.x; t < a.d; t += kChainThreads) order[t] = t;
  __syncthreads();
  const int g = threadIdx.x & 3;
  const uint32_t quad = threadIdx.x >> 2;
  for (uint32_t i = 0; i + 1 < a.d; i++) {
    const T* q = reinterpret_cast<const T*>(lrows + (uint64_t)order[i] * a.row_bytes);
    uint64_t best = ~0ull;
    for (uint32_t j = i + 1 + quad; j < a.d; j += kChainThreads / 4) {
      const T* x = reinterpret_cast<const T*>(lrows + (uint64_t)order[j] * a.row_bytes);
      const float dist = quad_distance<M, T>(q, x, a.dp, g);
      const uint64_t key = ((uint64_t)ord_of(dist) << 32) | j;
      if (g == 0) best = min_u64(best, key);
    }
    commit_link<kChainWaves>(a, i, best, wmin, order);
  }
}

template <int M, typename T>
__global__ void __launch_bounds__(256) ngt_relink_matrix_kernel(RelinkArgs a) {
  const int g = threadIdx.x & 3;
  const uint64_t quad = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 2;
  const uint64_t nquads = ((uint64_t)gridDim.x * blockDim.x) >> 2;
  const uint64_t np = (uint64_t)a.d * a.d;
  for (uint64_t p = quad; p < np; p += nquads) {
    const uint32_t r = (uint32_t)(p / a.d), c = (uint32_t)(p - (uint64_t)r * a.d);
    float dist = 0.f;
    if (r != c)
      dist = quad_distance<M, T>(row_ptr<T>(a.rows, a.row_bytes, a.ids[r]), row_ptr<T>(a.rows, a.row_bytes, a.ids[c]),
                                 a.dp, g);
    if (g == 0) a.matrix[p] = dist;
  }
}

__global__ void __launch_bounds__(kMatrixChainThreads) ngt_relink_chain_kernel(RelinkArgs a) {
  extern __shared__ uint4 smem[];
  uint64_t* wmin = reinterpret_cast<uint64_t*>(smem);
  uint32_t* order = reinterpret_cast<uint32_t*>(wmin + kMatrixChainWaves);
  for (uint32_t t = threadIdx.x; t < a.d; t += kMatrixChainThreads) order[t] = t;
  __syncthreads();
  for (uint32_t i = 0; i + 1 < a.d; i++) {
    const float* mrow = a.matrix + (uint64_t)order[i] * a.d;
    uint64_t best = ~0ull;
    for (uint32_t j = i + 1 + threadIdx.x; j < a.d; j += kMatrixChainThreads)
      best = min_u64(best, ((uint64_t)ord_of(mrow[order[j]]) << 32) | j);
    commit_link<kMatrixChainWaves>(a, i, best, wmin, order);
  }
}

}  // namespace

size_t fast_lds_bytes(uint32_t d, uint64_t row_bytes, uint32_t cap) {
  if (d > cap || d > kFastCap || (row_bytes & 15)) return 0;
  const size_t need = (size_t)d * row_bytes + kChainWaves * sizeof(uint64_t) + (size_t)d * sizeof(uint32_t);
  return need <= kFastLdsBytes ? need : 0;
}

hipError_t launch_relink_fast(const RelinkArgs& a, int metric, int otype, hipStream_t s) {
  if (a.d < 2) return hipSuccess;
  const size_t lds = fast_lds_bytes(a.d, a.row_bytes, kFastCap);
  if (lds == 0) return hipErrorInvalidValue;
#define L_RF(MM, TT) \
  hipLaunchKernelGGL((ngt_relink_fast_kernel<MM, TT>), dim3(1), dim3(kChainThreads), lds, s, a)
  NGT_STORED_DISPATCH(metric, otype, L_RF);
#undef L_RF
  return hipGetLastError();
}

hipError_t launch_relink_matrix(const RelinkArgs& a, int metric, int otype, hipStream_t s) {
  if (a.d < 2) return hipSuccess;
  if (a.d > kMaxList || !a.matrix) return hipErrorInvalidValue;
  uint64_t blocks = ((uint64_t)a.d * a.d * 4 + 255) / 256;
  if (blocks > 16384) blocks = 16384;
#define L_RM(MM, TT) \
  hipLaunchKernelGGL((ngt_relink_matrix_kernel<MM, TT>), dim3((uint32_t)blocks), dim3(256), 0, s, a)
  NGT_STORED_DISPATCH(metric, otype, L_RM);
#undef L_RM
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const size_t lds = kMatrixChainWaves * sizeof(uint64_t) + (size_t)a.d * sizeof(uint32_t);
  hipLaunchKernelGGL(ngt_relink_chain_kernel, dim3(1), dim3(kMatrixChainThreads), lds, s, a);
  return hipGetLastError();
}

}  // namespace removal
}  // namespace ngt_amd
