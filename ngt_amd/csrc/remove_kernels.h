// remove_kernels.h -- launchers of the relink chain of object removal
// (remove_kernels.hip) used by build.cpp: NeighborhoodGraph::removeEdgesReliably's
// loop over the removed node's neighbours (lib/NGT/Graph.cpp:739-845).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ngt_amd {
namespace removal {

// Longest neighbour list whose rows the one-workgroup chain keeps in LDS (when
// they also fit kFastLdsBytes); longer lists (hubs) go through the d x d
// distance matrix in HBM.
constexpr uint32_t kFastCap = 96;
constexpr size_t kFastLdsBytes = 60 * 1024;
// the matrix path's limit: d * d floats in HBM, the current order in LDS
constexpr uint32_t kMaxList = 12288;

struct RelinkArgs {
  const uint8_t* rows;     // [nrows][row_bytes]
  uint64_t row_bytes;
  int dp;
  const uint32_t* ids;     // [d] neighbour ids in list order, each in [1, nrows)
  uint32_t d;
  float* matrix;           // matrix path: [d][d], comparator(row a, row b) at a * d + b
  uint32_t* link_a;        // [d - 1] id at position i of the current order
  uint32_t* link_b;        // [d - 1] id of the first strict minimum among later positions
  float* link_dist;        // [d - 1]
};

// LDS bytes of the one-launch chain for d rows, 0 when it does not take them
size_t fast_lds_bytes(uint32_t d, uint64_t row_bytes, uint32_t cap);
hipError_t launch_relink_fast(const RelinkArgs& a, int metric, int otype, hipStream_t s);
hipError_t launch_relink_matrix(const RelinkArgs& a, int metric, int otype, hipStream_t s);

}  // namespace removal
}  // namespace ngt_amd
