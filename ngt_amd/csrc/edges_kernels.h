// edges_kernels.h -- launchers of the ANNG re-cut kernels (edges_kernels.hip)
// used by edges_api.cpp: GraphReconstructor::reconstructANNGFromANNG
// (lib/NGT/GraphReconstructor.h:721-801) on a CSR graph in HBM (onng_kernels.h:
// node v's list ids/dists[off[v] .. off[v+1]), slot 0 the dummy).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "onng_kernels.h"

namespace ngt_amd {
namespace edges {

// The selection pass.  Of node v's list, walked in order, the entries (m, d)
// with m < v are selected until K are; a distance below its predecessor's (the
// first entry's predecessor is 0) ends the list's walk.  A selected entry goes
// to v's list as (m, d) and to m's list as (v, d).  count adds the lengths to
// cnt (zeroed by the caller); fill writes packed (distance, id) keys at
// lists_off[u] + a cursor (cur zeroed by the caller).  Every id of G must lie
// in [1, n) (onng::check_lists).
void count_recut(uint32_t n, onng::Csr G, uint32_t K, uint32_t* cnt, hipStream_t s);
void fill_recut(uint32_t n, onng::Csr G, uint32_t K, const uint64_t* lists_off, uint32_t* cur, uint64_t* keys,
                hipStream_t s);

}  // namespace edges
}  // namespace ngt_amd
