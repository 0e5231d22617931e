// refine_kernels.h -- launchers of the refine-anng merge kernels
// (refine_kernels.hip) used by refine.cpp.  Graphs are CSR in HBM with
// distances (onng::Csr: node v's list ids/d[off[v] .. off[v+1]), slot 0 the
// dummy); the scan, the per-list sort and the adjacent-id dedupe are
// onng_kernels.h's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "onng_kernels.h"

namespace ngt_amd {
namespace refine {

using onng::Csr;

// Longest list the one-wave LDS sort takes (onng::sort_lists); longer lists are
// sorted by a block in global memory.  Every other kernel here works in global
// memory on lists of any length.
constexpr uint32_t kFastCap = onng::kFastCap;

// Error words (min node id, 0xffffffff = none): a result id outside [1, n), a
// result count above the stride.
enum { kErrResultId = 0, kErrResultCount = 1, kErrWords = 2 };

// One block of search results: query q is node first + q, its results
// ids/d[q * stride .. + cnt[q]) in result order.
struct Results {
  uint32_t first, count, stride;
  const uint32_t* ids;
  const float* d;
  const uint32_t* cnt;
};

// The lists after the outgoing step: a batch node's is keys[boff[i + 1] ..
// + bcnt[i + 1]) with i = v - first (packed (distance, id) keys), every other
// node's is G's.
struct Lists {
  Csr G;
  uint32_t first, count;
  const uint64_t* boff;
  const uint32_t* bcnt;
  const uint64_t* bkeys;
};

// *out = max(*out, in[0 .. n)).
void max_u32(const uint32_t* in, uint64_t n, uint32_t* out, hipStream_t s);

// cnt[q] = 0 for the queries whose row is not a stored object.
void mask_counts(const uint8_t* valid, uint32_t first, uint32_t count, uint32_t* cnt, hipStream_t s);

// Outgoing step, before the sort: blen[i + 1] = |G[first + i]| + the results of
// query i other than the node itself (blen[0] = 0); fill writes the keys of the
// list, then of those results, at boff[i + 1].
void batch_len(uint32_t n, Csr G, Results R, uint32_t* blen, uint32_t* err, hipStream_t s);
void batch_fill(uint32_t n, Csr G, Results R, const uint64_t* boff, uint64_t* keys, hipStream_t s);

// Incoming step.  For every result (t, d) of query node s with t != s, K =
// (d, s) and X = the first element of t's list (L) that is not below K:
//   X is K                          -> nothing (the edge exists);
//   X has another id, or no X       -> K joins t's candidates, to be inserted;
//   X has id s at a larger distance -> K joins them with X in cx ("open": it
//                                      is inserted iff an earlier insertion
//                                      lies between K and X).
// count adds to ccnt[t] (and to ropen[t] for the open ones); fill writes
// ckeys/cx[coff[t] + cursor] (cx = 0 unless open).
void incoming(uint32_t n, Lists L, Results R, bool fill, uint32_t* ccnt, uint32_t* ropen, const uint64_t* coff,
              uint64_t* ckeys, uint64_t* cx, hipStream_t s);
// Decides the open candidates of every target: K is inserted iff a candidate
// of a lower source id that is not open lies strictly between K and X (such a
// candidate is always inserted; refine_kernels.hip has the argument).  A
// candidate that is not inserted gets the key ~0 (it sorts last); ins[t] = the
// number inserted.
void resolve(uint32_t n, const uint64_t* coff, const uint32_t* ropen, uint64_t* ckeys, const uint64_t* cx,
             uint32_t* ins, hipStream_t s);

// nlen[v] = |L[v]| + ins[v] (ins may be null); emit merges L[v] with the first
// ins[v] keys of csorted[coff[v] ..) into ids/d at noff[v].
void new_len(uint32_t n, Lists L, const uint32_t* ins, uint32_t* nlen, hipStream_t s);
void emit(uint32_t n, Lists L, const uint32_t* ins, const uint64_t* coff, const uint64_t* csorted,
          const uint64_t* noff, uint32_t* ids, float* d, hipStream_t s);

// Final prune: nlen[v] = min(|G[v]|, k); copy the first nlen[v] of each list.
void prune_len(uint32_t n, Csr G, uint32_t k, uint32_t* nlen, hipStream_t s);
void prune_copy(uint32_t n, Csr G, const uint64_t* noff, uint32_t* ids, float* d, hipStream_t s);

}  // namespace refine
}  // namespace ngt_amd
