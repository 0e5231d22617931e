// onng_kernels.h -- launchers of the ONNG reconstruction kernels
// (onng_kernels.hip) used by onng.cpp.  Everything works on CSR graphs in HBM:
// node v's list is ids/dists[off[v] .. off[v+1]), slot 0 the dummy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ngt_amd {
namespace onng {

// Longest list the one-wave LDS sort and the LDS id table hold; longer lists
// (hubs) take the paths that work in global memory.
constexpr uint32_t kFastCap = 1024;
// Blocks of the hub form of the candidate kernel (each owns a global table).
constexpr uint32_t kHubBlocks = 64;

// Edge flags of path adjustment.
enum : uint8_t { kUndecided = 0, kKept = 1, kDropped = 2 };

// Error words (min node id, 0xffffffff = none).
enum { kErrBadId = 0, kErrRepeated = 1, kErrOrder = 2, kErrTable = 3, kErrWords = 4 };

struct Csr {
  const uint64_t* off;
  const uint32_t* ids;
  const float* d;
};

// out[i] = sum of in[0..i), out[n] = the total.
void scan_u32(const uint32_t* in, uint64_t n, uint64_t* out, hipStream_t s);

// Lists L[u] = base(u) + {(v, d) : (u, d) among the first min(take, |S[v]|)
// entries of S[v]}, base(u) = nothing if o == 0, the first o entries of B1[u]
// if it has that many, else the whole of B2[u].  count adds the lengths to cnt
// (zeroed by the caller); fill writes packed (distance, id) keys at
// lists_off[u] + a cursor (cur zeroed by the caller).
void count_lists(uint32_t n, Csr S, uint32_t take, Csr B1, Csr B2, uint32_t o, uint32_t* cnt, uint32_t* err,
                 hipStream_t s);
void fill_lists(uint32_t n, Csr S, uint32_t take, Csr B1, Csr B2, uint32_t o, const uint64_t* lists_off,
                uint32_t* cur, uint64_t* keys, hipStream_t s);
// keys_out = every list of keys_in in ascending key order (lists of up to
// kFastCap keys by one wave in LDS, longer ones by a block in global memory).
void sort_lists(uint32_t n, const uint64_t* off, const uint64_t* keys_in, uint64_t* keys_out, bool any_long,
                hipStream_t s);
// Drops every key whose id equals its predecessor's; the kept keys go to the
// front of the list's range in keys_out, their number to cnt.
void unique_lists(uint32_t n, const uint64_t* off, const uint64_t* keys_sorted, uint64_t* keys_out, uint32_t* cnt,
                  hipStream_t s);
void unpack_lists(uint32_t n, const uint64_t* off_in, const uint64_t* keys, const uint64_t* off_out, uint32_t* ids,
                  float* d, hipStream_t s);

// err[kErrBadId] / err[kErrOrder]: the first node with an id outside [1, n) /
// a list that is not in (distance, id) order.
void check_lists(uint32_t n, Csr G, uint32_t* err, hipStream_t s);

// Path adjustment, phase A: for every edge slot e = off[v] + r of node v the
// candidates (rank of p in v, rank of dst in p) with d(v,p) < d(v,dst) and
// d(p,dst) < d(v,dst).  fill == false counts into ccnt[e]; fill == true writes
// cand[coff[e] + cursor].  hub_table: kHubBlocks tables of hub_slots (a power
// of two >= twice the longest list) {id, rank} words, or null when no list is
// longer than kFastCap.  Repeated ids in a list set err[kErrRepeated].
void candidates(uint32_t n, Csr G, bool fill, uint32_t* ccnt, const uint64_t* coff, uint2* cand, uint32_t* hub_table,
                uint32_t hub_slots, uint32_t* err, hipStream_t s);

// Phase B.  alive_init: the nodes with a list; decide: one rank-r decision per
// work item from the committed flags (0 = still waiting for a lower id of the
// same rank); commit: store the decisions, queue the rest.  counters[0] =
// items still undecided, counters[1] = nodes alive at rank r + 1.
void alive_init(uint32_t n, const uint64_t* off, uint32_t* alive, uint32_t* counters, hipStream_t s);
void decide(const uint32_t* work, uint32_t nwork, uint32_t r, Csr G, const uint64_t* coff, const uint2* cand,
            const uint8_t* flag, const uint32_t* outcnt, uint64_t min_edges, uint8_t* dec, hipStream_t s);
void commit(const uint32_t* work, uint32_t nwork, uint32_t r, const uint64_t* off, const uint8_t* dec, uint8_t* flag,
            uint32_t* outcnt, uint32_t* next_work, uint32_t* next_alive, uint32_t* counters, hipStream_t s);
void emit_kept(uint32_t n, Csr G, const uint8_t* flag, const uint64_t* off_out, uint32_t* ids, float* d,
               hipStream_t s);

}  // namespace onng
}  // namespace ngt_amd
