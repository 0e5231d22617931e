// onng_kernels.hip -- gfx950 kernels of the ONNG reconstruction: the edge
// adjustment of GraphReconstructor::reconstructGraph / convertToANNG
// (GraphReconstructor.h:389-561) as count, scan, scatter, per-list sort and
// dedupe, and the path adjustment of adjustPathsEffectively (:197-386) as a
// candidate extraction (phase A) and a rank-synchronous decision (phase B).
// No distance is computed: every comparison is on the stored floats.
//
// No kernel waits for another block: phase B's decide kernel reads only flags
// committed by earlier launches and reports "still waiting" instead.
#include "onng_kernels.h"

#include <algorithm>

#include "ngt_device.h"

namespace ngt_amd {
namespace onng {
namespace {

constexpr uint32_t kNone = 0xffffffffu;

// ObjectDistance::operator< compares floats, for which -0 == +0.
__device__ __forceinline__ uint64_t list_key(float d, uint32_t id) { return make_key(d == 0.f ? 0.f : d, id); }

__device__ __forceinline__ uint32_t hash_id(uint32_t id) { return (id * 2654435761u) >> 8; }

// ---------------------------------------------------------------------------
// exclusive scan, one block, 8 values per thread and step
// ---------------------------------------------------------------------------
constexpr int kScanThreads = 1024, kScanPer = 8;
__global__ __launch_bounds__(kScanThreads) void k_scan(const uint32_t* __restrict__ in, uint64_t n,
                                                       uint64_t* __restrict__ out) {
  __shared__ uint64_t part[kScanThreads];
  __shared__ uint64_t carry;
  const uint32_t t = threadIdx.x;
  if (t == 0) carry = 0;
  __syncthreads();
  for (uint64_t base = 0; base < n; base += (uint64_t)kScanThreads * kScanPer) {
    const uint64_t i0 = base + (uint64_t)t * kScanPer;
    uint32_t x[kScanPer];
    uint64_t sum = 0;
#pragma unroll
    for (int k = 0; k < kScanPer; k++) {
      x[k] = i0 + k < n ? in[i0 + k] : 0u;
      sum += x[k];
    }
    part[t] = sum;
    __syncthreads();
    for (int s = 1; s < kScanThreads; s <<= 1) {
      const uint64_t o = t >= (uint32_t)s ? part[t - s] : 0;
      __syncthreads();
      part[t] += o;
      __syncthreads();
    }
    const uint64_t c = carry;
    uint64_t run = c + part[t] - sum;
#pragma unroll
    for (int k = 0; k < kScanPer; k++) {
      if (i0 + k < n) out[i0 + k] = run;
      run += x[k];
    }
    __syncthreads();
    if (t == kScanThreads - 1) carry = c + part[t];
    __syncthreads();
  }
  if (t == 0) out[n] = carry;
}

// ---------------------------------------------------------------------------
// list construction: one wave per source node
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t base_of(uint32_t v, const Csr& B1, const Csr& B2, uint32_t o, const Csr*& from) {
  from = &B1;
  if (o == 0) return 0;
  if (B1.off[v + 1] - B1.off[v] >= o) return o;
  from = &B2;
  return (uint32_t)(B2.off[v + 1] - B2.off[v]);
}

template <bool FILL>
__global__ __launch_bounds__(256) void k_lists(uint32_t n, Csr S, uint32_t take, Csr B1, Csr B2, uint32_t o,
                                               uint32_t* __restrict__ cnt, uint32_t* __restrict__ err,
                                               const uint64_t* __restrict__ lists_off, uint64_t* __restrict__ keys) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t nw = (uint64_t)gridDim.x * 4;
  for (uint64_t vv = 1 + (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); vv < n; vv += nw) {
    const uint32_t v = (uint32_t)vv;
    const Csr* from;
    const uint32_t bl = base_of(v, B1, B2, o, from);
    if (!FILL) {
      if (lane == 0 && bl) atomicAdd(&cnt[v], bl);
    } else if (bl) {
      uint32_t p0 = 0;
      if (lane == 0) p0 = atomicAdd(&cnt[v], bl);
      p0 = __shfl(p0, 0, 64);
      const uint64_t ob = lists_off[v], ol = lists_off[v + 1] - ob, fb = from->off[v];
      for (uint32_t j = lane; j < bl; j += 64)
        if ((uint64_t)p0 + j < ol) keys[ob + p0 + j] = list_key(from->d[fb + j], from->ids[fb + j]);
    }
    const uint64_t sb = S.off[v], sl = S.off[v + 1] - sb;
    const uint32_t t = sl < take ? (uint32_t)sl : take;
    for (uint32_t j = lane; j < t; j += 64) {
      const uint32_t u = S.ids[sb + j];
      if (u == 0 || u >= n) {
        if (!FILL) atomicMin(&err[kErrBadId], v);
        continue;
      }
      const uint32_t pos = atomicAdd(&cnt[u], 1u);
      if (FILL) {
        const uint64_t ob = lists_off[u];
        if (ob + pos < lists_off[u + 1]) keys[ob + pos] = list_key(S.d[sb + j], v);
      }
    }
  }
}

// One wave per list of up to kFastCap keys: the keys in LDS, every lane ranks
// its keys against all of them (equal keys by position) and stores each at its
// rank.
__global__ __launch_bounds__(64) void k_sort_wave(uint32_t n, const uint64_t* __restrict__ off,
                                                  const uint64_t* __restrict__ in, uint64_t* __restrict__ out) {
  __shared__ uint64_t sk[kFastCap];
  const uint32_t lane = threadIdx.x;
  for (uint64_t v = 1 + (uint64_t)blockIdx.x; v < n; v += gridDim.x) {
    const uint64_t b = off[v], len64 = off[v + 1] - b;
    if (len64 == 0 || len64 > kFastCap) continue;  // uniform: v is the block's
    const uint32_t len = (uint32_t)len64;
    __syncthreads();
    for (uint32_t i = lane; i < len; i += 64) sk[i] = in[b + i];
    __syncthreads();
    for (uint32_t i = lane; i < len; i += 64) {
      const uint64_t k = sk[i];
      uint32_t r = 0;
      for (uint32_t j = 0; j < len; j++) {
        const uint64_t x = sk[j];
        r += (x < k) || (x == k && j < i);
      }
      out[b + r] = k;
    }
  }
}

// Hub lists: the same ranking by a block, every pass over the list in global
// memory.
__global__ __launch_bounds__(256) void k_sort_hub(uint32_t n, const uint64_t* __restrict__ off,
                                                  const uint64_t* __restrict__ in, uint64_t* __restrict__ out) {
  for (uint64_t v = 1 + (uint64_t)blockIdx.x; v < n; v += gridDim.x) {
    const uint64_t b = off[v], len = off[v + 1] - b;
    if (len <= kFastCap) continue;
    for (uint64_t i = threadIdx.x; i < len; i += 256) {
      const uint64_t k = in[b + i];
      uint64_t r = 0;
      for (uint64_t j = 0; j < len; j++) {
        const uint64_t x = in[b + j];
        r += (x < k) || (x == k && j < i);
      }
      out[b + r] = k;
    }
  }
}

__global__ __launch_bounds__(256) void k_unique(uint32_t n, const uint64_t* __restrict__ off,
                                                const uint64_t* __restrict__ in, uint64_t* __restrict__ out,
                                                uint32_t* __restrict__ cnt) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t nw = (uint64_t)gridDim.x * 4;
  for (uint64_t v = 1 + (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); v < n; v += nw) {
    const uint64_t b = off[v], len = off[v + 1] - b;
    uint32_t running = 0;
    for (uint64_t base = 0; base < len; base += 64) {
      const uint64_t i = base + lane;
      bool keep = false;
      uint64_t k = 0;
      if (i < len) {
        k = in[b + i];
        const uint32_t prev = i ? key_id(in[b + i - 1]) : 0u;  // the reference's prev starts at 0
        keep = key_id(k) != prev;
      }
      const uint64_t m = ballot64(keep);
      if (keep) out[b + running + mbcnt(m)] = k;
      running += (uint32_t)__popcll(m);
    }
    if (lane == 0) cnt[v] = running;
  }
}

__global__ __launch_bounds__(256) void k_unpack(uint32_t n, const uint64_t* __restrict__ off_in,
                                                const uint64_t* __restrict__ keys,
                                                const uint64_t* __restrict__ off_out, uint32_t* __restrict__ ids,
                                                float* __restrict__ d) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t nw = (uint64_t)gridDim.x * 4;
  for (uint64_t v = 1 + (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); v < n; v += nw) {
    const uint64_t ib = off_in[v], ob = off_out[v], len = off_out[v + 1] - ob;
    for (uint64_t i = lane; i < len; i += 64) {
      const uint64_t k = keys[ib + i];
      ids[ob + i] = key_id(k);
      d[ob + i] = key_dist(k);
    }
  }
}

__global__ __launch_bounds__(256) void k_check(uint32_t n, Csr G, uint32_t* __restrict__ err) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t nw = (uint64_t)gridDim.x * 4;
  for (uint64_t v = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); v < n; v += nw) {
    const uint64_t b = G.off[v], len = G.off[v + 1] - b;
    for (uint64_t j = lane; j < len; j += 64) {
      const uint32_t id = G.ids[b + j];
      if (id == 0 || id >= n || v == 0) atomicMin(&err[kErrBadId], (uint32_t)v);
      if (j && list_key(G.d[b + j - 1], G.ids[b + j - 1]) > list_key(G.d[b + j], id))
        atomicMin(&err[kErrOrder], (uint32_t)v);
    }
  }
}

// ---------------------------------------------------------------------------
// path adjustment, phase A: a block per node v.  v's list goes into an open-
// addressing table id -> rank (LDS, or the block's global table for a hub);
// wave w streams the lists of the path nodes p = tmp[v][w], [w + 4], ... and
// probes every entry.
// ---------------------------------------------------------------------------
template <bool HUB, bool FILL>
__global__ __launch_bounds__(256) void k_candidates(uint32_t n, Csr G, uint32_t* __restrict__ ccnt,
                                                    const uint64_t* __restrict__ coff, uint2* __restrict__ cand,
                                                    uint32_t* __restrict__ hub_table, uint32_t hub_slots,
                                                    uint32_t* __restrict__ err) {
  __shared__ uint32_t s_id[HUB ? 1 : 2 * kFastCap];
  __shared__ uint32_t s_rk[HUB ? 1 : 2 * kFastCap];
  uint32_t* const tab_id = HUB ? hub_table + (size_t)blockIdx.x * hub_slots * 2 : s_id;
  uint32_t* const tab_rk = HUB ? tab_id + hub_slots : s_rk;
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (uint64_t vv = 1 + (uint64_t)blockIdx.x; vv < n; vv += gridDim.x) {
    const uint32_t v = (uint32_t)vv;
    const uint64_t b = G.off[v], len64 = G.off[v + 1] - b;
    if (len64 == 0 || HUB != (len64 > kFastCap)) continue;  // uniform: v is the block's
    const uint32_t len = (uint32_t)len64;
    uint32_t slots = 2 * kFastCap;
    if (HUB) {
      while ((uint64_t)slots < 2 * len64) slots <<= 1;
      if (slots > hub_slots) {  // the host sized the tables from the longest list
        if (threadIdx.x == 0) atomicMin(&err[kErrTable], v);
        continue;
      }
    }
    const uint32_t mask = slots - 1;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < slots; i += 256) tab_id[i] = 0;
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < len; j += 256) {
      const uint32_t id = G.ids[b + j];
      uint32_t h = hash_id(id) & mask;
      for (;;) {  // at most len <= slots / 2 ids: an empty slot always exists
        const uint32_t old = atomicCAS(&tab_id[h], 0u, id);
        if (old == 0) {
          tab_rk[h] = j;
          break;
        }
        if (old == id) {
          if (!FILL) atomicMin(&err[kErrRepeated], v);
          break;
        }
        h = (h + 1) & mask;
      }
    }
    __syncthreads();
    for (uint32_t sni = wave; sni < len; sni += 4) {
      const uint32_t p = G.ids[b + sni];
      const float dp = G.d[b + sni];
      const uint64_t pb = G.off[p], pl = G.off[p + 1] - pb;
      for (uint64_t pni = lane; pni < pl; pni += 64) {
        const uint32_t dst = G.ids[pb + pni];
        uint32_t h = hash_id(dst) & mask, r = kNone;
        for (;;) {
          const uint32_t t = tab_id[h];
          if (t == 0) break;
          if (t == dst) {
            r = tab_rk[h];
            break;
          }
          h = (h + 1) & mask;
        }
        if (r == kNone) continue;
        const float dd = G.d[b + r];
        if (dp < dd && G.d[pb + pni] < dd) {
          const uint64_t e = b + r;
          const uint32_t pos = atomicAdd(&ccnt[e], 1u);
          if (FILL) {
            const uint64_t c0 = coff[e];
            if (c0 + pos < coff[e + 1]) cand[c0 + pos] = make_uint2(sni, (uint32_t)pni);
          }
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// phase B
// ---------------------------------------------------------------------------
__global__ void k_alive_init(uint32_t n, const uint64_t* __restrict__ off, uint32_t* __restrict__ alive,
                             uint32_t* __restrict__ counters) {
  const uint64_t v = 1 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (v < n && off[v + 1] > off[v]) alive[atomicAdd(&counters[1], 1u)] = (uint32_t)v;
}

__global__ void k_decide(const uint32_t* __restrict__ work, uint32_t nwork, uint32_t r, Csr G,
                         const uint64_t* __restrict__ coff, const uint2* __restrict__ cand,
                         const uint8_t* __restrict__ flag, const uint32_t* __restrict__ outcnt, uint64_t min_edges,
                         uint8_t* __restrict__ dec) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nwork) return;
  const uint32_t v = work[i];
  const uint64_t b = G.off[v], len = G.off[v + 1] - b, e = b + r;
  uint8_t d = kKept;
  // once |out[v]| + |tmp[v]| - r <= minE it stays so: the rest of the list is kept
  if ((uint64_t)outcnt[v] + len - r > min_edges) {
    bool waiting = false;
    for (uint64_t c = coff[e], ce = coff[e + 1]; c < ce; c++) {
      const uint2 k = cand[c];  // (rank of p in v, rank of dst in p); k.x < r
      if (flag[b + k.x] != kKept) continue;
      if (k.y > r) continue;  // p reaches dst at a later rank: not in out[p] yet
      const uint32_t p = G.ids[b + k.x];
      if (k.y == r && p > v) continue;  // same rank, higher id: not processed yet
      const uint8_t f = flag[G.off[p] + k.y];
      if (f == kKept) {
        d = kDropped;
        break;
      }
      if (f == kUndecided) waiting = true;  // same rank, lower id, decided by a later launch
    }
    if (d == kKept && waiting) d = kUndecided;
  }
  dec[i] = d;
}

__global__ void k_commit(const uint32_t* __restrict__ work, uint32_t nwork, uint32_t r,
                         const uint64_t* __restrict__ off, const uint8_t* __restrict__ dec,
                         uint8_t* __restrict__ flag, uint32_t* __restrict__ outcnt, uint32_t* __restrict__ next_work,
                         uint32_t* __restrict__ next_alive, uint32_t* __restrict__ counters) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nwork) return;
  const uint32_t v = work[i];
  const uint8_t d = dec[i];
  if (d == kUndecided) {
    next_work[atomicAdd(&counters[0], 1u)] = v;
    return;
  }
  flag[off[v] + r] = d;
  if (d == kKept) outcnt[v] += 1;
  if (off[v + 1] - off[v] > (uint64_t)r + 1) next_alive[atomicAdd(&counters[1], 1u)] = v;
}

__global__ __launch_bounds__(256) void k_emit(uint32_t n, Csr G, const uint8_t* __restrict__ flag,
                                              const uint64_t* __restrict__ off_out, uint32_t* __restrict__ ids,
                                              float* __restrict__ d) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t nw = (uint64_t)gridDim.x * 4;
  for (uint64_t v = 1 + (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); v < n; v += nw) {
    const uint64_t b = G.off[v], len = G.off[v + 1] - b, ob = off_out[v], ol = off_out[v + 1] - ob;
    uint64_t running = 0;
    for (uint64_t base = 0; base < len; base += 64) {
      const uint64_t i = base + lane;
      const bool keep = i < len && flag[b + i] == kKept;
      const uint64_t m = ballot64(keep);
      const uint64_t pos = running + mbcnt(m);
      if (keep && pos < ol) {
        ids[ob + pos] = G.ids[b + i];
        d[ob + pos] = G.d[b + i];
      }
      running += (uint64_t)__popcll(m);
    }
  }
}

uint32_t wave_grid(uint32_t n) { return std::max(1u, std::min((n + 3) / 4, 1u << 18)); }
uint32_t node_grid(uint32_t n) { return std::max(1u, std::min(n, 1u << 16)); }

}  // namespace

void scan_u32(const uint32_t* in, uint64_t n, uint64_t* out, hipStream_t s) {
  hipLaunchKernelGGL(k_scan, dim3(1), dim3(kScanThreads), 0, s, in, n, out);
}

void count_lists(uint32_t n, Csr S, uint32_t take, Csr B1, Csr B2, uint32_t o, uint32_t* cnt, uint32_t* err,
                 hipStream_t s) {
  hipLaunchKernelGGL(k_lists<false>, dim3(wave_grid(n)), dim3(256), 0, s, n, S, take, B1, B2, o, cnt, err,
                     (const uint64_t*)nullptr, (uint64_t*)nullptr);
}
void fill_lists(uint32_t n, Csr S, uint32_t take, Csr B1, Csr B2, uint32_t o, const uint64_t* lists_off,
                uint32_t* cur, uint64_t* keys, hipStream_t s) {
  hipLaunchKernelGGL(k_lists<true>, dim3(wave_grid(n)), dim3(256), 0, s, n, S, take, B1, B2, o, cur,
                     (uint32_t*)nullptr, lists_off, keys);
}
void sort_lists(uint32_t n, const uint64_t* off, const uint64_t* keys_in, uint64_t* keys_out, bool any_long,
                hipStream_t s) {
  hipLaunchKernelGGL(k_sort_wave, dim3(node_grid(n)), dim3(64), 0, s, n, off, keys_in, keys_out);
  if (any_long) hipLaunchKernelGGL(k_sort_hub, dim3(std::min(node_grid(n), 4096u)), dim3(256), 0, s, n, off, keys_in, keys_out);
}
void unique_lists(uint32_t n, const uint64_t* off, const uint64_t* keys_sorted, uint64_t* keys_out, uint32_t* cnt,
                  hipStream_t s) {
  hipLaunchKernelGGL(k_unique, dim3(wave_grid(n)), dim3(256), 0, s, n, off, keys_sorted, keys_out, cnt);
}
void unpack_lists(uint32_t n, const uint64_t* off_in, const uint64_t* keys, const uint64_t* off_out, uint32_t* ids,
                  float* d, hipStream_t s) {
  hipLaunchKernelGGL(k_unpack, dim3(wave_grid(n)), dim3(256), 0, s, n, off_in, keys, off_out, ids, d);
}
void check_lists(uint32_t n, Csr G, uint32_t* err, hipStream_t s) {
  hipLaunchKernelGGL(k_check, dim3(wave_grid(n)), dim3(256), 0, s, n, G, err);
}

void candidates(uint32_t n, Csr G, bool fill, uint32_t* ccnt, const uint64_t* coff, uint2* cand, uint32_t* hub_table,
                uint32_t hub_slots, uint32_t* err, hipStream_t s) {
  const dim3 g(node_grid(n)), b(256);
  if (fill) hipLaunchKernelGGL((k_candidates<false, true>), g, b, 0, s, n, G, ccnt, coff, cand, hub_table, hub_slots, err);
  else hipLaunchKernelGGL((k_candidates<false, false>), g, b, 0, s, n, G, ccnt, coff, cand, hub_table, hub_slots, err);
  if (!hub_table) return;
  const dim3 gh(kHubBlocks);
  if (fill) hipLaunchKernelGGL((k_candidates<true, true>), gh, b, 0, s, n, G, ccnt, coff, cand, hub_table, hub_slots, err);
  else hipLaunchKernelGGL((k_candidates<true, false>), gh, b, 0, s, n, G, ccnt, coff, cand, hub_table, hub_slots, err);
}

void alive_init(uint32_t n, const uint64_t* off, uint32_t* alive, uint32_t* counters, hipStream_t s) {
  hipLaunchKernelGGL(k_alive_init, dim3((n + 255) / 256), dim3(256), 0, s, n, off, alive, counters);
}
void decide(const uint32_t* work, uint32_t nwork, uint32_t r, Csr G, const uint64_t* coff, const uint2* cand,
            const uint8_t* flag, const uint32_t* outcnt, uint64_t min_edges, uint8_t* dec, hipStream_t s) {
  hipLaunchKernelGGL(k_decide, dim3((nwork + 255) / 256), dim3(256), 0, s, work, nwork, r, G, coff, cand, flag,
                     outcnt, min_edges, dec);
}
void commit(const uint32_t* work, uint32_t nwork, uint32_t r, const uint64_t* off, const uint8_t* dec, uint8_t* flag,
            uint32_t* outcnt, uint32_t* next_work, uint32_t* next_alive, uint32_t* counters, hipStream_t s) {
  hipLaunchKernelGGL(k_commit, dim3((nwork + 255) / 256), dim3(256), 0, s, work, nwork, r, off, dec, flag, outcnt,
                     next_work, next_alive, counters);
}
void emit_kept(uint32_t n, Csr G, const uint8_t* flag, const uint64_t* off_out, uint32_t* ids, float* d,
               hipStream_t s) {
  hipLaunchKernelGGL(k_emit, dim3(wave_grid(n)), dim3(256), 0, s, n, G, flag, off_out, ids, d);
}

}  // namespace onng
}  // namespace ngt_amd
