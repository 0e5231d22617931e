// refine_kernels.hip -- gfx950 kernels of GraphReconstructor::refineANNG
// (GraphReconstructor.h:803-924) between two search launches: the outgoing
// step (append the results, sort, drop adjacent repeats of an id), the incoming
// step (addEdge of every result's reverse, Graph.h:845-873) and the final
// prune, as count, scan, scatter on CSR graphs in HBM.  The scan, the per-list
// sort and the dedupe are onng_kernels.hip's.  No distance is computed: every
// comparison is on the stored floats, packed as (distance, id) keys.
//
// The incoming step by rule.  The reference walks the batch's nodes s in
// ascending id and, for each result (t, d) with t != s, takes lower_bound of
// K = (d, s) in t's list as it stands at that moment; it inserts K there unless
// the element at that position has id s.  Fix a target t, let L be its list
// after the outgoing step (sorted), and let the sources that name t be
// s_1 < s_2 < ... with keys K_1, K_2, ...; a search returns no id twice, so
// each source names t once and the K_i have distinct ids.  When s_i's turn
// comes the list is L plus the K_j (j < i) that were inserted.  Let X be the
// first element of L not below K_i and Y the first inserted K_j (j < i) not
// below K_i; Y has another id than s_i, so Y > K_i.  lower_bound yields the
// smaller of X and Y, and that element has id s_i exactly when X has id s_i and
// Y does not lie below X.  Hence
//   (a) no X, or X has another id:  K_i is inserted, whatever was inserted before;
//   (b) X == K_i:                   nothing is inserted (Y > K_i = X);
//   (c) X = (d', s_i) with d' > d:  K_i is inserted iff some inserted K_j with
//                                   j < i lies strictly between K_i and X.
// (a) and (b) do not depend on the order at all.  Neither does (c): a K_j
// strictly between K_i and X is itself of case (a).  X is the first element of
// L not below K_i and K_j lies between the two, so X is also the first element
// of L not below K_j, and X has the id s_i, not s_j.  So "some inserted K_j"
// is "some candidate K_j of case (a) from a source with a lower id", which is
// known before anything is inserted: k_resolve decides every (c) candidate of a
// target on its own, one wave per target, and no workgroup waits for another.
// The final list is L plus the inserted keys in key order: no two of these keys
// are equal ((b) removed the only possible equals), so the order of insertion
// does not show in the result.
//
// Lists grow without bound (an ANNG's hubs): every kernel here walks lists in
// global memory with a wave per list and binary searches; only the sort has a
// one-wave LDS form (refine::kFastCap) with onng's global-memory form above it.
#include "refine_kernels.h"

#include <algorithm>

#include "ngt_device.h"

namespace ngt_amd {
namespace refine {
namespace {

constexpr uint64_t kDropped = ~0ull;

// ObjectDistance::operator< compares floats, for which -0 == +0.
__device__ __forceinline__ uint64_t list_key(float d, uint32_t id) { return make_key(d == 0.f ? 0.f : d, id); }

// A list of the state after the outgoing step.
struct View {
  const uint64_t* keys;  // batch node: packed keys; else null
  const uint32_t* ids;
  const float* d;
  uint64_t len;
  __device__ __forceinline__ uint64_t key(uint64_t i) const { return keys ? keys[i] : list_key(d[i], ids[i]); }
  // the first position whose key is not below k
  __device__ __forceinline__ uint64_t lower_bound(uint64_t k) const {
    uint64_t lo = 0, hi = len;
    while (lo < hi) {
      const uint64_t mid = (lo + hi) >> 1;
      if (key(mid) < k) lo = mid + 1;
      else hi = mid;
    }
    return lo;
  }
};

__device__ __forceinline__ View view_of(const Lists& L, uint32_t v) {
  View w;
  const uint32_t i = v - L.first;  // wraps for v < first
  if (i < L.count) {
    w.keys = L.bkeys + L.boff[i + 1];
    w.ids = nullptr;
    w.d = nullptr;
    w.len = L.bcnt[i + 1];
  } else {
    const uint64_t b = L.G.off[v];
    w.keys = nullptr;
    w.ids = L.G.ids + b;
    w.d = L.G.d + b;
    w.len = L.G.off[v + 1] - b;
  }
  return w;
}

__device__ __forceinline__ uint64_t lower_bound_keys(const uint64_t* keys, uint64_t len, uint64_t k) {
  uint64_t lo = 0, hi = len;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if (keys[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_mask(const uint8_t* __restrict__ valid, uint32_t first, uint32_t count,
                                              uint32_t* __restrict__ cnt) {
  const uint32_t q = blockIdx.x * 256 + threadIdx.x;
  if (q < count && !valid[first + q]) cnt[q] = 0;
}

// ---------------------------------------------------------------------------
// outgoing step: one wave per batch node
// ---------------------------------------------------------------------------
template <bool FILL>
__global__ __launch_bounds__(256) void k_batch(uint32_t n, Csr G, Results R, uint32_t* __restrict__ blen,
                                               uint32_t* __restrict__ err,
                                               const uint64_t* __restrict__ boff, uint64_t* __restrict__ keys) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t nw = (uint64_t)gridDim.x * 4;
  if (!FILL && blockIdx.x == 0 && threadIdx.x == 0) blen[0] = 0;
  for (uint64_t q = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); q < R.count; q += nw) {
    const uint32_t v = R.first + (uint32_t)q;
    const uint64_t gb = G.off[v], gl = G.off[v + 1] - gb;
    uint32_t rc = R.cnt[q];
    if (rc > R.stride) {
      if (!FILL && lane == 0) atomicMin(&err[kErrResultCount], v);
      rc = R.stride;
    }
    const uint64_t ob = FILL ? boff[q + 1] : 0, ol = FILL ? boff[q + 2] - ob : 0;
    if (FILL)
      for (uint64_t j = lane; j < gl && j < ol; j += 64) keys[ob + j] = list_key(G.d[gb + j], G.ids[gb + j]);
    uint32_t running = 0;
    for (uint32_t base = 0; base < rc; base += 64) {
      const uint32_t j = base + lane;
      bool take = false;
      uint32_t id = 0;
      if (j < rc) {
        id = R.ids[(uint64_t)q * R.stride + j];
        if (id == 0 || id >= n) {
          if (!FILL) atomicMin(&err[kErrResultId], v);
        } else {
          take = id != v;
        }
      }
      const uint64_t m = ballot64(take);
      if (FILL && take) {
        const uint64_t pos = gl + running + mbcnt(m);
        if (pos < ol) keys[ob + pos] = list_key(R.d[(uint64_t)q * R.stride + j], id);
      }
      running += (uint32_t)__popcll(m);
    }
    if (!FILL && lane == 0) blen[q + 1] = (uint32_t)(gl + running);
  }
}

// ---------------------------------------------------------------------------
// incoming step: one thread per result slot
// ---------------------------------------------------------------------------
template <bool FILL>
__global__ __launch_bounds__(256) void k_incoming(uint32_t n, Lists L, Results R, uint32_t* __restrict__ ccnt,
                                                  uint32_t* __restrict__ ropen, const uint64_t* __restrict__ coff,
                                                  uint64_t* __restrict__ ckeys, uint64_t* __restrict__ cx) {
  const uint64_t total = (uint64_t)R.count * R.stride;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
    const uint64_t q = i / R.stride;
    const uint32_t j = (uint32_t)(i - q * R.stride);
    if (j >= R.cnt[q]) continue;
    const uint32_t s = R.first + (uint32_t)q, t = R.ids[i];
    if (t == s || t == 0 || t >= n) continue;  // bad ids were reported by k_batch
    const uint64_t K = list_key(R.d[i], s);
    const View w = view_of(L, t);
    const uint64_t p = w.lower_bound(K);
    uint64_t X = 0;  // 0 = case (a): insert
    if (p < w.len) {
      const uint64_t x = w.key(p);
      if (x == K) continue;  // case (b)
      if (key_id(x) == s) X = x;  // case (c)
    }
    if (!FILL) {
      atomicAdd(&ccnt[t], 1u);
      if (X) atomicAdd(&ropen[t], 1u);
    } else {
      const uint64_t b = coff[t];
      const uint64_t pos = b + atomicAdd(&ccnt[t], 1u);
      if (pos < coff[t + 1]) {
        ckeys[pos] = K;
        cx[pos] = X;
      }
    }
  }
}

// One wave per target with open candidates.  Only open entries (cx != 0) are
// written, and only the others are read as the keys that may lie between: the
// decisions do not depend on one another.
__global__ __launch_bounds__(256) void k_resolve(uint32_t n, const uint64_t* __restrict__ coff,
                                                 const uint32_t* __restrict__ ropen, uint64_t* ckeys,
                                                 const uint64_t* __restrict__ cx, uint32_t* __restrict__ ins) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t nw = (uint64_t)gridDim.x * 4;
  for (uint64_t t = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < n; t += nw) {
    const uint64_t b = coff[t], len = coff[t + 1] - b;
    uint32_t dropped = 0;
    if (ropen[t]) {
      for (uint64_t e = 0; e < len; e++) {  // uniform: every lane looks at entry e
        const uint64_t X = cx[b + e];
        if (X == 0) continue;
        const uint64_t K = ckeys[b + e];
        const uint32_t s = key_id(K);
        bool between = false;
        for (uint64_t f = lane; f < len; f += 64) {
          if (cx[b + f] != 0) continue;
          const uint64_t k = ckeys[b + f];
          between |= key_id(k) < s && K < k && k < X;
        }
        if (ballot64(between) == 0) {
          if (lane == 0) ckeys[b + e] = kDropped;
          dropped++;
        }
      }
    }
    if (lane == 0) ins[t] = (uint32_t)len - dropped;
  }
}

// ---------------------------------------------------------------------------
// the new lists
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_new_len(uint32_t n, Lists L, const uint32_t* __restrict__ ins,
                                                 uint32_t* __restrict__ nlen) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  uint64_t len = 0;
  if (v) len = view_of(L, v).len + (ins ? ins[v] : 0u);
  nlen[v] = (uint32_t)len;
}

__global__ __launch_bounds__(256) void k_emit(uint32_t n, Lists L, const uint32_t* __restrict__ ins,
                                              const uint64_t* __restrict__ coff, const uint64_t* __restrict__ csorted,
                                              const uint64_t* __restrict__ noff, uint32_t* __restrict__ ids,
                                              float* __restrict__ d) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t nw = (uint64_t)gridDim.x * 4;
  for (uint64_t vv = 1 + (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); vv < n; vv += nw) {
    const uint32_t v = (uint32_t)vv;
    const View w = view_of(L, v);
    const uint64_t ob = noff[v], ol = noff[v + 1] - ob;
    const uint64_t ni = ins ? ins[v] : 0u;
    const uint64_t* ck = ni ? csorted + coff[v] : nullptr;
    for (uint64_t i = lane; i < w.len; i += 64) {
      const uint64_t k = w.key(i);
      const uint64_t pos = i + (ni ? lower_bound_keys(ck, ni, k) : 0);
      if (pos < ol) {
        ids[ob + pos] = key_id(k);
        d[ob + pos] = key_dist(k);
      }
    }
    for (uint64_t j = lane; j < ni; j += 64) {
      const uint64_t k = ck[j];
      const uint64_t pos = j + w.lower_bound(k);
      if (pos < ol) {
        ids[ob + pos] = key_id(k);
        d[ob + pos] = key_dist(k);
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_prune_len(uint32_t n, Csr G, uint32_t k, uint32_t* __restrict__ nlen) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const uint64_t len = v ? G.off[v + 1] - G.off[v] : 0;
  nlen[v] = len > k ? k : (uint32_t)len;
}

// out = max(out, in[0 .. n)): a wave folds 64 values per step, one atomic per wave
__global__ __launch_bounds__(256) void k_max(const uint32_t* __restrict__ in, uint64_t n, uint32_t* __restrict__ out) {
  uint32_t m = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) m = max(m, in[i]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
  if ((threadIdx.x & 63) == 0 && m) atomicMax(out, m);
}

__global__ __launch_bounds__(256) void k_prune_copy(uint32_t n, Csr G, const uint64_t* __restrict__ noff,
                                                    uint32_t* __restrict__ ids, float* __restrict__ d) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t nw = (uint64_t)gridDim.x * 4;
  for (uint64_t v = 1 + (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); v < n; v += nw) {
    const uint64_t ib = G.off[v], ob = noff[v], len = noff[v + 1] - ob;
    for (uint64_t i = lane; i < len; i += 64) {
      ids[ob + i] = G.ids[ib + i];
      d[ob + i] = G.d[ib + i];
    }
  }
}

uint32_t wave_grid(uint64_t n) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + 3) / 4, 1u << 18)); }
uint32_t thread_grid(uint64_t n) { return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, 1u << 20)); }

}  // namespace

void mask_counts(const uint8_t* valid, uint32_t first, uint32_t count, uint32_t* cnt, hipStream_t s) {
  hipLaunchKernelGGL(k_mask, dim3((count + 255) / 256), dim3(256), 0, s, valid, first, count, cnt);
}

void max_u32(const uint32_t* in, uint64_t n, uint32_t* out, hipStream_t s) {
  hipLaunchKernelGGL(k_max, dim3(std::min(thread_grid(n), 1024u)), dim3(256), 0, s, in, n, out);
}

void batch_len(uint32_t n, Csr G, Results R, uint32_t* blen, uint32_t* err, hipStream_t s) {
  hipLaunchKernelGGL(k_batch<false>, dim3(wave_grid(R.count)), dim3(256), 0, s, n, G, R, blen, err,
                     (const uint64_t*)nullptr, (uint64_t*)nullptr);
}
void batch_fill(uint32_t n, Csr G, Results R, const uint64_t* boff, uint64_t* keys, hipStream_t s) {
  hipLaunchKernelGGL(k_batch<true>, dim3(wave_grid(R.count)), dim3(256), 0, s, n, G, R, (uint32_t*)nullptr,
                     (uint32_t*)nullptr, boff, keys);
}

void incoming(uint32_t n, Lists L, Results R, bool fill, uint32_t* ccnt, uint32_t* ropen, const uint64_t* coff,
              uint64_t* ckeys, uint64_t* cx, hipStream_t s) {
  const dim3 g(thread_grid((uint64_t)R.count * R.stride)), b(256);
  if (fill) hipLaunchKernelGGL(k_incoming<true>, g, b, 0, s, n, L, R, ccnt, ropen, coff, ckeys, cx);
  else hipLaunchKernelGGL(k_incoming<false>, g, b, 0, s, n, L, R, ccnt, ropen, coff, ckeys, cx);
}
void resolve(uint32_t n, const uint64_t* coff, const uint32_t* ropen, uint64_t* ckeys, const uint64_t* cx,
             uint32_t* ins, hipStream_t s) {
  hipLaunchKernelGGL(k_resolve, dim3(wave_grid(n)), dim3(256), 0, s, n, coff, ropen, ckeys, cx, ins);
}

void new_len(uint32_t n, Lists L, const uint32_t* ins, uint32_t* nlen, hipStream_t s) {
  hipLaunchKernelGGL(k_new_len, dim3((n + 255) / 256), dim3(256), 0, s, n, L, ins, nlen);
}
void emit(uint32_t n, Lists L, const uint32_t* ins, const uint64_t* coff, const uint64_t* csorted,
          const uint64_t* noff, uint32_t* ids, float* d, hipStream_t s) {
  hipLaunchKernelGGL(k_emit, dim3(wave_grid(n)), dim3(256), 0, s, n, L, ins, coff, csorted, noff, ids, d);
}

void prune_len(uint32_t n, Csr G, uint32_t k, uint32_t* nlen, hipStream_t s) {
  hipLaunchKernelGGL(k_prune_len, dim3((n + 255) / 256), dim3(256), 0, s, n, G, k, nlen);
}
void prune_copy(uint32_t n, Csr G, const uint64_t* noff, uint32_t* ids, float* d, hipStream_t s) {
  hipLaunchKernelGGL(k_prune_copy, dim3(wave_grid(n)), dim3(256), 0, s, n, G, noff, ids, d);
}

}  // namespace refine
}  // namespace ngt_amd
