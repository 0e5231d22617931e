// edges_kernels.hip -- gfx950 kernel of the ANNG re-cut
// (GraphReconstructor::reconstructANNGFromANNG, GraphReconstructor.h:721-801):
// which entries of every list survive a cut to K edges, and both directions of
// each as a count or as a packed key.  The lists are then sorted and deduped by
// the kernels of onng_kernels.hip.  No distance is computed: every comparison
// is on the stored floats.
//
// One wave per list, the list in chunks of 64.  Per chunk a ballot on "id < v"
// and a prefix count give every lower-id entry its rank among the list's
// lower-id entries; a ballot on "distance below its predecessor's" finds the
// entry at which the reference's walk of the list ends.  Every ballot and
// shuffle is executed by all 64 lanes; the loop bounds are wave-uniform.
#include "edges_kernels.h"

#include <algorithm>

#include "ngt_device.h"

namespace ngt_amd {
namespace edges {
namespace {

using onng::Csr;

// ObjectDistance::operator< compares floats, for which -0 == +0.
__device__ __forceinline__ uint64_t list_key(float d, uint32_t id) { return make_key(d == 0.f ? 0.f : d, id); }

template <bool FILL>
__global__ __launch_bounds__(256) void k_recut(uint32_t n, Csr G, uint32_t K, uint32_t* __restrict__ cnt,
                                               const uint64_t* __restrict__ lists_off, uint64_t* __restrict__ keys) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t nw = (uint64_t)gridDim.x * 4;
  for (uint64_t vv = 1 + (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6); vv < n; vv += nw) {
    const uint32_t v = (uint32_t)vv;
    const uint64_t b = G.off[v], len = G.off[v + 1] - b;
    const uint64_t vb = FILL ? lists_off[v] : 0, vl = FILL ? lists_off[v + 1] - vb : 0;
    uint32_t taken = 0;   // lower-id entries selected so far (wave-uniform)
    float last = 0.0f;    // the distance before this chunk (prevDistance starts at 0)
    for (uint64_t base = 0; base < len && taken < K; base += 64) {
      const uint64_t i = base + lane;
      const bool in = i < len;
      const uint32_t m = in ? G.ids[b + i] : 0u;
      const float d = in ? G.d[b + i] : 0.0f;
      float prev = __shfl_up(d, 1, 64);
      if (lane == 0) prev = last;
      const uint64_t mbad = ballot64(in && prev > d);
      // the walk ends at the first such entry: only the lanes below it count
      const uint64_t ok = mbad ? ((1ull << (__ffsll((unsigned long long)mbad) - 1)) - 1ull) : ~0ull;
      const bool lower = in && m != 0u && m < v && ((ok >> lane) & 1ull);
      const uint64_t mlow = ballot64(lower);
      const uint32_t rank = taken + mbcnt(mlow);
      const bool sel = lower && rank < K;
      const uint64_t msel = ballot64(sel);
      // v's own entries: one cursor step per chunk by lane 0
      uint32_t p0 = 0;
      if (lane == 0 && msel) p0 = atomicAdd(&cnt[v], (uint32_t)__popcll(msel));
      p0 = __shfl(p0, 0, 64);
      if (sel) {
        if (!FILL) {
          atomicAdd(&cnt[m], 1u);
        } else {
          const uint64_t pv = (uint64_t)p0 + mbcnt(msel);
          if (pv < vl) keys[vb + pv] = list_key(d, m);
          const uint32_t pos = atomicAdd(&cnt[m], 1u);
          const uint64_t ob = lists_off[m];
          if (ob + pos < lists_off[m + 1]) keys[ob + pos] = list_key(d, v);
        }
      }
      taken += (uint32_t)__popcll(mlow);
      if (mbad) break;
      last = __shfl(d, 63, 64);
    }
  }
}

uint32_t wave_grid(uint32_t n) { return std::max(1u, std::min((n + 3) / 4, 1u << 18)); }

}  // namespace

void count_recut(uint32_t n, Csr G, uint32_t K, uint32_t* cnt, hipStream_t s) {
  hipLaunchKernelGGL(k_recut<false>, dim3(wave_grid(n)), dim3(256), 0, s, n, G, K, cnt, (const uint64_t*)nullptr,
                     (uint64_t*)nullptr);
}
void fill_recut(uint32_t n, Csr G, uint32_t K, const uint64_t* lists_off, uint32_t* cur, uint64_t* keys,
                hipStream_t s) {
  hipLaunchKernelGGL(k_recut<true>, dim3(wave_grid(n)), dim3(256), 0, s, n, G, K, cur, lists_off, keys);
}

}  // namespace edges
}  // namespace ngt_amd
