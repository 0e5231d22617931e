// onng.cpp -- host side of ngt_amd_onng_*: the graph stages of
// GraphOptimizer::execute (lib/NGT/GraphOptimizer.h:230-296) on the device.
//
//   conversion       convertToANNG (GraphReconstructor.h:389-423), when the
//                    input is not an ANNG
//   edge adjustment  reconstructGraph(graph, out, o, i) (:425-561)
//   path adjustment  adjustPathsEffectively(out, minE) (:197-386)
//
// The first two build lists by count, scan and scatter and then sort and
// dedupe each list (onng_kernels.hip).  Path adjustment is restated as a rule
// on the lists tmp before the stage (each in (distance, id) order, no id
// twice): at rank r, nodes in ascending id, v drops its edge (dst, dd) =
// tmp[v][r] iff |out[v]| + |tmp[v]| - r > minE and some p in tmp[v] with
// d(v,p) < dd has dst in tmp[p] with d(p,dst) < dd while p is in out[v] and dst
// is in out[p] *at that moment* -- out[p] holds p's rank-r decision only when
// p < v.  Phase A extracts every such (v, dst, p) once; phase B walks the
// ranks, and within a rank relaunches the decision kernel until the chains of
// same-rank references to lower ids are resolved.  The lowest undecided id
// never waits, so every launch decides something; a launch that does not is an
// error, never a hang.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/ngt_amd.h"
#include "index_internal.h"
#include "onng_kernels.h"

using namespace ngt_amd;
using namespace ngt_amd::onng;

namespace {

struct Tracker {
  size_t cur = 0, peak = 0;
};

template <typename T>
struct Buf {
  T* p = nullptr;
  size_t n = 0;
  Tracker* t = nullptr;
  Buf() {}
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() { release(); }
  void release() {
    if (p) {
      (void)hipFree(p);
      t->cur -= std::max<size_t>(n, 1) * sizeof(T);
    }
    p = nullptr;
    n = 0;
  }
  hipError_t alloc(Tracker& tr, size_t count) {
    release();
    t = &tr;
    hipError_t e = hipMalloc((void**)&p, std::max<size_t>(count, 1) * sizeof(T));
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    n = count;
    tr.cur += std::max<size_t>(n, 1) * sizeof(T);
    tr.peak = std::max(tr.peak, tr.cur);
    return hipSuccess;
  }
  void swap(Buf& o) {
    std::swap(p, o.p);
    std::swap(n, o.n);
    std::swap(t, o.t);
  }
};

struct DevGraph {
  Buf<uint64_t> off;
  Buf<uint32_t> ids;
  Buf<float> d;
  uint64_t edges = 0;
  uint32_t maxlen = 0;
  Csr csr() const { return Csr{off.p, ids.p, d.p}; }
  void swap(DevGraph& o) {
    off.swap(o.off);
    ids.swap(o.ids);
    d.swap(o.d);
    std::swap(edges, o.edges);
    std::swap(maxlen, o.maxlen);
  }
};

struct Run {
  hipStream_t s = nullptr;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  Tracker mem;
  uint32_t n = 0;
  ~Run() {
    for (auto e : ev)
      if (e) (void)hipEventDestroy(e);
    if (s) (void)hipStreamDestroy(s);
  }
};

template <typename T>
int fetch(Run& R, T* host, const T* dev, size_t count) {
  HIP_OK(hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, R.s));
  HIP_OK(hipStreamSynchronize(R.s));
  return 0;
}

int max_of(Run& R, const uint32_t* dev, uint32_t n, uint32_t* out) {
  std::vector<uint32_t> h(n);
  if (fetch(R, h.data(), dev, n)) return -1;
  *out = 0;
  for (uint32_t x : h) *out = std::max(*out, x);
  return 0;
}

// L[u] = base(u) + the reversed first `take` edges of S, sorted by (distance,
// id), repeats dropped (onng_kernels.h: count_lists).
int build_lists(Run& R, Csr S, uint32_t take, Csr B1, Csr B2, uint32_t o, uint32_t* d_err, DevGraph& out) {
  const uint32_t n = R.n;
  Buf<uint32_t> cnt, cnt2;
  Buf<uint64_t> loff, keys_a, keys_b;
  HIP_OK(cnt.alloc(R.mem, n));
  HIP_OK(hipMemsetAsync(cnt.p, 0, (size_t)n * 4, R.s));
  count_lists(n, S, take, B1, B2, o, cnt.p, d_err, R.s);
  HIP_OK(loff.alloc(R.mem, (size_t)n + 1));
  scan_u32(cnt.p, n, loff.p, R.s);
  HIP_OK(hipGetLastError());
  uint64_t total = 0;
  if (fetch(R, &total, loff.p + n, 1)) return -1;
  uint32_t longest = 0;
  if (max_of(R, cnt.p, n, &longest)) return -1;
  HIP_OK(keys_a.alloc(R.mem, total));
  HIP_OK(keys_b.alloc(R.mem, total));
  HIP_OK(hipMemsetAsync(cnt.p, 0, (size_t)n * 4, R.s));
  fill_lists(n, S, take, B1, B2, o, loff.p, cnt.p, keys_a.p, R.s);
  sort_lists(n, loff.p, keys_a.p, keys_b.p, longest > kFastCap, R.s);
  HIP_OK(cnt2.alloc(R.mem, n));
  HIP_OK(hipMemsetAsync(cnt2.p, 0, (size_t)n * 4, R.s));
  unique_lists(n, loff.p, keys_b.p, keys_a.p, cnt2.p, R.s);
  keys_b.release();
  HIP_OK(out.off.alloc(R.mem, (size_t)n + 1));
  scan_u32(cnt2.p, n, out.off.p, R.s);
  HIP_OK(hipGetLastError());
  if (fetch(R, &out.edges, out.off.p + n, 1)) return -1;
  if (max_of(R, cnt2.p, n, &out.maxlen)) return -1;
  HIP_OK(out.ids.alloc(R.mem, out.edges));
  HIP_OK(out.d.alloc(R.mem, out.edges));
  unpack_lists(n, loff.p, keys_a.p, out.off.p, out.ids.p, out.d.p, R.s);
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(R.s));
  return 0;
}

int path_adjustment(Run& R, DevGraph& G, uint64_t min_edges, uint32_t* d_err, ngt_amd_onng_stats& st, DevGraph& out) {
  const uint32_t n = R.n;
  const uint64_t E = G.edges;
  uint32_t err[kErrWords];
  HIP_OK(hipEventRecord(R.ev[1], R.s));
  // ---- phase A: count, scan, fill
  Buf<uint32_t> ccnt, hub;
  Buf<uint64_t> coff;
  Buf<uint2> cand;
  uint32_t hub_slots = 0;
  if (G.maxlen > kFastCap) {
    hub_slots = 2 * kFastCap;
    while ((uint64_t)hub_slots < 2 * (uint64_t)G.maxlen) hub_slots <<= 1;
    HIP_OK(hub.alloc(R.mem, (size_t)kHubBlocks * hub_slots * 2));
  }
  HIP_OK(ccnt.alloc(R.mem, E));
  if (E) HIP_OK(hipMemsetAsync(ccnt.p, 0, E * 4, R.s));
  candidates(n, G.csr(), false, ccnt.p, nullptr, nullptr, hub.p, hub_slots, d_err, R.s);
  HIP_OK(hipGetLastError());
  if (fetch(R, err, d_err, kErrWords)) return -1;
  if (err[kErrOrder] != 0xffffffffu)
    return fail("ngt_amd_onng_reconstruct: path adjustment needs every list in (distance, id) order; the list of node %u is not",
                err[kErrOrder]);
  if (err[kErrRepeated] != 0xffffffffu)
    return fail("ngt_amd_onng_reconstruct: path adjustment needs lists without repeated ids; the list of node %u repeats an id",
                err[kErrRepeated]);
  if (err[kErrTable] != 0xffffffffu)
    return fail("ngt_amd_onng_reconstruct: internal error, hub table too small for node %u", err[kErrTable]);
  HIP_OK(coff.alloc(R.mem, E + 1));
  scan_u32(ccnt.p, E, coff.p, R.s);
  uint64_t C = 0;
  if (fetch(R, &C, coff.p + E, 1)) return -1;
  st.candidates = C;
  {
    // the candidates of all nodes are resident through phase B; they may take
    // at most half of the free memory
    size_t free_b = 0, total_b = 0;
    HIP_OK(hipMemGetInfo(&free_b, &total_b));
    if (C * sizeof(uint2) > free_b / 2)
      return fail("ngt_amd_onng_reconstruct: %llu path candidates (%llu bytes) exceed half of the free device memory (%llu bytes)",
                  (unsigned long long)C, (unsigned long long)(C * sizeof(uint2)), (unsigned long long)free_b);
  }
  HIP_OK(cand.alloc(R.mem, C));
  if (E) HIP_OK(hipMemsetAsync(ccnt.p, 0, E * 4, R.s));
  candidates(n, G.csr(), true, ccnt.p, coff.p, cand.p, hub.p, hub_slots, d_err, R.s);
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(R.ev[2], R.s));
  ccnt.release();
  hub.release();
  // ---- phase B
  Buf<uint8_t> flag, dec;
  Buf<uint32_t> outcnt, alive, next_alive, work_a, work_b, counters;
  HIP_OK(flag.alloc(R.mem, E));
  HIP_OK(dec.alloc(R.mem, n));
  HIP_OK(outcnt.alloc(R.mem, n));
  HIP_OK(alive.alloc(R.mem, n));
  HIP_OK(next_alive.alloc(R.mem, n));
  HIP_OK(work_a.alloc(R.mem, n));
  HIP_OK(work_b.alloc(R.mem, n));
  HIP_OK(counters.alloc(R.mem, 2));
  if (E) HIP_OK(hipMemsetAsync(flag.p, 0, E, R.s));
  HIP_OK(hipMemsetAsync(outcnt.p, 0, (size_t)n * 4, R.s));
  HIP_OK(hipMemsetAsync(counters.p, 0, 8, R.s));
  alive_init(n, G.off.p, alive.p, counters.p, R.s);
  uint32_t hc[2] = {0, 0};
  if (fetch(R, hc, counters.p, 2)) return -1;
  uint32_t nalive = hc[1];
  for (uint32_t r = 0; nalive > 0; r++) {
    HIP_OK(hipMemsetAsync(counters.p, 0, 8, R.s));
    const uint32_t* work = alive.p;
    uint32_t nwork = nalive, passes = 0;
    uint32_t* next_work = work_a.p;
    while (nwork > 0) {
      if (passes) HIP_OK(hipMemsetAsync(counters.p, 0, 4, R.s));
      decide(work, nwork, r, G.csr(), coff.p, cand.p, flag.p, outcnt.p, min_edges, dec.p, R.s);
      commit(work, nwork, r, G.off.p, dec.p, flag.p, outcnt.p, next_work, next_alive.p, counters.p, R.s);
      HIP_OK(hipGetLastError());
      if (fetch(R, hc, counters.p, 2)) return -1;
      passes++;
      st.phase_b_launches += 2;
      // the lowest undecided id waits for nobody
      if (hc[0] >= nwork || passes > nalive)
        return fail("ngt_amd_onng_reconstruct: path adjustment made no progress at rank %u (%u nodes undecided)", r, hc[0]);
      nwork = hc[0];
      work = next_work;
      next_work = next_work == work_a.p ? work_b.p : work_a.p;
    }
    st.max_passes_per_rank = std::max(st.max_passes_per_rank, passes);
    st.ranks = r + 1;
    alive.swap(next_alive);
    nalive = hc[1];
  }
  // ---- the kept edges, still in (distance, id) order
  HIP_OK(out.off.alloc(R.mem, (size_t)n + 1));
  scan_u32(outcnt.p, n, out.off.p, R.s);
  if (fetch(R, &out.edges, out.off.p + n, 1)) return -1;
  HIP_OK(out.ids.alloc(R.mem, out.edges));
  HIP_OK(out.d.alloc(R.mem, out.edges));
  emit_kept(n, G.csr(), flag.p, out.off.p, out.ids.p, out.d.p, R.s);
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(R.ev[3], R.s));
  HIP_OK(hipStreamSynchronize(R.s));
  return 0;
}

struct Result {
  std::vector<uint64_t> off;
  std::vector<uint32_t> ids;
  std::vector<float> d;
  ngt_amd_onng_stats stats{};
  bool ready = false;
};
thread_local Result t_result;

int run(int device, const uint64_t* offsets, const uint32_t* ids, const float* dists, uint64_t nrows,
        const ngt_amd_onng_params& p, Result& res) {
  res.ready = false;
  res.stats = ngt_amd_onng_stats{};
  if (nrows == 0 || nrows >= (1ull << 31)) return fail("ngt_amd_onng_reconstruct: %llu rows are not supported", (unsigned long long)nrows);
  if (p.outgoing < 0 || p.incoming < 0) return fail("ngt_amd_onng_reconstruct: outgoing and incoming must not be negative");
  // reconstructGraph refuses this (GraphReconstructor.h:428-431)
  if (p.incoming > 10000) return fail("ngt_amd_onng_reconstruct: something wrong. Edge size=%d", p.incoming);
  if (offsets[0] != 0) return fail("ngt_amd_onng_reconstruct: offsets[0] is not 0");
  uint32_t longest = 0;
  for (uint64_t v = 0; v < nrows; v++) {
    if (offsets[v + 1] < offsets[v]) return fail("ngt_amd_onng_reconstruct: offsets decrease at node %llu", (unsigned long long)v);
    if (offsets[v + 1] - offsets[v] >= (1ull << 31)) return fail("ngt_amd_onng_reconstruct: the list of node %llu is too long", (unsigned long long)v);
    longest = std::max(longest, (uint32_t)(offsets[v + 1] - offsets[v]));
  }
  const uint64_t E = offsets[nrows];
  if (E && (!ids || !dists)) return fail("ngt_amd_onng_reconstruct: ids or dists is null");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail("ngt_amd_onng_reconstruct: no HIP device available (the MI355X path has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail("ngt_amd_onng_reconstruct: device %d out of range", device);
  HIP_OK(hipSetDevice(device));

  Run R;
  R.n = (uint32_t)nrows;
  HIP_OK(hipStreamCreateWithFlags(&R.s, hipStreamDefault));
  for (auto& e : R.ev) HIP_OK(hipEventCreate(&e));
  const uint32_t n = R.n;
  const bool edge = p.outgoing > 0 || p.incoming > 0;

  DevGraph in, cur;
  Buf<uint32_t> d_err;
  HIP_OK(in.off.alloc(R.mem, (size_t)n + 1));
  HIP_OK(in.ids.alloc(R.mem, E));
  HIP_OK(in.d.alloc(R.mem, E));
  HIP_OK(d_err.alloc(R.mem, kErrWords));
  HIP_OK(hipMemcpyAsync(in.off.p, offsets, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, R.s));
  if (E) HIP_OK(hipMemcpyAsync(in.ids.p, ids, E * 4, hipMemcpyHostToDevice, R.s));
  if (E) HIP_OK(hipMemcpyAsync(in.d.p, dists, E * 4, hipMemcpyHostToDevice, R.s));
  HIP_OK(hipMemsetAsync(d_err.p, 0xff, kErrWords * 4, R.s));
  in.edges = E;
  in.maxlen = longest;
  check_lists(n, in.csr(), d_err.p, R.s);
  HIP_OK(hipGetLastError());
  uint32_t err[kErrWords];
  if (fetch(R, err, d_err.p, kErrWords)) return -1;
  if (err[kErrBadId] != 0xffffffffu)
    return fail("ngt_amd_onng_reconstruct: the list of node %u holds an id outside [1, %u)", err[kErrBadId], n);

  HIP_OK(hipEventRecord(R.ev[0], R.s));
  if (edge) {
    // sorted lists come out of this stage whatever went in
    HIP_OK(hipMemsetAsync(d_err.p, 0xff, kErrWords * 4, R.s));
    DevGraph conv;
    if (!p.input_is_anng) {
      if (build_lists(R, in.csr(), 0xffffffffu, in.csr(), in.csr(), 0xffffffffu, d_err.p, conv)) return -1;
    }
    const Csr graph = p.input_is_anng ? in.csr() : conv.csr();
    if (build_lists(R, graph, (uint32_t)p.incoming, graph, in.csr(), (uint32_t)p.outgoing, d_err.p, cur)) return -1;
  }
  DevGraph& tmp = edge ? cur : in;
  DevGraph fin;
  if (p.path_adjustment) {
    if (path_adjustment(R, tmp, p.min_edges, d_err.p, res.stats, fin)) return -1;
  } else {
    HIP_OK(hipEventRecord(R.ev[1], R.s));
  }
  DevGraph& last = p.path_adjustment ? fin : tmp;
  res.off.resize((size_t)n + 1);
  res.ids.resize(last.edges);
  res.d.resize(last.edges);
  HIP_OK(hipMemcpyAsync(res.off.data(), last.off.p, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, R.s));
  if (last.edges) HIP_OK(hipMemcpyAsync(res.ids.data(), last.ids.p, last.edges * 4, hipMemcpyDeviceToHost, R.s));
  if (last.edges) HIP_OK(hipMemcpyAsync(res.d.data(), last.d.p, last.edges * 4, hipMemcpyDeviceToHost, R.s));
  HIP_OK(hipStreamSynchronize(R.s));
  float ms = 0.f;
  HIP_OK(hipEventElapsedTime(&ms, R.ev[0], R.ev[1]));
  res.stats.edge_ms = ms;
  if (p.path_adjustment) {
    HIP_OK(hipEventElapsedTime(&ms, R.ev[1], R.ev[2]));
    res.stats.phase_a_ms = ms;
    HIP_OK(hipEventElapsedTime(&ms, R.ev[2], R.ev[3]));
    res.stats.phase_b_ms = ms;
  }
  res.stats.peak_device_bytes = R.mem.peak;
  res.ready = true;
  return 0;
}

}  // namespace

extern "C" uint32_t ngt_amd_onng_fast_path_capacity(void) { return kFastCap; }

extern "C" int ngt_amd_onng_reconstruct(int device, const uint64_t* offsets, const uint32_t* ids, const float* dists,
                                        uint64_t nrows, const ngt_amd_onng_params* params, uint64_t* out_nedges) {
  if (!offsets || !params || !out_nedges) return fail("ngt_amd_onng_reconstruct: bad arguments");
  *out_nedges = 0;
  if (run(device, offsets, ids, dists, nrows, *params, t_result)) {
    t_result = Result();
    return -1;
  }
  *out_nedges = t_result.ids.size();
  return 0;
}

extern "C" int ngt_amd_onng_get_graph(uint64_t* offsets, uint32_t* ids, float* dists) {
  if (!t_result.ready) return fail("ngt_amd_onng_get_graph: no reconstructed graph on this thread");
  if (!offsets) return fail("ngt_amd_onng_get_graph: bad arguments");
  memcpy(offsets, t_result.off.data(), t_result.off.size() * 8);
  if (ids && !t_result.ids.empty()) memcpy(ids, t_result.ids.data(), t_result.ids.size() * 4);
  if (dists && !t_result.d.empty()) memcpy(dists, t_result.d.data(), t_result.d.size() * 4);
  return 0;
}

extern "C" int ngt_amd_onng_last_stats(ngt_amd_onng_stats* stats) {
  if (!stats) return fail("ngt_amd_onng_last_stats: bad arguments");
  if (!t_result.ready) return fail("ngt_amd_onng_last_stats: no reconstructed graph on this thread");
  *stats = t_result.stats;
  return 0;
}
