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

#include <algorithm>

#include "../../include/ngt_amd.h"
#include "device_graph.h"
#include "index_internal.h"
#include "onng_kernels.h"

using namespace ngt_amd;
using namespace ngt_amd::onng;

namespace {

struct Run {
  OwnedStream st;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  DevMeter mem;  // every buffer of the run is charged here: stats.peak_device_bytes
  uint32_t n = 0;
  ~Run() {
    for (auto e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

// L[u] = base(u) + the reversed first `take` edges of S, sorted by (distance,
// id), repeats dropped (onng_kernels.h: count_lists).
int build_lists(Run& R, Csr S, uint32_t take, Csr B1, Csr B2, uint32_t o, uint32_t* d_err, DeviceGraph& out) {
  const uint32_t n = R.n;
  const hipStream_t s = R.st.s;
  DevBuf<uint32_t> cnt(&R.mem);
  DevBuf<uint64_t> loff(&R.mem), keys_a(&R.mem), keys_b(&R.mem);
  HIP_OK(cnt.alloc(n));
  HIP_OK(hipMemsetAsync(cnt.p, 0, (size_t)n * 4, s));
  count_lists(n, S, take, B1, B2, o, cnt.p, d_err, s);
  HIP_OK(loff.alloc((size_t)n + 1));
  scan_u32(cnt.p, n, loff.p, s);
  HIP_OK(hipGetLastError());
  uint64_t total = 0;
  if (fetch(s, &total, loff.p + n, 1)) return -1;
  uint32_t longest = 0;
  if (max_of(s, cnt.p, n, &longest)) return -1;
  HIP_OK(keys_a.alloc(total));
  HIP_OK(keys_b.alloc(total));
  HIP_OK(hipMemsetAsync(cnt.p, 0, (size_t)n * 4, s));
  fill_lists(n, S, take, B1, B2, o, loff.p, cnt.p, keys_a.p, s);
  return lists_from_keys(s, n, loff.p, keys_a, keys_b, longest, out);
}

int path_adjustment(Run& R, DeviceGraph& G, uint64_t min_edges, uint32_t* d_err, ngt_amd_onng_stats& st, DeviceGraph& out) {
  const uint32_t n = R.n;
  const hipStream_t s = R.st.s;
  const uint64_t E = G.edges;
  uint32_t err[kErrWords];
  HIP_OK(hipEventRecord(R.ev[1], s));
  // ---- phase A: count, scan, fill
  DevBuf<uint32_t> ccnt(&R.mem), hub(&R.mem);
  DevBuf<uint64_t> coff(&R.mem);
  DevBuf<uint2> cand(&R.mem);
  uint32_t hub_slots = 0;
  if (G.maxlen > kFastCap) {
    hub_slots = 2 * kFastCap;
    while ((uint64_t)hub_slots < 2 * (uint64_t)G.maxlen) hub_slots <<= 1;
    HIP_OK(hub.alloc((size_t)kHubBlocks * hub_slots * 2));
  }
  HIP_OK(ccnt.alloc(E));
  if (E) HIP_OK(hipMemsetAsync(ccnt.p, 0, E * 4, s));
  candidates(n, G.csr(), false, ccnt.p, nullptr, nullptr, hub.p, hub_slots, d_err, s);
  HIP_OK(hipGetLastError());
  if (fetch(s, err, d_err, kErrWords)) return -1;
  if (err[kErrOrder] != 0xffffffffu)
    return fail("ngt_amd_onng_reconstruct: path adjustment needs every list in (distance, id) order; the list of node %u is not",
                err[kErrOrder]);
  if (err[kErrRepeated] != 0xffffffffu)
    return fail("ngt_amd_onng_reconstruct: path adjustment needs lists without repeated ids; the list of node %u repeats an id",
                err[kErrRepeated]);
  if (err[kErrTable] != 0xffffffffu)
    return fail("ngt_amd_onng_reconstruct: internal error, hub table too small for node %u", err[kErrTable]);
  HIP_OK(coff.alloc(E + 1));
  scan_u32(ccnt.p, E, coff.p, s);
  uint64_t C = 0;
  if (fetch(s, &C, coff.p + E, 1)) return -1;
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
  HIP_OK(cand.alloc(C));
  if (E) HIP_OK(hipMemsetAsync(ccnt.p, 0, E * 4, s));
  candidates(n, G.csr(), true, ccnt.p, coff.p, cand.p, hub.p, hub_slots, d_err, s);
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(R.ev[2], s));
  ccnt.release();
  hub.release();
  // ---- phase B
  DevBuf<uint8_t> flag(&R.mem), dec(&R.mem);
  DevBuf<uint32_t> outcnt(&R.mem), alive(&R.mem), next_alive(&R.mem), work_a(&R.mem), work_b(&R.mem), counters(&R.mem);
  HIP_OK(flag.alloc(E));
  HIP_OK(dec.alloc(n));
  HIP_OK(outcnt.alloc(n));
  HIP_OK(alive.alloc(n));
  HIP_OK(next_alive.alloc(n));
  HIP_OK(work_a.alloc(n));
  HIP_OK(work_b.alloc(n));
  HIP_OK(counters.alloc(2));
  if (E) HIP_OK(hipMemsetAsync(flag.p, 0, E, s));
  HIP_OK(hipMemsetAsync(outcnt.p, 0, (size_t)n * 4, s));
  HIP_OK(hipMemsetAsync(counters.p, 0, 8, s));
  alive_init(n, G.off.p, alive.p, counters.p, s);
  uint32_t hc[2] = {0, 0};
  if (fetch(s, hc, counters.p, 2)) return -1;
  uint32_t nalive = hc[1];
  for (uint32_t r = 0; nalive > 0; r++) {
    HIP_OK(hipMemsetAsync(counters.p, 0, 8, s));
    const uint32_t* work = alive.p;
    uint32_t nwork = nalive, passes = 0;
    uint32_t* next_work = work_a.p;
    while (nwork > 0) {
      if (passes) HIP_OK(hipMemsetAsync(counters.p, 0, 4, s));
      decide(work, nwork, r, G.csr(), coff.p, cand.p, flag.p, outcnt.p, min_edges, dec.p, s);
      commit(work, nwork, r, G.off.p, dec.p, flag.p, outcnt.p, next_work, next_alive.p, counters.p, s);
      HIP_OK(hipGetLastError());
      if (fetch(s, hc, counters.p, 2)) return -1;
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
  HIP_OK(out.off.alloc((size_t)n + 1));
  scan_u32(outcnt.p, n, out.off.p, s);
  if (fetch(s, &out.edges, out.off.p + n, 1)) return -1;
  HIP_OK(out.ids.alloc(out.edges));
  HIP_OK(out.d.alloc(out.edges));
  emit_kept(n, G.csr(), flag.p, out.off.p, out.ids.p, out.d.p, s);
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(R.ev[3], s));
  HIP_OK(hipStreamSynchronize(s));
  return 0;
}

thread_local HostGraph t_graph;
thread_local ngt_amd_onng_stats t_stats;

int run(int device, const uint64_t* offsets, const uint32_t* ids, const float* dists, uint64_t nrows,
        const ngt_amd_onng_params& p, HostGraph& res, ngt_amd_onng_stats& stats) {
  res.ready = false;
  stats = ngt_amd_onng_stats{};
  uint32_t longest = 0;
  if (check_csr("ngt_amd_onng_reconstruct", offsets, ids, dists, nrows, false, &longest)) return -1;
  if (p.outgoing < 0 || p.incoming < 0) return fail("ngt_amd_onng_reconstruct: outgoing and incoming must not be negative");
  // reconstructGraph refuses this (GraphReconstructor.h:428-431)
  if (p.incoming > 10000) return fail("ngt_amd_onng_reconstruct: something wrong. Edge size=%d", p.incoming);
  if (select_device("ngt_amd_onng_reconstruct", device)) return -1;

  Run R;
  R.n = (uint32_t)nrows;
  if (R.st.create()) return -1;
  for (auto& e : R.ev) HIP_OK(hipEventCreate(&e));
  const uint32_t n = R.n;
  const hipStream_t s = R.st.s;
  const bool edge = p.outgoing > 0 || p.incoming > 0;

  DeviceGraph in(&R.mem), cur(&R.mem);
  if (upload_graph(s, n, offsets, ids, dists, in)) return -1;
  in.maxlen = longest;
  // the order word check_lists leaves in d_err is path adjustment's when no edge stage runs
  DevBuf<uint32_t> d_err(&R.mem);
  if (verify_lists("ngt_amd_onng_reconstruct", s, n, in, false, d_err)) return -1;

  HIP_OK(hipEventRecord(R.ev[0], s));
  if (edge) {
    // sorted lists come out of this stage whatever went in
    HIP_OK(hipMemsetAsync(d_err.p, 0xff, kErrWords * 4, s));
    DeviceGraph conv(&R.mem);
    if (!p.input_is_anng) {
      if (build_lists(R, in.csr(), 0xffffffffu, in.csr(), in.csr(), 0xffffffffu, d_err.p, conv)) return -1;
    }
    const Csr graph = p.input_is_anng ? in.csr() : conv.csr();
    if (build_lists(R, graph, (uint32_t)p.incoming, graph, in.csr(), (uint32_t)p.outgoing, d_err.p, cur)) return -1;
  }
  DeviceGraph& tmp = edge ? cur : in;
  DeviceGraph fin(&R.mem);
  if (p.path_adjustment) {
    if (path_adjustment(R, tmp, p.min_edges, d_err.p, stats, fin)) return -1;
  } else {
    HIP_OK(hipEventRecord(R.ev[1], s));
  }
  if (download_graph(s, n, p.path_adjustment ? fin : tmp, res)) return -1;
  float ms = 0.f;
  HIP_OK(hipEventElapsedTime(&ms, R.ev[0], R.ev[1]));
  stats.edge_ms = ms;
  if (p.path_adjustment) {
    HIP_OK(hipEventElapsedTime(&ms, R.ev[1], R.ev[2]));
    stats.phase_a_ms = ms;
    HIP_OK(hipEventElapsedTime(&ms, R.ev[2], R.ev[3]));
    stats.phase_b_ms = ms;
  }
  stats.peak_device_bytes = R.mem.peak;
  res.ready = true;
  return 0;
}

}  // namespace

extern "C" uint32_t ngt_amd_onng_fast_path_capacity(void) { return kFastCap; }

extern "C" int ngt_amd_onng_reconstruct(int device, const uint64_t* offsets, const uint32_t* ids, const float* dists,
                                        uint64_t nrows, const ngt_amd_onng_params* params, uint64_t* out_nedges) {
  if (!offsets || !params || !out_nedges) return fail("ngt_amd_onng_reconstruct: bad arguments");
  *out_nedges = 0;
  if (run(device, offsets, ids, dists, nrows, *params, t_graph, t_stats)) {
    t_graph = HostGraph();
    return -1;
  }
  *out_nedges = t_graph.ids.size();
  return 0;
}

extern "C" int ngt_amd_onng_get_graph(uint64_t* offsets, uint32_t* ids, float* dists) {
  return copy_out(t_graph, "ngt_amd_onng_get_graph", "reconstructed", offsets, ids, dists);
}

extern "C" int ngt_amd_onng_last_stats(ngt_amd_onng_stats* stats) {
  if (!stats) return fail("ngt_amd_onng_last_stats: bad arguments");
  if (!t_graph.ready) return fail("ngt_amd_onng_last_stats: no reconstructed graph on this thread");
  *stats = t_stats;
  return 0;
}
