// edges_api.cpp -- ngt_amd_recut_anng and ngt_amd_optimize_edges: the
// edge-count optimisation of edge_optimizer.cpp with its work on the device.
// Constructions run in a build session (build.cpp); a sample's graph is
// uploaded once, every edge count is cut from it in HBM (edges_kernels.hip,
// then the sort / dedupe / unpack kernels of onng_kernels.hip) and handed to
// the search as a device CSR; every batch is one ngt_amd_search with tree seeds.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <exception>
#include <map>
#include <string>
#include <vector>

#include "../../include/ngt_amd.h"
#include "device_graph.h"
#include "edge_optimizer.h"
#include "edges_kernels.h"
#include "index_internal.h"
#include "index_io.h"
#include "onng_kernels.h"

using namespace ngt_amd;
using onng::Csr;

namespace {

// reconstructANNGFromANNG(G, K) -> out: count, scan, fill, then per list sort,
// dedupe and unpack
int recut_device(hipStream_t s, uint32_t n, Csr G, uint32_t K, DeviceGraph& out) {
  DevBuf<uint32_t> cnt;
  DevBuf<uint64_t> loff, keys_a, keys_b;
  HIP_OK(cnt.alloc(n));
  HIP_OK(hipMemsetAsync(cnt.p, 0, (size_t)n * 4, s));
  edges::count_recut(n, G, K, cnt.p, s);
  HIP_OK(loff.alloc((size_t)n + 1));
  onng::scan_u32(cnt.p, n, loff.p, s);
  HIP_OK(hipGetLastError());
  uint64_t total = 0;
  if (fetch(s, &total, loff.p + n, 1)) return -1;
  uint32_t longest = 0;
  if (max_of(s, cnt.p, n, &longest)) return -1;
  HIP_OK(keys_a.alloc(total));
  HIP_OK(keys_b.alloc(total));
  HIP_OK(hipMemsetAsync(cnt.p, 0, (size_t)n * 4, s));
  edges::fill_recut(n, G, K, loff.p, cnt.p, keys_a.p, s);
  return lists_from_keys(s, n, loff.p, keys_a, keys_b, longest, out);
}

thread_local HostGraph t_graph;
thread_local std::vector<ngt_amd_edge_sample> t_trace;  // the samples of the thread's last optimisation

int recut_host_graph(int device, const uint64_t* offsets, const uint32_t* ids, const float* dists, uint64_t nrows,
                     uint32_t K, HostGraph& res) {
  res.ready = false;
  uint32_t longest = 0;
  if (check_csr("ngt_amd_recut_anng", offsets, ids, dists, nrows, false, &longest)) return -1;
  if (K == 0) return fail("ngt_amd_recut_anng: K must be positive");
  if (select_device("ngt_amd_recut_anng", device)) return -1;
  OwnedStream st;
  if (st.create()) return -1;
  const uint32_t n = (uint32_t)nrows;
  DeviceGraph in, out;
  if (upload_graph(st.s, n, offsets, ids, dists, in)) return -1;
  DevBuf<uint32_t> err;
  if (verify_lists("ngt_amd_recut_anng", st.s, n, in, false, err)) return -1;
  if (recut_device(st.s, n, in.csr(), K, out)) return -1;
  if (download_graph(st.s, n, out, res)) return -1;
  res.ready = true;
  return 0;
}

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

struct Optimizer {
  ngt_amd_index* ix;
  ngt_amd_build_params bp;
  OwnedStream st;
  GlibcRandHost rnd;
  // the last sample's state on the host: the graph the next construction starts
  // from (after a sample: its last re-cut), the nodes it holds, its tree
  HostGraph h;
  std::vector<uint8_t> node;
  uint64_t graph_rows = 0;
  bool have_prev = false, cut_since_build = false;
  HostTree tree;
  DeviceGraph src, cur;  // the sample's graph; the re-cut the index searches
  std::vector<double> build_ms, recut_ms, search_ms;

  ~Optimizer() {
    // an index that still reads the last re-cut takes its buffers over
    if (cur.off.p && ix->edge_off.p == cur.off.p && ix->edges.p == cur.ids.p) {
      ix->edge_off.take_from(cur.off);
      ix->edges.take_from(cur.ids);
    }
  }

  // createIndex(threads, end_id) into the graph and tree the sample before left
  int build(uint64_t end_id) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t n = (uint32_t)ix->nrows;
    if (cut_since_build) {  // the previous sample's last re-cut is the graph now
      if (download_graph(st.s, n, cur, h)) return -1;
      cut_since_build = false;
    }
    if (ngt_amd_build_begin(ix, &bp)) return -1;
    build_rand(ix) = rnd;  // the stream goes on where the query draw left it
    if (have_prev) {
      if (ngt_amd_build_set_graph(ix, h.off.data(), h.ids.data(), h.d.data(), graph_rows)) return -1;
      // a node whose re-cut list came out empty is still a node: not inserted again
      build_mark_nodes(ix, node, graph_rows);
      if (build_tree_from_host(ix, tree, (uint32_t)tree.in_parent.size(), tree.root)) return -1;
    }
    if (ngt_amd_build_insert(ix, 1, end_id)) return -1;
    rnd = build_rand(ix);
    uint64_t ne = 0;
    if (ngt_amd_build_graph_size(ix, &graph_rows, &ne)) return -1;
    if (build_graph_to_host(ix, n, h.off, h.ids, h.d)) return -1;
    node = build_nodes(ix);
    if (build_tree_to_host(ix, ix->row_bytes, tree)) return -1;
    tree.root = build_root(ix);
    have_prev = true;
    // the pseudo ground truth searches the sample's whole graph
    if (ngt_amd_index_set_graph(ix, h.off.data(), h.ids.data(), ne)) return -1;
    if (ngt_amd_index_set_tree(ix, tree.in_pivot.data(), (uint32_t)tree.in_parent.size(), tree.in_child.data(),
                               tree.in_border.data(), 5, tree.root, tree.leaf_off.data(),
                               (uint32_t)tree.leaf_parent.size(), tree.leaf_ids.data(), tree.leaf_ids.size()))
      return -1;
    build_ms.push_back(ms_since(t0));
    recut_ms.push_back(0.0);
    search_ms.push_back(0.0);
    return 0;
  }

  int extract() {
    const auto t0 = std::chrono::steady_clock::now();
    if (upload_graph(st.s, (uint32_t)ix->nrows, h.off.data(), h.ids.data(), h.d.data(), src)) return -1;
    HIP_OK(hipStreamSynchronize(st.s));
    recut_ms.back() += ms_since(t0);
    return 0;
  }

  int recut(size_t K) {
    const auto t0 = std::chrono::steady_clock::now();
    DeviceGraph next;
    if (recut_device(st.s, (uint32_t)ix->nrows, src.csr(), (uint32_t)std::min<size_t>(K, 0xffffffffu), next)) return -1;
    if (ngt_amd_index_set_graph_device(ix, next.off.p, next.ids.p, next.edges)) return -1;
    cur.swap(next);  // the index reads `cur` from here on; the one before is freed
    cut_since_build = true;
    recut_ms.back() += ms_since(t0);
    return 0;
  }
};

int optimize_edges(ngt_amd_index* ix, const ngt_amd_edge_params* prm, uint64_t* edge, float* accuracy,
                   ngt_amd_edge_sample* samples, uint32_t* nsamples) {
  if (!ix || !prm || !edge || !accuracy) return fail("ngt_amd_optimize_edges: bad arguments");
  const uint32_t capacity = samples && nsamples ? *nsamples : 0;
  if (nsamples) *nsamples = 0;
  t_trace.clear();
  *edge = 0;
  *accuracy = 0.0f;
  if (ix->nrows < 2 || !ix->rows.p) return fail("ngt_amd_optimize_edges: the index has no objects");
  if (ix->nrows >= (1ull << 31)) return fail("ngt_amd_optimize_edges: %llu rows are not supported", (unsigned long long)ix->nrows);
  if (prm->max_no_of_edges > 10000 || prm->max_no_of_edges > (uint64_t)INT32_MAX)
    return fail("ngt_amd_optimize_edges: max_no_of_edges %llu is not supported", (unsigned long long)prm->max_no_of_edges);
  if (prm->no_of_results > ix->nrows)
    return fail("ngt_amd_optimize_edges: %llu results asked of a repository of %llu slots",
                (unsigned long long)prm->no_of_results, (unsigned long long)ix->nrows);
  HIP_OK(hipSetDevice(ix->device));

  EdgeParams P;
  P.nqueries = prm->no_of_queries;
  P.nresults = prm->no_of_results;
  P.nthreads = prm->no_of_threads;
  P.target_accuracy = prm->target_accuracy;
  P.target_objects = prm->target_no_of_objects;
  P.sample_objects = prm->no_of_sample_objects;
  P.max_edges = prm->max_no_of_edges;

  Optimizer o;
  o.ix = ix;
  o.bp = prm->build;
  o.bp.edge_size_for_creation = (int32_t)std::max<uint64_t>(P.max_edges, 1);
  if (o.st.create()) return -1;
  o.rnd.seed(1);  // a fresh process's rand() stream

  // ---- extractAndRemoveRandomQueries
  std::map<uint64_t, std::vector<uint8_t>> fetched;
  bool copy_failed = false;
  auto row = [&](uint64_t id) -> const void* {
    std::vector<uint8_t>& r = fetched[id];
    if (r.empty()) {
      r.resize(ix->row_bytes);
      if (hipMemcpy(r.data(), ix->rows.p + id * ix->row_bytes, ix->row_bytes, hipMemcpyDeviceToHost) != hipSuccess)
        copy_failed = true;
    }
    return r.data();
  };
  std::vector<uint8_t> valid = ix->h_valid;
  std::vector<float> queries;
  size_t draws = 0;
  std::string e = edge_draw_queries([&] { return o.rnd.next(); }, row, valid, ix->nrows, ix->dim, ix->otype,
                                    P.nqueries, queries, &draws);
  if (copy_failed) return fail("ngt_amd_optimize_edges: reading the stored objects failed");
  if (!e.empty()) return fail("%s", e.c_str());
  {
    ServeHold serve_hold(ix);
    ix->h_valid = valid;
    HIP_OK(ix->valid.upload(ix->h_valid.data(), ix->nrows));
    ix->rows_version++;
  }

  std::vector<uint64_t> cnt;
  EdgeCallbacks cb;
  cb.build = [&](uint64_t end_id) -> std::string { return o.build(end_id) ? ngt_amd_last_error() : ""; };
  cb.extract = [&]() -> std::string { return o.extract() ? ngt_amd_last_error() : ""; };
  cb.recut = [&](size_t K) -> std::string { return o.recut(K) ? ngt_amd_last_error() : ""; };
  cb.search = [&](AccuracyBatch& b) -> std::string {
    const auto t0 = std::chrono::steady_clock::now();
    const ngt_amd_search_params p = library_search_params(ix->nrows, (uint32_t)b.size, b.epsilon, -1.0f /* FLT_MAX */,
                                                          b.edge_size, NGT_AMD_SEED_TREE);
    cnt.assign((size_t)b.nq * NGT_AMD_COUNTERS_PER_QUERY, 0);
    if (ngt_amd_search(ix, &p, b.queries, b.nq, nullptr, nullptr, b.ids.data(), b.dists.data(), b.n.data(),
                       cnt.data()))
      return ngt_amd_last_error();
    for (uint32_t q = 0; q < b.nq; q++) b.counts[q] = cnt[(size_t)q * NGT_AMD_COUNTERS_PER_QUERY];
    if (!o.search_ms.empty()) o.search_ms.back() += ms_since(t0);
    return "";
  };

  size_t est = 0;
  float acc = 0.0f;
  EdgeTrace trace;
  trace.draws = draws;
  e = edge_optimize(cb, valid, ix->nrows, ix->dim, ix->otype, queries, P, kAccuracyWorkGuard, est, acc, &trace);
  t_trace.clear();
  for (size_t i = 0; i < trace.samples.size(); i++) {
    const EdgeSample& s = trace.samples[i];
    ngt_amd_edge_sample d;
    memset(&d, 0, sizeof d);
    d.objects = s.objects;
    d.edge = s.edge;
    d.accuracy = s.accuracy;
    d.gain = s.gain;
    d.max_epsilon = s.max_epsilon;
    d.guard_fired = s.guard_fired ? 1 : 0;
    d.nsteps = (uint32_t)s.steps.size();
    for (size_t j = 0; j < s.steps.size() && j < NGT_AMD_EDGE_STEPS; j++) {
      d.step_edge[j] = s.steps[j].edge;
      d.step_accuracy[j] = s.steps[j].accuracy;
    }
    if (i < o.build_ms.size()) {
      d.build_ms = o.build_ms[i];
      d.recut_ms = o.recut_ms[i];
      d.search_ms = o.search_ms[i];
    }
    t_trace.push_back(d);
  }
  if (nsamples) *nsamples = (uint32_t)t_trace.size();
  for (size_t i = 0; i < t_trace.size() && i < capacity; i++) samples[i] = t_trace[i];
  if (!e.empty()) return fail("%s", e.c_str());
  *edge = est;
  *accuracy = acc;
  return 0;
}

}  // namespace

std::function<int()> ngt_amd::edge_fresh_rand() {
  GlibcRandHost r;
  r.seed(1);
  return [r]() mutable { return r.next(); };
}

extern "C" int ngt_amd_recut_anng(int device, const uint64_t* offsets, const uint32_t* ids, const float* dists,
                                  uint64_t nrows, uint32_t K, uint64_t* out_nedges) {
  if (!offsets || !out_nedges) return fail("ngt_amd_recut_anng: bad arguments");
  *out_nedges = 0;
  if (recut_host_graph(device, offsets, ids, dists, nrows, K, t_graph)) {
    t_graph = HostGraph();
    return -1;
  }
  *out_nedges = t_graph.ids.size();
  return 0;
}

extern "C" int ngt_amd_recut_get_graph(uint64_t* offsets, uint32_t* ids, float* dists) {
  return copy_out(t_graph, "ngt_amd_recut_get_graph", "re-cut", offsets, ids, dists);
}

extern "C" int ngt_amd_optimize_edges(ngt_amd_index* ix, const ngt_amd_edge_params* prm, uint64_t* edge,
                                      float* accuracy, ngt_amd_edge_sample* samples, uint32_t* nsamples) {
  try {  // no exception crosses the C boundary
    return optimize_edges(ix, prm, edge, accuracy, samples, nsamples);
  } catch (std::exception& err) {
    return fail("ngt_amd_optimize_edges: %s", err.what());
  }
}

extern "C" int ngt_amd_optimize_edges_last_trace(ngt_amd_edge_sample* samples, uint32_t* nsamples) {
  if (!nsamples) return fail("ngt_amd_optimize_edges_last_trace: bad arguments");
  const uint32_t capacity = samples ? *nsamples : 0;
  *nsamples = (uint32_t)t_trace.size();
  for (size_t i = 0; i < t_trace.size() && i < capacity; i++) samples[i] = t_trace[i];
  return 0;
}

extern "C" uint64_t ngt_amd_round_edges(uint64_t edge, uint64_t max_no_of_edges) {
  return edge_round(edge, max_no_of_edges);
}
