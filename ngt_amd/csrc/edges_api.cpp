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
#include "edge_optimizer.h"
#include "edges_kernels.h"
#include "index_internal.h"
#include "onng_kernels.h"

using namespace ngt_amd;
using onng::Csr;

namespace {

struct DevGraph {
  DevBuf<uint64_t> off;
  DevBuf<uint32_t> ids;
  DevBuf<float> d;
  uint64_t edges = 0;
  Csr csr() const { return Csr{off.p, ids.p, d.p}; }
  void swap(DevGraph& o) {
    std::swap(off.p, o.off.p);
    std::swap(off.n, o.off.n);
    std::swap(ids.p, o.ids.p);
    std::swap(ids.n, o.ids.n);
    std::swap(d.p, o.d.p);
    std::swap(d.n, o.d.n);
    std::swap(edges, o.edges);
  }
};

template <typename T>
int fetch(hipStream_t s, T* host, const T* dev, size_t count) {
  HIP_OK(hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  return 0;
}

// reconstructANNGFromANNG(G, K) -> out: count, scan, fill, then per list sort,
// dedupe and unpack
int recut_device(hipStream_t s, uint32_t n, Csr G, uint32_t K, DevGraph& out) {
  DevBuf<uint32_t> cnt, cnt2;
  DevBuf<uint64_t> loff, keys_a, keys_b;
  HIP_OK(cnt.alloc(n));
  HIP_OK(hipMemsetAsync(cnt.p, 0, (size_t)n * 4, s));
  edges::count_recut(n, G, K, cnt.p, s);
  HIP_OK(loff.alloc((size_t)n + 1));
  onng::scan_u32(cnt.p, n, loff.p, s);
  HIP_OK(hipGetLastError());
  uint64_t total = 0;
  if (fetch(s, &total, loff.p + n, 1)) return -1;
  std::vector<uint32_t> h(n);
  if (fetch(s, h.data(), cnt.p, n)) return -1;
  uint32_t longest = 0;
  for (uint32_t x : h) longest = std::max(longest, x);
  HIP_OK(keys_a.alloc(total));
  HIP_OK(keys_b.alloc(total));
  HIP_OK(hipMemsetAsync(cnt.p, 0, (size_t)n * 4, s));
  edges::fill_recut(n, G, K, loff.p, cnt.p, keys_a.p, s);
  onng::sort_lists(n, loff.p, keys_a.p, keys_b.p, longest > onng::kFastCap, s);
  HIP_OK(cnt2.alloc(n));
  HIP_OK(hipMemsetAsync(cnt2.p, 0, (size_t)n * 4, s));
  onng::unique_lists(n, loff.p, keys_b.p, keys_a.p, cnt2.p, s);
  HIP_OK(out.off.alloc((size_t)n + 1));
  onng::scan_u32(cnt2.p, n, out.off.p, s);
  HIP_OK(hipGetLastError());
  if (fetch(s, &out.edges, out.off.p + n, 1)) return -1;
  HIP_OK(out.ids.alloc(out.edges));
  HIP_OK(out.d.alloc(out.edges));
  onng::unpack_lists(n, loff.p, keys_a.p, out.off.p, out.ids.p, out.d.p, s);
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(s));
  return 0;
}

struct Stream {
  hipStream_t s = nullptr;
  ~Stream() {
    if (s) (void)hipStreamDestroy(s);
  }
};

struct Result {
  std::vector<uint64_t> off;
  std::vector<uint32_t> ids;
  std::vector<float> d;
  bool ready = false;
};
thread_local Result t_result;
thread_local std::vector<ngt_amd_edge_sample> t_trace;  // the samples of the thread's last optimisation

int download(hipStream_t s, uint32_t n, const DevGraph& g, std::vector<uint64_t>& off, std::vector<uint32_t>& ids,
             std::vector<float>& d) {
  off.resize((size_t)n + 1);
  ids.resize(g.edges);
  d.resize(g.edges);
  HIP_OK(hipMemcpyAsync(off.data(), g.off.p, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, s));
  if (g.edges) HIP_OK(hipMemcpyAsync(ids.data(), g.ids.p, g.edges * 4, hipMemcpyDeviceToHost, s));
  if (g.edges) HIP_OK(hipMemcpyAsync(d.data(), g.d.p, g.edges * 4, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  return 0;
}

int upload(hipStream_t s, uint32_t n, const uint64_t* off, const uint32_t* ids, const float* d, DevGraph& g) {
  const uint64_t E = off[n];
  HIP_OK(g.off.alloc((size_t)n + 1));
  HIP_OK(g.ids.alloc(E));
  HIP_OK(g.d.alloc(E));
  HIP_OK(hipMemcpyAsync(g.off.p, off, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, s));
  if (E) HIP_OK(hipMemcpyAsync(g.ids.p, ids, E * 4, hipMemcpyHostToDevice, s));
  if (E) HIP_OK(hipMemcpyAsync(g.d.p, d, E * 4, hipMemcpyHostToDevice, s));
  g.edges = E;
  return 0;
}

int recut_host_graph(int device, const uint64_t* offsets, const uint32_t* ids, const float* dists, uint64_t nrows,
                     uint32_t K, Result& res) {
  res.ready = false;
  if (nrows == 0 || nrows >= (1ull << 31)) return fail("ngt_amd_recut_anng: %llu rows are not supported", (unsigned long long)nrows);
  if (K == 0) return fail("ngt_amd_recut_anng: K must be positive");
  if (offsets[0] != 0) return fail("ngt_amd_recut_anng: offsets[0] is not 0");
  for (uint64_t v = 0; v < nrows; v++) {
    if (offsets[v + 1] < offsets[v]) return fail("ngt_amd_recut_anng: offsets decrease at node %llu", (unsigned long long)v);
    if (offsets[v + 1] - offsets[v] >= (1ull << 31)) return fail("ngt_amd_recut_anng: the list of node %llu is too long", (unsigned long long)v);
  }
  if (offsets[nrows] && (!ids || !dists)) return fail("ngt_amd_recut_anng: ids or dists is null");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail("ngt_amd_recut_anng: no HIP device available (the MI355X path has no CPU fallback)");
  if (device < 0 || device >= ndev) return fail("ngt_amd_recut_anng: device %d out of range", device);
  HIP_OK(hipSetDevice(device));
  Stream st;
  HIP_OK(hipStreamCreateWithFlags(&st.s, hipStreamDefault));
  const uint32_t n = (uint32_t)nrows;
  DevGraph in, out;
  if (upload(st.s, n, offsets, ids, dists, in)) return -1;
  DevBuf<uint32_t> d_err;
  HIP_OK(d_err.alloc(onng::kErrWords));
  HIP_OK(hipMemsetAsync(d_err.p, 0xff, onng::kErrWords * 4, st.s));
  onng::check_lists(n, in.csr(), d_err.p, st.s);
  HIP_OK(hipGetLastError());
  uint32_t err[onng::kErrWords];
  if (fetch(st.s, err, d_err.p, onng::kErrWords)) return -1;
  if (err[onng::kErrBadId] != 0xffffffffu)
    return fail("ngt_amd_recut_anng: the list of node %u holds an id outside [1, %u)", err[onng::kErrBadId], n);
  if (recut_device(st.s, n, in.csr(), K, out)) return -1;
  if (download(st.s, n, out, res.off, res.ids, res.d)) return -1;
  res.ready = true;
  return 0;
}

double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// The session's tree as the getters return it.
struct TreeCopy {
  std::vector<uint32_t> leaf_parent, leaf_ids, in_parent, in_child;
  std::vector<uint64_t> leaf_off;
  std::vector<float> leaf_dists, in_border;
  std::vector<uint8_t> leaf_has_pivot, leaf_pivot, in_pivot;
  uint32_t nl = 0, ni = 0, root = 0;
};

struct Optimizer {
  ngt_amd_index* ix;
  ngt_amd_build_params bp;
  Stream st;
  GlibcRandHost rnd;
  // the last sample's state on the host: the graph the next construction starts
  // from (after a sample: its last re-cut), the nodes it holds, its tree
  std::vector<uint64_t> h_off;
  std::vector<uint32_t> h_ids;
  std::vector<float> h_d;
  std::vector<uint8_t> node;
  uint64_t graph_rows = 0;
  bool have_prev = false, cut_since_build = false;
  TreeCopy tree;
  DevGraph src, cur;  // the sample's graph; the re-cut the index searches
  std::vector<double> build_ms, recut_ms, search_ms;

  ~Optimizer() {
    // an index that still reads the last re-cut takes its buffers over
    if (cur.off.p && ix->edge_off.p == cur.off.p && ix->edges.p == cur.ids.p) {
      ix->edge_off.owned = true;
      ix->edges.owned = true;
      cur.off.owned = false;
      cur.ids.owned = false;
    }
  }

  int fetch_tree() {
    uint64_t nli = 0;
    if (ngt_amd_build_tree_size(ix, &tree.nl, &tree.ni, &nli)) return -1;
    const uint64_t rb = ix->row_bytes;
    tree.leaf_parent.resize(tree.nl);
    tree.leaf_off.resize((size_t)tree.nl + 1);
    tree.leaf_ids.resize(nli);
    tree.leaf_dists.resize(nli);
    tree.leaf_has_pivot.resize(tree.nl);
    tree.leaf_pivot.resize((size_t)tree.nl * rb);
    tree.in_parent.resize(tree.ni);
    tree.in_pivot.resize((size_t)tree.ni * rb);
    tree.in_child.resize((size_t)tree.ni * 5);
    tree.in_border.resize((size_t)tree.ni * 4);
    if (ngt_amd_build_get_tree(ix, tree.leaf_parent.data(), tree.leaf_off.data(), tree.leaf_ids.data(),
                               tree.leaf_dists.data(), tree.leaf_has_pivot.data(), tree.leaf_pivot.data(),
                               tree.in_parent.data(), tree.in_pivot.data(), tree.in_child.data(), tree.in_border.data()))
      return -1;
    tree.root = ix->build->root;
    return 0;
  }

  // createIndex(threads, end_id) into the graph and tree the sample before left
  int build(uint64_t end_id) {
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t n = (uint32_t)ix->nrows;
    if (cut_since_build) {  // the previous sample's last re-cut is the graph now
      if (download(st.s, n, cur, h_off, h_ids, h_d)) return -1;
      cut_since_build = false;
    }
    if (ngt_amd_build_begin(ix, &bp)) return -1;
    ix->build->rnd = rnd;  // the stream goes on where the query draw left it
    if (have_prev) {
      if (ngt_amd_build_set_graph(ix, h_off.data(), h_ids.data(), h_d.data(), graph_rows)) return -1;
      // a node whose re-cut list came out empty is still a node: not inserted again
      BuildState& b = *ix->build;
      for (uint64_t v = 0; v < graph_rows; v++)
        if (node[v]) {
          b.in_graph[v] = 1;
          b.graph_size = std::max<uint64_t>(b.graph_size, v + 1);
        }
      if (ngt_amd_build_set_tree(ix, tree.leaf_parent.data(), tree.leaf_off.data(), tree.leaf_ids.data(),
                                 tree.leaf_dists.data(), tree.leaf_has_pivot.data(), tree.leaf_pivot.data(), tree.nl,
                                 tree.in_parent.data(), tree.in_pivot.data(), tree.in_child.data(),
                                 tree.in_border.data(), tree.ni, tree.root))
        return -1;
    }
    if (ngt_amd_build_insert(ix, 1, end_id)) return -1;
    rnd = ix->build->rnd;
    uint64_t gsize = 0, ne = 0;
    if (ngt_amd_build_graph_size(ix, &gsize, &ne)) return -1;
    std::vector<uint64_t> off(gsize + 1);
    h_ids.resize(ne);
    h_d.resize(ne);
    if (ngt_amd_build_get_graph(ix, off.data(), h_ids.data(), h_d.data())) return -1;
    h_off.assign((size_t)n + 1, ne);
    for (uint64_t v = 0; v <= gsize && v <= n; v++) h_off[v] = off[v];
    graph_rows = gsize;
    node.assign(ix->build->in_graph.begin(), ix->build->in_graph.end());
    if (fetch_tree()) return -1;
    have_prev = true;
    // the pseudo ground truth searches the sample's whole graph
    if (ngt_amd_index_set_graph(ix, h_off.data(), h_ids.data(), ne)) return -1;
    if (ngt_amd_index_set_tree(ix, tree.in_pivot.data(), tree.ni, tree.in_child.data(), tree.in_border.data(), 5,
                               tree.root, tree.leaf_off.data(), tree.nl, tree.leaf_ids.data(), tree.leaf_ids.size()))
      return -1;
    build_ms.push_back(ms_since(t0));
    recut_ms.push_back(0.0);
    search_ms.push_back(0.0);
    return 0;
  }

  int extract() {
    const auto t0 = std::chrono::steady_clock::now();
    if (upload(st.s, (uint32_t)ix->nrows, h_off.data(), h_ids.data(), h_d.data(), src)) return -1;
    HIP_OK(hipStreamSynchronize(st.s));
    recut_ms.back() += ms_since(t0);
    return 0;
  }

  int recut(size_t K) {
    const auto t0 = std::chrono::steady_clock::now();
    DevGraph next;
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
  HIP_OK(hipStreamCreateWithFlags(&o.st.s, hipStreamDefault));
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
    ngt_amd_search_params p{};
    p.k = (uint32_t)b.size;
    p.epsilon = b.epsilon;
    p.radius = -1.0f;  // FLT_MAX
    p.edge_size = b.edge_size;
    p.seed_mode = NGT_AMD_SEED_TREE;
    p.visited_hash_log2 = ix->nrows >= (1u << 18) ? -1 : 0;
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
  if (recut_host_graph(device, offsets, ids, dists, nrows, K, t_result)) {
    t_result = Result();
    return -1;
  }
  *out_nedges = t_result.ids.size();
  return 0;
}

extern "C" int ngt_amd_recut_get_graph(uint64_t* offsets, uint32_t* ids, float* dists) {
  if (!t_result.ready) return fail("ngt_amd_recut_get_graph: no re-cut graph on this thread");
  if (!offsets) return fail("ngt_amd_recut_get_graph: bad arguments");
  memcpy(offsets, t_result.off.data(), t_result.off.size() * 8);
  if (ids && !t_result.ids.empty()) memcpy(ids, t_result.ids.data(), t_result.ids.size() * 4);
  if (dists && !t_result.d.empty()) memcpy(dists, t_result.d.data(), t_result.d.size() * 4);
  return 0;
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
