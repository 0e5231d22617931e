// refine.cpp -- host side of ngt_amd_refine_*: GraphReconstructor::refineANNG
// (lib/NGT/GraphReconstructor.h:803-924) on the device.
//
// Per batch of batch_size ids in id order:
//   1. search     one ngt_amd_search_device launch (tree seeds on the device)
//                 whose queries are the batch's slice of the index's own row
//                 slab; ids, distances and counts stay in HBM;
//   2. outgoing   every batch node's list + its results without itself, sorted
//                 by (distance, id), adjacent repeats of an id dropped;
//   3. incoming   (noOfEdges == 0) addEdge of every result's reverse, by the
//                 rule of refine_kernels.hip;
//   then the whole CSR is rebuilt in HBM and the index's search adjacency (CSR
//   ids, padded copy, widest list, adj_version) is pointed at it.
// After the last batch, noOfEdges > 0 cuts every list to noOfEdges.  The host
// sees three totals per batch (to size the buffers) and the final graph.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <mutex>

#include "../../include/ngt_amd.h"
#include "device_graph.h"
#include "index_internal.h"
#include "prep_kernels.h"
#include "refine_kernels.h"

using namespace ngt_amd;
using namespace ngt_amd::refine;

namespace {

constexpr uint32_t kNone = 0xffffffffu;

// Buffers kept from batch to batch.  words: the two error words, then the
// longest batch list, the most candidates of a target, the longest new list.
enum { kWordBatchLen = kErrWords, kWordCand, kWordNewLen, kWords };

struct Work {
  hipStream_t s = nullptr;
  uint32_t n = 0;
  DevBuf<uint32_t> blen, bcnt, ccnt, ropen, ins, nlen, words;
  DevBuf<uint64_t> boff, bka, bkb, coff, cka, ckb, cx, noff;
  ngt_amd_refine_stats st{};
};

// The graph into HBM, refused unless every list is in (distance, id) order with
// ids of rows: lower_bound needs it.
int upload_lists(Work& W, const uint64_t* offsets, const uint32_t* ids, const float* dists, uint32_t longest,
                 DeviceGraph& G) {
  if (upload_graph(W.s, W.n, offsets, ids, dists, G)) return -1;
  G.maxlen = longest;
  DevBuf<uint32_t> err;
  return verify_lists("refine", W.s, W.n, G, true, err);
}

// Steps 2 and 3 for one block of results (device pointers): G -> out.
int merge_block(Work& W, const DeviceGraph& G, Results R, bool with_incoming, DeviceGraph& out) {
  const uint32_t n = W.n, m = R.count + 1;
  hipStream_t s = W.s;
  uint32_t words[kWords];
  HIP_OK(W.words.alloc(kWords));
  HIP_OK(hipMemsetAsync(W.words.p, 0xff, kErrWords * 4, s));
  HIP_OK(hipMemsetAsync(W.words.p + kErrWords, 0, (kWords - kErrWords) * 4, s));
  // ---- outgoing: the batch's lists as packed keys, sorted, repeats dropped
  HIP_OK(W.blen.alloc(m));
  HIP_OK(W.boff.alloc((size_t)m + 1));
  HIP_OK(W.bcnt.alloc(m));
  batch_len(n, G.csr(), R, W.blen.p, W.words.p, s);
  onng::scan_u32(W.blen.p, m, W.boff.p, s);
  max_u32(W.blen.p, m, W.words.p + kWordBatchLen, s);
  HIP_OK(hipGetLastError());
  uint64_t total = 0;
  HIP_OK(hipMemcpyAsync(&total, W.boff.p + m, 8, hipMemcpyDeviceToHost, s));
  if (fetch(s, words, W.words.p, kWords)) return -1;
  if (words[kErrResultCount] != kNone)
    return fail("refine: query %u has more results than the stride %u", words[kErrResultCount], R.stride);
  if (words[kErrResultId] != kNone)
    return fail("refine: a result of query %u is an id outside [1, %u)", words[kErrResultId], n);
  HIP_OK(W.bka.alloc(total));
  HIP_OK(W.bkb.alloc(total));
  batch_fill(n, G.csr(), R, W.boff.p, W.bka.p, s);
  onng::sort_lists(m, W.boff.p, W.bka.p, W.bkb.p, words[kWordBatchLen] > kFastCap, s);
  HIP_OK(hipMemsetAsync(W.bcnt.p, 0, (size_t)m * 4, s));
  onng::unique_lists(m, W.boff.p, W.bkb.p, W.bka.p, W.bcnt.p, s);
  W.st.launches += 6 + (words[kWordBatchLen] > kFastCap ? 1 : 0);
  const Lists L{G.csr(), R.first, R.count, W.boff.p, W.bcnt.p, W.bka.p};
  // ---- incoming: candidates per target, the open ones decided, sorted
  if (with_incoming) {
    HIP_OK(W.ccnt.alloc(n));
    HIP_OK(W.ropen.alloc(n));
    HIP_OK(W.coff.alloc((size_t)n + 1));
    HIP_OK(W.ins.alloc(n));
    HIP_OK(hipMemsetAsync(W.ccnt.p, 0, (size_t)n * 4, s));
    HIP_OK(hipMemsetAsync(W.ropen.p, 0, (size_t)n * 4, s));
    incoming(n, L, R, false, W.ccnt.p, W.ropen.p, nullptr, nullptr, nullptr, s);
    onng::scan_u32(W.ccnt.p, n, W.coff.p, s);
    max_u32(W.ccnt.p, n, W.words.p + kWordCand, s);
    HIP_OK(hipGetLastError());
    uint64_t C = 0;
    HIP_OK(hipMemcpyAsync(&C, W.coff.p + n, 8, hipMemcpyDeviceToHost, s));
    if (fetch(s, words, W.words.p, kWords)) return -1;
    HIP_OK(W.cka.alloc(C));
    HIP_OK(W.ckb.alloc(C));
    HIP_OK(W.cx.alloc(C));
    HIP_OK(hipMemsetAsync(W.ccnt.p, 0, (size_t)n * 4, s));
    incoming(n, L, R, true, W.ccnt.p, W.ropen.p, W.coff.p, W.cka.p, W.cx.p, s);
    resolve(n, W.coff.p, W.ropen.p, W.cka.p, W.cx.p, W.ins.p, s);
    onng::sort_lists(n, W.coff.p, W.cka.p, W.ckb.p, words[kWordCand] > kFastCap, s);
    W.st.candidates += C;
    W.st.launches += 6 + (words[kWordCand] > kFastCap ? 1 : 0);
  }
  // ---- the new CSR
  HIP_OK(W.nlen.alloc(n));
  HIP_OK(W.noff.alloc((size_t)n + 1));
  new_len(n, L, with_incoming ? W.ins.p : nullptr, W.nlen.p, s);
  onng::scan_u32(W.nlen.p, n, W.noff.p, s);
  max_u32(W.nlen.p, n, W.words.p + kWordNewLen, s);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpyAsync(&out.edges, W.noff.p + n, 8, hipMemcpyDeviceToHost, s));
  if (fetch(s, words, W.words.p, kWords)) return -1;
  out.maxlen = words[kWordNewLen];
  HIP_OK(out.off.alloc((size_t)n + 1));
  HIP_OK(out.ids.alloc(out.edges));
  HIP_OK(out.d.alloc(out.edges));
  HIP_OK(hipMemcpyAsync(out.off.p, W.noff.p, ((size_t)n + 1) * 8, hipMemcpyDeviceToDevice, s));
  emit(n, L, with_incoming ? W.ins.p : nullptr, W.coff.p, W.ckb.p, out.off.p, out.ids.p, out.d.p, s);
  HIP_OK(hipGetLastError());
  W.st.launches += 4;
  return 0;
}

int prune(Work& W, const DeviceGraph& G, uint32_t k, DeviceGraph& out) {
  const uint32_t n = W.n;
  hipStream_t s = W.s;
  HIP_OK(W.words.alloc(kWords));
  HIP_OK(hipMemsetAsync(W.words.p, 0, kWords * 4, s));
  HIP_OK(W.nlen.alloc(n));
  HIP_OK(out.off.alloc((size_t)n + 1));
  prune_len(n, G.csr(), k, W.nlen.p, s);
  onng::scan_u32(W.nlen.p, n, out.off.p, s);
  max_u32(W.nlen.p, n, W.words.p + kWordNewLen, s);
  HIP_OK(hipGetLastError());
  uint32_t words[kWords];
  HIP_OK(hipMemcpyAsync(&out.edges, out.off.p + n, 8, hipMemcpyDeviceToHost, s));
  if (fetch(s, words, W.words.p, kWords)) return -1;
  out.maxlen = words[kWordNewLen];
  HIP_OK(out.ids.alloc(out.edges));
  HIP_OK(out.d.alloc(out.edges));
  prune_copy(n, G.csr(), out.off.p, out.ids.p, out.d.p, s);
  HIP_OK(hipGetLastError());
  W.st.launches += 4;
  return 0;
}

thread_local HostGraph t_graph;
thread_local ngt_amd_refine_stats t_stats;

// G and the run's counters into the thread's result
int finish(Work& W, const DeviceGraph& G, HostGraph& res, ngt_amd_refine_stats& stats) {
  if (download_graph(W.s, W.n, G, res)) return -1;
  W.st.edges_out = G.edges;
  W.st.longest_list = G.maxlen;
  stats = W.st;
  res.ready = true;
  return 0;
}

// ---- the index's search adjacency, from the CSR in HBM ------------------------
// Points the index's CSR ids at G (not owned) and refreshes the padded copy,
// the widest list and adj_version; `es` is the resolved edge size of the
// refinement's searches.
int point_index_at(ngt_amd_index* ix, const DeviceGraph& G, uint64_t es, hipStream_t s) {
  std::lock_guard<std::mutex> lk(ix->mu);
  ix->edge_off.borrow(G.off.p, ix->nrows + 1);
  ix->edges.borrow(G.ids.p, G.edges);
  ix->nedges = G.edges;
  ix->has_graph = true;
  ix->max_degree = G.maxlen;
  const uint64_t need = adjacency_need(ix, es);
  if (need == 0 || need > 256) {  // the searches take the CSR path
    ix->adj.release();
    ix->adj_stride = 0;
  } else {
    const uint64_t stride = std::max<uint64_t>((need + 15) & ~15ull, ix->adj.p ? ix->adj_stride : 0);
    if (!ix->adj.p || ix->adj.n < ix->nrows * stride) {
      ix->adj.release();
      ix->adj_stride = 0;
      HIP_OK(ix->adj.alloc(ix->nrows * stride));
    }
    HIP_OK(launch_pad_adjacency(G.off.p, G.ids.p, ix->nrows, stride, ix->adj.p, s));
    ix->adj_stride = stride;
  }
  ix->adj_version++;
  return 0;
}

// The index keeps a graph whatever happens: G's arrays on success, the input
// graph again otherwise.
struct GraphGuard {
  ngt_amd_index* ix;
  const uint64_t* offsets;
  const uint32_t* ids;
  bool armed = false;
  ~GraphGuard() {
    if (!armed) return;
    {
      std::lock_guard<std::mutex> lk(ix->mu);
      ix->edge_off.release();
      ix->edges.release();
      ix->nedges = 0;
      ix->has_graph = false;
      ix->adj.release();
      ix->adj_stride = 0;
      ix->adj_version++;
    }
    (void)ngt_amd_index_set_graph(ix, offsets, ids, offsets[ix->nrows]);
  }
};

double seconds_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

int refine_index(ngt_amd_index* ix, const uint64_t* offsets, const uint32_t* ids, const float* dists,
                 const ngt_amd_refine_params& p, HostGraph& res, ngt_amd_refine_stats& stats) {
  res.ready = false;
  uint32_t longest = 0;
  if (check_csr("ngt_amd_refine_anng", offsets, ids, dists, ix->nrows, true, &longest)) return -1;
  if (!ix->rows.p || ix->nrows < 2) return fail("ngt_amd_refine_anng: the index has no objects");
  if (!ix->has_tree) return fail("ngt_amd_refine_anng: the index has no tree (the searches take their seeds from it)");
  if (p.batch_size == 0) return fail("ngt_amd_refine_anng: the batch size is 0");
  if (p.edge_size_for_creation <= 0 && p.num_edges == 0)
    return fail("ngt_amd_refine_anng: edge_size_for_creation must be > 0");
  // noOfSearchedEdges (GraphReconstructor.h:825)
  const int64_t size64 = p.num_edges < 0 ? -(int64_t)p.num_edges
                                         : std::max<int64_t>(p.num_edges, p.edge_size_for_creation);
  if (size64 <= 0 || size64 > (1 << 20)) return fail("ngt_amd_refine_anng: %lld results per search are not supported", (long long)size64);
  const uint32_t size = (uint32_t)size64;
  const uint64_t es = ngt_amd_resolve_edge_size(ix, p.explore_edge_size, p.epsilon);
  if (es == 0)
    return fail("NGT::getEdgeSize: Invalid edge size parameters %lld:%d", (long long)p.explore_edge_size,
                ix->edge_size_for_search);
  HIP_OK(hipSetDevice(ix->device));
  ServeHold serve_hold(ix);

  const auto t_all = std::chrono::steady_clock::now();
  Work W;
  W.s = ix->stream;
  W.n = (uint32_t)ix->nrows;
  const uint32_t n = W.n;
  W.st.edges_in = offsets[n];
  DeviceGraph cur, next;
  if (upload_lists(W, offsets, ids, dists, longest, cur)) return -1;
  GraphGuard guard{ix, offsets, ids};
  guard.armed = true;
  if (point_index_at(ix, cur, es, W.s)) return -1;

  // no allocation is sized by the batch size alone
  const uint32_t B = (uint32_t)std::min<uint64_t>(p.batch_size, n - 1);
  DevBuf<uint32_t> rid, rn;
  DevBuf<float> rd;
  HIP_OK(rid.alloc((size_t)B * size));
  HIP_OK(rd.alloc((size_t)B * size));
  HIP_OK(rn.alloc(B));
  const ngt_amd_search_params sp =
      library_search_params(ix->nrows, size, p.epsilon, FLT_MAX, p.explore_edge_size, NGT_AMD_SEED_TREE);
  for (uint64_t bid = 1; bid < n; bid += B) {
    const uint32_t count = (uint32_t)std::min<uint64_t>(B, n - bid);
    auto t0 = std::chrono::steady_clock::now();
    if (clear_device_error(ix, W.s)) return -1;
    if (ngt_amd_search_device(ix, &sp, ix->rows.p + bid * ix->row_bytes, ix->row_bytes, count, nullptr, nullptr, rid.p,
                              rd.p, rn.p, nullptr, W.s))
      return -1;
    int flag = 0;
    if (take_device_error(ix, W.s, &flag)) return -1;
    if (flag) return fail("ngt_amd_refine_anng: device error flag %d (%s)", flag, device_error_text(flag).c_str());
    W.st.search_ms += seconds_since(t0) * 1e3;
    t0 = std::chrono::steady_clock::now();
    mask_counts(ix->valid.p, (uint32_t)bid, count, rn.p, W.s);
    const Results R{(uint32_t)bid, count, size, rid.p, rd.p, rn.p};
    if (merge_block(W, cur, R, p.num_edges == 0, next)) return -1;
    W.st.launches += 1;
    HIP_OK(hipStreamSynchronize(W.s));
    W.st.merge_ms += seconds_since(t0) * 1e3;
    t0 = std::chrono::steady_clock::now();
    cur.swap(next);
    if (point_index_at(ix, cur, es, W.s)) return -1;
    HIP_OK(hipStreamSynchronize(W.s));
    W.st.refresh_ms += seconds_since(t0) * 1e3;
    W.st.batches++;
    W.st.searched += count;
  }
  if (p.num_edges > 0) {
    const auto t0 = std::chrono::steady_clock::now();
    if (prune(W, cur, (uint32_t)p.num_edges, next)) return -1;
    cur.swap(next);
    if (point_index_at(ix, cur, es, W.s)) return -1;
    HIP_OK(hipStreamSynchronize(W.s));
    W.st.merge_ms += seconds_since(t0) * 1e3;
  }
  if (finish(W, cur, res, stats)) return -1;
  // the index owns the final CSR from here on
  {
    std::lock_guard<std::mutex> lk(ix->mu);
    ix->edge_off.take_from(cur.off);
    ix->edges.take_from(cur.ids);
    ix->h_graph_empty.assign(n, 1);
    for (uint32_t v = 0; v < n; v++) ix->h_graph_empty[v] = res.off[v + 1] == res.off[v];
  }
  guard.armed = false;
  stats.total_ms = seconds_since(t_all) * 1e3;
  return 0;
}

}  // namespace

extern "C" uint32_t ngt_amd_refine_fast_path_capacity(void) { return kFastCap; }

extern "C" int ngt_amd_refine_merge(int device, const uint64_t* offsets, const uint32_t* ids, const float* dists,
                                    uint64_t nrows, uint32_t first_id, uint32_t count, uint32_t stride,
                                    const uint32_t* res_ids, const float* res_dists, const uint32_t* res_counts,
                                    int incoming, uint64_t* out_nedges) {
  if (!out_nedges) return fail("ngt_amd_refine_merge: bad arguments");
  *out_nedges = 0;
  t_graph = HostGraph();
  uint32_t longest = 0;
  if (check_csr("ngt_amd_refine_merge", offsets, ids, dists, nrows, true, &longest)) return -1;
  if (first_id < 1 || first_id >= nrows) return fail("ngt_amd_refine_merge: first id %u outside [1, %llu)", first_id, (unsigned long long)nrows);
  if (count && (!res_counts || (stride && (!res_ids || !res_dists)))) return fail("ngt_amd_refine_merge: bad arguments");
  // a last batch overhangs the rows: its tail holds no object
  const uint32_t used = (uint32_t)std::min<uint64_t>(count, nrows - first_id);
  if (select_device("ngt_amd_refine_merge", device)) return -1;
  OwnedStream st;
  if (st.create()) return -1;
  Work W;
  W.s = st.s;
  W.n = (uint32_t)nrows;
  W.st.edges_in = offsets[nrows];
  DeviceGraph G, out;
  if (upload_lists(W, offsets, ids, dists, longest, G)) return -1;
  DevBuf<uint32_t> rid, rn;
  DevBuf<float> rd;
  const size_t slots = (size_t)used * stride;
  HIP_OK(rid.alloc(slots));
  HIP_OK(rd.alloc(slots));
  HIP_OK(rn.alloc(used));
  if (slots) HIP_OK(hipMemcpyAsync(rid.p, res_ids, slots * 4, hipMemcpyHostToDevice, W.s));
  if (slots) HIP_OK(hipMemcpyAsync(rd.p, res_dists, slots * 4, hipMemcpyHostToDevice, W.s));
  if (used) HIP_OK(hipMemcpyAsync(rn.p, res_counts, (size_t)used * 4, hipMemcpyHostToDevice, W.s));
  const Results R{first_id, used, stride, rid.p, rd.p, rn.p};
  if (merge_block(W, G, R, incoming != 0, out)) return -1;
  W.st.batches = 1;
  W.st.searched = used;
  if (finish(W, out, t_graph, t_stats)) {
    t_graph = HostGraph();
    return -1;
  }
  *out_nedges = t_graph.ids.size();
  return 0;
}

extern "C" int ngt_amd_refine_prune(int device, const uint64_t* offsets, const uint32_t* ids, const float* dists,
                                    uint64_t nrows, uint32_t num_edges, uint64_t* out_nedges) {
  if (!out_nedges) return fail("ngt_amd_refine_prune: bad arguments");
  *out_nedges = 0;
  t_graph = HostGraph();
  uint32_t longest = 0;
  if (check_csr("ngt_amd_refine_prune", offsets, ids, dists, nrows, true, &longest)) return -1;
  if (select_device("ngt_amd_refine_prune", device)) return -1;
  OwnedStream st;
  if (st.create()) return -1;
  Work W;
  W.s = st.s;
  W.n = (uint32_t)nrows;
  W.st.edges_in = offsets[nrows];
  DeviceGraph G, out;
  if (upload_lists(W, offsets, ids, dists, longest, G)) return -1;
  if (prune(W, G, num_edges, out)) return -1;
  if (finish(W, out, t_graph, t_stats)) {
    t_graph = HostGraph();
    return -1;
  }
  *out_nedges = t_graph.ids.size();
  return 0;
}

extern "C" int ngt_amd_refine_anng(ngt_amd_index* ix, const uint64_t* offsets, const uint32_t* ids,
                                   const float* dists, uint64_t nrows, const ngt_amd_refine_params* params,
                                   uint64_t* out_nedges) {
  if (!ix || !params || !out_nedges) return fail("ngt_amd_refine_anng: bad arguments");
  *out_nedges = 0;
  t_graph = HostGraph();
  if (nrows != ix->nrows)
    return fail("ngt_amd_refine_anng: the graph has %llu rows, the index %llu", (unsigned long long)nrows,
                (unsigned long long)ix->nrows);
  if (refine_index(ix, offsets, ids, dists, *params, t_graph, t_stats)) {
    t_graph = HostGraph();
    return -1;
  }
  *out_nedges = t_graph.ids.size();
  return 0;
}

extern "C" int ngt_amd_refine_get_graph(uint64_t* offsets, uint32_t* ids, float* dists) {
  return copy_out(t_graph, "ngt_amd_refine_get_graph", "refined", offsets, ids, dists);
}

extern "C" int ngt_amd_refine_last_stats(ngt_amd_refine_stats* stats) {
  if (!stats) return fail("ngt_amd_refine_last_stats: bad arguments");
  if (!t_graph.ready) return fail("ngt_amd_refine_last_stats: no refined graph on this thread");
  *stats = t_stats;
  return 0;
}
