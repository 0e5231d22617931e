// build.cpp -- graph construction on the MI355X:
// GraphAndTreeIndex::createIndex(threadPoolSize) (lib/NGT/Index.cpp:1158-1257)
// for graphType ANNG, IANNG, ONNG and KNNG with the default (disabled) edge
// truncation.  The ANNG first; the other types follow below.
//
// Per creation batch of batchSizeForCreation objects, in id order
// (searchMultipleQueryForCreation, Index.cpp:631-671):
//   1. seeds: DVP-tree leaf descent of every batch object with
//      useAllNodesInLeaf (searchForNNGInsertion, Index.h:1457-1479) --
//      ngt_tree_seed_kernel over the tree under construction; an empty leaf
//      falls back to getRandomSeeds over the graph (Index.h:775-801) with the
//      rand() stream of a fresh process;
//   2. the insertion searches: one ngt_graph_search_kernel launch for the batch
//      (size edgeSizeForCreation, explorationCoefficient insertionRadiusCoefficient,
//      the first edgeSizeForSearch edges of each node);
//   3. insertMultipleSearchResults (Index.cpp:673-727): the batch's pairwise
//      distances (ngt_distances_kernel), merge, sort by (distance, id), cut to
//      edgeSizeForCreation, then insertANNGNode (Graph.h:611-625) -- the node's
//      edges and the reverse edges, sorted inserts (Graph.h:845-873);
//   4. DVPTree::insert of the batch (ngt_tree_insert_kernel).
// The graph being built is host-side (sorted edge lists, the reference's
// GraphRepository); the insertion searches read a padded HBM copy of each
// node's first edgeSizeForSearch edges, refreshed for the nodes a batch touched.
// Every rule on those lists -- the insertion rules, the sorted addEdge,
// getRandomSeeds, the host half of removal, the adjacency rows -- is stated in
// session_graph.h, pure host code; this file is the device work around them.
//
// IANNG and ONNG keep steps 1, 2 and 4 and the merge of step 3; only the
// insertion rule differs (NeighborhoodGraph::insertNode, Graph.h:533-562):
//   IANNG  insertIANNGNode (Graph.h:628-635): every reverse edge goes through
//          addEdgeDeletingExcessEdges (:888-934), which first drops the target's
//          edge at rank edgeSizeForCreation - 1, in both directions, when that
//          edge is not shorter than the new one and the node it leads to also
//          has one at that rank that is not longer;
//   ONNG   insertONNGNode (Graph.h:637-655): reverse edges for the first
//          incomingEdge results, the stored list cut to outgoingEdge afterwards.
// Both equal the reference at any creation thread count: it sorts a batch's
// jobs by their place in the batch before it merges and inserts them
// (Index.cpp:676-703).
//
// KNNG (insertKNNGNode, Graph.h:607-609) has no insertion search, no in-batch
// distances and no reverse edges.  Per batch:
//   a. the batch objects' exact edgeSizeForCreation + 1 nearest among all the
//      stored objects (searchForKNNGInsertion, Index.h:839-856: linearSearch
//      over the object repository as it stands, radius FLT_MAX) -- the
//      library's exact scan, ngt_amd_linear_search_device, with the stored rows
//      as the prepared queries, read where they lie in HBM; the validity flags
//      hide removed rows.  edgeSizeForCreation + 1 is therefore limited to a k
//      that function accepts: beyond it the call fails with that function's
//      message before the session's graph or tree change;
//   b. ngt_knng_lists_kernel: ObjectDistances::moveFrom (ObjectSpace.h:70-88)
//      -- the object itself leaves its list, or, when more than
//      edgeSizeForCreation exact duplicates with smaller ids kept it out of its
//      own E + 1 nearest, the nearest entry does (what the reference's release
//      build does; its debug build asserts there) -- written to the session's
//      lists and to the padded adjacency, with the tree-insertion flag;
//   c. DVPTree::insert of the batch in id order.  That is the reference run
//      with one creation thread: with more, its KNNG jobs reach the tree in
//      thread completion order (only the other types' are sorted) and its tre
//      does not repeat.
// The lists depend on neither the batch size nor the thread count, and a list
// never changes after its node's insertion; they make one trip to the host, for
// the graph mirror.
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "../../include/ngt_amd.h"
#include "index_internal.h"
#include "index_io.h"
#include "ngt_kernels.h"
#include "remove_kernels.h"
#include "session_graph.h"

using namespace ngt_amd;

namespace {

constexpr uint32_t kLeaf = 0x80000000u;
constexpr uint32_t kLeafCap = 112;  // >= leafObjectsSize + 1, multiple of 16

template <typename T>
int grow(DevBuf<T>& b, size_t old_count, size_t new_count) {
  if (b.p && b.n >= new_count) return 0;
  T* p = nullptr;
  HIP_OK(hipMalloc((void**)&p, std::max<size_t>(new_count, 1) * sizeof(T)));
  HIP_OK(hipMemset(p, 0, std::max<size_t>(new_count, 1) * sizeof(T)));
  if (b.p && old_count) HIP_OK(hipMemcpy(p, b.p, old_count * sizeof(T), hipMemcpyDeviceToDevice));
  b.release();
  b.p = p;
  b.n = new_count;
  return 0;
}

// room for `extra_leaves` / `extra_internal` more nodes
int ensure_tree_capacity(ngt_amd_index* ix, BuildState& b, uint32_t extra_leaves, uint32_t extra_internal) {
  const uint64_t rb = ix->row_bytes;
  if (b.n_leaf + extra_leaves > b.leaf_cap_nodes) {
    const uint32_t old = b.leaf_cap_nodes;
    const uint32_t cap = std::max<uint32_t>(b.n_leaf + extra_leaves, old * 2);
    if (grow(b.lf_parent, old, cap) || grow(b.lf_count, old, cap) || grow(b.lf_has_pivot, old, cap) ||
        grow(b.lf_ids, (size_t)old * kLeafCap, (size_t)cap * kLeafCap) ||
        grow(b.lf_dist, (size_t)old * kLeafCap, (size_t)cap * kLeafCap) ||
        grow(b.lf_pivot, (size_t)old * rb, (size_t)cap * rb))
      return -1;
    b.leaf_cap_nodes = cap;
  }
  if (b.n_internal + extra_internal > b.in_cap_nodes) {
    const uint32_t old = b.in_cap_nodes;
    const uint32_t cap = std::max<uint32_t>(b.n_internal + extra_internal, old * 2);
    if (grow(b.in_parent, old, cap) || grow(b.in_child, (size_t)old * 5, (size_t)cap * 5) ||
        grow(b.in_border, (size_t)old * 4, (size_t)cap * 4) || grow(b.in_pivot, (size_t)old * rb, (size_t)cap * rb))
      return -1;
    b.in_cap_nodes = cap;
  }
  return 0;
}

// NGT_AMD_BUILD_PROFILE=1: wall time per stage, summed over a call.  With a
// stream, every mark synchronises it first.
struct StageClock {
  bool on = ngt_amd::knob("NGT_AMD_BUILD_PROFILE") != nullptr;
  hipStream_t sync = nullptr;
  double st[6] = {0, 0, 0, 0, 0, 0};
  std::chrono::steady_clock::time_point t_last = std::chrono::steady_clock::now();
  void start() { t_last = std::chrono::steady_clock::now(); }
  void mark(int i) {
    if (!on) return;
    if (sync) (void)hipStreamSynchronize(sync);
    auto t = std::chrono::steady_clock::now();
    st[i] += std::chrono::duration<double>(t - t_last).count();
    t_last = t;
  }
};

}  // namespace

extern "C" int ngt_amd_build_begin(ngt_amd_index* ix, const ngt_amd_build_params* prm) {
  if (!ix || !prm) return fail("ngt_amd_build_begin: bad arguments");
  if (ix->nrows == 0) return fail("ngt_amd_build_begin: set the objects first");
  if (prm->edge_size_for_creation <= 0 || prm->batch_size_for_creation <= 0)
    return fail("ngt_amd_build_begin: edge_size_for_creation and batch_size_for_creation must be > 0");
  HIP_OK(hipSetDevice(ix->device));
  ServeHold serve_hold(ix);
  delete ix->build;
  auto* b = new BuildState();
  ix->build = b;
  SessionGraph& g = b->g;
  g.edge_size_for_creation = prm->edge_size_for_creation;
  b->edge_size_for_search = prm->edge_size_for_search;
  b->batch_size = prm->batch_size_for_creation;
  b->seed_size = prm->seed_size;
  b->epsilon_for_creation = prm->epsilon_for_creation;
  g.graph_type = prm->graph_type == 0 ? NGT_AMD_GRAPH_ANNG : prm->graph_type;
  if (g.graph_type != NGT_AMD_GRAPH_ANNG && g.graph_type != NGT_AMD_GRAPH_KNNG &&
      g.graph_type != NGT_AMD_GRAPH_ONNG && g.graph_type != NGT_AMD_GRAPH_IANNG)
    return fail("ngt_amd_build_begin: graph type %d unsupported (ANNG 1, KNNG 2, ONNG 4 and IANNG 5 are built)",
                prm->graph_type);
  g.reset(ix->nrows);
  b->rnd.seed(1);
  if (ensure_tree_capacity(ix, *b, 64, 16)) return -1;
  // the empty root leaf (DVPTree(), Tree.h:71-78): leaf 1, no parent, no objects
  const uint32_t c3[3] = {2u, 1u, kLeaf | 1u};
  HIP_OK(b->counts.upload(c3, 3));
  b->n_leaf = 2;
  b->n_internal = 1;
  b->root = kLeaf | 1u;
  // padded search adjacency: each node's first edgeSizeForSearch edges
  const int64_t es = prm->edge_size_for_search;
  if (es < 0 || es > 256) return fail("ngt_amd_build_begin: edge_size_for_search %lld unsupported", (long long)es);
  g.adj_stride = es == 0 ? 256 : (uint64_t)((es + 15) / 16 * 16);
  HIP_OK(ix->adj.alloc((size_t)ix->nrows * g.adj_stride));
  HIP_OK(hipMemset(ix->adj.p, 0, (size_t)ix->nrows * g.adj_stride * sizeof(uint32_t)));
  ix->adj_stride = g.adj_stride;
  ix->adj_version++;
  // the construction's searches read at most adj_stride edges of a list: the
  // padded copy is always the one to use (run_search never rebuilds it here)
  ix->max_degree = g.adj_stride;
  ix->has_graph = true;
  ix->edge_size_for_search = prm->edge_size_for_search;
  ix->seed_size = prm->seed_size;
  ix->seed_type = 0;
  return 0;
}

extern "C" int ngt_amd_build_set_onng_edges(ngt_amd_index* ix, int32_t outgoing_edge, int32_t incoming_edge) {
  if (!ix || !ix->build) return fail("ngt_amd_build_set_onng_edges: call ngt_amd_build_begin first");
  if (outgoing_edge < 1 || incoming_edge < 0)
    return fail("ngt_amd_build_set_onng_edges: outgoing_edge %d must be >= 1 and incoming_edge %d >= 0",
                outgoing_edge, incoming_edge);
  ix->build->g.outgoing_edge = outgoing_edge;
  ix->build->g.incoming_edge = incoming_edge;
  return 0;
}

namespace {

// the tree fields of a batch's DVPTree::insert launch; the caller adds the
// pre-located leaves, if it has them
TreeBuildArgs tree_insert_args(ngt_amd_index* ix, BuildState& b, const uint32_t* d_ids, const uint8_t* d_flag,
                               uint32_t n) {
  TreeBuildArgs ta{};
  ta.rows = ix->rows.p;
  ta.row_bytes = ix->row_bytes;
  ta.dp = (int)ix->dp;
  ta.lf_parent = b.lf_parent.p;
  ta.lf_has_pivot = b.lf_has_pivot.p;
  ta.lf_pivot = b.lf_pivot.p;
  ta.lf_count = b.lf_count.p;
  ta.lf_ids = b.lf_ids.p;
  ta.lf_dist = b.lf_dist.p;
  ta.leaf_cap = kLeafCap;
  ta.in_parent = b.in_parent.p;
  ta.in_pivot = b.in_pivot.p;
  ta.in_child = b.in_child.p;
  ta.in_border = b.in_border.p;
  ta.counts = b.counts.p;
  ta.leaf_cap_nodes = b.leaf_cap_nodes;
  ta.in_cap_nodes = b.in_cap_nodes;
  ta.leaf_size = 100;  // LeafNode::LeafObjectsSizeMax (Node.h:618)
  ta.ids = d_ids;
  ta.insert_flag = d_flag;
  // NGT_AMD_BUILD_REPL_CAP: a smaller table, so that small batches fill it
  ta.repl_cap = 256;
  if (const char* v = ngt_amd::knob("NGT_AMD_BUILD_REPL_CAP")) ta.repl_cap = (uint32_t)std::min(256, std::max(0, atoi(v)));
  ta.n = n;
  ta.error = ix->error.p;
  return ta;
}

// the end of a batch: the tree's node counts and the device error flags
int finish_batch(ngt_amd_index* ix, BuildState& b, hipStream_t s) {
  uint32_t hc[3];
  int herr = 0;
  HIP_OK(hipMemcpyAsync(hc, b.counts.p, sizeof hc, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(&herr, ix->error.p, sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  int serr = 0;  // the insertion searches' flag (their launch context on s)
  if (take_device_error(ix, s, &serr)) return -1;
  herr |= serr;
  if (herr) {
    (void)hipMemset(ix->error.p, 0, sizeof(int));
    return fail("ngt_amd_build_insert: device error flag %d (1 unchecked-set spill full; DVP tree: 2 already "
                "existed, 8 all split distances equal, 16 node capacity, 32 illegal pivot)", herr);
  }
  b.n_leaf = hc[0];
  b.n_internal = hc[1];
  b.root = hc[2];
  return 0;
}

// a search from given seeds over the property's edge size (sc.edgeSize default
// -> edgeSizeForSearch), visited ids hashed in LDS
ngt_amd_search_params seeded_search_params(uint32_t k, float epsilon, float radius) {
  ngt_amd_search_params p{};
  p.k = k;
  p.epsilon = epsilon;
  p.radius = radius;
  p.edge_size = -1;
  p.seed_mode = NGT_AMD_SEED_GIVEN;
  p.visited_hash_log2 = 0;
  return p;
}

int alloc_descent(DescentBufs& d, uint32_t nq) {
  HIP_OK(d.tseeds.alloc((size_t)nq * kTreeSeedStride));
  HIP_OK(d.tcnt.alloc(nq));
  HIP_OK(d.pleaf.alloc(nq));
  HIP_OK(d.pcnt.alloc(nq));
  HIP_OK(d.pdist.alloc(nq));
  return 0;
}

// A descent of nq prepared rows over the session's tree that writes each
// row's leaf, its object count and pivot distance next to the seeds; the
// caller sets seed_size, k and all_leaf_nodes.
TreeSeedArgs tree_descent_args(const ngt_amd_index* ix, const BuildState& b, const uint8_t* queries, uint32_t nq,
                               const DescentBufs& d) {
  TreeSeedArgs t{};
  t.queries = queries;
  t.query_bytes = ix->row_bytes;
  t.nq = nq;
  t.dp = (int)ix->dp;
  t.row_bytes = ix->row_bytes;
  t.in_pivot = b.in_pivot.p;
  t.in_child = b.in_child.p;
  t.in_border = b.in_border.p;
  t.children = 5;
  t.root = b.root;
  t.leaf_count = b.lf_count.p;
  t.leaf_stride = kLeafCap;
  t.leaf_ids = b.lf_ids.p;
  t.seeds = d.tseeds.p;
  t.seed_stride = kTreeSeedStride;
  t.seed_count = d.tcnt.p;
  t.out_leaf = d.pleaf.p;
  t.out_count = d.pcnt.p;
  t.out_pdist = d.pdist.p;
  t.leaf_pivot = b.lf_pivot.p;
  return t;
}

// The buffers of one ngt_amd_build_insert call, sized for a batch, and the
// batch in hand.  res_*: the insertion searches' results, or KNNG's exact
// E + 1 nearest; list_*: the lists to store, E wide.
struct InsertCall {
  ngt_amd_index* ix;
  BuildState& b;
  hipStream_t s;
  uint32_t B, E;
  const uint32_t* ids = nullptr;  // the batch: n object ids, ascending
  uint32_t n = 0;
  DevBuf<uint32_t> d_ids, d_seeds, d_res_ids, d_res_n, d_list_ids, d_list_n, d_dirty, d_vals;
  DevBuf<uint64_t> d_soff, d_cnt;
  DevBuf<float> d_res_d, d_list_d, d_pd;
  DevBuf<uint8_t> d_q, d_flag;
  DescentBufs descent;
  std::vector<uint32_t> h_tseeds, h_tcnt, h_list_ids, h_list_n;
  std::vector<float> h_list_d;
  std::vector<uint64_t> h_cnt;
  hipEvent_t ev_copy = nullptr;  // the lists have reached the host
  StageClock clk;
  // NGT_AMD_BUILD_PROFILE: the insertion searches' kernel time and counter sums
  double k_ms = 0, sum[NGT_AMD_COUNTERS_PER_QUERY] = {}, ex_max = 0, c5_max = 0;
  uint64_t nsearched = 0;

  InsertCall(ngt_amd_index* i, BuildState& bs)
      : ix(i), b(bs), s(i->stream), B((uint32_t)bs.batch_size), E((uint32_t)bs.g.edge_size_for_creation) {
    clk.sync = s;
  }
  ~InsertCall() {
    if (ev_copy) (void)hipEventDestroy(ev_copy);
  }
  bool knng() const { return b.g.graph_type == NGT_AMD_GRAPH_KNNG; }

  int alloc() {
    const uint32_t res_k = knng() ? E + 1 : E;
    HIP_OK(d_ids.alloc(B));
    HIP_OK(d_res_ids.alloc((size_t)B * res_k));
    HIP_OK(d_res_d.alloc((size_t)B * res_k));
    HIP_OK(d_res_n.alloc(B));
    HIP_OK(d_list_ids.alloc((size_t)B * E));
    HIP_OK(d_list_d.alloc((size_t)B * E));
    HIP_OK(d_list_n.alloc(B));
    HIP_OK(d_flag.alloc(B));
    h_list_ids.resize((size_t)B * E);
    h_list_d.resize((size_t)B * E);
    h_list_n.resize(B);
    if (knng()) return 0;  // its rows are queried where they lie; d_q only for a batch with gaps
    HIP_OK(hipEventCreateWithFlags(&ev_copy, hipEventDisableTiming));
    HIP_OK(d_q.alloc((size_t)B * ix->row_bytes));
    if (alloc_descent(descent, B)) return -1;
    h_tseeds.resize((size_t)B * kTreeSeedStride);
    h_tcnt.resize(B);
    if (clk.on) {
      HIP_OK(d_cnt.alloc((size_t)B * NGT_AMD_COUNTERS_PER_QUERY));
      h_cnt.resize((size_t)B * NGT_AMD_COUNTERS_PER_QUERY);
    }
    return 0;
  }
};

// ---- 1. seeds: all objects of the leaf each batch object descends to; the
//      same descent locates each object's leaf for step 4.  An empty leaf takes
//      getSeedsFromGraph's random seeds. -----------------------------------------
int seed_batch(InsertCall& c, std::vector<uint32_t>& seeds, std::vector<uint64_t>& soff) {
  const uint32_t n = c.n, SS = kTreeSeedStride;
  HIP_OK(launch_gather_rows(c.d_q.p, c.ix->rows.p, c.ix->row_bytes, c.d_ids.p, n, c.s));
  TreeSeedArgs t = tree_descent_args(c.ix, c.b, c.d_q.p, n, c.descent);
  t.seed_size = (uint32_t)std::max(c.b.seed_size, 0);
  t.k = c.E;
  t.all_leaf_nodes = 1;
  HIP_OK(launch_tree_seeds(t, c.ix->metric, c.ix->otype, c.s));
  HIP_OK(hipMemcpyAsync(c.h_tseeds.data(), c.descent.tseeds.p, (size_t)n * SS * sizeof(uint32_t),
                        hipMemcpyDeviceToHost, c.s));
  HIP_OK(hipMemcpyAsync(c.h_tcnt.data(), c.descent.tcnt.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c.s));
  HIP_OK(hipStreamSynchronize(c.s));
  c.clk.mark(0);
  soff.assign(n + 1, 0);
  for (uint32_t i = 0; i < n; i++) {
    seeds.insert(seeds.end(), c.h_tseeds.begin() + (size_t)i * SS, c.h_tseeds.begin() + (size_t)i * SS + c.h_tcnt[i]);
    if (c.h_tcnt[i] == 0) c.b.g.random_seeds(c.b.rnd, c.b.seed_size, seeds);
    soff[i + 1] = seeds.size();
  }
  return 0;
}

// ---- 2. insertion searches (searchForNNGInsertion, Index.h:1457-1479) ----------
int search_batch(InsertCall& c, const std::vector<uint32_t>& seeds, const std::vector<uint64_t>& soff) {
  const uint32_t n = c.n;
  if (seeds.empty()) {
    HIP_OK(hipMemsetAsync(c.d_res_n.p, 0, n * sizeof(uint32_t), c.s));
    c.clk.mark(1);
    return 0;
  }
  HIP_OK(c.d_seeds.upload(seeds.data(), seeds.size()));
  HIP_OK(c.d_soff.upload(soff.data(), n + 1));
  const ngt_amd_search_params p = seeded_search_params(c.E, c.b.epsilon_for_creation, FLT_MAX);
  if (ngt_amd_search_device(c.ix, &p, c.d_q.p, c.ix->row_bytes, n, c.d_seeds.p, c.d_soff.p, c.d_res_ids.p,
                            c.d_res_d.p, c.d_res_n.p, c.clk.on ? c.d_cnt.p : nullptr, c.s))
    return -1;
  if (c.clk.on) {
    HIP_OK(hipMemcpyAsync(c.h_cnt.data(), c.d_cnt.p, (size_t)n * NGT_AMD_COUNTERS_PER_QUERY * sizeof(uint64_t),
                          hipMemcpyDeviceToHost, c.s));
    HIP_OK(hipStreamSynchronize(c.s));
    c.k_ms += ngt_amd_last_search_kernel_ms(c.ix);
    uint64_t mx = 0;
    for (uint32_t i = 0; i < n; i++) {
      const uint64_t* q = c.h_cnt.data() + (size_t)i * NGT_AMD_COUNTERS_PER_QUERY;
      for (int j = 0; j < NGT_AMD_COUNTERS_PER_QUERY; j++) c.sum[j] += (double)q[j];
      mx = std::max(mx, q[2]);
      c.c5_max = std::max(c.c5_max, (double)q[5]);
    }
    c.ex_max += (double)mx;
    c.nsearched += n;
  }
  c.clk.mark(1);
  return 0;
}

// ---- 3. pairwise distances inside the batch (Index.cpp:690-703), then the
//      merge / sort / cut of insertMultipleSearchResults (:673-727) ---------------
int merge_batch(InsertCall& c) {
  const uint32_t n = c.n;
  const uint64_t npairs = (uint64_t)n * (n - 1) / 2;
  if (npairs) HIP_OK(c.d_pd.alloc(npairs));
  BatchPairArgs bp{};
  bp.rows = c.ix->rows.p;
  bp.row_bytes = c.ix->row_bytes;
  bp.dp = (int)c.ix->dp;
  bp.batch = c.d_q.p;
  bp.ids = c.d_ids.p;
  bp.n = n;
  bp.out = c.d_pd.p;
  HIP_OK(launch_batch_pairs(bp, c.ix->metric, c.ix->otype, c.s));
  BatchMergeArgs bm{};
  bm.res_ids = c.d_res_ids.p;
  bm.res_dists = c.d_res_d.p;
  bm.res_n = c.d_res_n.p;
  bm.K = c.E;
  bm.ids = c.d_ids.p;
  bm.pair = c.d_pd.p;
  bm.n = n;
  bm.out_ids = c.d_list_ids.p;
  bm.out_dists = c.d_list_d.p;
  bm.out_n = c.d_list_n.p;
  bm.flag = c.d_flag.p;
  HIP_OK(launch_batch_merge(bm, c.s));
  c.clk.mark(2);
  return 0;
}

// ---- 4. DVPTree::insert of the batch, behind the lists' copies to the host.
//      With the leaves step 1 located, the copies are marked by ev_copy: the
//      host graph work waits for that alone and overlaps the insertion. ---------
int tree_insert_batch(InsertCall& c, bool located) {
  const uint32_t n = c.n;
  TreeBuildArgs ta = tree_insert_args(c.ix, c.b, c.d_ids.p, c.d_flag.p, n);
  if (located) {
    ta.pre_leaf = c.descent.pleaf.p;
    ta.pre_count = c.descent.pcnt.p;
    ta.pre_dist = c.descent.pdist.p;
  }
  HIP_OK(hipMemcpyAsync(c.h_list_ids.data(), c.d_list_ids.p, (size_t)n * c.E * sizeof(uint32_t),
                        hipMemcpyDeviceToHost, c.s));
  HIP_OK(hipMemcpyAsync(c.h_list_d.data(), c.d_list_d.p, (size_t)n * c.E * sizeof(float), hipMemcpyDeviceToHost, c.s));
  HIP_OK(hipMemcpyAsync(c.h_list_n.data(), c.d_list_n.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c.s));
  if (located) HIP_OK(hipEventRecord(c.ev_copy, c.s));
  HIP_OK(launch_tree_insert(ta, c.ix->metric, c.ix->otype, c.s));
  return 0;
}

// NeighborhoodGraph::insertNode of the batch's objects in id order, from the
// lists on the host
int store_lists(InsertCall& c, std::vector<uint32_t>& dirty) {
  for (uint32_t i = 0; i < c.n; i++) {
    const uint32_t m = c.h_list_n[i];
    if (c.knng() && m > c.E) return fail("ngt_amd_build_insert: a KNNG list of %u entries", m);
    const std::string e = c.b.g.insert_node(c.ids[i], c.h_list_ids.data() + (size_t)i * c.E,
                                            c.h_list_d.data() + (size_t)i * c.E, m, dirty);
    if (!e.empty()) return fail("%s", e.c_str());
  }
  return 0;
}

// a batch of an ANNG, IANNG or ONNG: steps 1-4 of the header
int insert_batch(InsertCall& c) {
  std::vector<uint32_t> seeds, dirty;
  std::vector<uint64_t> soff;
  if (seed_batch(c, seeds, soff) || search_batch(c, seeds, soff) || merge_batch(c) || tree_insert_batch(c, true))
    return -1;
  c.clk.mark(4);
  HIP_OK(hipEventSynchronize(c.ev_copy));
  if (store_lists(c, dirty)) return -1;
  c.clk.mark(3);
  // refresh the padded adjacency of the touched nodes
  const std::vector<uint32_t> vals = c.b.g.adjacency_rows(dirty);
  HIP_OK(c.d_dirty.upload(dirty.data(), dirty.size()));
  HIP_OK(c.d_vals.upload(vals.data(), vals.size()));
  HIP_OK(launch_adj_scatter(c.ix->adj.p, c.b.g.adj_stride, c.d_dirty.p, c.d_vals.p, (uint32_t)dirty.size(), c.s));
  c.ix->adj_version++;
  if (finish_batch(c.ix, c.b, c.s)) return -1;
  c.clk.mark(5);
  return 0;
}

// a batch of a KNNG: steps a-c of the header
int insert_batch_knng(InsertCall& c) {
  ngt_amd_index* ix = c.ix;
  const uint32_t n = c.n, K1 = c.E + 1;
  const uint64_t rb = ix->row_bytes;
  // ---- a. the exact E + 1 nearest: the stored rows are the queries ------------
  const uint8_t* q = ix->rows.p + (uint64_t)c.ids[0] * rb;
  if (c.ids[n - 1] - c.ids[0] != n - 1) {  // removed rows in between: the batch's rows side by side
    HIP_OK(c.d_q.alloc((size_t)n * rb));
    HIP_OK(launch_gather_rows(c.d_q.p, ix->rows.p, rb, c.d_ids.p, n, c.s));
    q = c.d_q.p;
  }
  if (ngt_amd_linear_search_device(ix, q, rb, n, K1, (double)FLT_MAX, c.d_res_ids.p, c.d_res_d.p, c.d_res_n.p, c.s))
    return -1;
  c.clk.mark(0);
  // ---- b. moveFrom, the lists, the adjacency rows, the tree flags --------------
  KnngListArgs ka{};
  ka.res_ids = c.d_res_ids.p;
  ka.res_dists = c.d_res_d.p;
  ka.res_n = c.d_res_n.p;
  ka.K1 = K1;
  ka.ids = c.d_ids.p;
  ka.n = n;
  ka.out_ids = c.d_list_ids.p;
  ka.out_dists = c.d_list_d.p;
  ka.out_n = c.d_list_n.p;
  ka.flag = c.d_flag.p;
  ka.adj = ix->adj.p;
  ka.adj_stride = c.b.g.adj_stride;
  HIP_OK(launch_knng_lists(ka, c.s));
  // ---- c. DVPTree::insert of the batch, from the root ----------------------------
  if (tree_insert_batch(c, false)) return -1;
  ix->adj_version++;
  if (finish_batch(ix, c.b, c.s)) return -1;
  c.clk.mark(1);
  std::vector<uint32_t> dirty;  // stays empty: the kernel wrote the adjacency rows
  if (store_lists(c, dirty)) return -1;
  c.clk.mark(2);
  return 0;
}

}  // namespace

extern "C" int ngt_amd_build_insert(ngt_amd_index* ix, uint64_t first_id, uint64_t end_id) {
  if (!ix || !ix->build) return fail("ngt_amd_build_insert: call ngt_amd_build_begin first");
  HIP_OK(hipSetDevice(ix->device));
  ServeHold serve_hold(ix);
  // the insertion searches never rebuild the padded adjacency this call keeps
  // changing: build_begin set max_degree = adj_stride, so the copy always
  // holds every edge they read
  BuildState& b = *ix->build;
  if (end_id > ix->nrows) end_id = ix->nrows;
  if (first_id < 1) first_id = 1;
  std::vector<uint32_t> todo;
  for (uint64_t id = first_id; id < end_id; id++)
    if (ix->h_valid[id] && !b.g.in_graph[id]) todo.push_back((uint32_t)id);
  InsertCall c(ix, b);
  if (c.alloc()) return -1;
  for (size_t pos = 0; pos < todo.size(); pos += c.B) {
    c.ids = todo.data() + pos;
    c.n = (uint32_t)std::min<size_t>(c.B, todo.size() - pos);
    if (ensure_tree_capacity(ix, b, 4 * c.n + 4, c.n + 1)) return -1;
    HIP_OK(hipMemcpyAsync(c.d_ids.p, c.ids, c.n * sizeof(uint32_t), hipMemcpyHostToDevice, c.s));
    if (c.knng() ? insert_batch_knng(c) : insert_batch(c)) return -1;
  }
  if (!c.clk.on) return 0;
  const double* st = c.clk.st;
  if (c.knng()) {
    fprintf(stderr, "build_insert KNNG %zu objects: scan %.3f s, lists + tree insert %.3f s, host graph %.3f s\n",
            todo.size(), st[0], st[1], st[2]);
    return 0;
  }
  const double nq = (double)std::max<uint64_t>(c.nsearched, 1);
  fprintf(stderr, "build_insert %zu objects: seeds %.3f s, search %.3f s, pairs+merge %.3f s, host graph %.3f s, "
          "tree insert %.3f s, adjacency %.3f s; search kernel %.3f s, per query %.1f distances %.1f expansions, "
          "mean per-batch max expansions %.1f\n", todo.size(), st[0], st[1], st[2], st[3], st[4], st[5], c.k_ms / 1e3,
          c.sum[0] / nq, c.sum[2] / nq, c.ex_max / std::max<double>(1.0, (double)((todo.size() + c.B - 1) / c.B)));
  // counters [3], [5..7]: spilled-visited flag, max unchecked, 0, 0 -- or, in
  // the NGT_AMD_STAMPS build, rest/pop/adjacency/eval cycles
  fprintf(stderr, "build_insert counters per query: c3 %.4g c5 %.4g (max %.4g) c6 %.4g c7 %.4g\n", c.sum[3] / nq,
          c.sum[5] / nq, c.c5_max, c.sum[6] / nq, c.sum[7] / nq);
  return 0;
}

extern "C" int ngt_amd_build_set_graph(ngt_amd_index* ix, const uint64_t* offsets, const uint32_t* ids,
                                       const float* dists, uint64_t graph_rows) {
  if (!ix || !ix->build || !offsets || graph_rows > ix->nrows) return fail("ngt_amd_build_set_graph: bad arguments");
  if (offsets[graph_rows] && (!ids || !dists)) return fail("ngt_amd_build_set_graph: bad arguments");
  HIP_OK(hipSetDevice(ix->device));
  ServeHold serve_hold(ix);
  SessionGraph& g = ix->build->g;
  const std::string e = g.set_csr(offsets, ids, dists, graph_rows);
  if (!e.empty()) return fail("%s", e.c_str());
  std::vector<uint32_t> every(ix->nrows);
  for (uint64_t v = 0; v < ix->nrows; v++) every[v] = (uint32_t)v;
  const std::vector<uint32_t> adj = g.adjacency_rows(every);
  HIP_OK(hipMemcpy(ix->adj.p, adj.data(), adj.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  ix->adj_version++;
  return 0;
}

extern "C" int ngt_amd_build_set_tree(ngt_amd_index* ix, const uint32_t* leaf_parent, const uint64_t* leaf_off,
                                      const uint32_t* leaf_ids, const float* leaf_dists,
                                      const uint8_t* leaf_has_pivot, const void* leaf_pivot, uint32_t n_leaf,
                                      const uint32_t* in_parent, const void* in_pivot, const uint32_t* in_child,
                                      const float* in_border, uint32_t n_internal, uint32_t root) {
  if (!ix || !ix->build || !leaf_parent || !leaf_off || !leaf_has_pivot || !leaf_pivot || n_leaf < 2 ||
      n_internal < 1 || (n_internal > 1 && (!in_parent || !in_pivot || !in_child || !in_border)))
    return fail("ngt_amd_build_set_tree: bad arguments");
  HIP_OK(hipSetDevice(ix->device));
  BuildState& b = *ix->build;
  b.n_leaf = 2;
  b.n_internal = 1;
  if (ensure_tree_capacity(ix, b, n_leaf, n_internal)) return -1;
  const uint64_t rb = ix->row_bytes;
  std::vector<uint32_t> cnt(n_leaf), lids((size_t)n_leaf * kLeafCap, 0u);
  std::vector<float> ldst((size_t)n_leaf * kLeafCap, 0.f);
  for (uint32_t l = 0; l < n_leaf; l++) {
    const uint64_t c = leaf_off[l + 1] - leaf_off[l];
    if (c > kLeafCap - 1) return fail("ngt_amd_build_set_tree: leaf %u holds %llu objects", l, (unsigned long long)c);
    cnt[l] = (uint32_t)c;
    for (uint64_t j = 0; j < c; j++) {
      lids[(size_t)l * kLeafCap + j] = leaf_ids[leaf_off[l] + j];
      ldst[(size_t)l * kLeafCap + j] = leaf_dists ? leaf_dists[leaf_off[l] + j] : 0.f;
    }
  }
  HIP_OK(hipMemcpy(b.lf_count.p, cnt.data(), n_leaf * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(b.lf_ids.p, lids.data(), lids.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(b.lf_dist.p, ldst.data(), ldst.size() * sizeof(float), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(b.lf_parent.p, leaf_parent, n_leaf * sizeof(uint32_t), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(b.lf_has_pivot.p, leaf_has_pivot, n_leaf, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(b.lf_pivot.p, leaf_pivot, (size_t)n_leaf * rb, hipMemcpyHostToDevice));
  if (n_internal > 1) {
    HIP_OK(hipMemcpy(b.in_parent.p, in_parent, n_internal * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(b.in_pivot.p, in_pivot, (size_t)n_internal * rb, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(b.in_child.p, in_child, (size_t)n_internal * 5 * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(b.in_border.p, in_border, (size_t)n_internal * 4 * sizeof(float), hipMemcpyHostToDevice));
  }
  const uint32_t c3[3] = {n_leaf, n_internal, root};
  HIP_OK(b.counts.upload(c3, 3));
  b.n_leaf = n_leaf;
  b.n_internal = n_internal;
  b.root = root;
  return 0;
}

// ---- object removal ---------------------------------------------------------
// GraphAndTreeIndex::remove (lib/NGT/Index.h:1386-1455) on the session's graph
// and tree: the duplicate search (the graph-search kernel seeded with the
// object itself), DVPTree::remove / replace on the leaf the object descends to
// (the tree-seed kernel's descent; the leaf row is edited on the host), and
// NeighborhoodGraph::removeEdgesReliably (Graph.cpp:641-864, NGT_FORCED_REMOVE)
// on the host lists with the relink chain computed by remove_kernels.hip.
namespace {

uint32_t remove_fast_cap() {
  uint32_t cap = removal::kFastCap;
  if (const char* v = ngt_amd::knob("NGT_AMD_REMOVE_FAST_CAP")) cap = std::min<uint32_t>(cap, (uint32_t)std::max(0, atoi(v)));
  return cap;
}

// the relink chain over the rows of nbr[0..d) (host ids, each a stored row);
// without `wait` the links arrive once the index's stream is synchronised
int relink(ngt_amd_index* ix, RemoveScratch& sc, const uint32_t* nbr, uint32_t d, uint32_t* la, uint32_t* lb,
           float* ld, bool wait) {
  if (d < 2) return 0;
  if (d > removal::kMaxList)
    return fail("ngt_amd_remove_relink: a list of %u neighbours exceeds the supported %u", d, removal::kMaxList);
  hipStream_t s = ix->stream;
  HIP_OK(sc.ids.upload_async(nbr, d, s));
  HIP_OK(sc.la.alloc(d - 1));
  HIP_OK(sc.lb.alloc(d - 1));
  HIP_OK(sc.ld.alloc(d - 1));
  removal::RelinkArgs a{};
  a.rows = ix->rows.p;
  a.row_bytes = ix->row_bytes;
  a.dp = (int)ix->dp;
  a.ids = sc.ids.p;
  a.d = d;
  a.link_a = sc.la.p;
  a.link_b = sc.lb.p;
  a.link_dist = sc.ld.p;
  if (removal::fast_lds_bytes(d, ix->row_bytes, remove_fast_cap())) {
    HIP_OK(removal::launch_relink_fast(a, ix->metric, ix->otype, s));
  } else {
    HIP_OK(sc.matrix.alloc((size_t)d * d));
    a.matrix = sc.matrix.p;
    HIP_OK(removal::launch_relink_matrix(a, ix->metric, ix->otype, s));
  }
  HIP_OK(hipMemcpyAsync(la, sc.la.p, (d - 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(lb, sc.lb.p, (d - 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(ld, sc.ld.p, (d - 1) * sizeof(float), hipMemcpyDeviceToHost, s));
  if (wait) HIP_OK(hipStreamSynchronize(s));
  return 0;
}

int drop_object(ngt_amd_index* ix, uint32_t id) {
  const uint8_t zero = 0;
  ix->h_valid[id] = 0;
  HIP_OK(hipMemcpy(ix->valid.p + id, &zero, 1, hipMemcpyHostToDevice));
  ix->rows_version++;
  return 0;
}

// a removal refused before anything changed
int refuse(const std::string& why) {
  fail("%s", why.c_str());
  return 2;
}

// DVPTree::remove / replace (Tree.h:178-202, Node.cpp:229-280) on the leaf the
// object descended to: 0 done, 2 refused, -1 device failure
int edit_leaf(BuildState& b, uint32_t id, uint32_t replace_id, uint32_t leaf, uint32_t cnt) {
  if (leaf == 0 || leaf >= b.n_leaf || cnt >= kLeafCap)
    return fail("ngt_amd_build_remove: the tree descent of %u ended at leaf %u with %u objects", id, leaf, cnt);
  uint32_t lids[kLeafCap];
  float ldst[kLeafCap];
  if (cnt) {
    HIP_OK(hipMemcpy(lids, b.lf_ids.p + (size_t)leaf * kLeafCap, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(ldst, b.lf_dist.p + (size_t)leaf * kLeafCap, cnt * sizeof(float), hipMemcpyDeviceToHost));
  }
  uint32_t at = 0;
  while (at < cnt && lids[at] != id) at++;
  if (replace_id != 0) {
    // the duplicate takes the leaf entry; a leaf without the entry is ignored (Index.h:1448-1452)
    if (at < cnt)
      HIP_OK(hipMemcpy(b.lf_ids.p + (size_t)leaf * kLeafCap + at, &replace_id, sizeof(uint32_t), hipMemcpyHostToDevice));
    return 0;
  }
  if (at == cnt) {
    fail("remove:: cannot remove from tree. id=%u VpTree::remove: Inner error. Cannot remove object. leafNode=%u:"
         "VpTree::Leaf::remove: Warning. Cannot find the specified object. ID=%u,0 idx=%u If the same objects "
         "were inserted into the index, ignore this message.", id, leaf, id, at);
    return 2;
  }
  for (uint32_t j = at; j + 1 < cnt; j++) {
    lids[j] = lids[j + 1];
    ldst[j] = ldst[j + 1];
  }
  cnt--;
  if (cnt > at) {
    HIP_OK(hipMemcpy(b.lf_ids.p + (size_t)leaf * kLeafCap + at, lids + at, (cnt - at) * sizeof(uint32_t),
                     hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(b.lf_dist.p + (size_t)leaf * kLeafCap + at, ldst + at, (cnt - at) * sizeof(float),
                     hipMemcpyHostToDevice));
  }
  HIP_OK(hipMemcpy(b.lf_count.p + leaf, &cnt, sizeof(uint32_t), hipMemcpyHostToDevice));
  // an emptied leaf stays in place; the collapse of an all-empty subtree
  // (removeEmptyNodes, Tree.cpp:338-397) is not reproduced
  return 0;
}

// 0 removed, 1 no such object, 2 refused (nothing changed), -1 device failure
// clk: seconds spent enqueueing, waiting, on the leaf, on the lists, on the adjacency
int remove_one(ngt_amd_index* ix, BuildState& b, RemoveScratch& sc, uint32_t id, StageClock& clk) {
  clk.start();
  SessionGraph& g = b.g;
  hipStream_t s = ix->stream;
  const uint64_t rb = ix->row_bytes;
  if (id == 0 || id >= ix->nrows || !ix->h_valid[id]) {
    fail("get: Not in-memory or invalid offset of node. idx=%u size=%llu", id, (unsigned long long)ix->nrows);
    return 1;
  }
  if (!g.has_node(ix->h_valid, id)) return drop_object(ix, id);  // Index.h:1411-1422

  // Nothing is edited before every check: the lists the duplicate search
  // expands -- the node's own and, below, its duplicate's -- and the
  // neighbours to relink.
  std::string e = g.evaluated_edges_exist(ix->h_valid, id, b.edge_size_for_search);
  if (!e.empty()) return refuse(e);
  std::vector<uint32_t> nbr;
  std::vector<float> nbr_d;
  e = g.removal_neighbours(ix->h_valid, id, nbr, nbr_d);
  if (!e.empty()) return refuse(e);
  const uint32_t d = (uint32_t)nbr.size();
  if (d > removal::kMaxList) {
    fail("ngt_amd_build_remove: node %u has %u neighbours, more than the supported %u", id, d, removal::kMaxList);
    return 2;
  }

  // ---- the duplicate search (Index.h:1423-1432) ---------------------------
  const uint8_t* d_row = ix->rows.p + (uint64_t)id * rb;
  const uint64_t soff[2] = {0, 1};
  HIP_OK(sc.seed.upload_async(&id, 1, s));
  HIP_OK(sc.soff.upload_async(soff, 2, s));
  HIP_OK(sc.oi.alloc(2));
  HIP_OK(sc.od.alloc(2));
  HIP_OK(sc.on.alloc(1));
  const ngt_amd_search_params p = seeded_search_params(2, 0.1f, 0.0f);
  if (ngt_amd_search_device(ix, &p, d_row, rb, 1, sc.seed.p, sc.soff.p, sc.oi.p, sc.od.p, sc.on.p, nullptr, s))
    return -1;
  uint32_t found[2] = {0, 0}, nfound = 0;
  HIP_OK(hipMemcpyAsync(found, sc.oi.p, sizeof found, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(&nfound, sc.on.p, sizeof nfound, hipMemcpyDeviceToHost, s));

  // ---- the descent to the object's leaf (Tree.h:156-176) and the relink
  //      chain of the neighbours, behind the search on the same stream: the
  //      three need nothing from one another, so one wait serves them all ----
  if (alloc_descent(sc.descent, 1)) return -1;
  TreeSeedArgs t = tree_descent_args(ix, b, d_row, 1, sc.descent);
  t.seed_size = 1;
  t.k = 1;
  t.all_leaf_nodes = 0;
  HIP_OK(launch_tree_seeds(t, ix->metric, ix->otype, s));
  uint32_t leaf = 0, cnt = 0;
  HIP_OK(hipMemcpyAsync(&leaf, sc.descent.pleaf.p, sizeof leaf, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(&cnt, sc.descent.pcnt.p, sizeof cnt, hipMemcpyDeviceToHost, s));
  std::vector<uint32_t> la(d ? d - 1 : 0), lb(d ? d - 1 : 0);
  std::vector<float> ld(d ? d - 1 : 0);
  if (relink(ix, sc, nbr.data(), d, la.data(), lb.data(), ld.data(), false)) return -1;
  int serr = 0;
  clk.mark(0);
  if (take_device_error(ix, s, &serr)) return -1;
  if (serr) return fail("ngt_amd_build_remove: device error flag %d in the duplicate search", serr);
  if (nfound == 0) {
    fail("Not found the specified id");
    return 2;
  }
  const uint32_t replace_id = nfound == 1 ? 0u : (found[0] == id ? found[1] : found[0]);
  if (replace_id != 0) {
    if (replace_id >= ix->nrows) return 2;
    e = g.evaluated_edges_exist(ix->h_valid, replace_id, b.edge_size_for_search);
    if (!e.empty()) return refuse(e);
  }
  clk.mark(1);

  if (const int r = edit_leaf(b, id, replace_id, leaf, cnt)) return r;
  clk.mark(2);

  // ---- removeEdgesReliably on the host lists, the padded adjacency of the
  //      touched nodes, the object ------------------------------------------------
  std::vector<uint32_t> dirty;
  g.apply_removal(id, nbr, nbr_d, la.data(), lb.data(), ld.data(), dirty);
  clk.mark(3);
  const std::vector<uint32_t> vals = g.adjacency_rows(dirty);
  HIP_OK(sc.dirty.upload_async(dirty.data(), dirty.size(), s));
  HIP_OK(sc.vals.upload_async(vals.data(), vals.size(), s));
  HIP_OK(launch_adj_scatter(ix->adj.p, g.adj_stride, sc.dirty.p, sc.vals.p, (uint32_t)dirty.size(), s));
  HIP_OK(hipStreamSynchronize(s));
  ix->adj_version++;
  b.longest_removed_list = std::max<uint64_t>(b.longest_removed_list, d);
  clk.mark(4);
  return drop_object(ix, id);
}

}  // namespace

extern "C" uint32_t ngt_amd_remove_fast_path_capacity(void) { return removal::kFastCap; }

extern "C" int ngt_amd_remove_relink(ngt_amd_index* ix, const uint32_t* nbr_ids, uint32_t d, uint32_t* link_a,
                                     uint32_t* link_b, float* link_dist) {
  if (!ix || (d && !nbr_ids) || (d > 1 && (!link_a || !link_b || !link_dist)))
    return fail("ngt_amd_remove_relink: bad arguments");
  if (ix->nrows == 0 || !ix->rows.p) return fail("ngt_amd_remove_relink: set the objects first");
  for (uint32_t i = 0; i < d; i++)
    if (nbr_ids[i] == 0 || nbr_ids[i] >= ix->nrows)
      return fail("ngt_amd_remove_relink: id %u out of range", nbr_ids[i]);
  HIP_OK(hipSetDevice(ix->device));
  RemoveScratch sc;
  return relink(ix, sc, nbr_ids, d, link_a, link_b, link_dist, true);
}

extern "C" int ngt_amd_build_remove(ngt_amd_index* ix, const uint32_t* ids, uint64_t n, uint8_t* status) {
  if (!ix || !ix->build || (n && (!ids || !status))) return fail("ngt_amd_build_remove: bad arguments");
  HIP_OK(hipSetDevice(ix->device));
  ServeHold serve_hold(ix);
  BuildState& b = *ix->build;
  RemoveScratch& sc = b.remove_scratch;  // no allocation per id once warm
  StageClock clk;  // no stream: the stages are timed as the host sees them
  for (uint64_t i = 0; i < n; i++) {
    const int r = remove_one(ix, b, sc, ids[i], clk);
    if (r < 0) return -1;
    status[i] = (uint8_t)r;
  }
  if (clk.on)
    fprintf(stderr, "build_remove %llu ids: enqueue %.3f s, wait %.3f s, leaf %.3f s, lists %.3f s, adjacency and "
            "flag %.3f s\n", (unsigned long long)n, clk.st[0], clk.st[1], clk.st[2], clk.st[3], clk.st[4]);
  return 0;
}

extern "C" uint64_t ngt_amd_build_longest_removed_list(const ngt_amd_index* ix) {
  return ix && ix->build ? ix->build->longest_removed_list : 0;
}

extern "C" int ngt_amd_build_graph_size(const ngt_amd_index* ix, uint64_t* graph_size, uint64_t* nedges) {
  if (!ix || !ix->build || !graph_size || !nedges) return fail("ngt_amd_build_graph_size: bad arguments");
  *graph_size = ix->build->g.graph_size;
  *nedges = ix->build->g.edge_count();
  return 0;
}

extern "C" int ngt_amd_build_get_graph(const ngt_amd_index* ix, uint64_t* offsets, uint32_t* ids, float* dists) {
  if (!ix || !ix->build || !offsets) return fail("ngt_amd_build_get_graph: bad arguments");
  ix->build->g.get_csr(offsets, ids, dists);
  return 0;
}

int ngt_amd::build_graph_to_host(const ngt_amd_index* ix, uint64_t nrows, std::vector<uint64_t>& off,
                                 std::vector<uint32_t>& ids, std::vector<float>& dists) {
  uint64_t gsize = 0, ne = 0;
  if (ngt_amd_build_graph_size(ix, &gsize, &ne)) return -1;
  std::vector<uint64_t> o(gsize + 1);
  ids.resize(ne);
  dists.resize(ne);
  if (ngt_amd_build_get_graph(ix, o.data(), ids.data(), dists.data())) return -1;
  off.assign(nrows + 1, ne);
  for (uint64_t v = 0; v <= nrows && v <= gsize; v++) off[v] = o[v];
  return 0;
}

void ngt_amd::build_mark_nodes(ngt_amd_index* ix, const std::vector<uint8_t>& node, uint64_t rows) {
  for (uint64_t v = 0; v < rows; v++)
    if (node[v]) ix->build->g.mark_node(v);
}

const std::vector<uint8_t>& ngt_amd::build_nodes(const ngt_amd_index* ix) { return ix->build->g.in_graph; }

GlibcRandHost& ngt_amd::build_rand(ngt_amd_index* ix) { return ix->build->rnd; }

uint32_t ngt_amd::build_root(const ngt_amd_index* ix) { return ix->build->root; }

extern "C" int ngt_amd_build_tree_size(const ngt_amd_index* ix, uint32_t* n_leaf, uint32_t* n_internal,
                                       uint64_t* n_leaf_ids) {
  if (!ix || !ix->build || !n_leaf || !n_internal || !n_leaf_ids) return fail("ngt_amd_build_tree_size: bad arguments");
  const BuildState& b = *ix->build;
  HIP_OK(hipSetDevice(ix->device));
  std::vector<uint32_t> cnt(b.n_leaf);
  HIP_OK(hipMemcpy(cnt.data(), b.lf_count.p, b.n_leaf * sizeof(uint32_t), hipMemcpyDeviceToHost));
  uint64_t t = 0;
  for (uint32_t i = 1; i < b.n_leaf; i++) t += cnt[i];
  *n_leaf = b.n_leaf;
  *n_internal = b.n_internal;
  *n_leaf_ids = t;
  return 0;
}

extern "C" int ngt_amd_build_get_tree(const ngt_amd_index* ix, uint32_t* leaf_parent, uint64_t* leaf_off,
                                      uint32_t* leaf_ids, float* leaf_dists, uint8_t* leaf_has_pivot,
                                      void* leaf_pivot, uint32_t* in_parent, void* in_pivot, uint32_t* in_child,
                                      float* in_border) {
  if (!ix || !ix->build || !leaf_parent || !leaf_off || !leaf_has_pivot || !leaf_pivot || !in_parent ||
      !in_pivot || !in_child || !in_border)
    return fail("ngt_amd_build_get_tree: bad arguments");
  const BuildState& b = *ix->build;
  HIP_OK(hipSetDevice(ix->device));
  const uint64_t rb = ix->row_bytes;
  const uint32_t nl = b.n_leaf, ni = b.n_internal;
  std::vector<uint32_t> cnt(nl), lids((size_t)nl * kLeafCap);
  std::vector<float> ldst((size_t)nl * kLeafCap);
  HIP_OK(hipMemcpy(cnt.data(), b.lf_count.p, nl * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(lids.data(), b.lf_ids.p, lids.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(ldst.data(), b.lf_dist.p, ldst.size() * sizeof(float), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(leaf_parent, b.lf_parent.p, nl * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(leaf_has_pivot, b.lf_has_pivot.p, nl, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(leaf_pivot, b.lf_pivot.p, (size_t)nl * rb, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(in_parent, b.in_parent.p, ni * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(in_pivot, b.in_pivot.p, (size_t)ni * rb, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(in_child, b.in_child.p, (size_t)ni * 5 * sizeof(uint32_t), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(in_border, b.in_border.p, (size_t)ni * 4 * sizeof(float), hipMemcpyDeviceToHost));
  uint64_t e = 0;
  leaf_off[0] = 0;
  for (uint32_t i = 0; i < nl; i++) {
    const uint32_t c = i == 0 ? 0 : cnt[i];
    for (uint32_t j = 0; j < c; j++) {
      if (leaf_ids) leaf_ids[e] = lids[(size_t)i * kLeafCap + j];
      if (leaf_dists) leaf_dists[e] = ldst[(size_t)i * kLeafCap + j];
      e++;
    }
    leaf_off[i + 1] = e;
  }
  return 0;
}

int ngt_amd::build_tree_to_host(const ngt_amd_index* ix, uint64_t row_bytes, HostTree& t) {
  uint32_t nl = 0, ni = 0;
  uint64_t nli = 0;
  if (ngt_amd_build_tree_size(ix, &nl, &ni, &nli)) return -1;
  t.leaf_parent.resize(nl);
  t.leaf_off.resize((size_t)nl + 1);
  t.leaf_ids.resize(nli);
  t.leaf_dists.resize(nli);
  t.leaf_has_pivot.resize(nl);
  t.leaf_pivot.resize((size_t)nl * row_bytes);
  t.in_parent.resize(ni);
  t.in_pivot.resize((size_t)ni * row_bytes);
  t.in_child.resize((size_t)ni * 5);
  t.in_border.resize((size_t)ni * 4);
  return ngt_amd_build_get_tree(ix, t.leaf_parent.data(), t.leaf_off.data(), t.leaf_ids.data(), t.leaf_dists.data(),
                                t.leaf_has_pivot.data(), t.leaf_pivot.data(), t.in_parent.data(), t.in_pivot.data(),
                                t.in_child.data(), t.in_border.data());
}

int ngt_amd::build_tree_from_host(ngt_amd_index* ix, const HostTree& t, uint32_t n_internal, uint32_t root) {
  return ngt_amd_build_set_tree(ix, t.leaf_parent.data(), t.leaf_off.data(), t.leaf_ids.data(), t.leaf_dists.data(),
                                t.leaf_has_pivot.data(), t.leaf_pivot.data(), (uint32_t)t.leaf_parent.size(),
                                t.in_parent.data(), t.in_pivot.data(), t.in_child.data(), t.in_border.data(),
                                n_internal, root);
}
