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
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "../../include/ngt_amd.h"
#include "index_internal.h"
#include "index_io.h"
#include "ngt_kernels.h"
#include "remove_kernels.h"

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

bool od_less(const std::pair<uint32_t, float>& a, const std::pair<uint32_t, float>& b) {
  // ObjectDistance::operator< (Common.h:1946-1952): distance, then id
  if (a.second != b.second) return a.second < b.second;
  return a.first < b.first;
}

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
  b->edge_size_for_creation = prm->edge_size_for_creation;
  b->edge_size_for_search = prm->edge_size_for_search;
  b->batch_size = prm->batch_size_for_creation;
  b->seed_size = prm->seed_size;
  b->epsilon_for_creation = prm->epsilon_for_creation;
  b->graph_type = prm->graph_type == 0 ? NGT_AMD_GRAPH_ANNG : prm->graph_type;
  if (b->graph_type != NGT_AMD_GRAPH_ANNG && b->graph_type != NGT_AMD_GRAPH_KNNG &&
      b->graph_type != NGT_AMD_GRAPH_ONNG && b->graph_type != NGT_AMD_GRAPH_IANNG)
    return fail("ngt_amd_build_begin: graph type %d unsupported (ANNG 1, KNNG 2, ONNG 4 and IANNG 5 are built)",
                prm->graph_type);
  b->graph.assign(ix->nrows, {});
  b->in_graph.assign(ix->nrows, 0);
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
  b->adj_stride = es == 0 ? 256 : (uint64_t)((es + 15) / 16 * 16);
  HIP_OK(ix->adj.alloc((size_t)ix->nrows * b->adj_stride));
  HIP_OK(hipMemset(ix->adj.p, 0, (size_t)ix->nrows * b->adj_stride * sizeof(uint32_t)));
  ix->adj_stride = b->adj_stride;
  ix->adj_version++;
  // the construction's searches read at most adj_stride edges of a list: the
  // padded copy is always the one to use (run_search never rebuilds it here)
  ix->max_degree = b->adj_stride;
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
  ix->build->outgoing_edge = outgoing_edge;
  ix->build->incoming_edge = incoming_edge;
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

// KNNG: steps a-c of the header for the objects of `todo`, in id order.
int insert_knng(ngt_amd_index* ix, BuildState& b, const std::vector<uint32_t>& todo) {
  hipStream_t s = ix->stream;
  const uint64_t rb = ix->row_bytes;
  const uint32_t B = (uint32_t)b.batch_size, E = (uint32_t)b.edge_size_for_creation, K1 = E + 1;
  DevBuf<uint32_t> d_ids, d_ri, d_rn, d_li, d_ln;
  DevBuf<float> d_rd, d_ld;
  DevBuf<uint8_t> d_q, d_flag;
  HIP_OK(d_ids.alloc(B));
  HIP_OK(d_ri.alloc((size_t)B * K1));
  HIP_OK(d_rd.alloc((size_t)B * K1));
  HIP_OK(d_rn.alloc(B));
  HIP_OK(d_li.alloc((size_t)B * E));
  HIP_OK(d_ld.alloc((size_t)B * E));
  HIP_OK(d_ln.alloc(B));
  HIP_OK(d_flag.alloc(B));
  std::vector<uint32_t> h_li((size_t)B * E), h_ln(B);
  std::vector<float> h_ld((size_t)B * E);
  // NGT_AMD_BUILD_PROFILE=1: per-stage wall time (stream synchronised at each mark)
  const bool prof = ngt_amd::knob("NGT_AMD_BUILD_PROFILE") != nullptr;
  double st[3] = {0, 0, 0};
  auto t_last = std::chrono::steady_clock::now();
  auto mark = [&](int i) {
    if (!prof) return;
    (void)hipStreamSynchronize(s);
    auto t = std::chrono::steady_clock::now();
    st[i] += std::chrono::duration<double>(t - t_last).count();
    t_last = t;
  };
  for (size_t pos = 0; pos < todo.size(); pos += B) {
    const uint32_t n = (uint32_t)std::min<size_t>(B, todo.size() - pos);
    const uint32_t* ids = todo.data() + pos;
    if (ensure_tree_capacity(ix, b, 4 * n + 4, n + 1)) return -1;
    HIP_OK(hipMemcpyAsync(d_ids.p, ids, n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    // ---- a. the exact E + 1 nearest: the stored rows are the queries ----------
    const uint8_t* q = ix->rows.p + (uint64_t)ids[0] * rb;
    if (ids[n - 1] - ids[0] != n - 1) {  // removed rows in between: the batch's rows side by side
      HIP_OK(d_q.alloc((size_t)n * rb));
      HIP_OK(launch_gather_rows(d_q.p, ix->rows.p, rb, d_ids.p, n, s));
      q = d_q.p;
    }
    if (ngt_amd_linear_search_device(ix, q, rb, n, K1, (double)FLT_MAX, d_ri.p, d_rd.p, d_rn.p, s)) return -1;
    mark(0);
    // ---- b. moveFrom, the lists, the adjacency rows, the tree flags ------------
    KnngListArgs ka{};
    ka.res_ids = d_ri.p;
    ka.res_dists = d_rd.p;
    ka.res_n = d_rn.p;
    ka.K1 = K1;
    ka.ids = d_ids.p;
    ka.n = n;
    ka.out_ids = d_li.p;
    ka.out_dists = d_ld.p;
    ka.out_n = d_ln.p;
    ka.flag = d_flag.p;
    ka.adj = ix->adj.p;
    ka.adj_stride = b.adj_stride;
    HIP_OK(launch_knng_lists(ka, s));
    HIP_OK(hipMemcpyAsync(h_li.data(), d_li.p, (size_t)n * E * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(h_ld.data(), d_ld.p, (size_t)n * E * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(h_ln.data(), d_ln.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    // ---- c. DVPTree::insert of the batch, from the root --------------------------
    HIP_OK(launch_tree_insert(tree_insert_args(ix, b, d_ids.p, d_flag.p, n), ix->metric, ix->otype, s));
    ix->adj_version++;
    if (finish_batch(ix, b, s)) return -1;
    mark(1);
    // ---- insertKNNGNode (Graph.h:607-609): the graph mirror ----------------------
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t id = ids[i];
      if (h_ln[i] > E) return fail("ngt_amd_build_insert: a KNNG list of %u entries", h_ln[i]);
      auto& objs = b.graph[id];
      objs.resize(h_ln[i]);
      for (uint32_t j = 0; j < h_ln[i]; j++) objs[j] = {h_li[(size_t)i * E + j], h_ld[(size_t)i * E + j]};
      b.in_graph[id] = 1;
      b.graph_size = std::max<uint64_t>(b.graph_size, (uint64_t)id + 1);
    }
    mark(2);
  }
  if (prof)
    fprintf(stderr, "build_insert KNNG %zu objects: scan %.3f s, lists + tree insert %.3f s, host graph %.3f s\n",
            todo.size(), st[0], st[1], st[2]);
  return 0;
}

// The reverse edge target <- (id, distance) of insertANNGNode / insertONNGNode:
// the sorted addEdge with the identity check (Graph.h:845-873).
int add_edge(BuildState& b, uint32_t target, uint32_t id, float distance, std::vector<uint32_t>& dirty) {
  auto& node = b.graph[target];
  const std::pair<uint32_t, float> e{id, distance};
  auto it = std::lower_bound(node.begin(), node.end(), e, od_less);
  if (it != node.end() && it->first == id) return fail("NGT::addEdge: already existed! %u:%u", it->first, id);
  if ((uint64_t)(it - node.begin()) < b.adj_stride) dirty.push_back(target);
  node.insert(it, e);
  return 0;
}

// addEdgeDeletingExcessEdges (Graph.h:888-934)
int add_edge_deleting_excess(BuildState& b, uint32_t target, uint32_t id, float distance,
                             std::vector<uint32_t>& dirty) {
  auto& node = b.graph[target];
  const size_t k_edge = (size_t)b.edge_size_for_creation - 1;
  if (node.size() > k_edge && node[k_edge].second >= distance) {
    const std::pair<uint32_t, float> last = node[k_edge];
    if (last.first >= b.graph.size() || !b.in_graph[last.first])
      return fail("get: Not in-memory or invalid offset of node. idx=%u size=%zu", last.first, b.graph.size());
    auto& linked = b.graph[last.first];
    if (linked.size() > k_edge && last.second >= linked[k_edge].second) {
      node.erase(node.begin() + k_edge);
      if (k_edge < b.adj_stride) dirty.push_back(target);
      const std::pair<uint32_t, float> back{target, last.second};
      auto it = std::lower_bound(linked.begin(), linked.end(), back, od_less);
      if (it == linked.end() || it->first != target) {
        char found[48] = "";
        if (it != linked.end()) snprintf(found, sizeof found, "%u:", it->first);
        // the reference prints the edge now at that rank of the shortened list
        const std::pair<uint32_t, float> now = node.size() > k_edge ? node[k_edge] : std::pair<uint32_t, float>{0u, 0.f};
        return fail("addEdge: Cannot remove. (b) %u,%u,%u,%g:NGT::removeEdge: Cannot found %s%u", target, id,
                    now.first, now.second, found, target);
      }
      if ((uint64_t)(it - linked.begin()) < b.adj_stride) dirty.push_back(last.first);
      linked.erase(it);
    }
  }
  return add_edge(b, target, id, distance, dirty);
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
  hipStream_t s = ix->stream;
  const uint64_t rb = ix->row_bytes;
  if (end_id > ix->nrows) end_id = ix->nrows;
  if (first_id < 1) first_id = 1;
  std::vector<uint32_t> todo;
  for (uint64_t id = first_id; id < end_id; id++)
    if (ix->h_valid[id] && !b.in_graph[id]) todo.push_back((uint32_t)id);
  if (b.graph_type == NGT_AMD_GRAPH_KNNG) return insert_knng(ix, b, todo);

  const uint32_t B = (uint32_t)b.batch_size, K = (uint32_t)b.edge_size_for_creation;
  struct Ev {
    hipEvent_t e = nullptr;
    ~Ev() {
      if (e) (void)hipEventDestroy(e);
    }
  } ev_copy;
  HIP_OK(hipEventCreateWithFlags(&ev_copy.e, hipEventDisableTiming));
  const uint32_t SS = kTreeSeedStride;
  DevBuf<uint32_t> d_ids, d_tseeds, d_tcnt, d_seeds, d_oi, d_on, d_dirty, d_vals;
  DevBuf<uint64_t> d_soff;
  DevBuf<float> d_od, d_pd;
  DevBuf<uint8_t> d_q, d_flag;
  HIP_OK(d_ids.alloc(B));
  HIP_OK(d_q.alloc((size_t)B * rb));
  HIP_OK(d_tseeds.alloc((size_t)B * SS));
  HIP_OK(d_tcnt.alloc(B));
  HIP_OK(d_oi.alloc((size_t)B * K));
  HIP_OK(d_od.alloc((size_t)B * K));
  HIP_OK(d_on.alloc(B));
  HIP_OK(d_flag.alloc(B));
  DevBuf<uint32_t> d_pleaf, d_pcnt;
  DevBuf<float> d_pdist;
  HIP_OK(d_pleaf.alloc(B));
  HIP_OK(d_pcnt.alloc(B));
  HIP_OK(d_pdist.alloc(B));
  DevBuf<uint32_t> d_mi, d_mn;
  DevBuf<float> d_md;
  HIP_OK(d_mi.alloc((size_t)B * K));
  HIP_OK(d_md.alloc((size_t)B * K));
  HIP_OK(d_mn.alloc(B));
  std::vector<uint32_t> h_tseeds((size_t)B * SS), h_tcnt(B), h_mi((size_t)B * K), h_mn(B);
  std::vector<float> h_md((size_t)B * K);
  // NGT_AMD_BUILD_PROFILE=1: per-stage wall time (stream synchronised at each mark)
  const bool prof = ngt_amd::knob("NGT_AMD_BUILD_PROFILE") != nullptr;
  double st[6] = {0, 0, 0, 0, 0, 0};
  auto t_last = std::chrono::steady_clock::now();
  DevBuf<uint64_t> d_cnt;
  std::vector<uint64_t> h_cnt;
  double k_ms = 0, dc = 0, ex = 0, ex_max = 0, c3 = 0, c5 = 0, c6 = 0, c7 = 0, c5_max = 0;
  uint64_t nsearched = 0;
  if (prof) {
    HIP_OK(d_cnt.alloc((size_t)B * NGT_AMD_COUNTERS_PER_QUERY));
    h_cnt.resize((size_t)B * NGT_AMD_COUNTERS_PER_QUERY);
  }
  auto mark = [&](int i) {
    if (!prof) return;
    (void)hipStreamSynchronize(s);
    auto t = std::chrono::steady_clock::now();
    st[i] += std::chrono::duration<double>(t - t_last).count();
    t_last = t;
  };

  for (size_t pos = 0; pos < todo.size(); pos += B) {
    const uint32_t n = (uint32_t)std::min<size_t>(B, todo.size() - pos);
    const uint32_t* ids = todo.data() + pos;
    if (ensure_tree_capacity(ix, b, 4 * n + 4, n + 1)) return -1;
    HIP_OK(hipMemcpyAsync(d_ids.p, ids, n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_OK(launch_gather_rows(d_q.p, ix->rows.p, rb, d_ids.p, n, s));

    // ---- 1. seeds: all objects of the leaf each batch object descends to --
    TreeSeedArgs t{};
    t.queries = d_q.p;
    t.query_bytes = rb;
    t.nq = n;
    t.dp = (int)ix->dp;
    t.row_bytes = rb;
    t.in_pivot = b.in_pivot.p;
    t.in_child = b.in_child.p;
    t.in_border = b.in_border.p;
    t.children = 5;
    t.root = b.root;
    t.leaf_count = b.lf_count.p;
    t.leaf_stride = kLeafCap;
    t.leaf_ids = b.lf_ids.p;
    t.seed_size = (uint32_t)std::max(b.seed_size, 0);
    t.k = K;
    t.all_leaf_nodes = 1;
    t.seeds = d_tseeds.p;
    t.seed_stride = SS;
    t.seed_count = d_tcnt.p;
    // the same descent locates each object's leaf for step 4
    t.out_leaf = d_pleaf.p;
    t.out_count = d_pcnt.p;
    t.out_pdist = d_pdist.p;
    t.leaf_pivot = b.lf_pivot.p;
    HIP_OK(launch_tree_seeds(t, ix->metric, ix->otype, s));
    HIP_OK(hipMemcpyAsync(h_tseeds.data(), d_tseeds.p, (size_t)n * SS * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(h_tcnt.data(), d_tcnt.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    mark(0);
    std::vector<uint32_t> seeds;
    std::vector<uint64_t> soff(n + 1, 0);
    for (uint32_t i = 0; i < n; i++) {
      const size_t start = seeds.size();
      for (uint32_t j = 0; j < h_tcnt[i]; j++) seeds.push_back(h_tseeds[(size_t)i * SS + j]);
      if (h_tcnt[i] == 0 && b.graph_size != 0) {
        // getSeedsFromGraph -> getRandomSeeds (Index.h:775-801, 1115-1135)
        const size_t repo = b.graph_size - 1;
        const size_t ss = std::min<size_t>(repo, (size_t)std::max(b.seed_size, 0));
        size_t empty = 0;
        while (seeds.size() - start < ss) {
          const double r = ((double)b.rnd.next() + 1.0) / ((double)2147483647 + 2.0);
          const size_t idx = (size_t)floor((double)repo * r) + 1;
          if (!b.in_graph[idx]) {
            if (++empty > repo) break;
            continue;
          }
          if (std::find(seeds.begin() + start, seeds.end(), (uint32_t)idx) != seeds.end()) continue;
          seeds.push_back((uint32_t)idx);
        }
      }
      soff[i + 1] = seeds.size();
    }

    // ---- 2. insertion searches (searchForNNGInsertion, Index.h:1457-1479) --
    if (!seeds.empty()) {
      HIP_OK(d_seeds.upload(seeds.data(), seeds.size()));
      HIP_OK(d_soff.upload(soff.data(), n + 1));
      ngt_amd_search_params p{};
      p.k = K;
      p.epsilon = b.epsilon_for_creation;
      p.radius = FLT_MAX;
      p.edge_size = -1;  // sc.edgeSize default -> edgeSizeForSearch
      p.seed_mode = NGT_AMD_SEED_GIVEN;
      p.visited_hash_log2 = 0;
      if (ngt_amd_search_device(ix, &p, d_q.p, rb, n, d_seeds.p, d_soff.p, d_oi.p, d_od.p, d_on.p,
                                prof ? d_cnt.p : nullptr, s))
        return -1;
      if (prof) {
        HIP_OK(hipMemcpyAsync(h_cnt.data(), d_cnt.p, (size_t)n * NGT_AMD_COUNTERS_PER_QUERY * sizeof(uint64_t),
                              hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
        k_ms += ngt_amd_last_search_kernel_ms(ix);
        uint64_t mx = 0;
        for (uint32_t i = 0; i < n; i++) {
          dc += (double)h_cnt[(size_t)i * NGT_AMD_COUNTERS_PER_QUERY];
          ex += (double)h_cnt[(size_t)i * NGT_AMD_COUNTERS_PER_QUERY + 2];
          mx = std::max(mx, h_cnt[(size_t)i * NGT_AMD_COUNTERS_PER_QUERY + 2]);
          const uint64_t* c = h_cnt.data() + (size_t)i * NGT_AMD_COUNTERS_PER_QUERY;
          c3 += (double)c[3];
          c5 += (double)c[5];
          c6 += (double)c[6];
          c7 += (double)c[7];
          c5_max = std::max(c5_max, (double)c[5]);
        }
        ex_max += (double)mx;
        nsearched += n;
      }
    } else {
      HIP_OK(hipMemsetAsync(d_on.p, 0, n * sizeof(uint32_t), s));
    }
    mark(1);

    // ---- 3. pairwise distances inside the batch (Index.cpp:690-703), then the
    //         merge / sort / cut of insertMultipleSearchResults (:673-727) -------
    const uint64_t npairs = (uint64_t)n * (n - 1) / 2;
    if (npairs) HIP_OK(d_pd.alloc(npairs));
    BatchPairArgs bp{};
    bp.rows = ix->rows.p;
    bp.row_bytes = rb;
    bp.dp = (int)ix->dp;
    bp.batch = d_q.p;
    bp.ids = d_ids.p;
    bp.n = n;
    bp.out = d_pd.p;
    HIP_OK(launch_batch_pairs(bp, ix->metric, ix->otype, s));
    BatchMergeArgs bm{};
    bm.res_ids = d_oi.p;
    bm.res_dists = d_od.p;
    bm.res_n = d_on.p;
    bm.K = K;
    bm.ids = d_ids.p;
    bm.pair = d_pd.p;
    bm.n = n;
    bm.out_ids = d_mi.p;
    bm.out_dists = d_md.p;
    bm.out_n = d_mn.p;
    bm.flag = d_flag.p;
    HIP_OK(launch_batch_merge(bm, s));
    mark(2);

    // ---- 4. DVPTree::insert of the batch (device, overlaps the host graph work)
    TreeBuildArgs ta = tree_insert_args(ix, b, d_ids.p, d_flag.p, n);
    ta.pre_leaf = d_pleaf.p;
    ta.pre_count = d_pcnt.p;
    ta.pre_dist = d_pdist.p;
    // the merged lists go to the host while the tree insertion runs
    HIP_OK(hipMemcpyAsync(h_mi.data(), d_mi.p, (size_t)n * K * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(h_md.data(), d_md.p, (size_t)n * K * sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_OK(hipMemcpyAsync(h_mn.data(), d_mn.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_OK(hipEventRecord(ev_copy.e, s));
    HIP_OK(launch_tree_insert(ta, ix->metric, ix->otype, s));
    mark(4);
    HIP_OK(hipEventSynchronize(ev_copy.e));

    // ---- insertANNGNode (Graph.h:611-625): the node, then the reverse edges;
    //      insertIANNGNode (:628-635) and insertONNGNode (:637-655) likewise ------
    std::vector<uint32_t> dirty;
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t id = ids[i];
      auto& objs = b.graph[id];
      objs.resize(h_mn[i]);
      for (uint32_t j = 0; j < h_mn[i]; j++) objs[j] = {h_mi[(size_t)i * K + j], h_md[(size_t)i * K + j]};
      b.in_graph[id] = 1;
      b.graph_size = std::max<uint64_t>(b.graph_size, (uint64_t)id + 1);
      dirty.push_back(id);
      if (b.graph_type == NGT_AMD_GRAPH_IANNG) {
        // the job's results, not the stored list: a deletion may shorten that one
        const std::vector<std::pair<uint32_t, float>> results(objs);
        for (const auto& r : results)
          if (add_edge_deleting_excess(b, r.first, id, r.second, dirty)) return -1;
      } else if (b.graph_type == NGT_AMD_GRAPH_ONNG) {
        const size_t in = std::min<size_t>(objs.size(), (size_t)b.incoming_edge);
        for (size_t j = 0; j < in; j++)
          if (add_edge(b, objs[j].first, id, objs[j].second, dirty)) return -1;
        if (objs.size() > (size_t)b.outgoing_edge) objs.resize(b.outgoing_edge);
      } else {
        for (const auto& r : objs)
          if (add_edge(b, r.first, id, r.second, dirty)) return -1;
      }
    }
    mark(3);

    // ---- refresh the padded adjacency of the touched nodes -----------------
    std::sort(dirty.begin(), dirty.end());
    dirty.erase(std::unique(dirty.begin(), dirty.end()), dirty.end());
    std::vector<uint32_t> vals(dirty.size() * b.adj_stride, 0u);
    for (size_t i = 0; i < dirty.size(); i++) {
      const auto& node = b.graph[dirty[i]];
      const size_t m = std::min<size_t>(node.size(), b.adj_stride);
      for (size_t j = 0; j < m; j++) vals[i * b.adj_stride + j] = node[j].first;
    }
    HIP_OK(d_dirty.upload(dirty.data(), dirty.size()));
    HIP_OK(d_vals.upload(vals.data(), vals.size()));
    HIP_OK(launch_adj_scatter(ix->adj.p, b.adj_stride, d_dirty.p, d_vals.p, (uint32_t)dirty.size(), s));
    ix->adj_version++;
    if (finish_batch(ix, b, s)) return -1;
    mark(5);
  }
  if (prof)
    fprintf(stderr, "build_insert %zu objects: seeds %.3f s, search %.3f s, pairs+merge %.3f s, host graph %.3f s, "
            "tree insert %.3f s, adjacency %.3f s; search kernel %.3f s, per query %.1f distances %.1f expansions, "
            "mean per-batch max expansions %.1f\n", todo.size(), st[0], st[1], st[2], st[3], st[4], st[5], k_ms / 1e3,
            dc / std::max<uint64_t>(nsearched, 1), ex / std::max<uint64_t>(nsearched, 1),
            ex_max / std::max<double>(1.0, (double)((todo.size() + B - 1) / B)));
  if (prof) {
    const double nq = (double)std::max<uint64_t>(nsearched, 1);
    // counters [3], [5..7]: spilled-visited flag, max unchecked, 0, 0 -- or, in
    // the NGT_AMD_STAMPS build, rest/pop/adjacency/eval cycles
    fprintf(stderr, "build_insert counters per query: c3 %.4g c5 %.4g (max %.4g) c6 %.4g c7 %.4g\n", c3 / nq,
            c5 / nq, c5_max, c6 / nq, c7 / nq);
  }
  return 0;
}

extern "C" int ngt_amd_build_set_graph(ngt_amd_index* ix, const uint64_t* offsets, const uint32_t* ids,
                                       const float* dists, uint64_t graph_rows) {
  if (!ix || !ix->build || !offsets || graph_rows > ix->nrows) return fail("ngt_amd_build_set_graph: bad arguments");
  if (offsets[graph_rows] && (!ids || !dists)) return fail("ngt_amd_build_set_graph: bad arguments");
  HIP_OK(hipSetDevice(ix->device));
  ServeHold serve_hold(ix);
  BuildState& b = *ix->build;
  const uint64_t S = b.adj_stride;
  std::vector<uint32_t> adj((size_t)ix->nrows * S, 0u);
  b.graph_size = 0;
  b.node_rows = graph_rows;
  for (uint64_t v = 0; v < graph_rows; v++) {
    const uint64_t e0 = offsets[v], e1 = offsets[v + 1];
    auto& node = b.graph[v];
    node.clear();
    for (uint64_t e = e0; e < e1; e++) {
      if (ids[e] == 0 || ids[e] >= ix->nrows) return fail("ngt_amd_build_set_graph: edge %u out of range", ids[e]);
      node.push_back({ids[e], dists[e]});
      if (e - e0 < S) adj[(size_t)v * S + (e - e0)] = ids[e];
    }
    b.in_graph[v] = e1 > e0 ? 1 : 0;
    if (e1 > e0) b.graph_size = v + 1;
  }
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

// a graph node exists: it has edges, or it lost them all to earlier removals
bool has_node(const ngt_amd_index* ix, const BuildState& b, uint32_t id) {
  return b.in_graph[id] || (ix->h_valid[id] && id < b.node_rows);
}

int drop_object(ngt_amd_index* ix, uint32_t id) {
  const uint8_t zero = 0;
  ix->h_valid[id] = 0;
  HIP_OK(hipMemcpy(ix->valid.p + id, &zero, 1, hipMemcpyHostToDevice));
  ix->rows_version++;
  return 0;
}

// 0 removed, 1 no such object, 2 refused (nothing changed), -1 device failure
// st (nullable): seconds spent enqueueing, waiting, on the leaf, on the lists, on the adjacency
int remove_one(ngt_amd_index* ix, BuildState& b, RemoveScratch& sc, uint32_t id, double* st) {
  auto t_last = std::chrono::steady_clock::now();
  auto mark = [&](int i) {
    if (!st) return;
    auto t = std::chrono::steady_clock::now();
    st[i] += std::chrono::duration<double>(t - t_last).count();
    t_last = t;
  };
  hipStream_t s = ix->stream;
  const uint64_t rb = ix->row_bytes;
  if (id == 0 || id >= ix->nrows || !ix->h_valid[id]) {
    fail("get: Not in-memory or invalid offset of node. idx=%u size=%llu", id, (unsigned long long)ix->nrows);
    return 1;
  }
  if (!has_node(ix, b, id)) return drop_object(ix, id);  // Index.h:1411-1422

  // The reference's search throws when it evaluates a neighbour whose object
  // is gone (Graph.cpp:603; a directed graph keeps edges to removed nodes),
  // which refuses the id before anything changes: the same test on the lists
  // the search expands -- the node's own and, below, its duplicate's.
  auto evaluated_edges_exist = [&](uint32_t v) {
    const auto& n = b.graph[v];
    const size_t lim = b.edge_size_for_search <= 0 ? n.size() : std::min<size_t>(n.size(), b.edge_size_for_search);
    for (size_t j = 0; j < lim; j++)
      if (n[j].first >= ix->nrows || !ix->h_valid[n[j].first]) {
        fail("get: Not in-memory or invalid offset of node. idx=%u size=%llu", n[j].first,
             (unsigned long long)ix->nrows);
        return false;
      }
    return true;
  };
  if (!evaluated_edges_exist(id)) return 2;

  // ---- the neighbours to relink (nothing is edited before every check) -----
  std::vector<uint32_t> nbr;
  std::vector<float> nbr_d;
  for (const auto& e : b.graph[id]) {
    if (e.first == id) continue;  // a self edge is erased
    if (e.first >= ix->nrows || !ix->h_valid[e.first] || !has_node(ix, b, e.first)) {
      fail("removeEdgesReliably : Relink error ID=%u: neighbour %u has no object or no node", id, e.first);
      return 2;
    }
    nbr.push_back(e.first);
    nbr_d.push_back(e.second);
  }
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
  ngt_amd_search_params p{};
  p.k = 2;
  p.epsilon = 0.1f;
  p.radius = 0.0f;
  p.edge_size = -1;
  p.seed_mode = NGT_AMD_SEED_GIVEN;
  p.visited_hash_log2 = 0;
  if (ngt_amd_search_device(ix, &p, d_row, rb, 1, sc.seed.p, sc.soff.p, sc.oi.p, sc.od.p, sc.on.p, nullptr, s))
    return -1;
  uint32_t found[2] = {0, 0}, nfound = 0;
  HIP_OK(hipMemcpyAsync(found, sc.oi.p, sizeof found, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(&nfound, sc.on.p, sizeof nfound, hipMemcpyDeviceToHost, s));

  // ---- the descent to the object's leaf (Tree.h:156-176) and the relink
  //      chain of the neighbours, behind the search on the same stream: the
  //      three need nothing from one another, so one wait serves them all ----
  TreeSeedArgs t{};
  HIP_OK(sc.tseeds.alloc(kTreeSeedStride));
  HIP_OK(sc.tcnt.alloc(1));
  HIP_OK(sc.pleaf.alloc(1));
  HIP_OK(sc.pcnt.alloc(1));
  HIP_OK(sc.pdist.alloc(1));
  t.queries = d_row;
  t.query_bytes = rb;
  t.nq = 1;
  t.dp = (int)ix->dp;
  t.row_bytes = rb;
  t.in_pivot = b.in_pivot.p;
  t.in_child = b.in_child.p;
  t.in_border = b.in_border.p;
  t.children = 5;
  t.root = b.root;
  t.leaf_count = b.lf_count.p;
  t.leaf_stride = kLeafCap;
  t.leaf_ids = b.lf_ids.p;
  t.seed_size = 1;
  t.k = 1;
  t.all_leaf_nodes = 0;
  t.seeds = sc.tseeds.p;
  t.seed_stride = kTreeSeedStride;
  t.seed_count = sc.tcnt.p;
  t.out_leaf = sc.pleaf.p;
  t.out_count = sc.pcnt.p;
  t.out_pdist = sc.pdist.p;
  t.leaf_pivot = b.lf_pivot.p;
  HIP_OK(launch_tree_seeds(t, ix->metric, ix->otype, s));
  uint32_t leaf = 0, cnt = 0;
  HIP_OK(hipMemcpyAsync(&leaf, sc.pleaf.p, sizeof leaf, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(&cnt, sc.pcnt.p, sizeof cnt, hipMemcpyDeviceToHost, s));
  std::vector<uint32_t> la(d ? d - 1 : 0), lb(d ? d - 1 : 0);
  std::vector<float> ld(d ? d - 1 : 0);
  if (relink(ix, sc, nbr.data(), d, la.data(), lb.data(), ld.data(), false)) return -1;
  int serr = 0;
  mark(0);
  if (take_device_error(ix, s, &serr)) return -1;
  if (serr) return fail("ngt_amd_build_remove: device error flag %d in the duplicate search", serr);
  if (nfound == 0) {
    fail("Not found the specified id");
    return 2;
  }
  const uint32_t replace_id = nfound == 1 ? 0u : (found[0] == id ? found[1] : found[0]);
  if (replace_id != 0 && (replace_id >= ix->nrows || !evaluated_edges_exist(replace_id))) return 2;

  mark(1);
  // ---- DVPTree::remove / replace (Tree.h:178-202, Node.cpp:229-280) --------
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
  } else {
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
  }

  mark(2);
  // ---- removeEdgesReliably on the host lists --------------------------------
  for (uint32_t i = 0; i < d; i++) {
    auto& n = b.graph[nbr[i]];
    const std::pair<uint32_t, float> e{id, nbr_d[i]};
    auto it = std::lower_bound(n.begin(), n.end(), e, od_less);
    if (it != n.end() && it->first == id) n.erase(it);  // else "cannot find an edge ... anyway continue"
  }
  for (uint32_t i = 0; i + 1 < d; i++) {
    auto link = [&](uint32_t from, uint32_t to) {
      auto& n = b.graph[from];
      const std::pair<uint32_t, float> e{to, ld[i]};
      auto it = std::lower_bound(n.begin(), n.end(), e, od_less);
      if (it == n.end() || it->first != to) n.insert(it, e);
    };
    link(la[i], lb[i]);
    link(lb[i], la[i]);
  }
  b.graph[id].clear();
  b.in_graph[id] = 0;

  mark(3);
  // ---- the padded adjacency of the touched nodes, the object ----------------
  std::vector<uint32_t> dirty(nbr);
  dirty.push_back(id);
  std::sort(dirty.begin(), dirty.end());
  dirty.erase(std::unique(dirty.begin(), dirty.end()), dirty.end());
  std::vector<uint32_t> vals(dirty.size() * b.adj_stride, 0u);
  for (size_t i = 0; i < dirty.size(); i++) {
    const auto& node = b.graph[dirty[i]];
    const size_t m = std::min<size_t>(node.size(), b.adj_stride);
    for (size_t j = 0; j < m; j++) vals[i * b.adj_stride + j] = node[j].first;
  }
  HIP_OK(sc.dirty.upload_async(dirty.data(), dirty.size(), s));
  HIP_OK(sc.vals.upload_async(vals.data(), vals.size(), s));
  HIP_OK(launch_adj_scatter(ix->adj.p, b.adj_stride, sc.dirty.p, sc.vals.p, (uint32_t)dirty.size(), s));
  HIP_OK(hipStreamSynchronize(s));
  ix->adj_version++;
  b.longest_removed_list = std::max<uint64_t>(b.longest_removed_list, d);
  mark(4);
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
  // NGT_AMD_BUILD_PROFILE=1: per-stage wall time on stderr
  const bool prof = ngt_amd::knob("NGT_AMD_BUILD_PROFILE") != nullptr;
  double st[5] = {0, 0, 0, 0, 0};
  for (uint64_t i = 0; i < n; i++) {
    const int r = remove_one(ix, b, sc, ids[i], prof ? st : nullptr);
    if (r < 0) return -1;
    status[i] = (uint8_t)r;
  }
  if (prof)
    fprintf(stderr, "build_remove %llu ids: enqueue %.3f s, wait %.3f s, leaf %.3f s, lists %.3f s, adjacency and "
            "flag %.3f s\n", (unsigned long long)n, st[0], st[1], st[2], st[3], st[4]);
  return 0;
}

extern "C" uint64_t ngt_amd_build_longest_removed_list(const ngt_amd_index* ix) {
  return ix && ix->build ? ix->build->longest_removed_list : 0;
}

extern "C" int ngt_amd_build_graph_size(const ngt_amd_index* ix, uint64_t* graph_size, uint64_t* nedges) {
  if (!ix || !ix->build || !graph_size || !nedges) return fail("ngt_amd_build_graph_size: bad arguments");
  const BuildState& b = *ix->build;
  *graph_size = b.graph_size;
  uint64_t e = 0;
  for (uint64_t v = 0; v < b.graph_size; v++) e += b.graph[v].size();
  *nedges = e;
  return 0;
}

extern "C" int ngt_amd_build_get_graph(const ngt_amd_index* ix, uint64_t* offsets, uint32_t* ids, float* dists) {
  if (!ix || !ix->build || !offsets) return fail("ngt_amd_build_get_graph: bad arguments");
  const BuildState& b = *ix->build;
  uint64_t e = 0;
  offsets[0] = 0;
  for (uint64_t v = 0; v < b.graph_size; v++) {
    for (const auto& x : b.graph[v]) {
      if (ids) ids[e] = x.first;
      if (dists) dists[e] = x.second;
      e++;
    }
    offsets[v + 1] = e;
  }
  return 0;
}

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
