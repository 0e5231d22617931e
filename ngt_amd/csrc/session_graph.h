// session_graph.h -- the graph repository of a build session and every rule
// that decides a built index's lists, as pure host code: no HIP include, no
// device call, so a host program drives it (tests/cxx/session_graph_host.cpp).
// build.cpp supplies the device work around it.
//
//   the sorted addEdge with its identity check        Graph.h:845-873
//   addEdgeDeletingExcessEdges                        Graph.h:888-934
//   insertKNNGNode / ANNG / IANNG / ONNG              Graph.h:533-562, 607-655
//   getRandomSeeds                                    Index.h:775-801
//   the host half of removeEdgesReliably              Graph.cpp:641-864
//   the padded adjacency rows the insertion searches read
//   the CSR form of the lists, in and out
//
// Lists are sorted by ObjectDistance::operator< (distance, then id).  A rule
// that can fail returns its message ("" on success), the convention of
// accuracy_table.h and edge_optimizer.h; nothing here prints or throws.  The
// rules that change lists append the nodes whose padded adjacency row changed
// to `dirty`: a node is dirty only when the changed rank is below adj_stride.
#pragma once
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ngt_amd.h"

namespace ngt_amd {

// glibc random(3) TYPE_3 (random_r), host side: the rand() stream of a fresh
// process (srand(1)), for getRandomSeeds.
struct GlibcRandHost {
  uint32_t s[31];
  int f = 3, r = 0;
  void seed(uint32_t sd) {
    int32_t word = (int32_t)(sd == 0 ? 1u : sd);
    s[0] = (uint32_t)word;
    for (int i = 1; i < 31; i++) {
      int32_t hi = word / 127773, lo = word % 127773;
      word = 16807 * lo - 2836 * hi;
      if (word < 0) word += 2147483647;
      s[i] = (uint32_t)word;
    }
    f = 3;
    r = 0;
    for (int i = 0; i < 310; i++) next();
  }
  int next() {
    s[f] += s[r];
    int res = (int)((s[f] >> 1) & 0x7fffffff);
    f = f == 30 ? 0 : f + 1;
    r = r == 30 ? 0 : r + 1;
    return res;
  }
};

// One GraphIndex::getRandomSeeds (Index.h:775-801) appended to `seeds`: up to
// min(repo, seed_size) distinct ids in 1..repo that are not empty slots, drawn
// from rnd.next() (a rand() value); more than repo empty draws end it.
template <typename Rand, typename IsEmpty>
void get_random_seeds(Rand& rnd, size_t repo, size_t seed_size, IsEmpty is_empty, std::vector<uint32_t>& seeds) {
  const size_t start = seeds.size();
  const size_t ss = std::min(repo, seed_size);
  size_t empty = 0;
  while (seeds.size() - start < ss) {
    const double random = ((double)rnd.next() + 1.0) / ((double)2147483647 + 2.0);  // RAND_MAX
    const size_t idx = (size_t)floor((double)repo * random) + 1;
    if (is_empty(idx)) {
      if (++empty > repo) break;
      continue;
    }
    if (std::find(seeds.begin() + start, seeds.end(), (uint32_t)idx) != seeds.end()) continue;
    seeds.push_back((uint32_t)idx);
  }
}

using Edge = std::pair<uint32_t, float>;  // (id, distance)

inline bool od_less(const Edge& a, const Edge& b) {
  // ObjectDistance::operator< (Common.h:1946-1952): distance, then id
  if (a.second != b.second) return a.second < b.second;
  return a.first < b.first;
}

#if defined(__GNUC__)
__attribute__((format(printf, 1, 2)))
#endif
inline std::string graph_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  return buf;
}

struct SessionGraph {
  std::vector<std::vector<Edge>> graph;  // graph repository, slot = object id
  std::vector<uint8_t> in_graph;
  uint64_t graph_size = 0;  // GraphRepository::size() (max inserted id + 1, 0 when empty)
  // the slots loaded by set_csr: a valid object below it has a node even with
  // no edges left (removal)
  uint64_t node_rows = 0;
  uint64_t adj_stride = 0;  // width of a padded adjacency row
  int32_t edge_size_for_creation = 10;
  int32_t graph_type = NGT_AMD_GRAPH_ANNG;         // the insertion rule
  int32_t outgoing_edge = 10, incoming_edge = 80;  // ONNG at insertion (Graph.h:637-655)

  void reset(uint64_t slots) {
    graph.assign(slots, {});
    in_graph.assign(slots, 0);
    graph_size = node_rows = 0;
  }

  // slot v is a node (it may have no edge): construction does not insert it again
  void mark_node(uint64_t v) {
    in_graph[v] = 1;
    graph_size = std::max<uint64_t>(graph_size, v + 1);
  }

  // The reverse edge target <- (id, distance) of insertANNGNode / insertONNGNode:
  // the sorted addEdge with the identity check (Graph.h:845-873).
  std::string add_edge(uint32_t target, uint32_t id, float distance, std::vector<uint32_t>& dirty) {
    auto& node = graph[target];
    const Edge e{id, distance};
    auto it = std::lower_bound(node.begin(), node.end(), e, od_less);
    if (it != node.end() && it->first == id) return graph_error("NGT::addEdge: already existed! %u:%u", it->first, id);
    if ((uint64_t)(it - node.begin()) < adj_stride) dirty.push_back(target);
    node.insert(it, e);
    return "";
  }

  // addEdgeDeletingExcessEdges (Graph.h:888-934)
  std::string add_edge_deleting_excess(uint32_t target, uint32_t id, float distance, std::vector<uint32_t>& dirty) {
    auto& node = graph[target];
    const size_t k_edge = (size_t)edge_size_for_creation - 1;
    if (node.size() > k_edge && node[k_edge].second >= distance) {
      const Edge last = node[k_edge];
      if (last.first >= graph.size() || !in_graph[last.first])
        return graph_error("get: Not in-memory or invalid offset of node. idx=%u size=%zu", last.first, graph.size());
      auto& linked = graph[last.first];
      if (linked.size() > k_edge && last.second >= linked[k_edge].second) {
        node.erase(node.begin() + k_edge);
        if (k_edge < adj_stride) dirty.push_back(target);
        const Edge back{target, last.second};
        auto it = std::lower_bound(linked.begin(), linked.end(), back, od_less);
        if (it == linked.end() || it->first != target) {
          char found[48] = "";
          if (it != linked.end()) snprintf(found, sizeof found, "%u:", it->first);
          // the reference prints the edge now at that rank of the shortened list
          const Edge now = node.size() > k_edge ? node[k_edge] : Edge{0u, 0.f};
          return graph_error("addEdge: Cannot remove. (b) %u,%u,%u,%g:NGT::removeEdge: Cannot found %s%u", target, id,
                             now.first, now.second, found, target);
        }
        if ((uint64_t)(it - linked.begin()) < adj_stride) dirty.push_back(last.first);
        linked.erase(it);
      }
    }
    return add_edge(target, id, distance, dirty);
  }

  // NeighborhoodGraph::insertNode (Graph.h:533-562) of batch object `id` with
  // its merged list: insertKNNGNode (:607-609) stores it; insertANNGNode
  // (:611-625) adds every reverse edge, insertIANNGNode (:628-635) through
  // add_edge_deleting_excess, insertONNGNode (:637-655) for the first
  // incoming_edge results, with the stored list cut to outgoing_edge afterwards.
  // A KNNG node's adjacency row is written on the device: it is not dirty.
  std::string insert_node(uint32_t id, const uint32_t* ids, const float* dists, uint32_t n,
                          std::vector<uint32_t>& dirty) {
    auto& objs = graph[id];
    objs.resize(n);
    for (uint32_t j = 0; j < n; j++) objs[j] = {ids[j], dists[j]};
    mark_node(id);
    if (graph_type == NGT_AMD_GRAPH_KNNG) return "";
    dirty.push_back(id);
    const bool onng = graph_type == NGT_AMD_GRAPH_ONNG, iannng = graph_type == NGT_AMD_GRAPH_IANNG;
    // the reverse edges follow the job's results, not the stored list: an
    // IANNG deletion may shorten that one
    const uint32_t in = onng ? (uint32_t)std::min<uint64_t>(n, (uint64_t)incoming_edge) : n;
    for (uint32_t j = 0; j < in; j++) {
      const std::string err = iannng ? add_edge_deleting_excess(ids[j], id, dists[j], dirty)
                                     : add_edge(ids[j], id, dists[j], dirty);
      if (!err.empty()) return err;
    }
    if (onng && n > (uint64_t)outgoing_edge) graph[id].resize(outgoing_edge);
    return "";
  }

  // getSeedsFromGraph -> getRandomSeeds (Index.h:775-801, 1115-1135) over the
  // repository as it stands; nothing when it is empty
  template <typename Rand>
  void random_seeds(Rand& rnd, int32_t seed_size, std::vector<uint32_t>& seeds) const {
    if (graph_size == 0) return;
    get_random_seeds(rnd, graph_size - 1, (size_t)std::max(seed_size, 0), [&](size_t idx) { return !in_graph[idx]; },
                     seeds);
  }

  // ---- removal (GraphAndTreeIndex::remove, Index.h:1386-1455): `valid` holds
  //      the object repository's flags, one per slot ---------------------------

  // a graph node exists: it has edges, or it lost them all to earlier removals
  bool has_node(const std::vector<uint8_t>& valid, uint32_t id) const {
    return in_graph[id] || (valid[id] && id < node_rows);
  }

  // The reference's search throws when it evaluates a neighbour whose object
  // is gone (Graph.cpp:603; a directed graph keeps edges to removed nodes): the
  // same test on the first edge_size_for_search edges (all when <= 0) of v.
  std::string evaluated_edges_exist(const std::vector<uint8_t>& valid, uint32_t v, int32_t edge_size_for_search) const {
    const auto& n = graph[v];
    const size_t lim = edge_size_for_search <= 0 ? n.size() : std::min<size_t>(n.size(), edge_size_for_search);
    for (size_t j = 0; j < lim; j++)
      if (n[j].first >= valid.size() || !valid[n[j].first])
        return graph_error("get: Not in-memory or invalid offset of node. idx=%u size=%llu", n[j].first,
                           (unsigned long long)valid.size());
    return "";
  }

  // the neighbours removeEdgesReliably relinks, in list order with their
  // distances; a self edge is skipped, a neighbour without object or node refuses
  std::string removal_neighbours(const std::vector<uint8_t>& valid, uint32_t id, std::vector<uint32_t>& nbr,
                                 std::vector<float>& nbr_d) const {
    for (const auto& e : graph[id]) {
      if (e.first == id) continue;  // a self edge is erased
      if (e.first >= valid.size() || !valid[e.first] || !has_node(valid, e.first))
        return graph_error("removeEdgesReliably : Relink error ID=%u: neighbour %u has no object or no node", id,
                           e.first);
      nbr.push_back(e.first);
      nbr_d.push_back(e.second);
    }
    return "";
  }

  // removeEdgesReliably (Graph.cpp:641-864, NGT_FORCED_REMOVE) given the relink
  // chain (link_a[i], link_b[i], link_dist[i]), i < nbr.size() - 1: the reverse
  // edges go under the identity rule (one at another distance stays: "cannot
  // find an edge ... anyway continue"), the two-way links are not duplicated,
  // the node is cleared.  Every neighbour and the node are dirty.
  void apply_removal(uint32_t id, const std::vector<uint32_t>& nbr, const std::vector<float>& nbr_d,
                     const uint32_t* link_a, const uint32_t* link_b, const float* link_dist,
                     std::vector<uint32_t>& dirty) {
    for (size_t i = 0; i < nbr.size(); i++) {
      auto& n = graph[nbr[i]];
      auto it = std::lower_bound(n.begin(), n.end(), Edge{id, nbr_d[i]}, od_less);
      if (it != n.end() && it->first == id) n.erase(it);
    }
    auto link = [&](uint32_t from, uint32_t to, float dist) {
      auto& n = graph[from];
      auto it = std::lower_bound(n.begin(), n.end(), Edge{to, dist}, od_less);
      if (it == n.end() || it->first != to) n.insert(it, Edge{to, dist});
    };
    for (size_t i = 0; i + 1 < nbr.size(); i++) {
      link(link_a[i], link_b[i], link_dist[i]);
      link(link_b[i], link_a[i], link_dist[i]);
    }
    graph[id].clear();
    in_graph[id] = 0;
    dirty.insert(dirty.end(), nbr.begin(), nbr.end());
    dirty.push_back(id);
  }

  // ---- the padded adjacency -------------------------------------------------

  // `dirty` sorted and de-duplicated in place; the zero-padded adj_stride-wide
  // rows of its nodes: the first adj_stride ids of each list
  std::vector<uint32_t> adjacency_rows(std::vector<uint32_t>& dirty) const {
    std::sort(dirty.begin(), dirty.end());
    dirty.erase(std::unique(dirty.begin(), dirty.end()), dirty.end());
    std::vector<uint32_t> vals(dirty.size() * adj_stride, 0u);
    for (size_t i = 0; i < dirty.size(); i++) {
      const auto& node = graph[dirty[i]];
      const size_t m = std::min<size_t>(node.size(), adj_stride);
      for (size_t j = 0; j < m; j++) vals[i * adj_stride + j] = node[j].first;
    }
    return vals;
  }

  // ---- CSR in and out ---------------------------------------------------------

  // the lists of slots 0..graph_rows from offsets [graph_rows + 1], ids and
  // dists; a slot with edges is in the graph
  std::string set_csr(const uint64_t* offsets, const uint32_t* ids, const float* dists, uint64_t graph_rows) {
    graph_size = 0;
    node_rows = graph_rows;
    for (uint64_t v = 0; v < graph_rows; v++) {
      auto& node = graph[v];
      node.clear();
      for (uint64_t e = offsets[v]; e < offsets[v + 1]; e++) {
        if (ids[e] == 0 || ids[e] >= graph.size())
          return graph_error("ngt_amd_build_set_graph: edge %u out of range", ids[e]);
        node.push_back({ids[e], dists[e]});
      }
      in_graph[v] = !node.empty();
      if (!node.empty()) graph_size = v + 1;
    }
    return "";
  }

  uint64_t edge_count() const {
    uint64_t e = 0;
    for (uint64_t v = 0; v < graph_size; v++) e += graph[v].size();
    return e;
  }

  // offsets [graph_size + 1]; ids and dists [edge_count()], either may be null
  void get_csr(uint64_t* offsets, uint32_t* ids, float* dists) const {
    uint64_t e = 0;
    offsets[0] = 0;
    for (uint64_t v = 0; v < graph_size; v++) {
      for (const auto& x : graph[v]) {
        if (ids) ids[e] = x.first;
        if (dists) dists[e] = x.second;
        e++;
      }
      offsets[v + 1] = e;
    }
  }
};

}  // namespace ngt_amd
