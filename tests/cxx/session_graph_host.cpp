// session_graph_host.cpp -- the list rules of a build session on the CPU
// (ngt_amd/csrc/session_graph.h) against a model restated here from the
// reference's text: Graph.h:533-562, 607-655, 845-934 (insertNode, the four
// insertion rules, addEdge, addEdgeDeletingExcessEdges), Graph.cpp:641-864
// (removeEdgesReliably, NGT_FORCED_REMOVE) and Index.h:775-801
// (getRandomSeeds).  The model uses another method than the module: its lists
// are appended to and re-sorted by an insertion sort, and what a binary search
// would stop at is found by a linear scan for the least entry not before the
// key -- no lower_bound.  For the generator the oracle is the C library:
// srand(s); rand().
//
// Directed cases on the smallest shapes at which a rule can go wrong (32 slots,
// edgeSizeForCreation 3, 16-wide adjacency rows, distances from {0, 0.5, 1} so
// ties dominate), then a differential run: random sequences of operations
// applied to module and model, compared after every operation -- the whole
// repository, the dirty set and the message.  Prints one line of counts; exits
// non-zero on any failure.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../ngt_amd/csrc/session_graph.h"

using namespace ngt_amd;

namespace {

long g_checks = 0, g_failures = 0, g_sequences = 0, g_operations = 0;

#define CHECK(cond)                                                 \
  do {                                                              \
    g_checks++;                                                     \
    if (!(cond)) {                                                  \
      g_failures++;                                                 \
      if (g_failures < 50) fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
    }                                                               \
  } while (0)

constexpr uint32_t kSlots = 32;
using List = std::vector<Edge>;

std::string text(const char* fmt, uint32_t a, uint32_t b) {
  char buf[256];
  snprintf(buf, sizeof buf, fmt, a, b);
  return buf;
}

// ---- the model ---------------------------------------------------------------
struct Model {
  std::vector<List> g = std::vector<List>(kSlots);
  std::vector<uint8_t> in = std::vector<uint8_t>(kSlots, 0);
  uint64_t size = 0, node_rows = 0;
  size_t E = 3, stride = 16;
  int type = NGT_AMD_GRAPH_ANNG, outgoing = 10, incoming = 80;
  std::vector<uint32_t> dirty;

  // ObjectDistance::operator<
  static bool before(const Edge& a, const Edge& b) {
    return a.second < b.second || (a.second == b.second && a.first < b.first);
  }
  static void sort_list(List& l) {
    for (size_t i = 1; i < l.size(); i++)
      for (size_t j = i; j > 0 && before(l[j], l[j - 1]); j--) std::swap(l[j], l[j - 1]);
  }
  // where std::lower_bound(l, e) stops: the least entry not before e, -1 for end()
  static int stop_at(const List& l, const Edge& e) {
    int at = -1;
    for (size_t i = 0; i < l.size(); i++)
      if (!before(l[i], e) && (at < 0 || before(l[i], l[(size_t)at]))) at = (int)i;
    return at;
  }
  static size_t rank_of(const List& l, const Edge& e) {
    size_t r = 0;
    for (const auto& x : l) r += before(x, e);
    return r;
  }
  void insert_sorted(uint32_t node, const Edge& e) {
    if (rank_of(g[node], e) < stride) dirty.push_back(node);
    g[node].push_back(e);
    sort_list(g[node]);
  }
  void repository_insert(uint32_t id, const List& results) {
    g[id] = results;
    in[id] = 1;
    if (size < (uint64_t)id + 1) size = (uint64_t)id + 1;
  }

  // addEdge(node, addID, addDistance, identityCheck = true), Graph.h:845-873
  std::string add_edge(uint32_t target, uint32_t id, float d) {
    const Edge e{id, d};
    const int at = stop_at(g[target], e);
    if (at >= 0 && g[target][(size_t)at].first == id) return text("NGT::addEdge: already existed! %u:%u", id, id);
    insert_sorted(target, e);
    return "";
  }

  // removeEdge(node, edge), Graph.h:719-744: "" or the exception's text
  std::string remove_edge(uint32_t node, const Edge& e) {
    List& l = g[node];
    const int at = stop_at(l, e);
    if (at >= 0 && l[(size_t)at].first == e.first) {
      if (rank_of(l, l[(size_t)at]) < stride) dirty.push_back(node);
      l.erase(l.begin() + at);
      return "";
    }
    char buf[96];
    if (at < 0)
      snprintf(buf, sizeof buf, "NGT::removeEdge: Cannot found %u", e.first);
    else
      snprintf(buf, sizeof buf, "NGT::removeEdge: Cannot found %u:%u", l[(size_t)at].first, e.first);
    return buf;
  }

  // addEdgeDeletingExcessEdges, Graph.h:888-934
  std::string add_edge_deleting_excess(uint32_t target, uint32_t id, float d) {
    const size_t k_edge = E - 1;
    if (g[target].size() > k_edge && g[target][k_edge].second >= d) {
      const Edge last = g[target][k_edge];
      if (last.first >= kSlots || !in[last.first]) {  // getNode throws
        char buf[128];
        snprintf(buf, sizeof buf, "get: Not in-memory or invalid offset of node. idx=%u size=%zu", last.first,
                 (size_t)kSlots);
        return buf;
      }
      const Edge linked_edge{target, last.second};
      if (g[last.first].size() > k_edge && last.second >= g[last.first][k_edge].second) {
        remove_edge(target, last);  // (a): the entry itself, always found
        const std::string why = remove_edge(last.first, linked_edge);
        if (!why.empty()) {
          // the reference prints node[kEdge] of the shortened list; past its end
          // (the reference reads out of bounds there) the module prints 0,0
          const Edge now = g[target].size() > k_edge ? g[target][k_edge] : Edge{0u, 0.f};
          char buf[256];
          snprintf(buf, sizeof buf, "addEdge: Cannot remove. (b) %u,%u,%u,%g:%s", target, id, now.first, now.second,
                   why.c_str());
          return buf;
        }
      }
    }
    return add_edge(target, id, d);
  }

  // insertNode, Graph.h:533-562, 607-655
  std::string insert_node(uint32_t id, List results) {
    std::string err;
    if (type == NGT_AMD_GRAPH_KNNG) {
      repository_insert(id, results);
    } else if (type == NGT_AMD_GRAPH_ANNG) {
      repository_insert(id, results);
      dirty.push_back(id);
      for (size_t i = 0; i < results.size() && err.empty(); i++) err = add_edge(results[i].first, id, results[i].second);
    } else if (type == NGT_AMD_GRAPH_IANNG) {
      repository_insert(id, results);
      dirty.push_back(id);
      for (size_t i = 0; i < results.size() && err.empty(); i++)
        err = add_edge_deleting_excess(results[i].first, id, results[i].second);
    } else {
      // the module stores the list first and cuts it afterwards: on a failure
      // the uncut list is what it leaves, so the model does the same
      repository_insert(id, results);
      dirty.push_back(id);
      int count = 0;
      for (size_t i = 0; i < results.size() && err.empty(); i++, count++) {
        if (count >= incoming) break;
        err = add_edge(results[i].first, id, results[i].second);
      }
      if (err.empty() && (int)results.size() > outgoing) {
        results.resize((size_t)outgoing);
        g[id] = results;
      }
    }
    return err;
  }

  bool has_node(const std::vector<uint8_t>& valid, uint32_t id) const {
    return in[id] || (valid[id] && id < node_rows);
  }

  // the objects and nodes removeEdgesReliably fetches (Graph.cpp:671-703):
  // "" and the neighbours, or the refusal
  std::string neighbours(const std::vector<uint8_t>& valid, uint32_t id, std::vector<uint32_t>& nbr,
                         std::vector<float>& nbr_d) const {
    for (size_t i = 0; i < g[id].size(); i++) {
      const uint32_t v = g[id][i].first;
      if (v == id) continue;
      if (v >= kSlots || !valid[v] || !has_node(valid, v)) {
        char buf[160];
        snprintf(buf, sizeof buf, "removeEdgesReliably : Relink error ID=%u: neighbour %u has no object or no node", id,
                 v);
        return buf;
      }
      nbr.push_back(v);
      nbr_d.push_back(g[id][i].second);
    }
    return "";
  }

  // Graph.cpp:705-864 with the chain given
  void remove(uint32_t id, const std::vector<uint32_t>& nbr, const std::vector<float>& nbr_d,
              const std::vector<uint32_t>& la, const std::vector<uint32_t>& lb, const std::vector<float>& ld) {
    for (size_t i = 0; i < nbr.size(); i++) {
      List& n = g[nbr[i]];
      const int at = stop_at(n, Edge{id, nbr_d[i]});
      if (at >= 0 && n[(size_t)at].first == id) n.erase(n.begin() + at);  // else "anyway continue..."
    }
    for (size_t i = 0; i + 1 < nbr.size(); i++) {
      for (int side = 0; side < 2; side++) {
        const uint32_t from = side ? lb[i] : la[i], to = side ? la[i] : lb[i];
        const Edge obj{to, ld[i]};
        const int at = stop_at(g[from], obj);
        if (at < 0 || g[from][(size_t)at].first != to) {
          g[from].push_back(obj);
          sort_list(g[from]);
        }
      }
    }
    g[id].clear();
    in[id] = 0;
    dirty.insert(dirty.end(), nbr.begin(), nbr.end());
    dirty.push_back(id);
  }
};

// sorted, without repeats; by counting, not std::sort + std::unique
std::vector<uint32_t> as_set(const std::vector<uint32_t>& v) {
  std::vector<uint32_t> out;
  for (uint32_t id = 0; id < kSlots; id++)
    for (uint32_t x : v)
      if (x == id) {
        out.push_back(id);
        break;
      }
  return out;
}

// ---- module and model side by side: every operation goes to both, and the
//      message, the dirty set and the whole repository are compared -------------
struct Pair {
  SessionGraph s;
  Model m;
  std::vector<uint8_t> valid = std::vector<uint8_t>(kSlots, 0);

  Pair() {
    s.reset(kSlots);
    s.edge_size_for_creation = 3;
    s.adj_stride = 16;
  }
  void set_type(int type, int outgoing = 10, int incoming = 80) {
    s.graph_type = m.type = type;
    s.outgoing_edge = m.outgoing = outgoing;
    s.incoming_edge = m.incoming = incoming;
  }
  void set_node_rows(uint64_t rows) { s.node_rows = m.node_rows = rows; }
  // a node with this list, put there directly
  void put(uint32_t v, const List& l) {
    s.graph[v] = l;
    s.mark_node(v);
    m.repository_insert(v, l);
    valid[v] = 1;
  }
  void same_state() {
    CHECK(s.graph_size == m.size);
    bool lists = true, flags = true;
    for (uint32_t v = 0; v < kSlots; v++) {
      lists = lists && s.graph[v] == m.g[v];
      flags = flags && s.in_graph[v] == m.in[v];
    }
    CHECK(lists);
    CHECK(flags);
  }
  std::string same(const std::string& es, const std::string& em, std::vector<uint32_t>& dirty) {
    if (es != em) fprintf(stderr, "module: %s\nmodel:  %s\n", es.c_str(), em.c_str());
    CHECK(es == em);
    CHECK(as_set(dirty) == as_set(m.dirty));
    last_dirty = as_set(dirty);
    m.dirty.clear();
    same_state();
    return es;
  }
  std::vector<uint32_t> last_dirty;

  std::string insert(uint32_t id, const List& results) {
    std::vector<uint32_t> ids, dirty;
    std::vector<float> ds;
    for (const auto& e : results) {
      ids.push_back(e.first);
      ds.push_back(e.second);
    }
    const std::string es = s.insert_node(id, ids.data(), ds.data(), (uint32_t)results.size(), dirty);
    valid[id] = 1;
    return same(es, m.insert_node(id, results), dirty);
  }
  std::string add(uint32_t target, uint32_t id, float d) {
    std::vector<uint32_t> dirty;
    const std::string es = s.add_edge(target, id, d, dirty);
    return same(es, m.add_edge(target, id, d), dirty);
  }
  std::string add_deleting(uint32_t target, uint32_t id, float d) {
    std::vector<uint32_t> dirty;
    const std::string es = s.add_edge_deleting_excess(target, id, d, dirty);
    return same(es, m.add_edge_deleting_excess(target, id, d), dirty);
  }

  // GraphAndTreeIndex::remove's graph half with the relink chain chain(nbr)
  // makes: "dropped" for an object without a node, the refusal, or ""
  template <typename Chain>
  std::string remove(uint32_t id, int32_t edge_size_for_search, Chain chain) {
    const std::vector<List> before = s.graph;
    const std::vector<uint8_t> before_in = s.in_graph;
    CHECK(s.has_node(valid, id) == m.has_node(valid, id));
    if (!s.has_node(valid, id)) {
      valid[id] = 0;
      return "dropped";
    }
    std::string es = s.evaluated_edges_exist(valid, id, edge_size_for_search);
    std::string em;
    const size_t lim = edge_size_for_search <= 0 ? m.g[id].size() : std::min<size_t>(m.g[id].size(), edge_size_for_search);
    for (size_t j = 0; j < lim && em.empty(); j++)
      if (m.g[id][j].first >= kSlots || !valid[m.g[id][j].first])
        em = text("get: Not in-memory or invalid offset of node. idx=%u size=%u", m.g[id][j].first, kSlots);
    CHECK(es == em);
    std::vector<uint32_t> nbr, nbr_m, dirty;
    std::vector<float> nbr_d, nbr_dm;
    if (es.empty()) {
      es = s.removal_neighbours(valid, id, nbr, nbr_d);
      CHECK(es == m.neighbours(valid, id, nbr_m, nbr_dm));
    }
    if (!es.empty()) {  // a refusal leaves everything as it was
      CHECK(s.graph == before && s.in_graph == before_in);
      same_state();
      return es;
    }
    CHECK(nbr == nbr_m && nbr_d == nbr_dm);
    if (nbr != nbr_m) return "diverged";
    std::vector<uint32_t> la, lb;
    std::vector<float> ld;
    chain(nbr, la, lb, ld);
    s.apply_removal(id, nbr, nbr_d, la.data(), lb.data(), ld.data(), dirty);
    m.remove(id, nbr_m, nbr_dm, la, lb, ld);
    valid[id] = 0;
    return same("", "", dirty);
  }
};

bool holds(const List& l, uint32_t id) {
  for (const auto& e : l)
    if (e.first == id) return true;
  return false;
}

// ---- the sorted insert -------------------------------------------------------
void sorted_insert_cases() {
  Pair p;
  p.put(1, {{5, 0.5f}});
  for (uint32_t v = 2; v < kSlots; v++) p.put(v, {});
  CHECK(p.add(1, 3, 0.5f).empty());  // equal distance, smaller id
  CHECK((p.s.graph[1] == List{{3, 0.5f}, {5, 0.5f}}));
  CHECK(p.add(1, 7, 0.5f).empty());  // equal distance, larger id
  CHECK((p.s.graph[1] == List{{3, 0.5f}, {5, 0.5f}, {7, 0.5f}}));
  CHECK(p.add(1, 5, 0.5f) == "NGT::addEdge: already existed! 5:5");
  CHECK(p.s.graph[1].size() == 3);
  CHECK(p.add(1, 5, 1.0f).empty());  // the same id at another distance is inserted
  CHECK(p.add(1, 5, 0.0f).empty());
  CHECK((p.s.graph[1] == List{{5, 0.0f}, {3, 0.5f}, {5, 0.5f}, {7, 0.5f}, {5, 1.0f}}));

  // dirty at rank 15, not at rank 16: one list of 17 entries
  Pair q;
  for (uint32_t v = 1; v < kSlots; v++) q.put(v, {});
  for (uint32_t id = 2; id <= 17; id++) {
    CHECK(q.add(1, id, 0.5f).empty());
    CHECK(q.last_dirty == std::vector<uint32_t>{1});  // ranks 0..15
  }
  CHECK(q.add(1, 18, 0.5f).empty());  // rank 16
  CHECK(q.last_dirty.empty());
  CHECK(q.s.graph[1].size() == 17);
  CHECK(q.add(1, 19, 0.0f).empty());  // rank 0 of a long list
  CHECK(q.last_dirty == std::vector<uint32_t>{1});
}

// ---- addEdgeDeletingExcessEdges: target 1, its rank-2 edge leads to node 4,
//      the new edge is (10, 0.5) -------------------------------------------------
void iannng_cases() {
  // the rank-2 distance t of the target against the new 0.5: none, <, ==, >
  const float target_t[4] = {-1.f, 0.25f, 0.5f, 0.75f};
  // the linked node's rank-2 distance x against t (last.second <, ==, > x): none, or t + rel
  const float linked_rel[4] = {-1.f, 0.125f, 0.f, -0.125f};
  for (int a = 0; a < 4; a++)
    for (int b = 0; b < 4; b++) {
      Pair p;
      p.set_type(NGT_AMD_GRAPH_IANNG);
      for (uint32_t v = 1; v < kSlots; v++) p.put(v, {});
      const float t = a == 0 ? 0.5f : target_t[a];
      p.put(1, a == 0 ? List{{2, 0.f}, {3, 0.f}} : List{{2, 0.f}, {3, 0.f}, {4, t}});
      List linked;
      if (b == 0) linked = {{5, 0.f}, {1, t}};
      if (b == 1) linked = {{5, 0.f}, {1, t}, {7, t + linked_rel[b]}};          // t < x
      if (b == 2) linked = {{5, 0.f}, {6, 0.f}, {1, t}, {7, t}};                // t == x
      if (b == 3) linked = {{5, 0.f}, {6, 0.f}, {7, t + linked_rel[b]}, {1, t}};  // t > x
      p.put(4, linked);
      CHECK(p.add_deleting(1, 10, 0.5f).empty());
      const bool deleted = a >= 2 && b >= 2;  // t >= 0.5 and t >= x, both lists longer than E - 1
      CHECK(holds(p.s.graph[1], 4) == (a != 0 && !deleted));
      CHECK(holds(p.s.graph[4], 1) == !deleted);
      CHECK(holds(p.s.graph[1], 10));
      CHECK(p.s.graph[4].size() == linked.size() - (deleted ? 1 : 0));
    }

  // the reverse edge is absent at that distance
  Pair p;
  p.set_type(NGT_AMD_GRAPH_IANNG);
  for (uint32_t v = 1; v < kSlots; v++) p.put(v, {});
  p.put(1, {{2, 0.f}, {3, 0.f}, {4, 0.5f}, {8, 1.f}});
  p.put(4, {{5, 0.f}, {6, 0.f}, {7, 0.5f}, {1, 0.75f}});
  CHECK(p.add_deleting(1, 10, 0.5f) == "addEdge: Cannot remove. (b) 1,10,8,1:NGT::removeEdge: Cannot found 7:1");
  p.put(4, {{5, 0.f}, {6, 0.f}, {7, 0.5f}});
  p.put(1, {{2, 0.f}, {3, 0.f}, {4, 0.75f}, {8, 1.f}});
  CHECK(p.add_deleting(1, 10, 0.5f) == "addEdge: Cannot remove. (b) 1,10,8,1:NGT::removeEdge: Cannot found 1");
  // the rank-2 edge leads to a slot that is no node
  p.put(1, {{2, 0.f}, {3, 0.f}, {9, 0.5f}});
  p.s.in_graph[9] = p.m.in[9] = 0;
  CHECK(p.add_deleting(1, 10, 0.5f) == "get: Not in-memory or invalid offset of node. idx=9 size=32");

  // the job's own results, not the stored list, give the reverse edges: node 5
  // still holds an edge to the slot 10 that is inserted (a loaded graph whose
  // node 10 had no edge left); its deletion shortens 10's stored list
  Pair q;
  q.set_type(NGT_AMD_GRAPH_IANNG);
  for (uint32_t v = 1; v < kSlots; v++)
    if (v != 10) q.put(v, {});
  q.put(5, {{2, 0.f}, {3, 0.f}, {10, 0.5f}});
  CHECK(q.insert(10, {{5, 0.5f}, {6, 0.5f}, {7, 0.5f}}).empty());
  CHECK((q.s.graph[10] == List{{6, 0.5f}, {7, 0.5f}}));
  CHECK(holds(q.s.graph[5], 10) && holds(q.s.graph[6], 10) && holds(q.s.graph[7], 10));
}

void onng_knng_cases() {
  const List results = {{1, 0.f}, {2, 0.5f}, {3, 0.5f}};
  const int cases[5][2] = {{10, 0}, {10, 2}, {10, 5}, {2, 5}, {3, 5}};  // outgoing, incoming
  for (const auto& c : cases) {
    Pair p;
    p.set_type(NGT_AMD_GRAPH_ONNG, c[0], c[1]);
    for (uint32_t v = 1; v <= 3; v++) p.put(v, {});
    CHECK(p.insert(9, results).empty());
    for (uint32_t v = 1; v <= 3; v++) CHECK(holds(p.s.graph[v], 9) == ((int)v <= c[1]));  // also past the cut
    CHECK(p.s.graph[9].size() == (size_t)std::min(3, c[0]));
    CHECK(p.s.graph[9] == List(results.begin(), results.begin() + std::min(3, c[0])));
  }
  Pair p;
  p.set_type(NGT_AMD_GRAPH_KNNG);
  for (uint32_t v = 1; v <= 3; v++) p.put(v, {});
  CHECK(p.insert(9, results).empty());
  CHECK(p.s.graph[9] == results && p.s.in_graph[9] && p.s.graph_size == 10);
  CHECK(p.last_dirty.empty());
  for (uint32_t v = 1; v <= 3; v++) CHECK(p.s.graph[v].empty());
}

// ---- removal -------------------------------------------------------------------
void removal_cases() {
  Pair p;
  p.set_node_rows(16);
  p.put(1, {{4, 0.5f}, {3, 1.f}});
  p.put(2, {{4, 0.25f}});  // the reverse edge at another distance
  p.put(3, {{1, 0.5f}, {4, 0.5f}, {5, 0.5f}, {1, 1.f}});
  p.put(5, {{4, 0.5f}});
  p.put(4, {{4, 0.f}, {1, 0.5f}, {2, 0.5f}, {3, 0.5f}, {5, 0.5f}});  // with a self edge
  auto chain = [](const std::vector<uint32_t>& nbr, std::vector<uint32_t>& la, std::vector<uint32_t>& lb,
                  std::vector<float>& ld) {
    CHECK((nbr == std::vector<uint32_t>{1, 2, 3, 5}));  // the self edge is ignored
    la = {1, 3, 2};
    lb = {3, 2, 5};
    ld = {1.f, 0.5f, 0.5f};
  };
  CHECK(p.remove(4, 0, chain).empty());
  CHECK((p.s.graph[1] == List{{3, 1.f}}));                            // 1 - 3 at 1.0 was there: not added twice
  CHECK((p.s.graph[2] == List{{4, 0.25f}, {3, 0.5f}, {5, 0.5f}}));    // (4, 0.25) stays
  CHECK((p.s.graph[3] == List{{1, 0.5f}, {2, 0.5f}, {5, 0.5f}, {1, 1.f}}));  // 2 lands between the ties 1 and 5
  CHECK((p.s.graph[5] == List{{2, 0.5f}}));
  CHECK(p.s.graph[4].empty() && !p.s.in_graph[4]);
  CHECK((p.last_dirty == std::vector<uint32_t>{1, 2, 3, 4, 5}));
  CHECK(!p.s.has_node(p.valid, 4));  // remove() took the object
  p.valid[4] = 1;
  CHECK(p.s.has_node(p.valid, 4));   // a valid object below node_rows: a node without edges
  p.set_node_rows(4);
  CHECK(!p.s.has_node(p.valid, 4));
  CHECK(p.remove(4, 0, chain) == "dropped");

  // the three refusals: nothing changes (Pair::remove compares the repository)
  auto never = [](const std::vector<uint32_t>&, std::vector<uint32_t>&, std::vector<uint32_t>&, std::vector<float>&) {
    CHECK(false);
  };
  Pair q;
  q.set_node_rows(8);
  q.put(1, {{2, 0.f}, {3, 0.5f}, {20, 1.f}});
  q.put(2, {{1, 0.f}});
  q.put(3, {{1, 0.5f}});
  q.valid[20] = 1;  // an object past node_rows that is no node
  CHECK(q.remove(1, 0, never) == "removeEdgesReliably : Relink error ID=1: neighbour 20 has no object or no node");
  q.valid[3] = 0;   // an evaluated edge to a removed object
  CHECK(q.remove(1, 2, never) == "get: Not in-memory or invalid offset of node. idx=3 size=32");
  CHECK(q.remove(1, 0, never) == "get: Not in-memory or invalid offset of node. idx=3 size=32");
  // past the evaluated edges: the relink refuses it
  CHECK(q.remove(1, 1, never) == "removeEdgesReliably : Relink error ID=1: neighbour 3 has no object or no node");
}

// ---- getRandomSeeds ----------------------------------------------------------
struct CRand {
  int next() { return rand(); }
};

void random_seed_cases() {
  const unsigned seeds[3] = {1u, 0u, 12345u};
  for (unsigned sd : seeds) {
    GlibcRandHost r;
    r.seed(sd);
    srand(sd);
    bool equal = true;
    for (int i = 0; i < 1000; i++) equal = equal && r.next() == rand();
    CHECK(equal);
    // a draw over the C library's stream equals the one over the restated stream
    std::vector<uint32_t> a, b;
    CRand c;
    srand(sd);
    r.seed(sd);
    auto odd_empty = [](size_t idx) { return idx % 3 == 0; };
    get_random_seeds(r, 31, 10, odd_empty, a);
    get_random_seeds(c, 31, 10, odd_empty, b);
    CHECK(a == b && a.size() == 10);
  }
  SessionGraph g;
  g.reset(kSlots);
  for (uint32_t v = 1; v <= 5; v++) g.mark_node(v);
  GlibcRandHost r;
  r.seed(1);
  std::vector<uint32_t> s = {77};  // what the caller already holds stays
  g.random_seeds(r, 10, s);
  CHECK(s.size() == 6 && s[0] == 77);
  CHECK((as_set(std::vector<uint32_t>(s.begin() + 1, s.end())) == std::vector<uint32_t>{1, 2, 3, 4, 5}));
  // every slot empty: it ends after repo + 1 misses
  size_t asked = 0;
  std::vector<uint32_t> none;
  get_random_seeds(r, 5, 10, [&](size_t) { return ++asked > 0; }, none);
  CHECK(none.empty() && asked == 6);
  SessionGraph empty;
  empty.reset(kSlots);
  empty.random_seeds(r, 10, none);
  CHECK(none.empty());
}

// ---- CSR in and out, adjacency rows -------------------------------------------
void csr_cases() {
  // empty lists in the middle (3) and at the end (5..7)
  const std::vector<uint64_t> off = {0, 0, 2, 3, 3, 5, 5, 5, 5};
  const std::vector<uint32_t> ids = {2, 4, 1, 1, 2};
  const std::vector<float> ds = {0.f, 0.5f, 0.f, 0.5f, 1.f};
  SessionGraph g;
  g.reset(kSlots);
  g.adj_stride = 16;
  CHECK(g.set_csr(off.data(), ids.data(), ds.data(), 8).empty());
  CHECK(g.graph_size == 5 && g.node_rows == 8 && g.edge_count() == 5);
  for (uint32_t v = 0; v < kSlots; v++) CHECK(g.in_graph[v] == (v == 1 || v == 2 || v == 4));
  std::vector<uint64_t> off2(g.graph_size + 1, 99);
  std::vector<uint32_t> ids2(5);
  std::vector<float> ds2(5);
  g.get_csr(off2.data(), ids2.data(), ds2.data());
  CHECK(off2 == std::vector<uint64_t>(off.begin(), off.begin() + 6) && ids2 == ids && ds2 == ds);
  g.get_csr(off2.data(), nullptr, nullptr);
  g.mark_node(6);
  CHECK(g.graph_size == 7 && g.in_graph[6] && g.graph[6].empty());
  const std::vector<uint32_t> bad = {2, 32, 1, 1, 2}, zero = {2, 0, 1, 1, 2};
  CHECK(g.set_csr(off.data(), bad.data(), ds.data(), 8) == "ngt_amd_build_set_graph: edge 32 out of range");
  CHECK(g.set_csr(off.data(), zero.data(), ds.data(), 8) == "ngt_amd_build_set_graph: edge 0 out of range");

  // adjacency rows: 16 ids of a 20-entry list and no more; a 3-entry list zero padded
  Pair p;
  List l20, l3 = {{7, 0.f}, {8, 0.5f}, {9, 1.f}};
  for (uint32_t i = 0; i < 20; i++) l20.push_back({i + 2, 0.5f});
  p.put(1, l20);
  p.put(30, l3);
  std::vector<uint32_t> dirty = {30, 1, 30, 1};
  const std::vector<uint32_t> rows = p.s.adjacency_rows(dirty);
  CHECK((dirty == std::vector<uint32_t>{1, 30}) && rows.size() == 32);
  for (uint32_t j = 0; j < 16; j++) {
    CHECK(rows[j] == j + 2);
    CHECK(rows[16 + j] == (j < 3 ? l3[j].first : 0u));
  }
}

// ---- the differential run ---------------------------------------------------
struct Lcg {
  uint64_t x;
  uint32_t below(uint32_t n) {
    x = x * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((x >> 33) % n);
  }
  float distance() { return 0.5f * (float)below(3); }
};

// up to `most` distinct nodes in the graph other than id, sorted by (distance, id)
List draw_results(Lcg& r, const Pair& p, uint32_t id, uint32_t most) {
  List l;
  const uint32_t want = r.below(most + 1);
  for (uint32_t tries = 0; tries < 40 && l.size() < want; tries++) {
    const uint32_t v = 1 + r.below(kSlots - 1);
    if (v != id && p.s.in_graph[v] && !holds(l, v)) l.push_back({v, r.distance()});
  }
  Model::sort_list(l);
  return l;
}

uint32_t free_slot(Lcg& r, const Pair& p) {
  for (uint32_t tries = 0; tries < 8; tries++) {
    const uint32_t v = 1 + r.below(kSlots - 1);
    if (!p.s.in_graph[v]) return v;
  }
  return 0;
}

// the three reverse-edge insertion rules mixed, with bare edge insertions and
// nodes inserted again
void insertion_sequence(uint64_t seed) {
  Lcg r{seed};
  Pair p;
  const int types[3] = {NGT_AMD_GRAPH_ANNG, NGT_AMD_GRAPH_IANNG, NGT_AMD_GRAPH_ONNG};
  const int outgoing = 1 + (int)r.below(4), incoming = (int)r.below(5);
  for (int op = 0; op < 64; op++, g_operations++) {
    const uint32_t what = r.below(10);
    uint32_t id = what < 6 ? free_slot(r, p) : 0;
    if (id == 0 && what == 0) id = 1 + r.below(kSlots - 1);  // a node inserted again
    if (id != 0) {
      p.set_type(types[r.below(3)], outgoing, incoming);
      p.insert(id, draw_results(r, p, id, 4));
      continue;
    }
    const uint32_t target = 1 + r.below(kSlots - 1), from = 1 + r.below(kSlots - 1);
    if (!p.s.in_graph[target]) continue;
    if (r.below(2))
      p.add(target, from, r.distance());
    else
      p.add_deleting(target, from, r.distance());
  }
  g_sequences++;
}

// insertions and removals on an ANNG, with objects that leave without their node
void removal_sequence(uint64_t seed) {
  Lcg r{seed};
  Pair p;
  const uint64_t node_rows[3] = {0, 16, kSlots};
  const int32_t edge_sizes[4] = {0, 1, 2, 40};
  p.set_node_rows(node_rows[r.below(3)]);
  const int32_t es = edge_sizes[r.below(4)];
  auto chain = [&](const std::vector<uint32_t>& nbr, std::vector<uint32_t>& la, std::vector<uint32_t>& lb,
                   std::vector<float>& ld) {
    std::vector<uint32_t> order(nbr);
    for (size_t i = 0; i + 1 < order.size(); i++) {
      const size_t j = i + 1 + r.below((uint32_t)(order.size() - i - 1));
      la.push_back(order[i]);
      lb.push_back(order[j]);
      ld.push_back(r.distance());
      std::swap(order[i + 1], order[j]);
    }
  };
  for (int op = 0; op < 64; op++, g_operations++) {
    const uint32_t what = r.below(20);
    const uint32_t id = what < 11 ? free_slot(r, p) : 0;
    if (id != 0) {
      p.insert(id, draw_results(r, p, id, 5));
    } else if (what == 19) {
      p.valid[1 + r.below(kSlots - 1)] = 0;
    } else {
      const uint32_t v = 1 + r.below(kSlots - 1);
      if (p.valid[v]) p.remove(v, es, chain);
    }
  }
  g_sequences++;
}

}  // namespace

int main() {
  sorted_insert_cases();
  iannng_cases();
  onng_knng_cases();
  removal_cases();
  random_seed_cases();
  csr_cases();
  for (uint64_t s = 1; s <= 200; s++) insertion_sequence(s);
  for (uint64_t s = 1; s <= 200; s++) removal_sequence(1000 + s);
  printf("sequences %ld operations %ld checks %ld failures %ld\n", g_sequences, g_operations, g_checks, g_failures);
  return g_failures == 0 ? 0 : 1;
}
