// search_plan.cpp -- see search_plan.h.
#include "search_plan.h"

#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "knobs.h"
#include "search_layout.h"

namespace ngt_amd {

PlanKnobs read_plan_knobs() {
  PlanKnobs kn;
  kn.la = knob("NGT_AMD_LA");
  kn.filter = knob("NGT_AMD_FILTER");
  kn.no_stream = knob("NGT_AMD_NO_STREAM");
  kn.adj = knob("NGT_AMD_ADJ");
  kn.ht_log2 = knob("NGT_AMD_HT_LOG2");
  kn.cq_cap = knob("NGT_AMD_CQ_CAP");
  kn.accepted_only = knob("NGT_AMD_ACCEPTED_ONLY");
  kn.vfilter = knob("NGT_AMD_VFILTER");
  kn.la_lmax = knob("NGT_AMD_LA_LMAX");
  kn.lat = knob("NGT_AMD_LAT");
  kn.lat_tail = knob("NGT_AMD_LAT_TAIL");
  kn.lat_slots = knob("NGT_AMD_LAT_SLOTS");
  kn.lat_hop = knob("NGT_AMD_LAT_HOP");
  kn.lat_feed = knob("NGT_AMD_LAT_FEED");
  kn.sched = knob("NGT_AMD_SCHED");
  kn.sched_frac = knob("NGT_AMD_SCHED_FRAC");
  kn.sched_b = knob("NGT_AMD_SCHED_B");
  return kn;
}

void apply_visited_knobs(const PlanKnobs& kn, uint32_t& ht_log2, uint32_t& cq_cap, uint32_t& vf_log2,
                         bool keep_filter) {
  if (const char* v = kn.ht_log2) ht_log2 = (uint32_t)std::max(8, std::min(15, atoi(v)));
  if (const char* v = kn.cq_cap) cq_cap = (uint32_t)std::max(64, std::min(8192, atoi(v)));
  if (const char* v = kn.vfilter) {
    const int f = atoi(v);
    if (f > 0) vf_log2 = (uint32_t)std::max(11, std::min(18, f));
    else if (!keep_filter) vf_log2 = 0u;
  }
}

namespace {

// the fields of SearchArgs the LDS layouts (search_layout.h) read
SearchArgs layout_args(const PlanShape& sh, uint32_t k, const SearchPlan& p) {
  SearchArgs a{};
  a.nrows = (uint32_t)sh.nrows;
  a.dp = (int)sh.dp;
  a.adj_stride = sh.adj_stride;
  a.edge_size = sh.edge_size;
  a.k = k;
  a.ht_log2 = p.ht_log2;
  a.cq_cap = p.cq_cap;
  a.vf_log2 = p.vf_log2;
  a.la_lmax = p.la_lmax;
  a.la_sh_log2 = p.la_sh_log2;
  a.lat_slots = p.lat_slots;
  a.lat_tail = p.lat_tail;
  // search_lds_bytes only asks whether there is a filter copy
  a.fcodes = p.use_filter ? reinterpret_cast<const uint8_t*>(&sh) : nullptr;
  return a;
}
size_t one_lds(const PlanShape& sh, uint32_t k, const SearchPlan& p) {
  return search_lds_bytes(layout_args(sh, k, p), sh.otype);
}
size_t la_lds(const PlanShape& sh, uint32_t k, const SearchPlan& p, int la_mode) {
  return search_la_lds_bytes(layout_args(sh, k, p), (int)la_targets(la_mode));
}
size_t lat_lds(const PlanShape& sh, uint32_t k, const SearchPlan& p) {
  return search_lat_lds_bytes(layout_args(sh, k, p));
}

// the longest list a search reads from the padded adjacency
uint32_t list_cap(const PlanShape& sh) { return (uint32_t)std::min<uint64_t>(sh.adj_stride, sh.edge_size); }

size_t lds_limit(const PlanShape& sh) {
  return std::max<size_t>(64 * 1024, std::min<size_t>(sh.lds_per_block, sh.lds_per_cu));
}

// Which search kernel a launch takes: -1 the one-expansion-per-pop kernel
// (search_kernels.hip; every metric), 0 / 1 the lookahead kernel
// (search_la.hip; L2 over float rows of 96/128 elements with the padded
// adjacency) in its throughput (a wave per query) or latency (eight waves per
// query: launches of under two queries per CU -- single C-API calls,
// coalesced batches, construction batches) form.  NGT_AMD_LA=0 turns the
// lookahead kernel off, =1 keeps only the throughput form (for any list
// length), =2 only latency.
int lookahead_mode(const PlanShape& sh, bool use_adj, const ngt_amd_search_params& prm, uint32_t nq,
                   const PlanKnobs& kn) {
  const int env = kn.la ? atoi(kn.la) : 3;
  if (env == 0) return -1;
  if (sh.metric != NGT_AMD_DISTANCE_L2 || sh.otype != NGT_AMD_OBJECT_FLOAT || (sh.dp != 128 && sh.dp != 96))
    return -1;
  if (!use_adj || sh.adj_stride > 256) return -1;
  if (prm.distance_filter < 0) return -1;  // the lookahead kernel always filters
  if (kn.filter && atoi(kn.filter) == 0) return -1;
  const int mode = nq < 2u * (uint32_t)sh.cu_count ? 1 : 0;
  // a wave per query pays off on short lists (an NGT index at its
  // EdgeSizeForSearch of 40: ~4 lists per step); long lists (the C2 kNN graph,
  // ~136 ids) fill a step with one list, and the one-expansion kernel's
  // chunk pipeline with 16 waves per CU is faster there
  const uint64_t deg = list_cap(sh);
  if (mode == 0 && deg > 64 && env != 1) return -1;
  if ((env & (1 << mode)) == 0) return -1;
  return mode;
}

}  // namespace

bool plan_speculating(const PlanShape& sh, uint32_t k, const PlanKnobs& kn, SearchPlan& p) {
  const size_t lds_max = lds_limit(sh);
  SearchPlan b = p;
  b.lat_slots = list_cap(sh) <= 64 ? 32u : 16u;
  b.lat_tail = 4096u;
  // hop prefetch of each list part's nearest fresh neighbour (search_lat.hip);
  // NGT_AMD_LAT_HOP=0 turns it off (A/B)
  b.lat_hop = kn.lat_hop ? (atoi(kn.lat_hop) != 0 ? 1u : 0u) : 1u;
  // head entries kept speculated; NGT_AMD_LAT_FEED=n (A/B)
  b.lat_feed = kn.lat_feed ? (uint32_t)std::max(1, std::min(64, atoi(kn.lat_feed))) : 0u;
  while (lat_lds(sh, k, b) > lds_max && b.lat_tail > 512u) b.lat_tail -= 256u;
  while (lat_lds(sh, k, b) > lds_max && b.lat_slots > 8u) b.lat_slots -= 2u;
  // test knobs: a small tail forces the HBM spill, few slots the orphan path
  if (const char* v = kn.lat_tail) b.lat_tail = (uint32_t)std::max(128, std::min(4096, atoi(v)));
  if (const char* v = kn.lat_slots) b.lat_slots = (uint32_t)std::max(2, std::min(64, atoi(v)));
  b.lds_bytes = lat_lds(sh, k, b);
  if (b.lds_bytes > lds_max) return false;
  b.kernel = kPlanSpeculating;
  p = b;
  return true;
}

SearchPlan plan_search(const PlanShape& sh, const ngt_amd_search_params& prm, uint32_t nq, const PlanKnobs& kn) {
  SearchPlan p;
  const uint32_t k = prm.k;
  p.use_adj = sh.adj_stride != 0 && !(kn.adj && atoi(kn.adj) == 0);
  // LDS capacities of the visited hash and the unchecked array; overridable
  // (NGT_AMD_HT_LOG2 / NGT_AMD_CQ_CAP) so tests can force the exact HBM
  // overflow paths.
  p.ht_log2 = 12;
  p.cq_cap = 1024;
  p.vf_log2 = 0;
  // Small launches (construction batches) leave most of the chip idle and
  // their time is the slowest query's: give each query a larger LDS visited
  // hash and unchecked array (57 KB, two per CU) so long searches stay out
  // of the HBM epochs and the HBM spill.
  if (nq <= 2048 && prm.visited_hash_log2 == 0) {
    p.ht_log2 = 13;
    p.cq_cap = 3072;
    p.vf_log2 = 15;  // for the long ones that outgrow the hash (61.5 KB in all)
    if (one_lds(sh, k, p) > 64 * 1024) {  // large k: the default sizes
      p.ht_log2 = 12;
      p.cq_cap = 1024;
      p.vf_log2 = 0;
    }
    // up to one wave per CU (a construction batch of 200): each query may take
    // most of its CU's LDS, so the slowest searches -- which decide the batch
    // time -- keep their visited set and unchecked keys out of HBM (a pop
    // otherwise rescans the HBM spill: the tail of 1M ANNG construction)
    if (nq <= (uint32_t)sh.cu_count && sh.lds_per_block >= 128 * 1024) {
      SearchPlan b = p;
      b.ht_log2 = 14;
      b.cq_cap = 8192;
      b.vf_log2 = 15;
      if (one_lds(sh, k, b) <= sh.lds_per_block) p = b;
    }
  }
  if (prm.visited_hash_log2 < 0) {
    // HBM-epoch visited set (searches visiting ~1e5 ids, the C2 bench): a
    // 32 Kbit LDS filter proves most fresh ids unvisited without their HBM
    // probe, paid for by a 512-key unchecked array (same 9 KB of LDS, 16
    // waves per CU); measured +8 % QPS on C2 at identical results.
    // Long rows (C3: 3,840 B) dwarf the 128-B probe and their searches
    // saturate any LDS-sized filter: epochs alone there.
    p.ht_log2 = 0;
    // 512 unchecked keys in LDS (exact HBM spill beyond): C3's long rows then
    // fit 16 waves per CU instead of 11 (+6 % QPS).  Long cosine/angle rows
    // run at 12 waves per CU (search_kernels.hip), whose LDS holds 768: 794
    // vs 808 ms per C3 launch (profiles/r5zk)
    p.cq_cap = 512;
    if (sh.row_bytes > 1024 && sh.otype == NGT_AMD_OBJECT_FLOAT &&
        (sh.metric == NGT_AMD_DISTANCE_COSINE || sh.metric == NGT_AMD_DISTANCE_ANGLE))
      p.cq_cap = 768;
    if (sh.row_bytes <= 1024) {
      p.vf_log2 = 15;
      // -2: the filter and epochs hold accepted ids only (a few thousand per
      // query instead of ~7e4), so the filter stays sparse and almost no
      // neighbour costs an HBM probe or a mark store; rejected neighbours met
      // again are re-evaluated (search_common.h: not_accepted).  C2: +33 % QPS
      // at identical results for +14 % distance evaluations.
      p.accepted_only = prm.visited_hash_log2 == -2;
    }
  }
  else if (prm.visited_hash_log2 > 0) p.ht_log2 = (uint32_t)std::max(8, std::min(15, prm.visited_hash_log2));
  apply_visited_knobs(kn, p.ht_log2, p.cq_cap, p.vf_log2);
  if (const char* v = kn.accepted_only) p.accepted_only = atoi(v) != 0;
  // 1-byte filter copy for throughput launches over L2 float rows of 96/128
  // elements: a neighbour the bound places outside the exploration radius
  // costs Dp bytes instead of 4 Dp (filter_kernels.hip); latency-bound small
  // launches (construction batches) skip it, since a surviving neighbour then
  // costs a second round trip.  NGT_AMD_FILTER=0/1 forces it off/on.
  const int force = kn.filter ? atoi(kn.filter) : -1;
  // L2 rows of 96/128 floats (integer bound, pipelined expansion) or
  // cosine/angle long rows (streamed comparator; search_common.h filter_cos_u8)
  const bool shape = sh.otype == NGT_AMD_OBJECT_FLOAT &&
                     ((sh.metric == NGT_AMD_DISTANCE_L2 && (sh.dp == 128 || sh.dp == 96)) ||
                      ((sh.metric == NGT_AMD_DISTANCE_COSINE || sh.metric == NGT_AMD_DISTANCE_ANGLE) &&
                       sh.dp > 128 && sh.dp % 64 == 0 && !kn.no_stream));
  const bool want = force >= 0 ? force != 0
                               : (prm.distance_filter != 0 ? prm.distance_filter > 0
                                                           : nq >= 2u * (uint32_t)sh.cu_count);
  // the lookahead kernel (search_la.hip) shares one filter round trip
  // among a step's expansions, so it takes the filter at every launch size
  int la_mode = lookahead_mode(sh, p.use_adj, prm, nq, kn);
  p.use_filter = shape && (want || la_mode >= 0);
  if (!p.use_filter) la_mode = -1;
  if (la_mode >= 0) {
    // one step's target lists (<= 256 ids each) and the exact per-step id set
    const uint32_t env_lmax = kn.la_lmax ? (uint32_t)std::max(256, std::min(8192, atoi(kn.la_lmax))) : 0u;
    // list capacity: the targets' lists of the longest kind (t0's always fits)
    const uint32_t deg_cap = list_cap(sh);
    const uint32_t P = la_targets(la_mode);
    p.la_lmax = env_lmax ? env_lmax
                         : (la_mode == 0 ? std::max<uint32_t>(deg_cap, std::min<uint32_t>(256u, (P * deg_cap + 15) & ~15u))
                                         : 2048u);
    p.la_lmax = std::max<uint32_t>(p.la_lmax, deg_cap);
    // per-step id set: twice the ids a step can insert -- every list entry
    // with the full visited set; the accepted-only set inserts only accepted
    // ids, and the commit loop stops before a target could overfill it, so
    // there 4 x the longest list is plenty (and keeps 12 waves per CU)
    const uint32_t sh_want = (la_mode == 0 && p.accepted_only) ? std::min<uint32_t>(2u * p.la_lmax, 4u * deg_cap)
                                                               : 2u * p.la_lmax;
    p.la_sh_log2 = 1;
    while ((1u << p.la_sh_log2) < sh_want) p.la_sh_log2++;
    if (p.vf_log2 == 0) p.vf_log2 = 15;
    p.cq_cap = la_mode == 0 ? 512u : 2048u;
    if (la_mode == 0 && la_wpe() == 4) {
      p.vf_log2 = 14;
      p.cq_cap = 256u;
    }
    apply_visited_knobs(kn, p.ht_log2, p.cq_cap, p.vf_log2, true);
  }
  const size_t lds_max = lds_limit(sh);
  // latency launches: the speculating kernel (search_lat.hip) when the exact
  // LDS visited bitmap of every object fits one CU's LDS with its slots
  bool lat = false;
  if (la_mode == 1 && !(kn.lat && atoi(kn.lat) == 0) && list_cap(sh) <= 256u && k <= 64u)
    lat = plan_speculating(sh, k, kn, p);  // lists of <= 256 ids, results in one wave's registers
  if (!lat && la_mode >= 0 && la_lds(sh, k, p, la_mode) > lds_max) la_mode = -1;  // large k
  if (!lat) {
    p.kernel = la_mode < 0 ? kPlanOneExpansion : la_mode == 0 ? kPlanLookaheadWave : kPlanLookaheadEight;
    p.lds_bytes = la_mode >= 0 ? la_lds(sh, k, p, la_mode) : one_lds(sh, k, p);
  }
  // full visited set unless the caller asked for the accepted-only one
  p.la_full = la_mode >= 0 && !lat && !p.accepted_only;
  if (p.lds_bytes > lds_max) {
    char buf[160];
    snprintf(buf, sizeof buf, "search: k=%u needs %zu bytes of LDS per query (max %zu)", k, p.lds_bytes, lds_max);
    p.error = buf;
  }
  // "probe and resume" (ngt_amd_api.cpp launch_planned): the
  // one-expansion kernel's accepted-only filtered path
  p.sched_shape = p.kernel == kPlanOneExpansion && p.accepted_only && p.ht_log2 == 0 && p.vf_log2 != 0 && p.use_adj &&
                  p.use_filter && k <= 64;
  // NGT_AMD_SCHED=0: every search one launch in query order
  p.sched_on = p.sched_shape && (kn.sched ? atoi(kn.sched) : 1) != 0;
  p.sched_frac = kn.sched_frac ? std::max(0.01, std::min(0.9, atof(kn.sched_frac))) : 0.25;
  p.sched_forced = kn.sched_b ? (uint32_t)std::max(0, atoi(kn.sched_b)) : 0u;
  return p;
}

}  // namespace ngt_amd
