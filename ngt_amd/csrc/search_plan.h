// search_plan.h -- launch planning of the graph search: which kernel a launch
// takes and with which LDS capacities, as pure arithmetic on the index's
// shape, the caller's parameters and the test knobs.  No HIP call, no lock,
// no allocation and no per-process cache, so a host program can tabulate it
// (tests/cxx/search_plan_table.cpp).  run_search (ngt_amd_api.cpp) executes
// a plan; serve.cpp and qg_api.cpp share the parts they need.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>

#include "../../include/ngt_amd.h"

namespace ngt_amd {

struct PlanShape {
  int metric, otype;
  uint32_t dp;
  uint64_t row_bytes, nrows;
  int cu_count;
  size_t lds_per_block, lds_per_cu;
  uint64_t adj_stride;  // 0: no padded copy holds this search's lists
  uint64_t edge_size;   // resolved getEdgeSize()
};

// The planning knobs as the environment gives them:
// null = unset.  Read once per launch, so a test process can switch them.
struct PlanKnobs {
  const char *la, *filter, *no_stream, *adj, *ht_log2, *cq_cap, *accepted_only, *vfilter, *la_lmax, *lat, *lat_tail,
      *lat_slots, *lat_hop, *lat_feed, *sched, *sched_frac, *sched_b;
};
PlanKnobs read_plan_knobs();

enum PlanKernel : int {
  kPlanOneExpansion = 0,  // search_kernels.hip; every metric
  kPlanLookaheadWave,     // search_la.hip, throughput form: a wave per query
  kPlanLookaheadEight,    // search_la.hip, latency form: eight waves per query
  kPlanSpeculating,       // search_lat.hip
};

struct SearchPlan {
  PlanKernel kernel = kPlanOneExpansion;
  uint32_t ht_log2 = 12, cq_cap = 1024, vf_log2 = 0, accepted_only = 0;
  bool use_adj = false;     // the padded adjacency (NGT_AMD_ADJ=0: the CSR lists)
  bool use_filter = false;  // the 1-byte filter copy
  uint32_t la_lmax = 0, la_sh_log2 = 0;
  bool la_full = false;     // lookahead kernel: full visited set (else accepted-only)
  uint32_t lat_slots = 0, lat_tail = 0, lat_hop = 0, lat_feed = 0;
  size_t lds_bytes = 0;     // dynamic LDS per workgroup
  bool sched_shape = false; // eligible for "probe and resume" (and counts its expansions)
  bool sched_on = false;    // ... and NGT_AMD_SCHED does not turn it off
  double sched_frac = 0.25; // probe budget / mean expansions of earlier launches
  uint32_t sched_forced = 0;  // test knob: a fixed budget for every eligible launch
  std::string error;        // empty, or why no kernel can run this search
  // SearchCtx::launch_la: -1 none, 0 / 1 the lookahead forms (1 also for the speculating kernel)
  int la_mode() const { return kernel == kPlanOneExpansion ? -1 : kernel == kPlanLookaheadWave ? 0 : 1; }
};

SearchPlan plan_search(const PlanShape& sh, const ngt_amd_search_params& prm, uint32_t nq, const PlanKnobs& kn);

// The speculating kernel's slots and LDS tail for lists of min(adj_stride,
// edge_size) <= 256 ids and k <= 64: false when its exact visited bitmap of
// every object does not fit one CU's LDS beside them (p is then unchanged).
bool plan_speculating(const PlanShape& sh, uint32_t k, const PlanKnobs& kn, SearchPlan& p);

// NGT_AMD_HT_LOG2 / _CQ_CAP / _VFILTER over a search's visited-set sizes.
// keep_filter: NGT_AMD_VFILTER <= 0 does not take the LDS filter away (the
// lookahead kernel always has one).
void apply_visited_knobs(const PlanKnobs& kn, uint32_t& ht_log2, uint32_t& cq_cap, uint32_t& vf_log2,
                         bool keep_filter = false);

}  // namespace ngt_amd
