// search_plan_table.cpp -- prints plan_search (ngt_amd/csrc/search_plan.cpp)
// over a table of shapes, parameters and knobs: one line per case, the inputs,
// " | ", then every field of SearchPlan.  Links search_plan.cpp only; no
// device.  tests/test_search_plan.py compares the output with
// tests/golden/search_plan_table.txt.
#include <stdio.h>
#include <string.h>

#include "../../include/ngt_amd.h"
#include "search_plan.h"

using namespace ngt_amd;

static const char* kColumns =
    "# metric dp nq k visited_hash_log2 distance_filter adj_stride/edge_size lds_per_block nrows knob=value"
    " | kernel ht_log2 cq_cap vf_log2 accepted_only use_adj use_filter la_lmax la_sh_log2 la_full"
    " lat_slots lat_tail lat_hop lat_feed lds_bytes sched_shape sched_on sched_frac sched_forced error\n"
    "# float rows; cu_count 256, lds_per_cu 163840; kernel: one = one-expansion, law = lookahead wave per query,\n"
    "# la8 = lookahead eight-wave, spec = speculating\n";

struct Knob {
  const char* name;
  const char* PlanKnobs::*field;
  const char* value;
};

static void row(int metric, uint32_t dp, uint32_t nq, uint32_t k, int vis, int filt, uint64_t adj, uint64_t es,
                size_t lds_per_block, uint64_t nrows, const Knob* knob = nullptr) {
  PlanShape sh{};
  sh.metric = metric;
  sh.otype = NGT_AMD_OBJECT_FLOAT;
  sh.dp = dp;
  sh.row_bytes = 4ull * dp;
  sh.nrows = nrows;
  sh.cu_count = 256;
  sh.lds_per_block = lds_per_block;
  sh.lds_per_cu = 163840;
  sh.adj_stride = adj;
  sh.edge_size = es;
  ngt_amd_search_params prm;
  memset(&prm, 0, sizeof prm);
  prm.k = k;
  prm.visited_hash_log2 = vis;
  prm.distance_filter = filt;
  PlanKnobs kn{};
  if (knob) kn.*(knob->field) = knob->value;
  const SearchPlan p = plan_search(sh, prm, nq, kn);
  static const char* kern[] = {"one", "law", "la8", "spec"};
  printf("%s %u %u %u %d %d %llu/%llu %zu %llu ", metric == NGT_AMD_DISTANCE_L2 ? "L2" : "cos", dp, nq, k, vis, filt,
         (unsigned long long)adj, (unsigned long long)es, lds_per_block, (unsigned long long)nrows);
  if (knob) printf("%s=%s", knob->name, knob->value);
  else printf("-");
  printf(" | %s %u %u %u %u %d %d %u %u %d %u %u %u %u %zu %d %d %g %u %s\n", kern[p.kernel], p.ht_log2, p.cq_cap,
         p.vf_log2, p.accepted_only, (int)p.use_adj, (int)p.use_filter, p.la_lmax, p.la_sh_log2, (int)p.la_full,
         p.lat_slots, p.lat_tail, p.lat_hop, p.lat_feed, p.lds_bytes, (int)p.sched_shape, (int)p.sched_on,
         p.sched_frac, p.sched_forced, p.error.empty() ? "-" : p.error.c_str());
}

int main() {
  const int L2 = NGT_AMD_DISTANCE_L2, COS = NGT_AMD_DISTANCE_COSINE;
  fputs(kColumns, stdout);
  puts("# shapes whose plans were derived by hand from the code before the planning moved");
  row(COS, 128, 1000, 10, 0, 0, 40, 40, 65536, 100000);
  row(COS, 128, 200, 10, 0, 0, 40, 40, 163840, 100000);
  row(COS, 128, 1000, 500, 0, 0, 40, 40, 65536, 100000);
  row(L2, 128, 10000, 10, -2, 0, 256, 136, 65536, 100000);
  row(L2, 128, 10000, 10, -2, 0, 40, 40, 65536, 100000);
  row(L2, 128, 1, 10, 0, 0, 40, 40, 163840, 100000);
  row(L2, 128, 1, 10, 0, 0, 40, 40, 163840, 10000000);  // the visited bitmap does not fit: eight-wave lookahead

  puts("# one row per knob, on a shape where it matters");
  const int nk = 19;
  const Knob knobs[nk] = {
      {"NGT_AMD_LA", &PlanKnobs::la, "0"},
      {"NGT_AMD_LA", &PlanKnobs::la, "1"},
      {"NGT_AMD_FILTER", &PlanKnobs::filter, "0"},
      {"NGT_AMD_FILTER", &PlanKnobs::filter, "1"},
      {"NGT_AMD_NO_STREAM", &PlanKnobs::no_stream, "1"},
      {"NGT_AMD_ADJ", &PlanKnobs::adj, "0"},
      {"NGT_AMD_HT_LOG2", &PlanKnobs::ht_log2, "9"},
      {"NGT_AMD_CQ_CAP", &PlanKnobs::cq_cap, "128"},
      {"NGT_AMD_ACCEPTED_ONLY", &PlanKnobs::accepted_only, "1"},
      {"NGT_AMD_VFILTER", &PlanKnobs::vfilter, "0"},
      {"NGT_AMD_LA_LMAX", &PlanKnobs::la_lmax, "512"},
      {"NGT_AMD_LAT", &PlanKnobs::lat, "0"},
      {"NGT_AMD_LAT_TAIL", &PlanKnobs::lat_tail, "128"},
      {"NGT_AMD_LAT_SLOTS", &PlanKnobs::lat_slots, "4"},
      {"NGT_AMD_LAT_HOP", &PlanKnobs::lat_hop, "0"},
      {"NGT_AMD_LAT_FEED", &PlanKnobs::lat_feed, "8"},
      {"NGT_AMD_SCHED", &PlanKnobs::sched, "0"},
      {"NGT_AMD_SCHED_FRAC", &PlanKnobs::sched_frac, "0.12"},
      {"NGT_AMD_SCHED_B", &PlanKnobs::sched_b, "40"},
  };
  for (int i = 0; i < nk; i++) {
    const Knob& kb = knobs[i];
    const char* n = kb.name + 8;  // past NGT_AMD_
    if (!strncmp(n, "LAT", 3)) {
      row(L2, 128, 1, 10, 0, 0, 40, 40, 163840, 100000, &kb);  // a single query: the speculating kernel
    } else if (!strncmp(n, "SCHED", 5)) {
      row(L2, 128, 10000, 10, -2, 0, 256, 136, 65536, 100000, &kb);  // the scheduled shape
    } else if (!strcmp(n, "NO_STREAM")) {
      row(COS, 960, 10000, 10, -1, 0, 40, 40, 65536, 100000, &kb);  // long cosine rows: the streamed filter
    } else if (!strcmp(n, "ACCEPTED_ONLY") || !strcmp(n, "FILTER")) {
      row(L2, 128, 10000, 10, -1, 0, 256, 136, 65536, 100000, &kb);
      row(L2, 128, 10000, 10, -1, 0, 40, 40, 65536, 100000, &kb);
    } else {
      // throughput launches: lookahead on the short lists, one-expansion on the long
      row(L2, 128, 10000, 10, -2, 0, 40, 40, 65536, 100000, &kb);
      row(L2, 128, 10000, 10, -2, 0, 256, 136, 65536, 100000, &kb);
    }
  }

  puts("# the cross product, no knobs");
  const int metrics[] = {L2, COS};
  const uint32_t dps[] = {96, 128, 960}, nqs[] = {1, 200, 600, 10000}, ks[] = {10, 100, 500};
  const int viss[] = {0, 12, -1, -2}, filts[] = {-1, 0, 1};
  const uint64_t adjs[][2] = {{0, 40}, {40, 40}, {256, 136}, {512, 300}};
  const size_t ldss[] = {65536, 163840};
  for (int m : metrics)
    for (uint32_t dp : dps)
      for (uint32_t nq : nqs)
        for (uint32_t k : ks)
          for (int vis : viss)
            for (int filt : filts)
              for (auto& adj : adjs)
                for (size_t lds : ldss) row(m, dp, nq, k, vis, filt, adj[0], adj[1], lds, 100000);
  return 0;
}
