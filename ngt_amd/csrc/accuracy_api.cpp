// accuracy_api.cpp -- ngt_amd_accuracy_table: the accuracy-table procedure of
// accuracy_table.cpp with its searches on the device.  Every batch is one
// ngt_amd_search with tree seeds; the only other device work is reading the
// stored objects the queries are the means of.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <exception>
#include <map>
#include <string>
#include <vector>

#include "../../include/ngt_amd.h"
#include "accuracy_table.h"
#include "index_internal.h"

using namespace ngt_amd;

static int accuracy_table(ngt_amd_index* ix, uint64_t nresults, uint64_t nqueries, float* eps_out, double* acc_out,
                          uint32_t* n, float* max_epsilon) {
  if (!ix || !eps_out || !acc_out || !n) return fail("ngt_amd_accuracy_table: bad arguments");
  const uint32_t capacity = *n;
  *n = 0;
  // decided before any device work
  std::string e = accuracy_refusal(ix->edge_size_for_search, nresults);
  if (!e.empty()) return fail("%s", e.c_str());
  if (ix->nrows < 2 || !ix->rows.p) return fail("ngt_amd_accuracy_table: the index has no objects");
  // every batch holds nqueries x nresults results on the host: neither may exceed
  // the repository (no search returns more results, no walk visits more ids)
  if (nresults > ix->nrows)
    return fail("ngt_amd_accuracy_table: %llu results asked of a repository of %llu slots",
                (unsigned long long)nresults, (unsigned long long)ix->nrows);
  if (nqueries > ix->nrows)
    return fail("ngt_amd_accuracy_table: %llu queries asked of a repository of %llu slots",
                (unsigned long long)nqueries, (unsigned long long)ix->nrows);
  if (!ix->has_graph || !ix->has_tree)
    return fail("ngt_amd_accuracy_table: the index needs a graph and a tree (the searches take tree seeds)");
  HIP_OK(hipSetDevice(ix->device));

  std::map<uint64_t, std::vector<uint8_t>> fetched;  // the stored objects read back, by id
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
  std::vector<float> queries;
  e = accuracy_extract_queries(row, ix->h_valid.data(), ix->nrows, ix->dim, ix->otype, nqueries, queries);
  if (copy_failed) return fail("ngt_amd_accuracy_table: reading the stored objects failed");
  if (!e.empty()) return fail("%s", e.c_str());

  std::vector<uint64_t> cnt;
  AccuracySearch search = [&](AccuracyBatch& b) -> std::string {
    const ngt_amd_search_params p = library_search_params(ix->nrows, (uint32_t)b.size, b.epsilon, -1.0f /* FLT_MAX */,
                                                          b.edge_size, NGT_AMD_SEED_TREE);
    cnt.assign((size_t)b.nq * NGT_AMD_COUNTERS_PER_QUERY, 0);
    if (ngt_amd_search(ix, &p, b.queries, b.nq, nullptr, nullptr, b.ids.data(), b.dists.data(), b.n.data(),
                       cnt.data()))
      return ngt_amd_last_error();
    for (uint32_t q = 0; q < b.nq; q++) b.counts[q] = cnt[(size_t)q * NGT_AMD_COUNTERS_PER_QUERY];
    return "";
  };
  std::vector<std::pair<float, double>> table;
  AccuracyTrace trace;
  e = accuracy_generate(search, queries, ix->dim, ix->otype, nresults, kAccuracyWorkGuard, table, &trace);
  if (!e.empty()) return fail("%s", e.c_str());
  if (max_epsilon) *max_epsilon = trace.max_epsilon;
  *n = (uint32_t)table.size();
  if (table.size() > capacity)
    return fail("ngt_amd_accuracy_table: the table has %zu entries, the arrays hold %u", table.size(), capacity);
  for (size_t i = 0; i < table.size(); i++) {
    eps_out[i] = table[i].first;
    acc_out[i] = table[i].second;
  }
  return 0;
}

extern "C" int ngt_amd_accuracy_table(ngt_amd_index* ix, uint64_t nresults, uint64_t nqueries, float* eps_out,
                                      double* acc_out, uint32_t* n, float* max_epsilon) {
  try {  // no exception crosses the C boundary
    return accuracy_table(ix, nresults, nqueries, eps_out, acc_out, n, max_epsilon);
  } catch (std::exception& err) {
    return fail("ngt_amd_accuracy_table: %s", err.what());
  }
}
