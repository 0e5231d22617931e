// edge_optimizer.h -- the reference's edge-count optimisation
// (GraphOptimizer::optimizeNumberOfEdgesForANNG, lib/NGT/GraphOptimizer.h:
// 386-543, with Optimizer::extractAndRemoveRandomQueries, lib/NGT/Optimizer.h:
// 1113-1137) as pure host arithmetic around callbacks: the query draw over a
// passed-in rand() stream, the sample loop (12500, 25000, ... stored objects),
// per sample the pseudo ground truth and the walk over the edge counts 5, 10,
// 20, 30, ..., the estimate for the target object count and the rounding of the
// path form.  float where the reference has float, double where it has
// double, size_t where it has size_t.  No HIP call and no file: construction,
// graph extraction, the re-cut to K edges and the searches enter through
// EdgeCallbacks, so a host program can drive the whole procedure
// (tests/cxx/edge_optimizer_host.cpp).  ngt_amd_optimize_edges (edges_api.cpp)
// supplies the device work.
//
// Two deliberate differences from the reference.  The maxEpsilon loop's
// wall-clock clause is a guard on work, as in accuracy_table.h.  And where the
// reference's estimate converts a negative, non-finite or too large double to
// size_t -- the last sample's gain it divides by is 0 when the sample stopped
// at its first edge count, and may be negative -- which is undefined, this
// restatement returns the reference's "Cannot optimize the number of edges."
// error with a clause that says why.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <functional>
#include <string>
#include <vector>

#include "accuracy_table.h"

namespace ngt_amd {

// GraphOptimizer::ANNGEdgeOptimizationParameter (GraphOptimizer.h:34-52)
struct EdgeParams {
  size_t nqueries = 200;
  size_t nresults = 50;
  size_t nthreads = 16;  // accepted and unused: the construction's result does not depend on it
  float target_accuracy = 0.9f;
  size_t target_objects = 0;  // 0: the object repository size
  size_t sample_objects = 100000;
  size_t max_edges = 100;
};

struct EdgeCallbacks {
  // createIndex(threads, end_id): insert the stored objects below end_id that
  // have no node yet into the graph and tree the previous sample left
  std::function<std::string(uint64_t)> build;
  // extractGraph: keep the current graph as the source of the re-cuts
  std::function<std::string()> extract;
  // reconstructANNGFromANNG(extracted graph, index, K)
  std::function<std::string(size_t)> recut;
  AccuracySearch search;
};

struct EdgeStep {
  size_t edge;
  double accuracy;
};
struct EdgeSample {
  size_t objects = 0;  // noOfObjects
  size_t edge = 0;
  double accuracy = 0.0, gain = 0.0;
  float max_epsilon = 0.0f;
  bool guard_fired = false;
  std::vector<EdgeStep> steps;  // per K the accuracy
};
struct EdgeTrace {
  size_t draws = 0;  // rand() values the query draw took
  std::vector<EdgeSample> samples;
};

// The rand() stream of a fresh process (glibc, seed 1) as the library restates
// it (edges_api.cpp): what the reference's CLI draws the queries from.
std::function<int()> edge_fresh_rand();

// extractAndRemoveRandomQueries: draws over next() (the rand() stream) until
// nqueries stored objects are drawn; a drawn object becomes a query (its
// values as floats) and its flag in valid [osize] is cleared.  draws receives
// the number of values taken.
std::string edge_draw_queries(const std::function<int()>& next, const std::function<const void*(uint64_t)>& row,
                              std::vector<uint8_t>& valid, uint64_t osize, uint32_t dim, int object_type,
                              size_t nqueries, std::vector<float>& queries, size_t* draws);

// The per-sample walk (GraphOptimizer.h:386-433) on the index as build() left it.
std::string edge_optimize_sample(const EdgeCallbacks& cb, const std::vector<float>& queries, uint32_t dim,
                                 int object_type, size_t nresults, float target_accuracy, size_t max_edges,
                                 double guard, EdgeSample& sample);

// The estimate (:479-508) from the samples.  target_no: the sample size the
// loop stopped at (the refusal of fewer than two samples prints it).
std::string edge_estimate(const std::vector<EdgeSample>& samples, size_t target_objects, float target_accuracy,
                          uint64_t osize, size_t target_no, size_t& edge, float& accuracy);

// The path form's rounding and cap (:528-531).
size_t edge_round(size_t edge, size_t max_edges);

// optimizeNumberOfEdgesForANNG(index, parameter) after the queries are drawn
// and the graph and tree are cleared: the sample loop and the estimate.  valid
// [osize] is the repository after the draw.
std::string edge_optimize(const EdgeCallbacks& cb, const std::vector<uint8_t>& valid, uint64_t osize, uint32_t dim,
                          int object_type, const std::vector<float>& queries, EdgeParams params, double guard,
                          size_t& edge, float& accuracy, EdgeTrace* trace = nullptr);

}  // namespace ngt_amd
