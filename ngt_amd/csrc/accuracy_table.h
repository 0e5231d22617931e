// accuracy_table.h -- the reference's accuracy-table generation
// (Optimizer::generateAccuracyTable, lib/NGT/Optimizer.h:1495-1573) as pure
// host arithmetic around a search callback: query extraction (:1139-1199),
// the maxEpsilon loop and the pseudo ground truth (:1425-1493), the epsilon
// sweep with its evaluation (:108-128, :175-276, :345-507), the table filter
// and Index::AccuracyTable::getString.  float where the reference has float,
// double where it has double.  No HIP call and no file: the searches enter
// through AccuracySearch, so a host program can drive the whole procedure
// (tests/cxx/accuracy_table_host.cpp).  ngt_amd_accuracy_table
// (accuracy_api.cpp) supplies the device searches.
//
// The one deliberate difference from the reference: its maxEpsilon loop also
// stops when the wall time of the batch's last query exceeds 40 x that
// query's time at epsilon 0 (:1459-1464), which no second run reproduces.
// Here the same test is made on work: the last query's distance computations
// exceed 40 x their count at epsilon 0.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <functional>
#include <string>
#include <utility>
#include <vector>

namespace ngt_amd {

constexpr size_t kAccuracySweepSize = 20;    // Command::SearchParameters() (Command.h:39-52)
constexpr double kAccuracyWorkGuard = 40.0;  // the reference's factor on time (:1461)

// One batch over `queries` ([nq][dim] floats, converted to the object type by
// the search as Index::allocateObject does).  The callback fills ids/dists
// [nq][size] ascending, n [nq] and counts [nq] (distance computations).
struct AccuracyBatch {
  const float* queries;
  uint32_t nq, dim;
  size_t size;
  float epsilon;
  int64_t edge_size;  // SearchContainer::edgeSize: -1 the property's, 0 all edges
  std::vector<uint32_t> ids;
  std::vector<float> dists;
  std::vector<uint32_t> n;
  std::vector<uint64_t> counts;
};
// Returns an empty string, or the error that ends the procedure.
typedef std::function<std::string(AccuracyBatch&)> AccuracySearch;

// `stream << x` with the stream's defaults (6 significant digits).
std::string format_stream(float x);
std::string format_stream(double x);

// The refusals decided before any search: EdgeSizeForSearch other than 0 / -2
// (:1500-1504), and fewer ground-truth results than the sweep's result size
// (loadGroundTruth, :247-251).  Empty when the procedure may run.
std::string accuracy_refusal(int32_t edge_size_for_search, size_t nresults);

// extractQueries(nqueries, queries): row(id) returns the stored object
// (element type by object_type: 1 uint8, 2 float), valid [osize].
std::string accuracy_extract_queries(const std::function<const void*(uint64_t)>& row, const uint8_t* valid,
                                     uint64_t osize, uint32_t dim, int object_type, size_t nqueries,
                                     std::vector<float>& queries);
// outputObject (:1004-1031) per query, then Index::allocateObject(line):
// the queries every search after the maxEpsilon loop takes.
std::string accuracy_query_text(const std::vector<float>& queries, uint32_t dim, int object_type);
std::vector<float> accuracy_parse_queries(const std::string& text);

struct AccuracyTrace {
  float max_epsilon = 0.0f;
  bool guard_fired = false;  // the work guard, not the identity rule, ended the maxEpsilon loop
};

// The parts the edge-count optimisation (edge_optimizer.h) shares with the
// table: one batch with its outputs sized and checked; the maxEpsilon loop and
// the pseudo ground truth of generatePseudoGroundTruth (:1425-1493) -- `rounded`
// receives the queries the query stream's text gives back, which every later
// search takes; and evaluate (:175-226) of one batch against that ground truth
// over the batch's own result size (a float mean, returned as double).
struct AccuracyGroundTruth {  // per query: ids and distances as the evaluation output prints them
  std::vector<std::vector<uint32_t>> ids;
  std::vector<std::vector<double>> dists;
};
std::string accuracy_run_batch(const AccuracySearch& search, AccuracyBatch& b);
std::string accuracy_pseudo_ground_truth(const AccuracySearch& search, const std::vector<float>& queries, uint32_t dim,
                                         int object_type, size_t nresults, double guard, std::vector<float>& rounded,
                                         AccuracyGroundTruth& gt, AccuracyTrace& trace);
std::string accuracy_evaluate(const AccuracyGroundTruth& gt, const AccuracyBatch& b, double& accuracy);

// The whole procedure on extracted queries.  guard <= 0 leaves the work guard
// out (the identity rule and e < 10 alone).
std::string accuracy_generate(const AccuracySearch& search, const std::vector<float>& queries, uint32_t dim,
                              int object_type, size_t nresults, double guard,
                              std::vector<std::pair<float, double>>& table, AccuracyTrace* trace = nullptr);
// Index::AccuracyTable::getString
std::string accuracy_table_string(const std::vector<std::pair<float, double>>& table);

}  // namespace ngt_amd
