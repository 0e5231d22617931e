/*
 * NGT/GraphOptimizer.h -- NGT::GraphOptimizer of NGT 1.13.8
 * (lib/NGT/GraphOptimizer.h) served by the MI355X build.
 *
 * Header-only, like NGT/Index.h: the public fields the reference's CLI sets
 * (Command.cpp:740-756) are plain members, and execute() hands them to the
 * `ngt_optimizer_*` C API of libngt_amd.so, which runs the edge and path
 * adjustment on the GPU and writes the output index.
 *
 *   set, setExtension      lib/NGT/GraphOptimizer.h:545-591 (negative or zero
 *                          keeps the old value)
 *   setProcessingModes     :628-634
 *   execute                :230-300
 *   optimizeSearchParameters :302-384
 *   optimizeNumberOfEdgesForANNG(path, parameter) :511-543
 *
 * Of the three tuning steps, searchParameterOptimization and
 * prefetchParameterOptimization minimise measured query time and are not
 * implemented by this build.  All three default to true as in the reference,
 * and execute() throws while one of them is on -- switch them off as `ngt
 * reconstruct-graph -s n` does.  optimizeSearchParameters(path) with
 * accuracyTableGeneration alone (`ngt optimize-search-parameters -m a`)
 * generates the accuracy table on the GPU and rewrites path/prf; it throws
 * while one of the other two is on.  optimizeNumberOfEdgesForANNG(path,
 * parameter) (`ngt optimize-#-of-edges`) runs its constructions, re-cuts and
 * searches on the GPU, stores the new EdgeSizeForCreation in path/prf and
 * returns it with the estimated accuracy; where the reference's estimate is
 * undefined (it divides by a last sample's accuracy gain of 0 or less, or
 * converts a negative or non-finite double to size_t) it throws the
 * reference's "Cannot optimize the number of edges." with the reason.
 * adjustSearchCoefficients is outside this build's scope.
 */
#ifndef NGT_AMD_CXX_GRAPH_OPTIMIZER_H
#define NGT_AMD_CXX_GRAPH_OPTIMIZER_H

#include <string>
#include <utility>

#include "Index.h"

namespace NGT {

class GraphOptimizer {
 public:
  explicit GraphOptimizer(bool unlog = false) {
    init();
    logDisabled = unlog;
  }
  GraphOptimizer(int outgoing, int incoming, int nofqs, int nofrs, float baseAccuracyFrom, float baseAccuracyTo,
                 float rateAccuracyFrom, float rateAccuracyTo, double gte, double m, bool unlog) {
    init();
    set(outgoing, incoming, nofqs, nofrs, baseAccuracyFrom, baseAccuracyTo, rateAccuracyFrom, rateAccuracyTo, gte, m);
    logDisabled = unlog;
  }

  struct ANNGEdgeOptimizationParameter {  // lib/NGT/GraphOptimizer.h:34-52
    ANNGEdgeOptimizationParameter() { initialize(); }
    void initialize() {
      noOfQueries = 200;
      noOfResults = 50;
      noOfThreads = 16;
      targetAccuracy = 0.9f;
      targetNoOfObjects = 0;
      noOfSampleObjects = 100000;
      maxNoOfEdges = 100;
    }
    size_t noOfQueries;
    size_t noOfResults;
    size_t noOfThreads;
    float targetAccuracy;
    size_t targetNoOfObjects;
    size_t noOfSampleObjects;
    size_t maxNoOfEdges;
  };

  void init() {
    numOfOutgoingEdges = 10;
    numOfIncomingEdges = 120;
    minNumOfEdges = 0;
    numOfQueries = 100;
    numOfResults = 20;
    baseAccuracyRange = std::pair<float, float>(0.30f, 0.50f);
    rateAccuracyRange = std::pair<float, float>(0.80f, 0.90f);
    gtEpsilon = 0.1;
    margin = 0.2;
    logDisabled = false;
    shortcutReduction = true;
    searchParameterOptimization = true;
    prefetchParameterOptimization = true;
    accuracyTableGeneration = true;
  }

  void set(int outgoing, int incoming, int nofqs, int nofrs) {
    if (outgoing >= 0) numOfOutgoingEdges = (size_t)outgoing;
    if (incoming >= 0) numOfIncomingEdges = (size_t)incoming;
    if (nofqs > 0) numOfQueries = (size_t)nofqs;
    if (nofrs > 0) numOfResults = (size_t)nofrs;
  }
  void setExtension(float baseAccuracyFrom, float baseAccuracyTo, float rateAccuracyFrom, float rateAccuracyTo,
                    double gte, double m) {
    if (baseAccuracyFrom > 0.0) baseAccuracyRange.first = baseAccuracyFrom;
    if (baseAccuracyTo > 0.0) baseAccuracyRange.second = baseAccuracyTo;
    if (rateAccuracyFrom > 0.0) rateAccuracyRange.first = rateAccuracyFrom;
    if (rateAccuracyTo > 0.0) rateAccuracyRange.second = rateAccuracyTo;
    if (gte >= -1.0) gtEpsilon = gte;
    if (m > 0.0) margin = m;
  }
  void set(int outgoing, int incoming, int nofqs, int nofrs, float baseAccuracyFrom, float baseAccuracyTo,
           float rateAccuracyFrom, float rateAccuracyTo, double gte, double m) {
    set(outgoing, incoming, nofqs, nofrs);
    setExtension(baseAccuracyFrom, baseAccuracyTo, rateAccuracyFrom, rateAccuracyTo, gte, m);
  }
  void setProcessingModes(bool shortcut = true, bool searchParameter = true, bool prefetchParameter = true,
                          bool accuracyTable = true) {
    shortcutReduction = shortcut;
    searchParameterOptimization = searchParameter;
    prefetchParameterOptimization = prefetchParameter;
    accuracyTableGeneration = accuracyTable;
  }

  void optimizeSearchParameters(const std::string outIndexPath) {
    detail::Err err;
    NGTOptimizer opt = ngt_create_optimizer(logDisabled, err);
    if (opt == NULL) err.raise("GraphOptimizer::optimizeSearchParameters");
    bool ok = ngt_optimizer_set_minimum(opt, (int)numOfOutgoingEdges, (int)numOfIncomingEdges, (int)numOfQueries,
                                        (int)numOfResults, err) &&
              ngt_optimizer_set_processing_modes(opt, searchParameterOptimization, prefetchParameterOptimization,
                                                 accuracyTableGeneration, err) &&
              ngt_optimizer_optimize_search_parameters(opt, outIndexPath.c_str(), err);
    ngt_destroy_optimizer(opt);
    if (!ok) err.raise("GraphOptimizer::optimizeSearchParameters");
  }

  std::pair<size_t, float> optimizeNumberOfEdgesForANNG(const std::string indexPath,
                                                        ANNGEdgeOptimizationParameter &parameter) {
    detail::Err err;
    NGTAnngEdgeOptimizationParameter p = ngt_get_anng_edge_optimization_parameter();
    p.no_of_queries = parameter.noOfQueries;
    p.no_of_results = parameter.noOfResults;
    p.no_of_threads = parameter.noOfThreads;
    p.target_accuracy = parameter.targetAccuracy;
    p.target_no_of_objects = parameter.targetNoOfObjects;
    p.no_of_sample_objects = parameter.noOfSampleObjects;
    p.max_of_no_of_edges = parameter.maxNoOfEdges;
    p.log = false;
    size_t edge = 0;
    float accuracy = 0.0f;
    if (!ngt_optimize_number_of_edges_with_result(indexPath.c_str(), p, &edge, &accuracy, err))
      err.raise("GraphOptimizer::optimizeNumberOfEdgesForANNG");
    return std::make_pair(edge, accuracy);
  }

  void execute(const std::string inIndexPath, const std::string outIndexPath) {
    detail::Err err;
    NGTOptimizer opt = ngt_create_optimizer(logDisabled, err);
    if (opt == NULL) err.raise("GraphOptimizer::execute");
    // the members are size_t; values the C setters would ignore (negative) cannot occur
    bool ok = ngt_optimizer_set_minimum(opt, (int)numOfOutgoingEdges, (int)numOfIncomingEdges, (int)numOfQueries,
                                        (int)numOfResults, err) &&
              ngt_optimizer_set_extension(opt, baseAccuracyRange.first, baseAccuracyRange.second,
                                          rateAccuracyRange.first, rateAccuracyRange.second, gtEpsilon, margin, err) &&
              ngt_optimizer_set_shortcut_reduction(opt, shortcutReduction, minNumOfEdges, err) &&
              ngt_optimizer_set_processing_modes(opt, searchParameterOptimization, prefetchParameterOptimization,
                                                 accuracyTableGeneration, err) &&
              ngt_optimizer_execute(opt, inIndexPath.c_str(), outIndexPath.c_str(), err);
    ngt_destroy_optimizer(opt);
    if (!ok) err.raise("GraphOptimizer::execute");
  }

  size_t numOfOutgoingEdges;
  size_t numOfIncomingEdges;
  size_t minNumOfEdges;
  std::pair<float, float> baseAccuracyRange;
  std::pair<float, float> rateAccuracyRange;
  size_t numOfQueries;
  size_t numOfResults;
  double gtEpsilon;
  double margin;
  bool logDisabled;
  bool shortcutReduction;
  bool searchParameterOptimization;
  bool prefetchParameterOptimization;
  bool accuracyTableGeneration;
};

}  // namespace NGT

#endif
