// What `ngt optimize-search-parameters -m a [-q queries] [-n results] index`
// does (Command.cpp:762-803), written against NGT/GraphOptimizer.h.
#include <cstdlib>
#include <iostream>

#include "NGT/GraphOptimizer.h"

int main(int argc, char** argv) {
  if (argc < 2) {
    std::cerr << "usage: accuracy_sample index [queries [results [mode(a|s|p|-)]]]" << std::endl;
    return 2;
  }
  try {
    const size_t nOfQueries = argc > 2 ? (size_t)atol(argv[2]) : 100;
    const size_t nOfResults = argc > 3 ? (size_t)atol(argv[3]) : 20;
    const char mode = argc > 4 ? argv[4][0] : 'a';
    NGT::GraphOptimizer graphOptimizer(true);
    graphOptimizer.searchParameterOptimization = (mode == '-' || mode == 's') ? true : false;
    graphOptimizer.prefetchParameterOptimization = (mode == '-' || mode == 'p') ? true : false;
    graphOptimizer.accuracyTableGeneration = (mode == '-' || mode == 'a') ? true : false;
    graphOptimizer.numOfQueries = nOfQueries;
    graphOptimizer.numOfResults = nOfResults;
    graphOptimizer.set(0, 0, nOfQueries, nOfResults);
    graphOptimizer.optimizeSearchParameters(argv[1]);
  } catch (NGT::Exception& err) {
    std::cerr << "error: " << err.what() << std::endl;
    return 1;
  }
  std::cout << "Successfully completed." << std::endl;
  return 0;
}
