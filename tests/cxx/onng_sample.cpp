// What `ngt reconstruct-graph -m S -s n -o <o> -i <i> -E <minE> in out` does
// (Command.cpp:740-756), written against NGT/GraphOptimizer.h.
#include <cstdlib>
#include <iostream>

#include "NGT/GraphOptimizer.h"

int main(int argc, char** argv) {
  if (argc < 6) {
    std::cerr << "usage: onng_sample in out outgoing incoming min-edges [tuning]" << std::endl;
    return 2;
  }
  try {
    NGT::GraphOptimizer optimizer(true);
    optimizer.shortcutReduction = true;
    const bool tuning = argc > 6;
    optimizer.searchParameterOptimization = tuning;
    optimizer.prefetchParameterOptimization = tuning;
    optimizer.accuracyTableGeneration = tuning;
    optimizer.minNumOfEdges = (size_t)atol(argv[5]);
    optimizer.set(atoi(argv[3]), atoi(argv[4]), -1, -1);
    optimizer.execute(argv[1], argv[2]);
  } catch (NGT::Exception& err) {
    std::cerr << "error: " << err.what() << std::endl;
    return 1;
  }
  std::cout << "Successfully completed." << std::endl;
  return 0;
}
