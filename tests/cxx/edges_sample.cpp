// What `ngt optimize-#-of-edges [-q queries] [-k results] [-a accuracy]
// [-o objects] [-s sample objects] [-e max edges] index` does
// (Command.cpp:1030-1059), written against NGT/GraphOptimizer.h.  The options
// follow the index path here.
#include <cstdlib>
#include <cstring>
#include <iostream>

#include "NGT/GraphOptimizer.h"

int main(int argc, char** argv) {
  if (argc < 2 || argc % 2 != 0) {
    std::cerr << "usage: edges_sample index [-q n] [-k n] [-a x] [-o n] [-s n] [-e n]" << std::endl;
    return 2;
  }
  try {
    NGT::GraphOptimizer::ANNGEdgeOptimizationParameter parameter;
    for (int i = 2; i + 1 < argc; i += 2) {
      if (strcmp(argv[i], "-q") == 0) parameter.noOfQueries = (size_t)atol(argv[i + 1]);
      else if (strcmp(argv[i], "-k") == 0) parameter.noOfResults = (size_t)atol(argv[i + 1]);
      else if (strcmp(argv[i], "-a") == 0) parameter.targetAccuracy = (float)atof(argv[i + 1]);
      else if (strcmp(argv[i], "-o") == 0) parameter.targetNoOfObjects = (size_t)atol(argv[i + 1]);
      else if (strcmp(argv[i], "-s") == 0) parameter.noOfSampleObjects = (size_t)atol(argv[i + 1]);
      else if (strcmp(argv[i], "-e") == 0) parameter.maxNoOfEdges = (size_t)atol(argv[i + 1]);
    }
    NGT::GraphOptimizer graphOptimizer(false);
    auto optimizedEdge = graphOptimizer.optimizeNumberOfEdgesForANNG(argv[1], parameter);
    std::cout << "The optimized # of edges=" << optimizedEdge.first << "(" << optimizedEdge.second << ")" << std::endl;
  } catch (NGT::Exception& err) {
    std::cerr << "error: " << err.what() << std::endl;
    return 1;
  }
  std::cout << "Successfully completed." << std::endl;
  return 0;
}
