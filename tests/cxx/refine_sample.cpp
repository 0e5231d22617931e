// What `ngt refine-anng [-e epsilon] [-a expected-accuracy] [-k edges]
// [-E explored-edges] [-b batch-size] in out` does (Command.cpp:806-848),
// written against NGT/GraphReconstructor.h.
#include <climits>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "NGT/GraphReconstructor.h"

int main(int argc, char** argv) {
  float epsilon = 0.1f, expectedAccuracy = 0.0f;
  int noOfEdges = 0, exploreEdgeSize = INT_MIN;
  size_t batchSize = 10000;
  std::vector<std::string> paths;
  for (int i = 1; i < argc; i++) {
    const bool option = argv[i][0] == '-' && strlen(argv[i]) == 2 && i + 1 < argc;
    if (!option) {
      paths.push_back(argv[i]);
      continue;
    }
    const char* v = argv[++i];
    switch (argv[i - 1][1]) {
      case 'e': epsilon = (float)atof(v); break;
      case 'a': expectedAccuracy = (float)atof(v); break;
      case 'k': noOfEdges = atoi(v); break;
      case 'E': exploreEdgeSize = (int)atof(v); break;
      case 'b': batchSize = (size_t)atol(v); break;
      default:
        std::cerr << "unknown option " << argv[i - 1] << std::endl;
        return 2;
    }
  }
  if (paths.size() != 2) {
    std::cerr << "usage: refine_sample [-e epsilon] [-a expected-accuracy] [-k edges] [-E explored-edges] "
                 "[-b batch-size] anng-index refined-anng-index" << std::endl;
    return 2;
  }
  try {
    NGT::Index index(paths[0]);
    NGT::GraphReconstructor::refineANNG(index, epsilon, expectedAccuracy, noOfEdges, exploreEdgeSize, batchSize);
    index.saveIndex(paths[1]);
  } catch (NGT::Exception& err) {
    std::cerr << "Error!! Cannot refine the index. " << err.what() << std::endl;
    return 1;
  }
  return 0;
}
