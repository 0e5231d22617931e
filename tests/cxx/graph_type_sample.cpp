// graph_type_sample.cpp -- a KNNG built through the reference's C++ API:
// NGT::Property::graphType = GraphTypeKNNG, then NGT::Index::create, append,
// createIndex and save, compiled against include/ and linked with
// libngt_amd.so.  Test infrastructure: tests/test_gpu_graph_types.py builds it
// and compares the files it saves with the reference's `ngt create -g k -p 1`.
//
//   graph_type_sample <index> <data.tsv> <dim>
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "NGT/Index.h"

int main(int argc, char** argv) {
  if (argc < 4) {
    std::cerr << "usage: graph_type_sample <index> <data.tsv> <dim>" << std::endl;
    return 2;
  }
  try {
    const std::string path = argv[1];
    NGT::Property property;
    property.dimension = atoi(argv[3]);
    property.objectType = NGT::ObjectSpace::ObjectType::Float;
    property.distanceType = NGT::Property::distanceOf("L2");
    property.graphType = NGT::Property::GraphType::GraphTypeKNNG;
    property.edgeSizeForCreation = 10;
    property.edgeSizeForSearch = 40;
    property.batchSizeForCreation = 200;
    NGT::Index::create(path, property);
    NGT::Index index(path);
    NGT::Property stored;
    index.getProperty(stored);
    if (stored.graphType != NGT::Property::GraphType::GraphTypeKNNG) {
      std::cerr << "the created index is not a KNNG: graphType " << stored.graphType << std::endl;
      return 1;
    }
    std::ifstream is(argv[2]);
    std::string line;
    while (std::getline(is, line)) {
      std::vector<float> v;
      std::stringstream ls(line);
      float x;
      while (ls >> x) v.push_back(x);
      if (v.empty()) continue;
      v.resize(property.dimension);
      index.append(v);
    }
    index.createIndex(1);
    index.save();
    printf("objects %zu\n", index.getObjectRepositorySize() - 1);
    return 0;
  } catch (NGT::Exception& err) {
    std::cerr << "Error " << err.what() << std::endl;
    return 1;
  }
}
