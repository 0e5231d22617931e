// `ngt remove index ids-file` (lib/NGT/Command.cpp:452-532) written against
// include/NGT/Index.h: NGT::Index::remove(database, objects) opens the index,
// removes the ids in order -- one that cannot be removed is passed over -- and
// saves it in place.  With a third argument "one" the ids go through
// Index::remove(id) one call each instead, a refusal printed and passed over.
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "NGT/Index.h"

int main(int argc, char** argv) {
  if (argc < 3) {
    std::cerr << "usage: remove_sample index ids-file [one]" << std::endl;
    return 2;
  }
  const std::string database = argv[1];
  std::ifstream is(argv[2]);
  if (!is) {
    std::cerr << "cannot open " << argv[2] << std::endl;
    return 2;
  }
  std::vector<NGT::ObjectID> objects;
  std::string line;
  while (std::getline(is, line))
    if (!line.empty()) objects.push_back((NGT::ObjectID)std::strtol(line.c_str(), nullptr, 10));
  try {
    if (argc > 3 && std::string(argv[3]) == "one") {
      NGT::Index index(database);
      for (NGT::ObjectID id : objects) {
        try {
          index.remove(id);
        } catch (NGT::Exception& err) {
          std::cout << "refused " << id << " : " << err.what() << std::endl;
        }
      }
      index.saveIndex(database);
    } else {
      NGT::Index::remove(database, objects);
    }
  } catch (NGT::Exception& err) {
    std::cerr << "remove_sample: " << err.what() << std::endl;
    return 1;
  }
  std::cout << "removed " << objects.size() << " ids" << std::endl;
  return 0;
}
