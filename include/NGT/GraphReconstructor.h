/*
 * NGT/GraphReconstructor.h -- NGT::GraphReconstructor::refineANNG of NGT 1.13.8
 * (lib/NGT/GraphReconstructor.h:803-924) served by the MI355X build.
 *
 * Header-only, like NGT/Index.h: refineANNG hands its arguments to
 * ngt_refine_anng of libngt_amd.so, which searches every stored object on the
 * GPU in batches and merges the results into the graph there (outgoing edges,
 * incoming edges when noOfEdges == 0, the final prune when noOfEdges > 0).  The
 * index is refined in place; Index::saveIndex then writes what `ngt
 * refine-anng` writes.  Errors surface as NGT::Exception carrying the
 * reference's text after "GraphReconstructor::refineANNG: ".
 *
 * Two deviations: on an error the index's graph is left as it was (the
 * reference keeps the batches it finished), and batchSize == 0 is an error
 * (the reference never leaves its loop).  `unlog` only silenced the reference's
 * progress lines; this build prints none.  The other members of the
 * reference's GraphReconstructor are reached through NGT::GraphOptimizer
 * (NGT/GraphOptimizer.h) or are outside this build's scope.
 */
#ifndef NGT_AMD_CXX_GRAPH_RECONSTRUCTOR_H
#define NGT_AMD_CXX_GRAPH_RECONSTRUCTOR_H

#include <climits>
#include <cstddef>

#include "Index.h"

namespace NGT {

class GraphReconstructor {
 public:
  static void refineANNG(NGT::Index& index, bool unlog, float epsilon = 0.1, float accuracy = 0.0, int noOfEdges = 0,
                         int exploreEdgeSize = INT_MIN, size_t batchSize = 10000) {
    (void)unlog;
    refineANNG(index, epsilon, accuracy, noOfEdges, exploreEdgeSize, batchSize);
  }

  static void refineANNG(NGT::Index& index, float epsilon = 0.1, float accuracy = 0.0, int noOfEdges = 0,
                         int exploreEdgeSize = INT_MIN, size_t batchSize = 10000) {
    detail::Err err;
    if (!ngt_refine_anng(index.getHandle(), epsilon, accuracy, noOfEdges, exploreEdgeSize, batchSize, err))
      err.raise("NGT::GraphReconstructor::refineANNG");
  }
};

}  // namespace NGT

#endif
