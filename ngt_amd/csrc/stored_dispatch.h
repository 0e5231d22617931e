// stored_dispatch.h -- the metric x stored-type combinations whose objects a
// build session holds: the table construction (build_kernels.hip) and removal
// (remove_kernels.hip) instantiate their distance kernels from.  LAUNCH(metric,
// type) is expanded for the combination at hand; any other makes the enclosing
// function return hipErrorInvalidValue.  Search's NGT_DISPATCH
// (search_kernels.hip) is a wider table and stays its own.
#pragma once

#define NGT_STORED_DISPATCH(METRIC, OTYPE, LAUNCH)                             \
  do {                                                                         \
    if ((OTYPE) == kFloat) {                                                   \
      switch (METRIC) {                                                        \
        case kL1: LAUNCH(kL1, float); break;                                   \
        case kL2: LAUNCH(kL2, float); break;                                   \
        case kAngle: LAUNCH(kAngle, float); break;                             \
        case kCosine: LAUNCH(kCosine, float); break;                           \
        case kNormalizedAngle: LAUNCH(kNormalizedAngle, float); break;         \
        case kNormalizedCosine: LAUNCH(kNormalizedCosine, float); break;       \
        case kNormalizedL2: LAUNCH(kNormalizedL2, float); break;               \
        case kSparseJaccard: LAUNCH(kSparseJaccard, float); break;             \
        case kPoincare: LAUNCH(kPoincare, float); break;                       \
        case kLorentz: LAUNCH(kLorentz, float); break;                         \
        default: return hipErrorInvalidValue;                                  \
      }                                                                        \
    } else if ((OTYPE) == kUint8) {                                            \
      switch (METRIC) {                                                        \
        case kL1: LAUNCH(kL1, uint8_t); break;                                 \
        case kL2: LAUNCH(kL2, uint8_t); break;                                 \
        case kHamming: LAUNCH(kHamming, uint8_t); break;                       \
        case kJaccard: LAUNCH(kJaccard, uint8_t); break;                       \
        case kAngle: LAUNCH(kAngle, uint8_t); break;                           \
        case kCosine: LAUNCH(kCosine, uint8_t); break;                         \
        case kNormalizedAngle: LAUNCH(kNormalizedAngle, uint8_t); break;       \
        case kNormalizedCosine: LAUNCH(kNormalizedCosine, uint8_t); break;     \
        case kNormalizedL2: LAUNCH(kNormalizedL2, uint8_t); break;             \
        default: return hipErrorInvalidValue;                                  \
      }                                                                        \
    } else {                                                                   \
      return hipErrorInvalidValue;                                             \
    }                                                                          \
  } while (0)
