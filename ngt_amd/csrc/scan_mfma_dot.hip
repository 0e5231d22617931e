// scan_mfma_dot.hip -- ngt_scan_mfma_kernel (scan_mfma_kernel.h) for the dot
// family: Angle, and one instantiation for Normalized Cosine / L2 / Angle whose
// finish is picked at run time (MfmaScanArgs::fin).  3-pass filter only.  A
// translation unit of its own because it is compiled without packed fp32
// operations, as scan_mfma_wide.hip is (the comparator's scalar FMA chains on
// one lane), while scan_mfma.hip keeps its flags and its code.
#include "scan_mfma_kernel.h"

namespace ngt_amd {

hipError_t launch_scan_mfma_dot(const MfmaScanArgs& a, int metric, size_t lds, uint32_t grid, hipStream_t s) {
  if (metric == kAngle) launch_scan_mfma_t<kAngle, 3>(a, lds, grid, s);
  else if (metric == kNormalizedAngle || metric == kNormalizedCosine || metric == kNormalizedL2)
    launch_scan_mfma_t<kScanDot, 3>(a, lds, grid, s);
  else return hipErrorNotSupported;
  return hipGetLastError();
}

}  // namespace ngt_amd
