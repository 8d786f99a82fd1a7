// hl_ingest.hip -- k_ingest and k_ingest_edge (hl_ingest.h) in a translation unit of their own.
// It is compiled without the product's device scheduling flag: under
// -amdgpu-sched-strategy=iterative-ilp the register allocator of the ROCm 7.2
// compiler crashes on the planar-RGB kernel (VirtRegAuxInfo::isRematerializable),
// and a bandwidth-bound kernel with one straight-line tile per lane has
// nothing to gain from that strategy.  hl_encoder.hip calls launch_ingest.
#include <hip/hip_runtime.h>

#define HL_INGEST_KERNELS 1
#include "hl_ingest.h"
