// hl_scale.hip -- k_scale (hl_scale.h) in a translation unit of its own, built
// and linked like hl_ingest.hip: without the product's device scheduling flag
// (a bandwidth-bound kernel has nothing to gain from it), after the product's
// sources, so that the library's first code object stays hl_encoder.hip's.
// hl_encoder.hip calls launch_scale.
#include <hip/hip_runtime.h>

#define HL_SCALE_KERNELS 1
#include "hl_scale.h"
