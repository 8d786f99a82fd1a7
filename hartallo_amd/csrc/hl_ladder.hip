// hl_ladder.hip -- k_scale_fan (hl_ladder.h) in a translation unit of its own,
// built and linked like hl_scale.hip: without the product's device scheduling
// flag, after the product's sources and the two objects before it, so that the
// library's first five code objects stay what they were.  hl_encoder.hip calls
// launch_ladder.
#include <hip/hip_runtime.h>

#define HL_LADDER_KERNELS 1
#include "hl_ladder.h"
