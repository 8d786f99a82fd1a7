// Test-only host build of the layer pyramid (hartallo_amd/csrc/hl_pyramid.h):
// the per-span code k_pyramid's lanes run, looped over a plane on the host
// (tests/test_emu_pyramid.py).
#include "../../hartallo_amd/csrc/hl_pyramid.h"

// Levels 1..K of one dense plane of w x h samples (w a multiple of 8, h of
// 2^K); dst[j] = the plane of level j + 1, (w >> (j + 1)) x (h >> (j + 1)).
// Returns 0, or -1 for a size or K the kernel does not take.
extern "C" int32_t pyr_emu_plane(const uint8_t* src, int32_t w, int32_t h, int32_t K, uint8_t* const* dst)
{
    if (!src || !dst || w <= 0 || h <= 0 || K < 1 || K > 3 || (w & 7) || (h & ((1 << K) - 1))) return -1;
    for (int j = 0; j < K; ++j)
        if (!dst[j]) return -1;
    if (K == 1) hl::pyr_plane<1>(src, w, h, dst);
    else if (K == 2) hl::pyr_plane<2>(src, w, h, dst);
    else hl::pyr_plane<3>(src, w, h, dst);
    return 0;
}
