// Test-only host build of the quality metric (hartallo_amd/csrc/hl_quality.h):
// the staging indices and the per-strip and per-window code k_quality's
// workgroups run, looped over a plane pair on the host
// (tests/test_emu_quality.py).
#include "../../hartallo_amd/csrc/hl_quality.h"

// One dense w x h plane pair (a = source, b = reconstruction): *sse = sum
// (a - b)^2, *ssim_q30 = sum Q; mb (or null; w, h multiples of 16 then) = the
// SSE of every 16x16 macroblock.  Returns 0, or -1 for a size the kernel does
// not take.
extern "C" int32_t quality_emu_plane(const uint8_t* a, const uint8_t* b, int32_t w, int32_t h, uint64_t* sse, int64_t* ssim_q30, uint32_t* mb)
{
    if (!a || !b || !sse || !ssim_q30 || w <= 0 || h <= 0 || (w & 7) || (h & 7) || (mb && ((w & 15) || (h & 15)))) return -1;
    *sse = 0;
    *ssim_q30 = 0;
    hl::quality_plane_host(a, b, w, h, sse, ssim_q30, mb);
    return 0;
}

// floor(num 2^30 / den) as the kernel forms it (den > 0)
extern "C" int64_t quality_emu_div30(int64_t num, int64_t den) { return hl::q_div30(num, den); }
