// Test-only host build of the scene-cut analysis (hartallo_amd/csrc/hl_scene.h):
// the staging indices and per-macroblock code k_scene's workgroups run, looped
// over a frame pair on the host (tests/test_emu_scene.py).
#include "../../hartallo_amd/csrc/hl_scene.h"

// One dense w x h luma frame against the previous one, search range R:
// mb[2 a] = inter, mb[2 a + 1] = intra of macroblock a; sums[0] = P,
// sums[1] = I.  Returns 0, or -1 for a size or range the kernel does not take.
extern "C" int32_t scene_emu_frame(const uint8_t* cur, const uint8_t* prev, int32_t w, int32_t h, int32_t R, uint32_t* mb, uint64_t* sums)
{
    if (!cur || !prev || !mb || !sums || w <= 0 || h <= 0 || (w & 15) || (h & 15) || R < 0 || R > hl::kScMaxR) return -1;
    sums[0] = sums[1] = 0;
    hl::scene_frame_host(cur, prev, w, h, R, mb, sums);
    return 0;
}
