// Test-only host build of the rendition ladder (hl_amd_encode_ladder_frames,
// hartallo_amd/csrc/hl_ladder.h): one frame ingest (hl_ingest.h) per frame at
// the source size, then k_scale_fan's block selection and per-lane functions
// looped over a launch in the kernel's order -- ld_frames -- into every rung's
// planes (tests/test_emu_ladder.py).
#include <vector>

#include "../../hartallo_amd/csrc/hl_ingest.h"
#include "../../hartallo_amd/csrc/hl_ladder.h"

// the rungs of a ladder from sizes[4 r ..] = dw, dh, w, h; false for what the library refuses
static bool ladder_args(int32_t sw, int32_t sh, int32_t count, const int32_t* sizes, hl::LdArgs* A)
{
    if (count < 1 || count > hl::kLdMaxRungs || !sizes || sw <= 0 || sh <= 0) return false;
    *A = hl::LdArgs{};
    A->count = count;
    for (int r = 0; r < count; ++r)
        if (!hl::sk_parm(sw, sh, (sw + 15) & ~15, sizes[4 * r], sizes[4 * r + 1], sizes[4 * r + 2], sizes[4 * r + 3], &A->rung[r].parm)) return false;
    return true;
}

// n frames of sw x sh samples in format fmt (frame i's planes and pitches at
// [3 i ..], as hl_amd_frame_t has them; pitch 0 = dense), each converted into
// intermediate I420 planes of the source size rounded up to 16, and fanned out
// to `count` rungs: out[r] holds rung r's n frames, Y | U | V dense at its coded
// size w_r x h_r, one after another.  Returns 0, or -1 for what the library refuses.
extern "C" int32_t ladder_emu_frames(int32_t fmt, int32_t matrix, int32_t range, int32_t sw, int32_t sh, int32_t count, const int32_t* sizes, int32_t n,
                                     const uint8_t* const* planes, const int64_t* pitches, uint8_t* const* out)
{
    hl::LdArgs A;
    if (fmt < 0 || fmt >= hl::IN_FORMATS || matrix < 0 || matrix > 1 || range < 0 || range > 1 || n < 1 || !planes || !pitches || !out ||
        !ladder_args(sw, sh, count, sizes, &A))
        return -1;
    const int SW = (sw + 15) & ~15, SH = (sh + 15) & ~15;
    const size_t fb = (size_t)SW * SH * 3 / 2;
    std::vector<uint8_t> mid(fb * n);
    std::vector<hl::SkFrame> tab(n);
    const hl::InCoef C = hl::in_coef_of(matrix, range);
    for (int i = 0; i < n; ++i) {
        hl::InFrame F{};
        for (int c = 0; c < hl::in_planes(fmt); ++c) {
            const int64_t rb = hl::in_row_bytes(fmt, c, sw), pitch = pitches[3 * i + c];
            if (!planes[3 * i + c] || pitch < 0 || (pitch && pitch < rb)) return -1;
            F.plane[c] = planes[3 * i + c];
            F.pitch[c] = pitch ? pitch : rb;
        }
        F.dst[0] = mid.data() + fb * i;
        F.dst[1] = F.dst[0] + (size_t)SW * SH;
        F.dst[2] = F.dst[1] + (size_t)SW * SH / 4;
        switch (fmt) {
        case hl::IN_I420: hl::in_frame_display<hl::IN_I420>(F, C, SW, SH, sw, sh); break;
        case hl::IN_NV12: hl::in_frame_display<hl::IN_NV12>(F, C, SW, SH, sw, sh); break;
        case hl::IN_RGB24: hl::in_frame_display<hl::IN_RGB24>(F, C, SW, SH, sw, sh); break;
        case hl::IN_RGBA32: hl::in_frame_display<hl::IN_RGBA32>(F, C, SW, SH, sw, sh); break;
        default: hl::in_frame_display<hl::IN_RGBP>(F, C, SW, SH, sw, sh); break;
        }
        tab[i] = hl::SkFrame{{F.dst[0], F.dst[1], F.dst[2]}, {nullptr, nullptr, nullptr}};
    }
    A.tab = tab.data();
    for (int r = 0; r < count; ++r) {
        if (!out[r]) return -1;
        const size_t ny = (size_t)A.rung[r].parm.W * A.rung[r].parm.H;
        A.rung[r].dst[0] = out[r];
        A.rung[r].dst[1] = out[r] + ny;
        A.rung[r].dst[2] = out[r] + ny + ny / 4;
        A.rung[r].stride = ny + ny / 2;
    }
    if (!hl::ld_args_ok(A)) return -1;
    std::vector<uint32_t> lds(hl::ld_lds_bytes(A) / sizeof(uint32_t));
    hl::ld_frames(A, n, lds.data());
    return 0;
}

// what a launch of this ladder is given: out[0] = grid x, out[1] = dynamic LDS
// bytes, out[2 + r] = rung r's luma tile count
extern "C" int32_t ladder_emu_geometry(int32_t sw, int32_t sh, int32_t count, const int32_t* sizes, int32_t* out)
{
    hl::LdArgs A;
    if (!out || !ladder_args(sw, sh, count, sizes, &A)) return -1;
    out[0] = hl::ld_grid_x(A);
    out[1] = (int32_t)hl::ld_lds_bytes(A);
    for (int r = 0; r < count; ++r) out[2 + r] = hl::sk_tiles_x(A.rung[r].parm, 0) * hl::sk_tiles_y(A.rung[r].parm, 0);
    return 0;
}

// workgroup (x, c, z) of a launch of `count` rungs: out = frame, rung, whether it has a tile
extern "C" int32_t ladder_emu_block(int32_t sw, int32_t sh, int32_t count, const int32_t* sizes, int32_t x, int32_t c, int32_t z, int32_t* out3)
{
    hl::LdArgs A;
    if (!out3 || c < 0 || c > 2 || x < 0 || z < 0 || !ladder_args(sw, sh, count, sizes, &A)) return -1;
    uint8_t dummy[4] = {};
    for (int r = 0; r < count; ++r)
        for (int k = 0; k < 3; ++k) A.rung[r].dst[k] = dummy;  // (selected, not written)
    A.one = hl::SkFrame{{dummy, dummy, dummy}, {nullptr, nullptr, nullptr}};
    const hl::LdBlock B = hl::ld_block(A, x, c, z);
    out3[0] = B.k;
    out3[1] = B.r;
    out3[2] = B.on ? 1 : 0;
    return 0;
}
