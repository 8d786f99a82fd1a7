// Test-only host build of the frame ingest (hartallo_amd/csrc/hl_ingest.h):
// the per-tile code k_ingest's lanes run, looped over a frame on the host
// (tests/test_emu_ingest.py).
#include "../../hartallo_amd/csrc/hl_ingest.h"

// The coefficient table of (matrix, range): y[3], u[3], v[3] (signed), off.
// Returns 0, or -1 for an unknown matrix or range.
extern "C" int32_t in_emu_coef(int32_t matrix, int32_t range, int32_t out10[10])
{
    if (matrix < 0 || matrix > 1 || range < 0 || range > 1 || !out10) return -1;
    const hl::InCoef c = hl::in_coef_of(matrix, range);
    for (int i = 0; i < 3; ++i) {
        out10[i] = (int32_t)c.y[i];
        out10[3 + i] = (int32_t)c.u[i];
        out10[6 + i] = (int32_t)c.v[i];
    }
    out10[9] = (int32_t)c.off;
    return 0;
}

// One frame of w x h samples (multiples of 16) in format fmt, planes and
// pitches as hl_amd_frame_t has them (pitch 0 = dense), into the dense planes
// y, u, v.  Returns 0, or -1 for what the library refuses.
extern "C" int32_t in_emu_frame(int32_t fmt, int32_t matrix, int32_t range, int32_t w, int32_t h, const uint8_t* const* planes,
                                const int64_t* pitches, uint8_t* y, uint8_t* u, uint8_t* v)
{
    if (fmt < 0 || fmt >= hl::IN_FORMATS || matrix < 0 || matrix > 1 || range < 0 || range > 1 || w <= 0 || h <= 0 || (w & 15) || (h & 15) ||
        !planes || !pitches || !y || !u || !v)
        return -1;
    hl::InFrame F{};
    for (int c = 0; c < hl::in_planes(fmt); ++c) {
        const int64_t rb = hl::in_row_bytes(fmt, c, w);
        if (!planes[c] || pitches[c] < 0 || (pitches[c] && pitches[c] < rb)) return -1;
        F.plane[c] = planes[c];
        F.pitch[c] = pitches[c] ? pitches[c] : rb;
    }
    F.dst[0] = y;
    F.dst[1] = u;
    F.dst[2] = v;
    const hl::InCoef C = hl::in_coef_of(matrix, range);
    switch (fmt) {
    case hl::IN_I420: hl::in_frame<hl::IN_I420>(F, C, w, h); break;
    case hl::IN_NV12: hl::in_frame<hl::IN_NV12>(F, C, w, h); break;
    case hl::IN_RGB24: hl::in_frame<hl::IN_RGB24>(F, C, w, h); break;
    case hl::IN_RGBA32: hl::in_frame<hl::IN_RGBA32>(F, C, w, h); break;
    default: hl::in_frame<hl::IN_RGBP>(F, C, w, h); break;
    }
    return 0;
}

extern "C" int32_t in_emu_lanes(int32_t* x, int32_t* y)
{
    *x = hl::kInLanesX;
    *y = hl::kInLanesY;
    return 0;
}
