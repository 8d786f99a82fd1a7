// Test-only host build of what a display size below the coded size adds
// (hl_amd_set_display_size): the frame ingest's full and edge tiles
// (hartallo_amd/csrc/hl_ingest.h in_tile, in_tile_edge) looped over a frame in
// the order of the kernels' lanes, and the quality metric over a window
// (hartallo_amd/csrc/hl_quality.h quality_plane_window_host)
// (tests/test_emu_display.py).
#include "../../hartallo_amd/csrc/hl_ingest.h"
#include "../../hartallo_amd/csrc/hl_quality.h"

// One frame of dw x dh samples in format fmt, planes and pitches as
// hl_amd_frame_t has them (pitch 0 = dense), into the dense planes y, u, v of
// the coded size w x h.  Returns 0, or -1 for what the library refuses.
extern "C" int32_t display_emu_frame(int32_t fmt, int32_t matrix, int32_t range, int32_t w, int32_t h, int32_t dw, int32_t dh,
                                     const uint8_t* const* planes, const int64_t* pitches, uint8_t* y, uint8_t* u, uint8_t* v)
{
    if (fmt < 0 || fmt >= hl::IN_FORMATS || matrix < 0 || matrix > 1 || range < 0 || range > 1 || w <= 0 || h <= 0 || (w & 15) || (h & 15) ||
        ((dw | dh) & 1) || dw <= w - 16 || dw > w || dh <= h - 16 || dh > h || dw <= 0 || dh <= 0 || !planes || !pitches || !y || !u || !v)
        return -1;
    hl::InFrame F{};
    for (int c = 0; c < hl::in_planes(fmt); ++c) {
        const int64_t rb = hl::in_row_bytes(fmt, c, dw);
        if (!planes[c] || pitches[c] < 0 || (pitches[c] && pitches[c] < rb)) return -1;
        F.plane[c] = planes[c];
        F.pitch[c] = pitches[c] ? pitches[c] : rb;
    }
    F.dst[0] = y;
    F.dst[1] = u;
    F.dst[2] = v;
    const hl::InCoef C = hl::in_coef_of(matrix, range);
    switch (fmt) {
    case hl::IN_I420: hl::in_frame_display<hl::IN_I420>(F, C, w, h, dw, dh); break;
    case hl::IN_NV12: hl::in_frame_display<hl::IN_NV12>(F, C, w, h, dw, dh); break;
    case hl::IN_RGB24: hl::in_frame_display<hl::IN_RGB24>(F, C, w, h, dw, dh); break;
    case hl::IN_RGBA32: hl::in_frame_display<hl::IN_RGBA32>(F, C, w, h, dw, dh); break;
    default: hl::in_frame_display<hl::IN_RGBP>(F, C, w, h, dw, dh); break;
    }
    return 0;
}

// full tiles and edge tiles of such a frame, and the tile of edge lane i
extern "C" int32_t display_emu_tiles(int32_t w, int32_t h, int32_t dw, int32_t dh, int32_t* full, int32_t* edge)
{
    *full = hl::in_full_x(dw) * hl::in_full_y(dh);
    *edge = hl::in_edge_tiles(w, h, dw, dh);
    return 0;
}

extern "C" int32_t display_emu_edge_at(int32_t i, int32_t w, int32_t h, int32_t dw, int32_t dh, int32_t* tx, int32_t* ty)
{
    if (i < 0 || i >= hl::in_edge_tiles(w, h, dw, dh)) return -1;
    int x, y;
    hl::in_edge_at(i, w, h, dw, dh, &x, &y);
    *tx = x;
    *ty = y;
    return 0;
}

// One dense w x h plane pair measured over its top-left ww x wh samples:
// *sse, *ssim_q30, mb (or null; w, h multiples of 16 then) as
// quality_emu_plane gives them for the whole plane; *windows = the 8x8
// windows counted.  Returns 0, or -1 for what the kernel does not take.
extern "C" int32_t display_emu_quality(const uint8_t* a, const uint8_t* b, int32_t w, int32_t h, int32_t ww, int32_t wh, uint64_t* sse,
                                       int64_t* ssim_q30, uint64_t* windows, uint32_t* mb)
{
    if (!a || !b || !sse || !ssim_q30 || !windows || w <= 0 || h <= 0 || (w & 7) || (h & 7) || (mb && ((w & 15) || (h & 15))) || ww <= 0 ||
        ww > w || wh <= 0 || wh > h)
        return -1;
    *sse = 0;
    *ssim_q30 = 0;
    *windows = hl::q_windows(ww, wh);
    hl::quality_plane_window_host(a, b, w, h, ww, wh, sse, ssim_q30, mb);
    return 0;
}
