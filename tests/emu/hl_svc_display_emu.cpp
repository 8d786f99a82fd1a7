// Test-only host build of what the access unit's display size adds to the
// frame ingest (hl_amd_set_au_display_size): frames whose margins go up to
// max_margin - 2 samples, max_margin = 16 << K for the top layer of K + 1
// spatial layers -- the full tiles (hartallo_amd/csrc/hl_ingest.h in_tile) and
// the edge tiles (in_tile_edge) in the order of the kernels' lanes, and the
// enumeration of the edge tiles (in_edge_tiles, in_edge_at)
// (tests/test_emu_svc_display.py).
#include "../../hartallo_amd/csrc/hl_ingest.h"

// launch_ingest's contract for the sizes
static bool sizes_ok(int32_t w, int32_t h, int32_t dw, int32_t dh, int32_t max_margin)
{
    return w > 0 && h > 0 && !(w & 15) && !(h & 15) && !((dw | dh) & 1) && max_margin >= 16 && max_margin <= 128 && dw > w - max_margin && dw <= w &&
           dh > h - max_margin && dh <= h && dw > 0 && dh > 0;
}

// One frame of dw x dh samples in format fmt, planes and pitches as
// hl_amd_frame_t has them (pitch 0 = dense), into the dense planes y, u, v of
// the coded size w x h.  Returns 0, or -1 for what launch_ingest refuses.
extern "C" int32_t svcd_emu_frame(int32_t fmt, int32_t matrix, int32_t range, int32_t w, int32_t h, int32_t dw, int32_t dh, int32_t max_margin,
                                  const uint8_t* const* planes, const int64_t* pitches, uint8_t* y, uint8_t* u, uint8_t* v)
{
    if (fmt < 0 || fmt >= hl::IN_FORMATS || matrix < 0 || matrix > 1 || range < 0 || range > 1 || !sizes_ok(w, h, dw, dh, max_margin) || !planes ||
        !pitches || !y || !u || !v)
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

// full tiles and edge tiles of such a frame
extern "C" int32_t svcd_emu_tiles(int32_t w, int32_t h, int32_t dw, int32_t dh, int32_t max_margin, int32_t* full, int32_t* edge)
{
    if (!sizes_ok(w, h, dw, dh, max_margin)) return -1;
    *full = hl::in_full_x(dw) * hl::in_full_y(dh);
    *edge = hl::in_edge_tiles(w, h, dw, dh);
    return 0;
}

// the tile of every edge lane: tx[i], ty[i] for i < the edge tiles (the arrays hold that many)
extern "C" int32_t svcd_emu_edge_all(int32_t w, int32_t h, int32_t dw, int32_t dh, int32_t max_margin, int32_t* tx, int32_t* ty)
{
    if (!sizes_ok(w, h, dw, dh, max_margin)) return -1;
    const int n = hl::in_edge_tiles(w, h, dw, dh);
    for (int i = 0; i < n; ++i) {
        int x, y;
        hl::in_edge_at(i, w, h, dw, dh, &x, &y);
        tx[i] = x;
        ty[i] = y;
    }
    return n;
}
