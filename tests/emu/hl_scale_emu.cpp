// Test-only host build of the area downscaler (hl_amd_set_source_size,
// hartallo_amd/csrc/hl_scale.h): the tap derivation, the accumulation, the
// rounding division and the clamped edge that k_scale's lanes run, looped over
// a frame in the order of the kernel's lanes, behind the frame ingest
// (hl_ingest.h) at the source size (tests/test_emu_scale.py).
#include <vector>

#include "../../hartallo_amd/csrc/hl_ingest.h"
#include "../../hartallo_amd/csrc/hl_scale.h"

// One frame of sw x sh samples in format fmt, planes and pitches as
// hl_amd_frame_t has them (pitch 0 = dense), converted into the intermediate
// I420 planes of the source size rounded up to 16 and scaled to dw x dh in the
// dense planes y, u, v of the coded size w x h.  Returns 0, or -1 for what the
// library refuses.
extern "C" int32_t scale_emu_frame(int32_t fmt, int32_t matrix, int32_t range, int32_t sw, int32_t sh, int32_t dw, int32_t dh, int32_t w, int32_t h,
                                   const uint8_t* const* planes, const int64_t* pitches, uint8_t* y, uint8_t* u, uint8_t* v)
{
    if (fmt < 0 || fmt >= hl::IN_FORMATS || matrix < 0 || matrix > 1 || range < 0 || range > 1 || !planes || !pitches || !y || !u || !v || sw <= 0 ||
        sh <= 0)
        return -1;
    const int SW = (sw + 15) & ~15, SH = (sh + 15) & ~15;
    hl::SkParm P;
    if (!hl::sk_parm(sw, sh, SW, dw, dh, w, h, &P)) return -1;
    std::vector<uint8_t> mid((size_t)SW * SH * 3 / 2);
    hl::InFrame F{};
    for (int c = 0; c < hl::in_planes(fmt); ++c) {
        const int64_t rb = hl::in_row_bytes(fmt, c, sw);
        if (!planes[c] || pitches[c] < 0 || (pitches[c] && pitches[c] < rb)) return -1;
        F.plane[c] = planes[c];
        F.pitch[c] = pitches[c] ? pitches[c] : rb;
    }
    F.dst[0] = mid.data();
    F.dst[1] = F.dst[0] + (size_t)SW * SH;
    F.dst[2] = F.dst[1] + (size_t)SW * SH / 4;
    const hl::InCoef C = hl::in_coef_of(matrix, range);
    switch (fmt) {
    case hl::IN_I420: hl::in_frame_display<hl::IN_I420>(F, C, SW, SH, sw, sh); break;
    case hl::IN_NV12: hl::in_frame_display<hl::IN_NV12>(F, C, SW, SH, sw, sh); break;
    case hl::IN_RGB24: hl::in_frame_display<hl::IN_RGB24>(F, C, SW, SH, sw, sh); break;
    case hl::IN_RGBA32: hl::in_frame_display<hl::IN_RGBA32>(F, C, SW, SH, sw, sh); break;
    default: hl::in_frame_display<hl::IN_RGBP>(F, C, SW, SH, sw, sh); break;
    }
    const hl::SkFrame S{{F.dst[0], F.dst[1], F.dst[2]}, {y, u, v}};
    std::vector<uint32_t> lds(hl::sk_lds_bytes(P.lrows) / sizeof(uint32_t));
    hl::sk_frame(S, P, lds.data());
    return 0;
}

// One dense plane of s_w x s_h samples of any parity scaled to d_w x d_h
// (dense): the luma path of the per-lane functions on a coded size rounded up
// to 16, cropped.  Returns 0, or -1 for axes the scaler refuses.
extern "C" int32_t scale_emu_plane(const uint8_t* src, int32_t s_w, int32_t s_h, uint8_t* dst, int32_t d_w, int32_t d_h)
{
    if (!src || !dst || d_w <= 0 || d_h <= 0) return -1;
    const int W = (d_w + 15) & ~15, H = (d_h + 15) & ~15;
    hl::SkParm P;
    if (!hl::sk_parm_any(s_w, s_h, s_w, d_w, d_h, W, H, &P)) return -1;
    std::vector<uint8_t> out((size_t)W * H);
    std::vector<uint32_t> lds(hl::sk_lds_bytes(P.lrows) / sizeof(uint32_t));
    for (int tile = 0; tile < hl::sk_tiles_x(P, 0) * hl::sk_tiles_y(P, 0); ++tile) {
        const hl::SkTile T = hl::sk_tile(P, 0, tile);
        for (int lane = 0; lane < hl::kSkLanes; ++lane) hl::sk_reduce(src, P, T, lds.data(), lane & 63, lane >> 6, 4);
        for (int lane = 0; lane < hl::kSkLanes; ++lane) hl::sk_output(out.data(), P, T, lds.data(), lane & 15, lane >> 4);
    }
    for (int r = 0; r < d_h; ++r) memcpy(dst + (size_t)r * d_w, out.data() + (size_t)r * W, (size_t)d_w);
    return 0;
}

// floor(n / D) through the host-computed reciprocal and the correction step
extern "C" uint32_t scale_emu_div(uint32_t n, uint32_t D) { return hl::sk_div(n, D, hl::sk_recip(D)); }

// what a launch of this geometry is given: the reduced ratios, D, the largest tap counts and a tile's LDS rows
extern "C" int32_t scale_emu_parm(int32_t sw, int32_t sh, int32_t dw, int32_t dh, int32_t w, int32_t h, uint32_t* out9)
{
    hl::SkParm P;
    if (!out9 || !hl::sk_parm(sw, sh, (sw + 15) & ~15, dw, dh, w, h, &P)) return -1;
    const uint32_t v[9] = {P.srw, P.drw, P.srh, P.drh, P.D, P.M, (uint32_t)P.ntw, (uint32_t)P.nth, (uint32_t)P.lrows};
    memcpy(out9, v, sizeof(v));
    return 0;
}
