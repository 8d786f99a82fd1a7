// The read contract of frames whose margins are wider than a macroblock (the
// top layer of an encoder with spatial layers, hl_amd_set_au_display_size:
// margins up to (16 << K) - 2) under AddressSanitizer +
// UndefinedBehaviorSanitizer (a stand-alone program,
// tests/test_emu_svc_display.py): the full tiles (in_tile) and the edge tiles
// (in_tile_edge, hartallo_amd/csrc/hl_ingest.h) -- a right band of several tile
// columns, a bottom band of up to 63 tile rows, enumerated by in_edge_at -- are
// looped in the order of the kernels' lanes over frames whose planes are heap
// blocks of exactly pitch * (rows - 1) + row bytes for the display size, so
// that a read past a row or past the last plane row, or a write past a
// destination plane of the coded size, is a heap-buffer-overflow.  Every
// output sample is checked against a scalar statement of the definition
// (clamped coordinates), every edge tile must be visited exactly once, and the
// bytes between the rows must reach no output.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../hartallo_amd/csrc/hl_ingest.h"

using namespace hl;

static uint32_t rng_state = 97531;
static uint8_t rnd8()
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return (uint8_t)(rng_state >> 24);
}

struct Planes {
    uint8_t* p[3] = {nullptr, nullptr, nullptr};
    ~Planes()
    {
        for (uint8_t* q : p) free(q);
    }
};

static void run(int fmt, const InFrame& F, const InCoef& C, int W, int H, int dW, int dH)
{
    switch (fmt) {
    case IN_I420: in_frame_display<IN_I420>(F, C, W, H, dW, dH); break;
    case IN_NV12: in_frame_display<IN_NV12>(F, C, W, H, dW, dH); break;
    case IN_RGB24: in_frame_display<IN_RGB24>(F, C, W, H, dW, dH); break;
    case IN_RGBA32: in_frame_display<IN_RGBA32>(F, C, W, H, dW, dH); break;
    default: in_frame_display<IN_RGBP>(F, C, W, H, dW, dH); break;
    }
}

// sample (x, y) of channel ch (R, G, B, or Y, U, V at their own resolution) of the dense content
static int sample(int fmt, const std::vector<std::vector<uint8_t>>& content, int dW, int ch, int x, int y)
{
    switch (fmt) {
    case IN_I420: return content[ch][(size_t)y * (ch ? dW / 2 : dW) + x];
    case IN_NV12: return ch ? content[1][(size_t)y * dW + 2 * x + (ch - 1)] : content[0][(size_t)y * dW + x];
    case IN_RGB24: return content[0][((size_t)y * dW + x) * 3 + ch];
    case IN_RGBA32: return content[0][((size_t)y * dW + x) * 4 + ch];
    default: return content[ch][(size_t)y * dW + x];
    }
}

// the definition: the dense converted planes of the dW x dH frame, then the clamp
static std::vector<uint8_t> model(int fmt, const std::vector<std::vector<uint8_t>>& content, const InCoef& C, int W, int H, int dW, int dH)
{
    std::vector<uint8_t> y((size_t)dW * dH), u((size_t)dW * dH / 4), v(u.size());
    const bool rgb = fmt >= IN_RGB24;
    for (int j = 0; j < dH; ++j)
        for (int i = 0; i < dW; ++i) {
            if (!rgb) y[(size_t)j * dW + i] = (uint8_t)sample(fmt, content, dW, 0, i, j);
            else {
                const int64_t R = sample(fmt, content, dW, 0, i, j), G = sample(fmt, content, dW, 1, i, j), B = sample(fmt, content, dW, 2, i, j);
                y[(size_t)j * dW + i] = (uint8_t)(((int64_t)C.y[0] * R + (int64_t)C.y[1] * G + (int64_t)C.y[2] * B + ((int64_t)C.off << 16) + 32768) >> 16);
            }
        }
    for (int j = 0; j < dH / 2; ++j)
        for (int i = 0; i < dW / 2; ++i) {
            if (!rgb) {
                u[(size_t)j * (dW / 2) + i] = (uint8_t)sample(fmt, content, dW, 1, i, j);
                v[(size_t)j * (dW / 2) + i] = (uint8_t)sample(fmt, content, dW, 2, i, j);
                continue;
            }
            int64_t s[3] = {0, 0, 0};
            for (int c = 0; c < 3; ++c)
                for (int k = 0; k < 4; ++k) s[c] += sample(fmt, content, dW, c, 2 * i + (k & 1), 2 * j + (k >> 1));
            const int64_t cu = (int32_t)C.u[0] * s[0] + (int32_t)C.u[1] * s[1] + (int32_t)C.u[2] * s[2] + (128 << 18) + (1 << 17);
            const int64_t cv = (int32_t)C.v[0] * s[0] + (int32_t)C.v[1] * s[1] + (int32_t)C.v[2] * s[2] + (128 << 18) + (1 << 17);
            u[(size_t)j * (dW / 2) + i] = (uint8_t)((cu >> 18) < 255 ? (cu >> 18) : 255);
            v[(size_t)j * (dW / 2) + i] = (uint8_t)((cv >> 18) < 255 ? (cv >> 18) : 255);
        }
    std::vector<uint8_t> out;
    for (int j = 0; j < H; ++j)
        for (int i = 0; i < W; ++i) out.push_back(y[(size_t)(j < dH ? j : dH - 1) * dW + (i < dW ? i : dW - 1)]);
    for (const auto* p : {&u, &v})
        for (int j = 0; j < H / 2; ++j)
            for (int i = 0; i < W / 2; ++i) out.push_back((*p)[(size_t)(j < dH / 2 ? j : dH / 2 - 1) * (dW / 2) + (i < dW / 2 ? i : dW / 2 - 1)]);
    return out;
}

// the edge lanes visit every tile that is not full exactly once
static int cover(int W, int H, int dW, int dH)
{
    const int tw = W >> 4, th = H >> 1, n = in_edge_tiles(W, H, dW, dH);
    std::vector<int> seen((size_t)tw * th, 0);
    for (int i = 0; i < n; ++i) {
        int tx, ty;
        in_edge_at(i, W, H, dW, dH, &tx, &ty);
        if (tx < 0 || tx >= tw || ty < 0 || ty >= th) {
            printf("%dx%d in %dx%d: edge lane %d is tile (%d, %d)\n", dW, dH, W, H, i, tx, ty);
            return 1;
        }
        ++seen[(size_t)ty * tw + tx];
    }
    int bad = 0;
    for (int ty = 0; ty < th; ++ty)
        for (int tx = 0; tx < tw; ++tx) bad += seen[(size_t)ty * tw + tx] != ((tx < in_full_x(dW) && ty < in_full_y(dH)) ? 0 : 1);
    if (bad) printf("%dx%d in %dx%d: %d tiles are not visited exactly once by the edge lanes\n", dW, dH, W, H, bad);
    return bad != 0;
}

// one frame of format fmt with `pad` bytes between its rows; returns the number of failed checks
static int one(int fmt, int W, int H, int dW, int dH, int pad, int matrix, int range)
{
    const int np = in_planes(fmt);
    std::vector<std::vector<uint8_t>> content(np);  // the rows' own bytes, dense
    for (int c = 0; c < np; ++c) {
        content[c].resize((size_t)in_row_bytes(fmt, c, dW) * in_rows(fmt, c, dH));
        for (uint8_t& b : content[c]) b = rnd8();
    }
    const size_t ny = (size_t)W * H, nc = ny / 4;
    const InCoef C = in_coef_of(matrix, range);
    std::vector<uint8_t> out[2];
    for (int fill = 0; fill < 2; ++fill) {
        Planes src, dst;
        InFrame F{};
        for (int c = 0; c < np; ++c) {
            const size_t rb = (size_t)in_row_bytes(fmt, c, dW), rows = (size_t)in_rows(fmt, c, dH), pitch = rb + pad;
            const size_t bytes = pitch * (rows - 1) + rb;  // nothing after the last row
            src.p[c] = (uint8_t*)malloc(bytes);
            for (size_t i = 0; i < bytes; ++i) src.p[c][i] = fill ? 0x5A : 0xC3;
            for (size_t r = 0; r < rows; ++r) memcpy(src.p[c] + r * pitch, content[c].data() + r * rb, rb);
            F.plane[c] = src.p[c];
            F.pitch[c] = (int64_t)pitch;
        }
        for (int c = 0; c < 3; ++c) {
            F.dst[c] = dst.p[c] = (uint8_t*)malloc(c ? nc : ny);  // exactly the dense planes of the coded size
            memset(dst.p[c], 0xEE, c ? nc : ny);
        }
        run(fmt, F, C, W, H, dW, dH);
        out[fill].assign(dst.p[0], dst.p[0] + ny);
        out[fill].insert(out[fill].end(), dst.p[1], dst.p[1] + nc);
        out[fill].insert(out[fill].end(), dst.p[2], dst.p[2] + nc);
    }
    int bad = 0;
    if (out[0] != out[1]) {
        printf("format %d %dx%d in %dx%d pad %d: the bytes between the rows reached the output\n", fmt, dW, dH, W, H, pad);
        ++bad;
    }
    if (out[0] != model(fmt, content, C, W, H, dW, dH)) {
        printf("format %d %dx%d in %dx%d pad %d: not the edge replication of the converted planes\n", fmt, dW, dH, W, H, pad);
        ++bad;
    }
    return bad;
}

int main()
{
    int bad = 0, runs = 0;
    // coded size, display size: K = 1 (margins 28, 20), K = 2 (56, 56: the test
    // fixture's shape), K = 3 with the widest margins (126: 8 tile columns, 63
    // tile rows, no full tile), the right band across the 64-lane workgroup
    // column of k_ingest's grid (tiles 64..67) over a display height of 8, and
    // a bottom band alone
    const int sizes[][4] = {{64, 64, 36, 44}, {256, 192, 200, 136}, {128, 128, 2, 2}, {1088, 64, 1032, 8}, {128, 128, 128, 72}};
    const int pads[] = {0, 2, 24};
    for (const auto& s : sizes) bad += cover(s[0], s[1], s[2], s[3]);
    for (int fmt = 0; fmt < IN_FORMATS; ++fmt)
        for (const auto& s : sizes)
            for (int pad : pads)
                for (int mr = 0; mr < (fmt >= IN_RGB24 ? 4 : 1); mr += 3, ++runs) bad += one(fmt, s[0], s[1], s[2], s[3], pad, mr >> 1, mr & 1);
    if (bad) {
        printf("ingest wide margins: %d checks of %d runs failed\n", bad, runs);
        return 1;
    }
    printf("ingest wide margins ok: %d runs\n", runs);
    return 0;
}
