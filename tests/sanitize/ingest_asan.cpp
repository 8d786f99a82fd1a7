// The frame ingest's read contract under AddressSanitizer +
// UndefinedBehaviorSanitizer (a stand-alone program, tests/test_ingest_asan.py):
// the per-tile code k_ingest's lanes run (hartallo_amd/csrc/hl_ingest.h) is
// looped over frames whose planes are heap blocks of exactly
// pitch * (rows - 1) + row bytes, so that a read past a plane's last row, or
// a write past a destination plane, is a heap-buffer-overflow.  The program
// itself checks that the bytes between the rows reach no output (two fills of
// the padding give the same planes) and that I420 and NV12 are copies.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../hartallo_amd/csrc/hl_ingest.h"

using namespace hl;

static uint32_t rng_state = 12345;
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

static void run(int fmt, const InFrame& F, const InCoef& C, int W, int H)
{
    switch (fmt) {
    case IN_I420: in_frame<IN_I420>(F, C, W, H); break;
    case IN_NV12: in_frame<IN_NV12>(F, C, W, H); break;
    case IN_RGB24: in_frame<IN_RGB24>(F, C, W, H); break;
    case IN_RGBA32: in_frame<IN_RGBA32>(F, C, W, H); break;
    default: in_frame<IN_RGBP>(F, C, W, H); break;
    }
}

// one frame of format fmt with `pad` bytes between its rows; returns the number of failed checks
static int one(int fmt, int W, int H, int pad, int matrix, int range)
{
    const int np = in_planes(fmt);
    std::vector<std::vector<uint8_t>> content(np);  // the rows' own bytes, dense
    for (int c = 0; c < np; ++c) {
        content[c].resize((size_t)in_row_bytes(fmt, c, W) * in_rows(fmt, c, H));
        for (uint8_t& b : content[c]) b = rnd8();
    }
    const size_t ny = (size_t)W * H, nc = ny / 4;
    std::vector<uint8_t> out[2];
    for (int fill = 0; fill < 2; ++fill) {
        Planes src, dst;
        InFrame F{};
        for (int c = 0; c < np; ++c) {
            const size_t rb = (size_t)in_row_bytes(fmt, c, W), rows = (size_t)in_rows(fmt, c, H), pitch = rb + pad;
            const size_t bytes = pitch * (rows - 1) + rb;  // nothing after the last row
            src.p[c] = (uint8_t*)malloc(bytes);
            for (size_t i = 0; i < bytes; ++i) src.p[c][i] = fill ? 0x5A : 0xC3;
            for (size_t r = 0; r < rows; ++r) memcpy(src.p[c] + r * pitch, content[c].data() + r * rb, rb);
            F.plane[c] = src.p[c];
            F.pitch[c] = (int64_t)pitch;
        }
        for (int c = 0; c < 3; ++c) F.dst[c] = dst.p[c] = (uint8_t*)malloc(c ? nc : ny);  // exactly the dense planes
        run(fmt, F, in_coef_of(matrix, range), W, H);
        out[fill].assign(dst.p[0], dst.p[0] + ny);
        out[fill].insert(out[fill].end(), dst.p[1], dst.p[1] + nc);
        out[fill].insert(out[fill].end(), dst.p[2], dst.p[2] + nc);
    }
    int bad = 0;
    if (out[0] != out[1]) {
        printf("format %d %dx%d pad %d: the bytes between the rows reached the output\n", fmt, W, H, pad);
        ++bad;
    }
    if (fmt == IN_I420 || fmt == IN_NV12) {
        std::vector<uint8_t> want(content[0]);
        if (fmt == IN_I420) {
            want.insert(want.end(), content[1].begin(), content[1].end());
            want.insert(want.end(), content[2].begin(), content[2].end());
        }
        else {
            for (int k = 0; k < 2; ++k)
                for (size_t i = 0; i < nc; ++i) want.push_back(content[1][2 * i + k]);
        }
        if (out[0] != want) {
            printf("format %d %dx%d pad %d: not a copy\n", fmt, W, H, pad);
            ++bad;
        }
    }
    return bad;
}

int main()
{
    int bad = 0, runs = 0;
    const int sizes[][2] = {{16, 16}, {48, 32}, {176, 144}};
    const int pads[] = {0, 4, 24};
    for (int fmt = 0; fmt < IN_FORMATS; ++fmt)
        for (const auto& s : sizes)
            for (int pad : pads)
                for (int mr = 0; mr < (fmt >= IN_RGB24 ? 4 : 1); ++mr, ++runs) bad += one(fmt, s[0], s[1], pad, mr >> 1, mr & 1);
    if (bad) {
        printf("ingest: %d of %d runs failed\n", bad, runs);
        return 1;
    }
    printf("ingest ok: %d runs\n", runs);
    return 0;
}
