// The area downscaler behind the frame ingest (hl_amd_set_source_size) under
// AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone program,
// tests/test_scale_asan.py): frames of the source size whose planes are heap
// blocks of exactly pitch * (rows - 1) + row bytes go through the ingest's
// tiles (hartallo_amd/csrc/hl_ingest.h) into an intermediate buffer of exactly
// the source size rounded up to 16, and through k_scale's per-lane functions
// (hartallo_amd/csrc/hl_scale.h, in the order of the kernel's lanes, the LDS a
// heap block of exactly sk_lds_bytes) into destination planes of exactly the
// coded size, so that a read or write one byte outside any of them is a
// heap-buffer-overflow.  The program checks every output sample against a
// scalar statement of the definition in 64-bit integers, and that the bytes
// between the rows reach no output.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../hartallo_amd/csrc/hl_ingest.h"
#include "../../hartallo_amd/csrc/hl_scale.h"

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

static void ingest(int fmt, const InFrame& F, const InCoef& C, int W, int H, int dW, int dH)
{
    switch (fmt) {
    case IN_I420: in_frame_display<IN_I420>(F, C, W, H, dW, dH); break;
    case IN_NV12: in_frame_display<IN_NV12>(F, C, W, H, dW, dH); break;
    case IN_RGB24: in_frame_display<IN_RGB24>(F, C, W, H, dW, dH); break;
    case IN_RGBA32: in_frame_display<IN_RGBA32>(F, C, W, H, dW, dH); break;
    default: in_frame_display<IN_RGBP>(F, C, W, H, dW, dH); break;
    }
}

static int64_t gcd64(int64_t a, int64_t b) { return b ? gcd64(b, a % b) : a; }

// the definition on one dense plane: s_w x s_h -> d_w x d_h, then the clamp to W x H
static std::vector<uint8_t> scale_model(const std::vector<uint8_t>& p, int s_w, int s_h, int d_w, int d_h, int W, int H)
{
    const int64_t srw = s_w / gcd64(s_w, d_w), drw = d_w / gcd64(s_w, d_w), srh = s_h / gcd64(s_h, d_h), drh = d_h / gcd64(s_h, d_h), D = srw * srh;
    std::vector<uint8_t> out((size_t)d_w * d_h);
    for (int64_t y = 0; y < d_h; ++y)
        for (int64_t x = 0; x < d_w; ++x) {
            int64_t acc = 0, sumw = 0;
            for (int64_t k = 0; k < s_h; ++k) {
                const int64_t wv = std::min((y + 1) * srh, (k + 1) * drh) - std::max(y * srh, k * drh);
                if (wv <= 0) continue;
                for (int64_t i = 0; i < s_w; ++i) {
                    const int64_t wh = std::min((x + 1) * srw, (i + 1) * drw) - std::max(x * srw, i * drw);
                    if (wh <= 0) continue;
                    acc += wv * wh * p[(size_t)k * s_w + i];
                    sumw += wv * wh;
                }
            }
            if (sumw != D) abort();  // (the weights of a sample sum to D)
            out[(size_t)y * d_w + x] = (uint8_t)((acc + (D >> 1)) / D);
        }
    std::vector<uint8_t> full((size_t)W * H);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) full[(size_t)y * W + x] = out[(size_t)(y < d_h ? y : d_h - 1) * d_w + (x < d_w ? x : d_w - 1)];
    return full;
}

// one I420 or NV12 frame with `pad` bytes between its rows (the ingest's RGB arithmetic has its own programs); returns the failed checks
static int one(int fmt, int sw, int sh, int dw, int dh, int W, int H, int pad, int kind)
{
    const int np = in_planes(fmt), SW = (sw + 15) & ~15, SH = (sh + 15) & ~15;
    std::vector<std::vector<uint8_t>> content(np);  // the rows' own bytes, dense
    for (int c = 0; c < np; ++c) {
        content[c].resize((size_t)in_row_bytes(fmt, c, sw) * in_rows(fmt, c, sh));
        size_t i = 0;
        for (uint8_t& b : content[c]) b = kind == 0 ? rnd8() : kind == 1 ? 255 : (uint8_t)(((i++ / in_row_bytes(fmt, c, sw) + i) & 1) * 255);
    }
    SkParm P;
    if (!sk_parm(sw, sh, SW, dw, dh, W, H, &P)) {
        printf("%dx%d -> %dx%d in %dx%d: refused\n", sw, sh, dw, dh, W, H);
        return 1;
    }
    const size_t ny = (size_t)W * H, nc = ny / 4, my = (size_t)SW * SH, mc = my / 4;
    std::vector<uint8_t> out[2];
    for (int fill = 0; fill < 2; ++fill) {
        Planes src, mid, dst;
        InFrame F{};
        for (int c = 0; c < np; ++c) {
            const size_t rb = (size_t)in_row_bytes(fmt, c, sw), rows = (size_t)in_rows(fmt, c, sh), pitch = rb + pad;
            const size_t bytes = pitch * (rows - 1) + rb;  // nothing after the last row
            src.p[c] = (uint8_t*)malloc(bytes);
            for (size_t i = 0; i < bytes; ++i) src.p[c][i] = fill ? 0x5A : 0xC3;
            for (size_t r = 0; r < rows; ++r) memcpy(src.p[c] + r * pitch, content[c].data() + r * rb, rb);
            F.plane[c] = src.p[c];
            F.pitch[c] = (int64_t)pitch;
        }
        SkFrame S{};
        for (int c = 0; c < 3; ++c) {
            S.src[c] = F.dst[c] = mid.p[c] = (uint8_t*)malloc(c ? mc : my);  // exactly the intermediate planes
            memset(mid.p[c], 0x77, c ? mc : my);
            S.dst[c] = dst.p[c] = (uint8_t*)malloc(c ? nc : ny);  // exactly the dense planes of the coded size
            memset(dst.p[c], 0xEE, c ? nc : ny);
        }
        ingest(fmt, F, in_coef_of(0, 0), SW, SH, sw, sh);
        uint32_t* lds = (uint32_t*)malloc(sk_lds_bytes(P.lrows));  // exactly a workgroup's LDS
        sk_frame(S, P, lds);
        free(lds);
        out[fill].assign(dst.p[0], dst.p[0] + ny);
        out[fill].insert(out[fill].end(), dst.p[1], dst.p[1] + nc);
        out[fill].insert(out[fill].end(), dst.p[2], dst.p[2] + nc);
    }
    int bad = 0;
    if (out[0] != out[1]) {
        printf("format %d %dx%d -> %dx%d pad %d: the bytes between the rows reached the output\n", fmt, sw, sh, dw, dh, pad);
        ++bad;
    }
    // the dense source planes Y, U, V
    std::vector<uint8_t> y = content[0], u((size_t)sw * sh / 4), v(u.size());
    if (fmt == IN_I420) {
        u = content[1];
        v = content[2];
    }
    else
        for (size_t i = 0; i < u.size(); ++i) {
            u[i] = content[1][2 * i];
            v[i] = content[1][2 * i + 1];
        }
    std::vector<uint8_t> want = scale_model(y, sw, sh, dw, dh, W, H);
    for (const auto* p : {&u, &v}) {
        const std::vector<uint8_t> c = scale_model(*p, sw / 2, sh / 2, dw / 2, dh / 2, W / 2, H / 2);
        want.insert(want.end(), c.begin(), c.end());
    }
    if (out[0] != want) {
        size_t at = 0;
        while (at < want.size() && out[0][at] == want[at]) ++at;
        printf("format %d %dx%d -> %dx%d in %dx%d pad %d kind %d: sample %zu is %d, the definition gives %d\n", fmt, sw, sh, dw, dh, W, H, pad, kind, at,
               out[0][at], want[at]);
        ++bad;
    }
    return bad;
}

int main()
{
    int bad = 0, runs = 0;
    // source, display, coded (tests/sk_testlib.py SHAPES)
    const int sizes[][6] = {{96, 64, 48, 32, 48, 32},   {72, 48, 48, 32, 48, 32},   {50, 34, 34, 18, 48, 32},       {48, 64, 48, 32, 48, 32},
                            {96, 32, 48, 32, 48, 32},   {382, 254, 48, 32, 48, 32}, {384, 256, 48, 32, 48, 32},     {1538, 26, 1026, 18, 1040, 32},
                            {352, 288, 176, 144, 176, 144}, {34, 18, 34, 18, 48, 32}};
    const int pads[] = {0, 6};
    for (int fmt = IN_I420; fmt <= IN_NV12; ++fmt)
        for (const auto& s : sizes)
            for (int pad : pads)
                for (int kind = 0; kind < 3; ++kind, ++runs) bad += one(fmt, s[0], s[1], s[2], s[3], s[4], s[5], pad, kind);
    // the division: every quotient's neighbourhood for the smallest and largest D
    for (uint32_t D : {1u, 2u, 3u, 9u, 425u, 16777215u, 16777216u})
        for (uint32_t q = 0; q <= 255; ++q)
            for (int k = -1; k <= 1; ++k, ++runs) {
                const uint64_t n = (uint64_t)q * D + k;
                if ((q == 0 && k < 0) || n > 255ull * D + (D >> 1)) continue;
                if (sk_div((uint32_t)n, D, sk_recip(D)) != (uint32_t)(n / D)) {
                    printf("sk_div(%llu, %u) is wrong\n", (unsigned long long)n, D);
                    ++bad;
                }
            }
    if (bad) {
        printf("scale: %d of %d checks failed\n", bad, runs);
        return 1;
    }
    printf("scale ok: %d checks\n", runs);
    return 0;
}
