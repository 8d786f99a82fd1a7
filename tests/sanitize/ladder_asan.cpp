// The rendition ladder's fan-out behind one frame ingest
// (hl_amd_encode_ladder_frames) under AddressSanitizer +
// UndefinedBehaviorSanitizer (a stand-alone program, tests/test_ladder_asan.py):
// two frames of the source size whose planes are heap blocks of exactly
// pitch * (rows - 1) + row bytes go through the ingest's tiles
// (hartallo_amd/csrc/hl_ingest.h) into an intermediate buffer of exactly two
// frames of the source size rounded up to 16, and through ld_frames
// (hartallo_amd/csrc/hl_ladder.h: k_scale_fan's block selection and k_scale's
// per-lane functions in the kernel's order, the LDS a heap block of exactly the
// launch's maximum) into every rung's planes of exactly two frames of its coded
// size, so that a read or write one byte outside any of them is a
// heap-buffer-overflow.  The program checks every output sample of every rung
// against a scalar statement of the definition in 64-bit integers, and that the
// bytes between the rows reach no output.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../hartallo_amd/csrc/hl_ingest.h"
#include "../../hartallo_amd/csrc/hl_ladder.h"

using namespace hl;

static uint32_t rng_state = 24680;
static uint8_t rnd8()
{
    rng_state = rng_state * 1664525u + 1013904223u;
    return (uint8_t)(rng_state >> 24);
}

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

// the overlap of output j with every source sample of the axis s -> d: (sample, weight) where it is positive
static std::vector<std::vector<std::pair<int64_t, int64_t>>> overlaps(int64_t s, int64_t d)
{
    const int64_t sr = s / gcd64(s, d), dr = d / gcd64(s, d);
    std::vector<std::vector<std::pair<int64_t, int64_t>>> w((size_t)d);
    for (int64_t j = 0; j < d; ++j) {
        int64_t sum = 0;
        for (int64_t i = 0; i < s; ++i) {
            const int64_t o = std::min((j + 1) * sr, (i + 1) * dr) - std::max(j * sr, i * dr);
            if (o > 0) {
                w[(size_t)j].push_back({i, o});
                sum += o;
            }
        }
        if (sum != sr) abort();  // (the weights of a sample sum to sr)
    }
    return w;
}

// the definition on one dense plane: s_w x s_h -> d_w x d_h, then the clamp to W x H
static std::vector<uint8_t> scale_model(const std::vector<uint8_t>& p, int s_w, int s_h, int d_w, int d_h, int W, int H)
{
    const int64_t D = (s_w / gcd64(s_w, d_w)) * (s_h / gcd64(s_h, d_h));
    const auto wh = overlaps(s_w, d_w), wv = overlaps(s_h, d_h);
    std::vector<uint8_t> out((size_t)d_w * d_h);
    for (int64_t y = 0; y < d_h; ++y)
        for (int64_t x = 0; x < d_w; ++x) {
            int64_t acc = 0;
            for (const auto& v : wv[(size_t)y])
                for (const auto& h : wh[(size_t)x]) acc += v.second * h.second * p[(size_t)v.first * s_w + (size_t)h.first];
            out[(size_t)y * d_w + x] = (uint8_t)((acc + (D >> 1)) / D);
        }
    std::vector<uint8_t> full((size_t)W * H);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) full[(size_t)y * W + x] = out[(size_t)(y < d_h ? y : d_h - 1) * d_w + (x < d_w ? x : d_w - 1)];
    return full;
}

struct Rung {
    int dw, dh, W, H;
};
constexpr int kFrames = 2;

// two I420 or NV12 frames with `pad` bytes between their rows through one ladder launch; returns the failed checks
static int one(int fmt, int sw, int sh, const std::vector<Rung>& rungs, int pad, int kind)
{
    const int np = in_planes(fmt), SW = (sw + 15) & ~15, SH = (sh + 15) & ~15, count = (int)rungs.size();
    std::vector<std::vector<uint8_t>> content[kFrames];  // the rows' own bytes, dense
    for (int k = 0; k < kFrames; ++k) {
        content[k].resize(np);
        for (int c = 0; c < np; ++c) {
            content[k][c].resize((size_t)in_row_bytes(fmt, c, sw) * in_rows(fmt, c, sh));
            size_t i = 0;
            for (uint8_t& b : content[k][c]) {
                b = kind == 0 || k == 1 ? rnd8() : kind == 1 ? 255 : (uint8_t)(((i / in_row_bytes(fmt, c, sw) + i) & 1) * 255);
                ++i;
            }
        }
    }
    LdArgs A{};
    A.count = count;
    for (int r = 0; r < count; ++r)
        if (!sk_parm(sw, sh, SW, rungs[r].dw, rungs[r].dh, rungs[r].W, rungs[r].H, &A.rung[r].parm)) {
            printf("%dx%d -> %dx%d in %dx%d: refused\n", sw, sh, rungs[r].dw, rungs[r].dh, rungs[r].W, rungs[r].H);
            return 1;
        }
    const size_t my = (size_t)SW * SH, mb = my + my / 2;
    std::vector<std::vector<uint8_t>> out[2];
    for (int fill = 0; fill < 2; ++fill) {
        std::vector<uint8_t*> blocks;
        uint8_t* mid = (uint8_t*)malloc(mb * kFrames);  // exactly the intermediate frames
        memset(mid, 0x77, mb * kFrames);
        blocks.push_back(mid);
        SkFrame* tab = (SkFrame*)malloc(sizeof(SkFrame) * kFrames);  // exactly the launch's table
        for (int k = 0; k < kFrames; ++k) {
            InFrame F{};
            for (int c = 0; c < np; ++c) {
                const size_t rb = (size_t)in_row_bytes(fmt, c, sw), rows = (size_t)in_rows(fmt, c, sh), pitch = rb + pad;
                const size_t bytes = pitch * (rows - 1) + rb;  // nothing after the last row
                uint8_t* p = (uint8_t*)malloc(bytes);
                blocks.push_back(p);
                for (size_t i = 0; i < bytes; ++i) p[i] = fill ? 0x5A : 0xC3;
                for (size_t r = 0; r < rows; ++r) memcpy(p + r * pitch, content[k][c].data() + r * rb, rb);
                F.plane[c] = p;
                F.pitch[c] = (int64_t)pitch;
            }
            F.dst[0] = mid + mb * k;
            F.dst[1] = F.dst[0] + my;
            F.dst[2] = F.dst[1] + my / 4;
            ingest(fmt, F, in_coef_of(0, 0), SW, SH, sw, sh);
            tab[k] = SkFrame{{F.dst[0], F.dst[1], F.dst[2]}, {nullptr, nullptr, nullptr}};
        }
        A.tab = tab;
        std::vector<uint8_t*> dst(count);
        for (int r = 0; r < count; ++r) {
            const size_t ny = (size_t)rungs[r].W * rungs[r].H, fb = ny + ny / 2;
            dst[r] = (uint8_t*)malloc(fb * kFrames);  // exactly the rung's dense frames of its coded size
            memset(dst[r], 0xEE, fb * kFrames);
            A.rung[r].dst[0] = dst[r];
            A.rung[r].dst[1] = dst[r] + ny;
            A.rung[r].dst[2] = dst[r] + ny + ny / 4;
            A.rung[r].stride = fb;
        }
        if (!ld_args_ok(A)) {
            printf("%dx%d: the launch is refused\n", sw, sh);
            return 1;
        }
        uint32_t* lds = (uint32_t*)malloc(ld_lds_bytes(A));  // exactly a workgroup's LDS: the launch's maximum
        ld_frames(A, kFrames, lds);
        free(lds);
        out[fill].resize(count);
        for (int r = 0; r < count; ++r) {
            const size_t fb = (size_t)rungs[r].W * rungs[r].H * 3 / 2;
            out[fill][r].assign(dst[r], dst[r] + fb * kFrames);
            free(dst[r]);
        }
        free(tab);
        for (uint8_t* p : blocks) free(p);
    }
    int bad = 0;
    if (out[0] != out[1]) {
        printf("format %d %dx%d pad %d: the bytes between the rows reached the output\n", fmt, sw, sh, pad);
        ++bad;
    }
    for (int r = 0; r < count; ++r) {
        std::vector<uint8_t> want;
        for (int k = 0; k < kFrames; ++k) {
            // the dense source planes Y, U, V
            std::vector<uint8_t> y = content[k][0], u((size_t)sw * sh / 4), v(u.size());
            if (fmt == IN_I420) {
                u = content[k][1];
                v = content[k][2];
            }
            else
                for (size_t i = 0; i < u.size(); ++i) {
                    u[i] = content[k][1][2 * i];
                    v[i] = content[k][1][2 * i + 1];
                }
            const Rung& R = rungs[r];
            const std::vector<uint8_t> Y = scale_model(y, sw, sh, R.dw, R.dh, R.W, R.H);
            want.insert(want.end(), Y.begin(), Y.end());
            for (const auto* p : {&u, &v}) {
                const std::vector<uint8_t> c = scale_model(*p, sw / 2, sh / 2, R.dw / 2, R.dh / 2, R.W / 2, R.H / 2);
                want.insert(want.end(), c.begin(), c.end());
            }
        }
        if (out[0][r] != want) {
            size_t at = 0;
            while (at < want.size() && out[0][r][at] == want[at]) ++at;
            printf("format %d %dx%d rung %d (%dx%d in %dx%d) pad %d kind %d: byte %zu is %d, the definition gives %d\n", fmt, sw, sh, r, rungs[r].dw,
                   rungs[r].dh, rungs[r].W, rungs[r].H, pad, kind, at, out[0][r][at], want[at]);
            ++bad;
        }
    }
    return bad;
}

int main()
{
    int bad = 0, runs = 0;
    // tests/ld_testlib.py LADDERS: L1 (the identity, 2:1, 48/17 and 32/9 with edges) and L3 (three and nine taps in one launch)
    const std::vector<Rung> L1 = {{96, 64, 96, 64}, {48, 32, 48, 32}, {34, 18, 48, 32}}, L3 = {{192, 128, 192, 128}, {48, 32, 48, 32}};
    const int pads[] = {0, 6};
    for (int fmt = IN_I420; fmt <= IN_NV12; ++fmt)
        for (int pad : pads)
            for (int kind = 0; kind < 3; ++kind, runs += 2) {
                bad += one(fmt, 96, 64, L1, pad, kind);
                bad += one(fmt, 382, 254, L3, pad, kind);
            }
    if (bad) {
        printf("ladder: %d checks failed in %d runs\n", bad, runs);
        return 1;
    }
    printf("ladder ok: %d runs\n", runs);
    return 0;
}
