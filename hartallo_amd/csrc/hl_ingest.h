// hl_ingest.h -- frames that are not dense planar I420 (hl_amd_encode_frame /
// hl_amd_encode_frames): pitched I420, NV12, packed RGB24 / RGBA32 and planar
// RGB, turned into the dense I420 planes the coding path takes.  No reference
// interface: hl_frame_video_t has neither a pitch nor a format.
//
// Definition (integers only, unsigned 32-bit):
//   I420, NV12   copies: de-pitched, NV12's chroma de-interleaved;
//   RGB          Y = (yr R + yg G + yb B + (off << 16) + (1 << 15)) >> 16 per
//                sample; per 2x2 block, from the sums SR, SG, SB of its four
//                samples (0..1020), centre-sited and rounded once,
//                U = min(255, (ur SR + ug SG + ub SB + (128 << 18) + (1 << 17)) >> 18)
//                and V likewise.  Both accumulators are non-negative and below
//                2^26, so the negative coefficients are carried as their 32-bit
//                two's complement and the sums wrap to the true value.
// The coefficients come from one constexpr function of (Kr, Kb, range),
// in_coef: s = 2^16 (full range) or 219 2^16 / 255 (limited), c = 2^16 or
// 224 2^16 / 255, rnd = round-half-up of the exact rational,
//   yr = rnd(Kr s), yb = rnd(Kb s), yg = rnd(s) - yr - yb,
//   ub = rnd(c / 2), ur = -rnd(Kr / (2 (1 - Kb)) c), ug = -(ur + ub),
//   vr = rnd(c / 2), vb = -rnd(Kb / (2 (1 - Kr)) c), vg = -(vr + vb),
// so a chroma row sums to zero and grey gives exactly 128.
//
// One lane owns a tile of 16 columns x 2 rows and works wholly in registers:
// every load of the tile (RGB24 2 x 48 bytes, RGBA32 2 x 64, RGBP 6 x 16, NV12
// 2 x 16 + 16, I420 2 x 16 + 8 + 8) stands before the first use in the source
// (the compiler keeps that for I420, NV12 and RGBP and issues the packed RGB
// kernels' loads in two or three groups), then two 16-byte luma rows and one
// 8-byte row each of U and V are stored.  No LDS, no
// cross-lane traffic, no atomics.  A workgroup is 64 x 4 lanes: a wave owns 64
// consecutive tiles of one row pair (its loads of a sample row are one
// contiguous run, 1 KiB of luma), the four waves four row pairs.  W and H are
// multiples of 16: there are no partial tiles, only lanes beyond the picture
// (frames of a display size below the coded size: in_tile_edge, further down).
// Only the bytes [plane + r pitch, plane + r pitch + row bytes) of a row are
// read.  Host and device run the same in_tile (the CPU suite builds it into
// tests/emu/libhl_ingest_emu.so).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define HL_IN_HD __host__ __device__ __forceinline__
#else
#define HL_IN_HD inline
#endif

namespace hl {

enum { IN_I420 = 0, IN_NV12, IN_RGB24, IN_RGBA32, IN_RGBP, IN_FORMATS };  // = HL_AMD_FORMAT_*

// lanes of a workgroup: kInLanesX tiles of a row pair, kInLanesY row pairs
constexpr int kInLanesX = 64, kInLanesY = 4;

// planes a format has, and the bytes and rows of plane c of a W x H picture
constexpr int in_planes(int fmt) { return fmt == IN_I420 || fmt == IN_RGBP ? 3 : fmt == IN_NV12 ? 2 : 1; }
constexpr int64_t in_row_bytes(int fmt, int c, int W)
{
    return fmt == IN_I420 ? (c ? W / 2 : W) : fmt == IN_RGB24 ? 3 * (int64_t)W : fmt == IN_RGBA32 ? 4 * (int64_t)W : W;
}
constexpr int in_rows(int fmt, int c, int H) { return (fmt == IN_I420 || fmt == IN_NV12) && c ? H / 2 : H; }

// y, u, v rows of the matrix (negative entries as two's complement) and the luma offset
struct InCoef {
    uint32_t y[3], u[3], v[3], off;
};

// round-half-up of p / q (p >= 0, q > 0)
constexpr uint32_t in_rnd(uint64_t p, uint64_t q) { return (uint32_t)((2 * p + q) / (2 * q)); }

// Kr = krn / den, Kb = kbn / den
constexpr InCoef in_coef(uint32_t krn, uint32_t kbn, uint32_t den, bool full)
{
    const uint64_t sn = full ? 65536ull : 219ull * 65536, sd = full ? 1 : 255;  // s = sn / sd
    const uint64_t cn = full ? 65536ull : 224ull * 65536, cd = full ? 1 : 255;  // c = cn / cd
    InCoef k{};
    k.y[0] = in_rnd(krn * sn, den * sd);
    k.y[2] = in_rnd(kbn * sn, den * sd);
    k.y[1] = in_rnd(sn, sd) - k.y[0] - k.y[2];
    k.u[2] = in_rnd(cn, 2 * cd);
    k.u[0] = 0u - in_rnd(krn * cn, 2 * (uint64_t)(den - kbn) * cd);
    k.u[1] = 0u - (k.u[0] + k.u[2]);
    k.v[0] = in_rnd(cn, 2 * cd);
    k.v[2] = 0u - in_rnd(kbn * cn, 2 * (uint64_t)(den - krn) * cd);
    k.v[1] = 0u - (k.v[0] + k.v[2]);
    k.off = full ? 0 : 16;
    return k;
}

// matrix 0 = BT.601 (Kr 299 / 1000, Kb 114 / 1000), 1 = BT.709 (2126 / 10000, 722 / 10000); range 0 = limited, 1 = full
constexpr InCoef in_coef_of(int matrix, int range)
{
    return matrix ? in_coef(2126, 722, 10000, range != 0) : in_coef(299, 114, 1000, range != 0);
}

// A frame as the tile code takes it: the pitches are the real ones (never 0);
// dst = the dense Y, U, V planes (widths W, W / 2, W / 2).
struct InFrame {
    const uint8_t* plane[3];
    int64_t pitch[3];
    uint8_t* dst[3];
};

// N 4-byte words of a row.  On the device the address is 4-byte aligned
// (planes and pitches are, and every tile starts a multiple of 4 bytes into
// its row); adjacent words merge into wider loads.
template <int N>
HL_IN_HD void in_load(const uint8_t* p, uint32_t* r)
{
#if defined(__HIP_DEVICE_COMPILE__)
    for (int j = 0; j < N; ++j) r[j] = reinterpret_cast<const uint32_t*>(p)[j];
#else
    memcpy(r, p, 4 * N);
#endif
}

// N words to a destination row (on the device 4 N-byte aligned: one store)
template <int N>
HL_IN_HD void in_store(uint8_t* p, const uint32_t* r)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (N == 4) *reinterpret_cast<uint4*>(p) = make_uint4(r[0], r[1], r[2], r[3]);
    else *reinterpret_cast<uint2*>(p) = make_uint2(r[0], r[1]);
#else
    memcpy(p, r, 4 * N);
#endif
}

HL_IN_HD uint32_t in_byte(const uint32_t* r, int b) { return (r[b >> 2] >> (8 * (b & 3))) & 0xFFu; }

// the bytes 0, 2 of a word in bits 0..15
HL_IN_HD uint32_t in_even(uint32_t w) { return (w & 0xFFu) | ((w >> 8) & 0xFF00u); }

// sample k (0..15) of a tile row held in a: packed RGB24 (12 words), RGBA32
// (16 words), or RGBP as R | G | B (4 words each)
template <int FMT>
HL_IN_HD void in_rgb(const uint32_t* a, int k, uint32_t& R, uint32_t& G, uint32_t& B)
{
    if constexpr (FMT == IN_RGB24) {
        R = in_byte(a, 3 * k);
        G = in_byte(a, 3 * k + 1);
        B = in_byte(a, 3 * k + 2);
    }
    else if constexpr (FMT == IN_RGBA32) {
        R = a[k] & 0xFFu;
        G = (a[k] >> 8) & 0xFFu;
        B = (a[k] >> 16) & 0xFFu;
    }
    else {
        R = in_byte(a, k);
        G = in_byte(a + 4, k);
        B = in_byte(a + 8, k);
    }
}

// Tile (tx, ty) of a W-wide picture: columns [16 tx, 16 tx + 16), rows 2 ty and
// 2 ty + 1.  The caller keeps 16 tx < W and 2 ty + 1 < the height.
template <int FMT>
HL_IN_HD void in_tile(const InFrame& F, const InCoef& C, int W, int tx, int ty)
{
    static_assert(FMT >= 0 && FMT < IN_FORMATS, "HL_AMD_FORMAT_*");
    uint32_t yo[2][4], uo[2], vo[2];
    if constexpr (FMT == IN_I420 || FMT == IN_NV12) {
        const uint8_t* py = F.plane[0] + (int64_t)(2 * ty) * F.pitch[0] + 16 * tx;
        in_load<4>(py, yo[0]);
        in_load<4>(py + F.pitch[0], yo[1]);
        if constexpr (FMT == IN_I420) {
            in_load<2>(F.plane[1] + (int64_t)ty * F.pitch[1] + 8 * tx, uo);
            in_load<2>(F.plane[2] + (int64_t)ty * F.pitch[2] + 8 * tx, vo);
        }
        else {
            uint32_t c[4];
            in_load<4>(F.plane[1] + (int64_t)ty * F.pitch[1] + 16 * tx, c);
            for (int j = 0; j < 2; ++j) {
                uo[j] = in_even(c[2 * j]) | (in_even(c[2 * j + 1]) << 16);
                vo[j] = in_even(c[2 * j] >> 8) | (in_even(c[2 * j + 1] >> 8) << 16);
            }
        }
    }
    else {
        constexpr int N = FMT == IN_RGBA32 ? 16 : 12;
        uint32_t a[2][N];
        if constexpr (FMT == IN_RGBP) {
            for (int c = 0; c < 3; ++c) {
                const uint8_t* p = F.plane[c] + (int64_t)(2 * ty) * F.pitch[c] + 16 * tx;
                in_load<4>(p, a[0] + 4 * c);
                in_load<4>(p + F.pitch[c], a[1] + 4 * c);
            }
        }
        else {
            const uint8_t* p = F.plane[0] + (int64_t)(2 * ty) * F.pitch[0] + 4 * N * tx;
            in_load<N>(p, a[0]);
            in_load<N>(p + F.pitch[0], a[1]);
        }
        for (int j = 0; j < 4; ++j) yo[0][j] = yo[1][j] = 0;
        uo[0] = uo[1] = vo[0] = vo[1] = 0;
        const uint32_t ybias = (C.off << 16) + (1u << 15), cbias = (128u << 18) + (1u << 17);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int b = 0; b < 8; ++b) {  // the tile's 2x2 blocks
            uint32_t s[3] = {0, 0, 0};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
            for (int i = 0; i < 4; ++i) {
                const int r = i >> 1, k = 2 * b + (i & 1);
                uint32_t R, G, B;
                in_rgb<FMT>(a[r], k, R, G, B);
                yo[r][k >> 2] |= ((C.y[0] * R + C.y[1] * G + C.y[2] * B + ybias) >> 16) << (8 * (k & 3));
                s[0] += R;
                s[1] += G;
                s[2] += B;
            }
            const uint32_t u = (C.u[0] * s[0] + C.u[1] * s[1] + C.u[2] * s[2] + cbias) >> 18;
            const uint32_t v = (C.v[0] * s[0] + C.v[1] * s[1] + C.v[2] * s[2] + cbias) >> 18;
            uo[b >> 2] |= (u < 255u ? u : 255u) << (8 * (b & 3));
            vo[b >> 2] |= (v < 255u ? v : 255u) << (8 * (b & 3));
        }
    }
    uint8_t* dy = F.dst[0] + (size_t)(2 * ty) * W + 16 * tx;
    in_store<4>(dy, yo[0]);
    in_store<4>(dy + W, yo[1]);
    in_store<2>(F.dst[1] + (size_t)ty * (W >> 1) + 8 * tx, uo);
    in_store<2>(F.dst[2] + (size_t)ty * (W >> 1) + 8 * tx, vo);
}

// Every tile of one frame (the host's loop; the kernel's lanes take one each)
template <int FMT>
inline void in_frame(const InFrame& F, const InCoef& C, int W, int H)
{
    for (int ty = 0; ty < (H >> 1); ++ty)
        for (int tx = 0; tx < (W >> 4); ++tx) in_tile<FMT>(F, C, W, tx, ty);
}

// ---- frames of a display size dW x dH below the coded size W x H -------------
// (hl_amd_set_display_size: dW, dH even, W - 16 < dW <= W, H - 16 < dH <= H.)
// The frame's planes have the rows and row bytes of dW x dH, and the coded
// picture is the edge replication of the converted planes, through clamped
// coordinates: luma (x, y) = the converted luma of source sample
// (min(x, dW - 1), min(y, dH - 1)), chroma (bx, by) = the converted chroma of
// source 2x2 block (min(bx, dW / 2 - 1), min(by, dH / 2 - 1)) -- for RGB that
// block's SR, SG, SB through the arithmetic above.  A tile is full when
// tx < (dW >> 4) and ty < (dH >> 1): in_tile as it is.  Every other tile of the
// coded picture (at most one tile column and seven tile rows; with spatial
// layers, hl_amd_set_au_display_size, the top layer's margins go up to
// (16 << K) - 2: several tile columns, up to 63 tile rows) is an edge tile:
// in_tile_edge, which loads single bytes by clamped coordinate -- a 4-byte
// word could cross the end of a row whose bytes are no multiple of 4 -- and
// stores what in_tile stores.

// tiles of a row pair and row pairs that are full
constexpr int in_full_x(int dW) { return dW >> 4; }
constexpr int in_full_y(int dH) { return dH >> 1; }
// edge tiles of a picture: the right band's (the tile columns right of the full
// ones: one within a macroblock's margin, up to eight for a top layer), then the
// bottom rows' left of it
constexpr int in_edge_tiles(int W, int H, int dW, int dH)
{
    return ((W >> 4) - in_full_x(dW)) * (H >> 1) + in_full_x(dW) * ((H >> 1) - in_full_y(dH));
}

template <int FMT>
HL_IN_HD void in_tile_edge(const InFrame& F, const InCoef& C, int W, int dW, int dH, int tx, int ty)
{
    static_assert(FMT >= 0 && FMT < IN_FORMATS, "HL_AMD_FORMAT_*");
    uint32_t yo[2][4], uo[2], vo[2];
    for (int j = 0; j < 4; ++j) yo[0][j] = yo[1][j] = 0;
    uo[0] = uo[1] = vo[0] = vo[1] = 0;
    const int cy = ty < (dH >> 1) ? ty : (dH >> 1) - 1;  // the source's chroma row (its row pair)
    if constexpr (FMT == IN_I420 || FMT == IN_NV12) {
        for (int r = 0; r < 2; ++r) {
            const int y = 2 * ty + r < dH ? 2 * ty + r : dH - 1;
            const uint8_t* py = F.plane[0] + (int64_t)y * F.pitch[0];
            for (int k = 0; k < 16; ++k) {
                const int x = 16 * tx + k < dW ? 16 * tx + k : dW - 1;
                yo[r][k >> 2] |= (uint32_t)py[x] << (8 * (k & 3));
            }
        }
        for (int b = 0; b < 8; ++b) {
            const int cx = 8 * tx + b < (dW >> 1) ? 8 * tx + b : (dW >> 1) - 1;
            uint32_t u, v;
            if constexpr (FMT == IN_I420) {
                u = (F.plane[1] + (int64_t)cy * F.pitch[1])[cx];
                v = (F.plane[2] + (int64_t)cy * F.pitch[2])[cx];
            }
            else {
                const uint8_t* pc = F.plane[1] + (int64_t)cy * F.pitch[1] + 2 * cx;
                u = pc[0];
                v = pc[1];
            }
            uo[b >> 2] |= u << (8 * (b & 3));
            vo[b >> 2] |= v << (8 * (b & 3));
        }
    }
    else {
        const uint32_t ybias = (C.off << 16) + (1u << 15), cbias = (128u << 18) + (1u << 17);
        const bool iny = ty < (dH >> 1);  // else both rows are the source's last row
        for (int b = 0; b < 8; ++b) {     // the tile's 2x2 blocks, each from one source block
            const bool inx = 8 * tx + b < (dW >> 1);  // else both columns are the source's last column
            const int cx = inx ? 8 * tx + b : (dW >> 1) - 1;
            uint32_t s[3] = {0, 0, 0}, yv[2][2];
            for (int r = 0; r < 2; ++r)
                for (int i = 0; i < 2; ++i) {
                    const int x = 2 * cx + i;
                    const int64_t row = (int64_t)(2 * cy + r);
                    uint32_t R, G, B;
                    if constexpr (FMT == IN_RGBP) {
                        R = (F.plane[0] + row * F.pitch[0])[x];
                        G = (F.plane[1] + row * F.pitch[1])[x];
                        B = (F.plane[2] + row * F.pitch[2])[x];
                    }
                    else {
                        const uint8_t* p = F.plane[0] + row * F.pitch[0] + (FMT == IN_RGBA32 ? 4 : 3) * x;
                        R = p[0];
                        G = p[1];
                        B = p[2];
                    }
                    yv[r][i] = (C.y[0] * R + C.y[1] * G + C.y[2] * B + ybias) >> 16;
                    s[0] += R;
                    s[1] += G;
                    s[2] += B;
                }
            for (int r = 0; r < 2; ++r)
                for (int i = 0; i < 2; ++i) {
                    const int k = 2 * b + i;
                    yo[r][k >> 2] |= yv[iny ? r : 1][inx ? i : 1] << (8 * (k & 3));
                }
            const uint32_t u = (C.u[0] * s[0] + C.u[1] * s[1] + C.u[2] * s[2] + cbias) >> 18;
            const uint32_t v = (C.v[0] * s[0] + C.v[1] * s[1] + C.v[2] * s[2] + cbias) >> 18;
            uo[b >> 2] |= (u < 255u ? u : 255u) << (8 * (b & 3));
            vo[b >> 2] |= (v < 255u ? v : 255u) << (8 * (b & 3));
        }
    }
    uint8_t* dy = F.dst[0] + (size_t)(2 * ty) * W + 16 * tx;
    in_store<4>(dy, yo[0]);
    in_store<4>(dy + W, yo[1]);
    in_store<2>(F.dst[1] + (size_t)ty * (W >> 1) + 8 * tx, uo);
    in_store<2>(F.dst[2] + (size_t)ty * (W >> 1) + 8 * tx, vo);
}

// Edge tile i (< in_edge_tiles) of a picture: the right band's tiles row pair
// by row pair (its ex tile columns left to right), then the bottom rows' tiles
// left of that band
HL_IN_HD void in_edge_at(int i, int W, int H, int dW, int dH, int* tx, int* ty)
{
    const int fx = in_full_x(dW), ex = (W >> 4) - fx, right = ex * (H >> 1);
    if (i < right) {  // (ex = 1 within a macroblock's margin: tx = fx, ty = i)
        *tx = fx + i % ex;
        *ty = i / ex;
    }
    else {  // (fx > 0: there are tiles left of the band)
        const int j = i - right;
        *ty = in_full_y(dH) + j / fx;
        *tx = j - (j / fx) * fx;
    }
}

// Every tile of one frame of the display size dW x dH into the coded W x H
// planes: the full tiles, then the edge tiles in the order of the kernel's lanes
template <int FMT>
inline void in_frame_display(const InFrame& F, const InCoef& C, int W, int H, int dW, int dH)
{
    for (int ty = 0; ty < in_full_y(dH); ++ty)
        for (int tx = 0; tx < in_full_x(dW); ++tx) in_tile<FMT>(F, C, W, tx, ty);
    for (int i = 0; i < in_edge_tiles(W, H, dW, dH); ++i) {
        int tx, ty;
        in_edge_at(i, W, H, dW, dH, &tx, &ty);
        in_tile_edge<FMT>(F, C, W, dW, dH, tx, ty);
    }
}

#if defined(__HIPCC__)
// One launch for every frame (grid z) of one format.
struct InArgs {
    InFrame one;         // the one frame, when tab is null
    const InFrame* tab;  // else the launch's frames (device memory)
    InCoef coef;         // RGB formats
    int32_t W, H;        // the coded size: the destination planes'
    int32_t dW, dH;      // the frames' size (the display size); 0, 0 = W, H
};

constexpr int kInEdgeLanes = 64;  // lanes of a workgroup of k_ingest_edge: one edge tile each

// `frames` frames of format fmt on `stream`: k_ingest on the full tiles and,
// for frames below the coded size, k_ingest_edge on the others.  The margins
// W - dW and H - dH must be below max_margin: 16 for the AVC path (a display
// size lies within the last macroblock column and row), 16 << K for the top
// layer of K + 1 spatial layers (hl_amd_set_au_display_size), whose edge tiles
// then form a right band of up to 1 << K tile columns and a bottom band of up
// to (8 << K) - 1 tile rows (in_edge_tiles and in_edge_at take any width).
hipError_t launch_ingest(const InArgs& A, int fmt, int frames, hipStream_t stream, int max_margin = 16);

#if defined(HL_INGEST_KERNELS)  // hl_ingest.hip: the one translation unit that holds the kernels
template <int FMT>
__global__ __launch_bounds__(kInLanesX * kInLanesY) void k_ingest(InArgs A)
{
    const int tx = blockIdx.x * kInLanesX + threadIdx.x, ty = blockIdx.y * kInLanesY + threadIdx.y;
    if (tx >= (A.dW >> 4) || ty >= (A.dH >> 1)) return;  // lanes beyond the full tiles (the picture's, without a display size)
    if (A.tab) {
        const InFrame F = A.tab[blockIdx.z];
        in_tile<FMT>(F, A.coef, A.W, tx, ty);
    }
    else in_tile<FMT>(A.one, A.coef, A.W, tx, ty);
}

// the edge tiles of every frame (grid z), one lane each
template <int FMT>
__global__ __launch_bounds__(kInEdgeLanes) void k_ingest_edge(InArgs A)
{
    const int i = blockIdx.x * kInEdgeLanes + threadIdx.x;
    if (i >= in_edge_tiles(A.W, A.H, A.dW, A.dH)) return;  // lanes beyond the edge tiles
    int tx, ty;
    in_edge_at(i, A.W, A.H, A.dW, A.dH, &tx, &ty);
    if (A.tab) {
        const InFrame F = A.tab[blockIdx.z];
        in_tile_edge<FMT>(F, A.coef, A.W, A.dW, A.dH, tx, ty);
    }
    else in_tile_edge<FMT>(A.one, A.coef, A.W, A.dW, A.dH, tx, ty);
}

hipError_t launch_ingest(const InArgs& A0, int fmt, int frames, hipStream_t stream, int max_margin)
{
    InArgs A = A0;
    if (!A.dW && !A.dH) {
        A.dW = A.W;
        A.dH = A.H;
    }
    if (fmt < 0 || fmt >= IN_FORMATS || frames < 1 || frames > 65535 || A.W <= 0 || A.H <= 0 || (A.W & 15) || (A.H & 15) || ((A.dW | A.dH) & 1) ||
        max_margin < 16 || max_margin > 128 || A.dW <= A.W - max_margin || A.dW > A.W || A.dH <= A.H - max_margin || A.dH > A.H || A.dW <= 0 ||
        A.dH <= 0)
        return hipErrorInvalidValue;
    if (in_full_x(A.dW) > 0) {  // (dH >= 2: a full row pair)
        const dim3 block(kInLanesX, kInLanesY);
        const dim3 grid((in_full_x(A.dW) + kInLanesX - 1) / kInLanesX, (in_full_y(A.dH) + kInLanesY - 1) / kInLanesY, frames);
        if (fmt == IN_I420) k_ingest<IN_I420><<<grid, block, 0, stream>>>(A);
        else if (fmt == IN_NV12) k_ingest<IN_NV12><<<grid, block, 0, stream>>>(A);
        else if (fmt == IN_RGB24) k_ingest<IN_RGB24><<<grid, block, 0, stream>>>(A);
        else if (fmt == IN_RGBA32) k_ingest<IN_RGBA32><<<grid, block, 0, stream>>>(A);
        else k_ingest<IN_RGBP><<<grid, block, 0, stream>>>(A);
        const hipError_t rc = hipGetLastError();
        if (rc != hipSuccess) return rc;
    }
    const int edge = in_edge_tiles(A.W, A.H, A.dW, A.dH);
    if (edge > 0) {
        const dim3 grid((edge + kInEdgeLanes - 1) / kInEdgeLanes, 1, frames);
        if (fmt == IN_I420) k_ingest_edge<IN_I420><<<grid, kInEdgeLanes, 0, stream>>>(A);
        else if (fmt == IN_NV12) k_ingest_edge<IN_NV12><<<grid, kInEdgeLanes, 0, stream>>>(A);
        else if (fmt == IN_RGB24) k_ingest_edge<IN_RGB24><<<grid, kInEdgeLanes, 0, stream>>>(A);
        else if (fmt == IN_RGBA32) k_ingest_edge<IN_RGBA32><<<grid, kInEdgeLanes, 0, stream>>>(A);
        else k_ingest_edge<IN_RGBP><<<grid, kInEdgeLanes, 0, stream>>>(A);
    }
    return hipGetLastError();
}
#endif  // HL_INGEST_KERNELS
#endif

}  // namespace hl
