// hl_scale.h -- frames larger than the picture (hl_amd_set_source_size): the
// area downscaler k_scale between the frame ingest (hl_ingest.h) and the
// unchanged coding path.  No reference interface: the reference has no scaler
// (test_encoder.c:100-111 reads one pre-scaled file per layer).
//
// Definition (integers only, unsigned 32-bit).  Per axis, a source length s and
// a destination length d with d <= s <= 8 d, s <= 4096: g = gcd(s, d),
// sr = s / g, dr = d / g.  Output sample j covers [j sr, (j + 1) sr), source
// sample i covers [i dr, (i + 1) dr), and
//   w(j, i) = max(0, min((j + 1) sr, (i + 1) dr) - max(j sr, i dr)).
// The taps of j are i = floor(j sr / dr) .. floor(((j + 1) sr - 1) / dr): at
// most ceil(sr / dr) + 1 <= 9, every weight positive, their sum sr.  A plane,
// with D = srw srh:
//   out(x, y) = floor((sum_k sum_i wv(y, k) wh(x, i) p(k, i) + (D >> 1)) / D),
// separable, unrounded, rounded once (half up).  A horizontal sum is at most
// 255 * 4096 and acc + (D >> 1) at most 255 * 2^24 + 2^23: all of it fits 32
// unsigned bits.  Luma goes sw x sh -> dw x dh, U and V go sw / 2 x sh / 2 ->
// dw / 2 x dh / 2 with the same sr, dr (chroma stays centre-sited, as in the
// ingest).  Beyond the display size the coded planes take
// out(min(x, dw - 1), min(y, dh - 1)): np.pad(mode="edge") of the scaled planes.
// 2:1 on both axes is the 2x2 box of synth._down2 / k_pyramid bit for bit; 4:1
// is NOT that box applied twice (the staged rounding of DESIGN.md §11: on a
// 96x64 noise plane 77 of 384 samples differ).
//
// k_scale: a workgroup of 256 lanes owns an output tile of 64 columns x 16
// rows of one plane (grid x: the tile, y: the plane, z: the frame).  Phase 1:
// lane = (column c = lane & 63, wave = lane >> 6) reduces the tile's footprint
// rows row0 + wave, row0 + wave + 4, ... horizontally -- byte loads at the
// column's taps, a wave's loads of one row lie in one run of at most 64 * 8 + 8
// bytes -- into LDS as one 32-bit sum per (footprint row, column).  Phase 2:
// lane = (word wx = lane & 15, row ry = lane >> 4) sums four adjacent columns
// vertically from LDS (one 16-byte read per tap), divides by the uniform D with
// a host-computed reciprocal and one correction step, and stores the four
// samples as one word.  The footprint of 16 output rows is at most
// ceil(16 srh / drh) + 1 rows: at ratio 8 that is 129 rows x 64 columns x 4
// bytes = 33,024 bytes of LDS (8,448 at 2:1).  No atomics, no inter-workgroup
// traffic; the tap loops run to the launch's uniform maximum tap count, with
// weight 0 and a clamped index for a sample that has fewer.  Every source byte
// is fetched from HBM about once (neighbouring tiles share at most one source
// row or column).  Host and device run the same per-lane functions (the CPU
// suite builds them into tests/emu/libhl_scale_emu.so).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define HL_SK_HD __host__ __device__ __forceinline__
#else
#define HL_SK_HD inline
#endif

namespace hl {

constexpr int kSkMaxTaps = 9, kSkMaxRatio = 8, kSkMaxSource = 4096;
constexpr int kSkTileW = 64, kSkTileH = 16, kSkLanes = 256;  // lanes = 64 columns x 4 waves = 16 words x 16 rows

constexpr uint32_t sk_gcd(uint32_t a, uint32_t b) { return b ? sk_gcd(b, a % b) : a; }

// an axis the scaler takes (the pure function's rule; the encoder's sizes are even as well)
constexpr bool sk_axis_ok(int64_t s, int64_t d) { return d > 0 && s >= d && s <= kSkMaxRatio * d && s <= kSkMaxSource; }

// first and last tap of output j, and the weight of source sample i in it (0 outside its taps)
HL_SK_HD uint32_t sk_first(uint32_t sr, uint32_t dr, uint32_t j) { return j * sr / dr; }
HL_SK_HD uint32_t sk_last(uint32_t sr, uint32_t dr, uint32_t j) { return ((j + 1) * sr - 1) / dr; }
HL_SK_HD uint32_t sk_weight(uint32_t sr, uint32_t dr, uint32_t j, uint32_t i)
{
    const uint32_t a = j * sr, b = i * dr;
    const uint32_t lo = a > b ? a : b, hi = a + sr < b + dr ? a + sr : b + dr;
    return hi > lo ? hi - lo : 0;
}

// the taps of output j: the first source sample, and kSkMaxTaps weights from it on (0 beyond the last tap)
struct SkTaps {
    uint32_t first, w[kSkMaxTaps];
};
HL_SK_HD SkTaps sk_taps_of(uint32_t sr, uint32_t dr, uint32_t j)
{
    SkTaps T;
    T.first = sk_first(sr, dr, j);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int t = 0; t < kSkMaxTaps; ++t) T.w[t] = sk_weight(sr, dr, j, T.first + (uint32_t)t);
    return T;
}

// hl_amd_scale_taps: the tap count of output j of the axis s -> d, *first and
// the weights; 0 for an axis the scaler refuses, j outside [0, d) or cap too small
inline int32_t sk_taps(int32_t s, int32_t d, int32_t j, int32_t* first, uint32_t* weights, int32_t cap)
{
    if (!first || !weights || !sk_axis_ok(s, d) || j < 0 || j >= d) return 0;
    const uint32_t g = sk_gcd((uint32_t)s, (uint32_t)d), sr = (uint32_t)s / g, dr = (uint32_t)d / g;
    const uint32_t a = sk_first(sr, dr, (uint32_t)j), n = sk_last(sr, dr, (uint32_t)j) - a + 1;
    if ((int64_t)cap < (int64_t)n) return 0;
    *first = (int32_t)a;
    for (uint32_t t = 0; t < n; ++t) weights[t] = sk_weight(sr, dr, (uint32_t)j, a + t);
    return (int32_t)n;
}

// the largest tap count of an axis (the outputs repeat with period dr)
inline int sk_max_taps(uint32_t sr, uint32_t dr)
{
    uint32_t m = 1;
    for (uint32_t j = 0; j < dr; ++j) {
        const uint32_t n = sk_last(sr, dr, j) - sk_first(sr, dr, j) + 1;
        m = n > m ? n : m;
    }
    return (int)m;
}

// floor(n / D) for every n < 2^32 and 1 <= D <= 2^24 (the definition needs
// n <= 255 D + (D >> 1)): M = min(2^32 - 1, floor(2^32 / D)) >= 2^32 / D - 1, so
// n / D - n M / 2^32 <= n / 2^32 < 1: the estimate is the quotient or one below it
constexpr uint32_t sk_recip(uint32_t D) { return D <= 1 ? 0xFFFFFFFFu : (uint32_t)((1ull << 32) / D); }
HL_SK_HD uint32_t sk_div(uint32_t n, uint32_t D, uint32_t M)
{
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t q = __umulhi(n, M);
#else
    uint32_t q = (uint32_t)(((uint64_t)n * M) >> 32);
#endif
    if (n - q * D >= D) ++q;
    return q;
}

// what a launch (or the host's loop) needs besides the planes: uniform
struct SkParm {
    uint32_t srw, drw, srh, drh, D, M;
    int32_t ntw, nth;  // the axes' largest tap counts
    int32_t lrows;     // footprint rows a tile can have: ceil(16 srh / drh) + 1
    int32_t sw, sh;    // the source's size (luma)
    int32_t sp;        // ... and the bytes between its luma rows (chroma: half)
    int32_t dw, dh;    // the display size: what the source is scaled to
    int32_t W, H;      // the coded size: the destination planes'
};

// sw x sh -> dw x dh in W x H, of any parity (one plane: the host build's single-plane export); false for axes the scaler refuses
inline bool sk_parm_any(int sw, int sh, int sp, int dw, int dh, int W, int H, SkParm* P)
{
    if (!sk_axis_ok(sw, dw) || !sk_axis_ok(sh, dh) || dw > W || dh > H || W <= 0 || H <= 0 || (W & 15) || (H & 15) || sp < sw) return false;
    const uint32_t gw = sk_gcd((uint32_t)sw, (uint32_t)dw), gh = sk_gcd((uint32_t)sh, (uint32_t)dh);
    P->srw = (uint32_t)sw / gw;
    P->drw = (uint32_t)dw / gw;
    P->srh = (uint32_t)sh / gh;
    P->drh = (uint32_t)dh / gh;
    P->D = P->srw * P->srh;
    P->M = sk_recip(P->D);
    P->ntw = sk_max_taps(P->srw, P->drw);
    P->nth = sk_max_taps(P->srh, P->drh);
    P->lrows = (int32_t)((kSkTileH * P->srh + P->drh - 1) / P->drh) + 1;
    P->sw = sw;
    P->sh = sh;
    P->sp = sp;
    P->dw = dw;
    P->dh = dh;
    P->W = W;
    P->H = H;
    return true;
}
// a frame: sw x sh (even) -> dw x dh (even) in W x H; false for what hl_amd_set_source_size refuses
inline bool sk_parm(int sw, int sh, int sp, int dw, int dh, int W, int H, SkParm* P)
{
    return !((sw | sh | sp | dw | dh) & 1) && sk_parm_any(sw, sh, sp, dw, dh, W, H, P);
}
constexpr size_t sk_lds_bytes(int lrows) { return (size_t)lrows * kSkTileW * sizeof(uint32_t); }

// a frame: the dense-pitched source planes (Y, U, V; pitches sp, sp / 2, sp / 2) and the dense destination planes
struct SkFrame {
    const uint8_t* src[3];
    uint8_t* dst[3];
};

// plane c's tiles
HL_SK_HD int sk_tiles_x(const SkParm& P, int c) { return ((P.W >> (c > 0)) + kSkTileW - 1) / kSkTileW; }
HL_SK_HD int sk_tiles_y(const SkParm& P, int c) { return ((P.H >> (c > 0)) + kSkTileH - 1) / kSkTileH; }

// a tile of plane c: its first column and row, and its footprint rows [row0, rowlast] of the source plane
struct SkTile {
    int32_t c, x0, y0, row0, rowlast;
};
HL_SK_HD SkTile sk_tile(const SkParm& P, int c, int tile)
{
    const int ntx = sk_tiles_x(P, c), dh = P.dh >> (c > 0);
    SkTile T;
    T.c = c;
    T.x0 = (tile % ntx) * kSkTileW;
    T.y0 = (tile / ntx) * kSkTileH;
    const int j0 = T.y0 < dh ? T.y0 : dh - 1, j1 = T.y0 + kSkTileH - 1 < dh ? T.y0 + kSkTileH - 1 : dh - 1;  // the clamped edge
    T.row0 = (int32_t)sk_first(P.srh, P.drh, (uint32_t)j0);
    T.rowlast = (int32_t)sk_last(P.srh, P.drh, (uint32_t)j1);  // (< the source's rows: (j1 + 1) srh <= dh srh = sh drh)
    if (T.rowlast > T.row0 + P.lrows - 1) T.rowlast = T.row0 + P.lrows - 1;  // (never: lrows is the bound)
    return T;
}

// Phase 1, column col (0..63) of the tile (src: the tile's source plane): the horizontal sums of the footprint
// rows row0 + r0, row0 + r0 + rstep, ... into lds[row][col]
HL_SK_HD void sk_reduce(const uint8_t* src, const SkParm& P, const SkTile& T, uint32_t* lds, int col, int r0, int rstep)
{
    const int sh1 = T.c > 0, sw = P.sw >> sh1, dw = P.dw >> sh1;
    const int x = T.x0 + col, j = x < dw ? x : dw - 1;  // the clamped edge (columns beyond the plane too: their sums are not used)
    const SkTaps K = sk_taps_of(P.srw, P.drw, (uint32_t)j);
    uint32_t at[kSkMaxTaps];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int t = 0; t < kSkMaxTaps; ++t) at[t] = K.first + (uint32_t)t < (uint32_t)sw ? K.first + (uint32_t)t : (uint32_t)sw - 1;  // (weight 0 beyond the taps)
    const int64_t pitch = P.sp >> sh1;
    for (int r = r0; r <= T.rowlast - T.row0; r += rstep) {
        const uint8_t* row = src + (int64_t)(T.row0 + r) * pitch;
        uint32_t h = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int t = 0; t < kSkMaxTaps; ++t)
            if (t < P.ntw) h += K.w[t] * row[at[t]];
        lds[r * kSkTileW + col] = h;
    }
}

// Phase 2, word wx (0..15) of row ry (0..15) of the tile (dst: its destination plane): four samples summed
// vertically from lds, divided and stored as one word
HL_SK_HD void sk_output(uint8_t* dst, const SkParm& P, const SkTile& T, const uint32_t* lds, int wx, int ry)
{
    const int sh1 = T.c > 0, W = P.W >> sh1, H = P.H >> sh1, dh = P.dh >> sh1;
    const int x = T.x0 + 4 * wx, y = T.y0 + ry;
    if (x >= W || y >= H) return;  // (W is a multiple of 8: whole words)
    const int j = y < dh ? y : dh - 1;  // the clamped edge
    const SkTaps K = sk_taps_of(P.srh, P.drh, (uint32_t)j);
    uint32_t acc[4] = {0, 0, 0, 0};
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int t = 0; t < kSkMaxTaps; ++t)
        if (t < P.nth) {
            const int i = (int)K.first + t < T.rowlast ? (int)K.first + t : T.rowlast;  // (weight 0 beyond the taps)
            const uint32_t* p = lds + (i - T.row0) * kSkTileW + 4 * wx;
#if defined(__HIP_DEVICE_COMPILE__)
            const uint4 v = *reinterpret_cast<const uint4*>(p);
            acc[0] += K.w[t] * v.x;
            acc[1] += K.w[t] * v.y;
            acc[2] += K.w[t] * v.z;
            acc[3] += K.w[t] * v.w;
#else
            for (int k = 0; k < 4; ++k) acc[k] += K.w[t] * p[k];
#endif
        }
    uint32_t word = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k) word |= sk_div(acc[k] + (P.D >> 1), P.D, P.M) << (8 * k);
    uint8_t* d = dst + (size_t)y * W + x;
#if defined(__HIP_DEVICE_COMPILE__)
    *reinterpret_cast<uint32_t*>(d) = word;
#else
    memcpy(d, &word, 4);
#endif
}

// Every tile of one frame, lanes in the kernel's order (the host's loop); lds: sk_lds_bytes(P.lrows)
inline void sk_frame(const SkFrame& F, const SkParm& P, uint32_t* lds)
{
    for (int c = 0; c < 3; ++c)
        for (int tile = 0; tile < sk_tiles_x(P, c) * sk_tiles_y(P, c); ++tile) {
            const SkTile T = sk_tile(P, c, tile);
            for (int lane = 0; lane < kSkLanes; ++lane) sk_reduce(F.src[c], P, T, lds, lane & 63, lane >> 6, 4);
            for (int lane = 0; lane < kSkLanes; ++lane) sk_output(F.dst[c], P, T, lds, lane & 15, lane >> 4);
        }
}

#if defined(__HIPCC__)
// One launch for every frame (grid z).
struct SkArgs {
    SkFrame one;         // the one frame, when tab is null
    const SkFrame* tab;  // else the launch's frames (device memory)
    SkParm parm;
};

// `frames` frames on `stream`
hipError_t launch_scale(const SkArgs& A, int frames, hipStream_t stream);

#if defined(HL_SCALE_KERNELS)  // hl_scale.hip: the one translation unit that holds the kernel
__global__ __launch_bounds__(kSkLanes) void k_scale(SkArgs A)
{
    extern __shared__ __align__(16) uint32_t sk_lds[];
    const int c = blockIdx.y;
    if ((int)blockIdx.x >= sk_tiles_x(A.parm, c) * sk_tiles_y(A.parm, c)) return;  // the chroma planes have fewer tiles (uniform)
    const SkFrame F = A.tab ? A.tab[blockIdx.z] : A.one;
    const uint8_t* src = c == 0 ? F.src[0] : c == 1 ? F.src[1] : F.src[2];  // (no indexed copy of F: that would live in scratch)
    uint8_t* dst = c == 0 ? F.dst[0] : c == 1 ? F.dst[1] : F.dst[2];
    const SkTile T = sk_tile(A.parm, c, blockIdx.x);
    sk_reduce(src, A.parm, T, sk_lds, threadIdx.x & 63, threadIdx.x >> 6, 4);
    __syncthreads();
    sk_output(dst, A.parm, T, sk_lds, threadIdx.x & 15, threadIdx.x >> 4);
}

hipError_t launch_scale(const SkArgs& A, int frames, hipStream_t stream)
{
    const SkParm& P = A.parm;
    SkParm Q;
    if (frames < 1 || frames > 65535 || !sk_parm(P.sw, P.sh, P.sp, P.dw, P.dh, P.W, P.H, &Q) || memcmp(&P, &Q, sizeof(Q)) != 0 ||
        P.lrows > kSkTileH * kSkMaxRatio + 1)
        return hipErrorInvalidValue;
    const dim3 grid(sk_tiles_x(P, 0) * sk_tiles_y(P, 0), 3, frames);
    k_scale<<<grid, kSkLanes, sk_lds_bytes(P.lrows), stream>>>(A);
    return hipGetLastError();
}
#endif  // HL_SCALE_KERNELS
#endif

}  // namespace hl
