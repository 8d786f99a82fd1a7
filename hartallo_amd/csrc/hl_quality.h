// hl_quality.h -- per-picture PSNR and SSIM sums of a coded picture against
// its source (hl_amd_set_quality).  No reference interface: the reference has
// nothing that measures a coded picture.
//
// Integers only, so every result is exact in any order.  Per plane (Y, U, V)
// of W x H samples, W and H multiples of 8, a = source, b = reconstruction:
//   per 4x4 block   s1 = sum a, s2 = sum b, ss = sum (a^2 + b^2), s12 = sum a b
//   sse             = sum over blocks of (ss - 2 s12)  (= sum (a - b)^2)
//   per 8x8 window  (the 2x2 blocks at every block position (bx, by),
//                   bx <= W/4 - 2, by <= H/4 - 2: stride 4) S1, S2, SS, S12 =
//                   the sums over its four blocks, C1 = 416, C2 = 235963,
//     var = 64 SS - S1^2 - S2^2        cov = 64 S12 - S1 S2
//     num = (2 S1 S2 + C1)(2 cov + C2) den = (S1^2 + S2^2 + C1)(var + C2) > 0
//     Q   = floor(num 2^30 / den)      (num may be negative)
//   ssim_q30        = sum over windows of Q
// |num| <= den (2 S1 S2 <= S1^2 + S2^2; |2 cov| <= var by Cauchy-Schwarz), and
// both stay below 2^59, so the quotient is formed by a 30-step restoring
// division on the 64-bit remainder (q_div30); nothing is floating point.
//
// k_quality: one workgroup of 256 lanes takes a tile of kQTileBX x kQTileBY =
// 64 x 8 blocks (256 x 32 samples) of one plane (grid z = 3 picture + plane)
// and needs the block sums of the tile plus one halo block column and one halo
// block row: 9 rows of 33 strips.  A lane owns a strip of 8 x 4 samples (two
// blocks) of both pictures -- four 8-byte row loads each, all eight issued
// before the first use; consecutive lanes own consecutive strips of a row (512
// contiguous bytes per wave and row).  Strips 256..296 (the last rows' and the
// halo's) are a second strip of lanes 0..40, loaded with the first.  A strip
// outside the plane is not loaded (its sums are zero; no window uses them).
// The block sums go to LDS packed into three words, s1 | s2 << 16, ss, s12
// (three arrays of 9 x 66 words, 7 128 bytes; a lane stores its two blocks'
// words side by side, and the window phase reads consecutive words in
// consecutive lanes: no bank conflicts).  Then one lane per window (two
// windows a lane) adds its four blocks and divides, 32 lanes add the luma SSE
// of the tile's 16 x 2 macroblocks from LDS (the tests' handle), the waves add
// their lanes' sums with shuffles, and lane 0 of the workgroup adds the two
// totals into the picture's sums with integer atomicAdd (exact in any order).
//
// With a display size (hl_amd_set_display_size) only the display rectangle of
// each plane is measured, a window of ww x wh samples at the plane's top left
// (dW x dH of luma, dW / 2 x dH / 2 of chroma: any size, odd ones too).  The
// strips are loaded as ever and the bytes of a strip outside the window are
// zeroed in both pictures (q_mask: a byte mask on the two words of a row, a
// zero row beyond the window), so every block sum, the SSE and the per-
// macroblock SSE are those of the window's samples without a second code
// path; the 8x8 windows counted are those wholly inside, (bx, by) with
// bx <= ww/4 - 2, by <= wh/4 - 2.  Without a display size no mask is applied.
//
// Host and device run the same per-strip and per-window code (the CPU suite
// builds it into tests/emu/libhl_quality_emu.so and libhl_display_emu.so).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define HL_Q_HD __host__ __device__ __forceinline__
#define HL_Q_UNROLL _Pragma("unroll")
#else
#define HL_Q_HD inline
#define HL_Q_UNROLL
#endif

namespace hl {

constexpr int kQTileBX = 64, kQTileBY = 8;       // blocks of a workgroup's tile (256 x 32 samples)
constexpr int kQStripsX = kQTileBX / 2 + 1;      // strips (two blocks) of a staged row: the tile's and the halo column's
constexpr int kQRows = kQTileBY + 1;             // staged block rows: the tile's and the halo row
constexpr int kQStrips = kQStripsX * kQRows;     // 297
constexpr int kQLdsW = 2 * kQStripsX;            // blocks of a staged row (66; the last one is never read)
constexpr int64_t kQC1 = 416, kQC2 = 235963;     // (0.01 255)^2 64^2, (0.03 255)^2 64 63: 8 bits, 64-sample windows

// acc + the four byte products of a and b
HL_Q_HD uint32_t q_dot4(uint32_t a, uint32_t b, uint32_t acc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_udot4(a, b, acc, false);
#else
    for (int i = 0; i < 4; ++i) acc += ((a >> (8 * i)) & 255u) * ((b >> (8 * i)) & 255u);
    return acc;
#endif
}

// Strip i (< kQStrips) of the tile whose first block is (bx0, by0), in a W x H
// plane: the index of its first block in the staged arrays; in *off the byte
// offset of its first row, or -1 when it lies outside the plane (strips are
// wholly in or out: W and H are multiples of 8); in *own whether it belongs to
// the tile itself (its SSE counts here), not to the halo.
HL_Q_HD int q_strip(int i, int bx0, int by0, int W, int H, ptrdiff_t* off, bool* own)
{
    const int r = i / kQStripsX, c = i - r * kQStripsX;
    const int x = 4 * bx0 + 8 * c, y = 4 * (by0 + r);
    *off = x < W && y < H ? (ptrdiff_t)y * W + x : (ptrdiff_t)-1;
    *own = r < kQTileBY && c < kQTileBX / 2;
    return r * kQLdsW + 2 * c;
}

// the packed sums of one 4x4 block: a[r], b[r] = row r's four samples of the source and the reconstruction
HL_Q_HD void q_block(const uint32_t a[4], const uint32_t b[4], uint32_t p[3])
{
    uint32_t s1 = 0, s2 = 0, ss = 0, s12 = 0;
    HL_Q_UNROLL
    for (int r = 0; r < 4; ++r) {
        s1 = q_dot4(a[r], 0x01010101u, s1);
        s2 = q_dot4(b[r], 0x01010101u, s2);
        ss = q_dot4(a[r], a[r], ss);
        ss = q_dot4(b[r], b[r], ss);
        s12 = q_dot4(a[r], b[r], s12);
    }
    p[0] = s1 | (s2 << 16);  // (each <= 16 * 255)
    p[1] = ss;
    p[2] = s12;
}

// sum (a - b)^2 of a block (or of any sum of blocks) from its ss and s12
HL_Q_HD uint32_t q_sse(uint32_t ss, uint32_t s12) { return ss - 2u * s12; }

// floor(num 2^30 / den), den > 0, |num| and den < 2^62 with |num| / den < 2^33
HL_Q_HD int64_t q_div30(int64_t num, int64_t den)
{
    const bool neg = num < 0;
    const uint64_t n = neg ? (uint64_t)0 - (uint64_t)num : (uint64_t)num, d = (uint64_t)den;
    uint64_t q = 0, r = n;
    if (n >= d) {  // (only n == d with this header's num and den)
        q = n / d;
        r = n % d;
    }
    for (int i = 0; i < 30; ++i) {
        r <<= 1;
        q <<= 1;
        if (r >= d) {
            r -= d;
            q |= 1u;
        }
    }
    return neg ? -(int64_t)(q + (r != 0)) : (int64_t)q;  // floor of a negative quotient
}

// Q of one window from the sums of its four blocks' packed words (the packed
// word adds without carry between its halves: S1, S2 <= 64 * 255)
HL_Q_HD int64_t q_window(uint32_t p0, uint32_t ssu, uint32_t s12u)
{
    const int64_t S1 = p0 & 0xFFFFu, S2 = p0 >> 16, SS = ssu, S12 = s12u;
    const int64_t var = 64 * SS - S1 * S1 - S2 * S2, cov = 64 * S12 - S1 * S2;
    const int64_t num = (2 * S1 * S2 + kQC1) * (2 * cov + kQC2);
    const int64_t den = (S1 * S1 + S2 * S2 + kQC1) * (var + kQC2);
    return q_div30(num, den);
}

// the window at block (wx, wy) of the staged arrays
HL_Q_HD int64_t q_window_at(const uint32_t* s0, const uint32_t* s1, const uint32_t* s2, int wx, int wy)
{
    const int i = wy * kQLdsW + wx;
    return q_window(s0[i] + s0[i + 1] + s0[i + kQLdsW] + s0[i + kQLdsW + 1], s1[i] + s1[i + 1] + s1[i + kQLdsW] + s1[i + kQLdsW + 1],
                    s2[i] + s2[i + 1] + s2[i + kQLdsW] + s2[i + kQLdsW + 1]);
}

// luma SSE of the tile's macroblock (mx, my) (mx < 16, my < 2) from the staged arrays
HL_Q_HD uint32_t q_mb_sse(const uint32_t* s1, const uint32_t* s2, int mx, int my)
{
    uint32_t ss = 0, s12 = 0;
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            const int i = (4 * my + r) * kQLdsW + 4 * mx + c;
            ss += s1[i];
            s12 += s2[i];
        }
    return q_sse(ss, s12);
}

// The bytes of sample row y of a strip at column x that lie inside the window
// of ww x wh samples (the plane's top-left rectangle), as masks of the row's
// two words; both 0 for a row beyond the window
HL_Q_HD void q_mask(int x, int y, int ww, int wh, uint32_t* lo, uint32_t* hi)
{
    const int left = ww - x, nv = y < wh ? (left < 0 ? 0 : left > 8 ? 8 : left) : 0;
    *lo = nv >= 4 ? 0xFFFFFFFFu : (1u << (8 * nv)) - 1u;
    *hi = nv <= 4 ? 0u : nv >= 8 ? 0xFFFFFFFFu : (1u << (8 * (nv - 4))) - 1u;
}

// the first sample of strip i of the tile whose first block is (bx0, by0)
HL_Q_HD void q_strip_xy(int i, int bx0, int by0, int* x, int* y)
{
    const int r = i / kQStripsX, c = i - r * kQStripsX;
    *x = 4 * bx0 + 8 * c;
    *y = 4 * (by0 + r);
}

// 8x8 windows (stride 4) that lie wholly inside a plane or window of w x h samples
constexpr uint64_t q_windows(int w, int h) { return (uint64_t)(w / 4 > 1 ? w / 4 - 1 : 0) * (uint64_t)(h / 4 > 1 ? h / 4 - 1 : 0); }

// One plane pair on the host, tile by tile as the kernel's workgroups take it
// (the same staging indices, the same per-strip and per-window code), measured
// over the window of ww x wh samples at the plane's top left (any size from
// 1 x 1 to W x H): the bytes of a loaded strip outside the window are zeroed in
// both pictures, so every sum is that of the window's samples, and the 8x8
// windows counted are those wholly inside it.
// *sse += sum (a - b)^2, *ssim += sum Q; mb (or null) = the SSE of every 16x16
// macroblock's part inside the window (W, H multiples of 16 then).
inline void quality_plane_window_host(const uint8_t* a, const uint8_t* b, int W, int H, int ww, int wh, uint64_t* sse, int64_t* ssim,
                                      uint32_t* mb)
{
    uint32_t s[3][kQRows * kQLdsW];
    for (int by0 = 0; 4 * by0 < H; by0 += kQTileBY)
        for (int bx0 = 0; 4 * bx0 < W; bx0 += kQTileBX) {
            memset(s, 0xA5, sizeof(s));  // (what the kernel leaves unwritten: nothing that is read)
            for (int i = 0; i < kQStrips; ++i) {
                ptrdiff_t off;
                bool own;
                const int at = q_strip(i, bx0, by0, W, H, &off, &own);
                int x, y;
                q_strip_xy(i, bx0, by0, &x, &y);
                uint32_t va[4][2] = {}, vb[4][2] = {};
                for (int r = 0; r < 4 && off >= 0; ++r) {
                    uint32_t m[2];
                    q_mask(x, y + r, ww, wh, &m[0], &m[1]);
                    memcpy(va[r], a + off + (ptrdiff_t)r * W, 8);
                    memcpy(vb[r], b + off + (ptrdiff_t)r * W, 8);
                    for (int h = 0; h < 2; ++h) {
                        va[r][h] &= m[h];
                        vb[r][h] &= m[h];
                    }
                }
                for (int h = 0; h < 2; ++h) {
                    const uint32_t ra[4] = {va[0][h], va[1][h], va[2][h], va[3][h]}, rb[4] = {vb[0][h], vb[1][h], vb[2][h], vb[3][h]};
                    uint32_t p[3];
                    q_block(ra, rb, p);
                    for (int k = 0; k < 3; ++k) s[k][at + h] = p[k];
                    if (own) *sse += q_sse(p[1], p[2]);
                }
            }
            for (int w = 0; w < kQTileBX * kQTileBY; ++w) {
                const int wx = w % kQTileBX, wy = w / kQTileBX;
                if (bx0 + wx <= ww / 4 - 2 && by0 + wy <= wh / 4 - 2) *ssim += q_window_at(s[0], s[1], s[2], wx, wy);
            }
            for (int m = 0; mb && m < 32; ++m) {
                const int mbx = bx0 / 4 + (m & 15), mby = by0 / 4 + (m >> 4);
                if (mbx < W / 16 && mby < H / 16) mb[(size_t)mby * (W / 16) + mbx] = q_mb_sse(s[1], s[2], m & 15, m >> 4);
            }
        }
}

// the whole plane (the window is the plane: every mask is all ones)
inline void quality_plane_host(const uint8_t* a, const uint8_t* b, int W, int H, uint64_t* sse, int64_t* ssim, uint32_t* mb)
{
    quality_plane_window_host(a, b, W, H, W, H, sse, ssim, mb);
}

#if defined(__HIPCC__)
// One launch for a group of pictures (grid z = 3 picture + plane).
struct QualityArgs {
    const uint8_t* const* tab;     // [pictures][6] source Y, U, V, reconstruction Y, U, V (device memory), or null:
    const uint8_t* one[6];         // ... the planes of a launch of one picture
    unsigned long long* sums;      // [pictures][3][2] sse, ssim_q30 (two's complement), zeroed before the launch
    uint32_t* mb;                  // [pictures][(W / 16)(H / 16)] luma SSE per macroblock
    int32_t W, H;                  // the luma size, multiples of 16; planes dense, 8-byte aligned
    int32_t dW, dH;                // the luma window measured (the display size, even), 0, 0: the whole picture
};

__global__ __launch_bounds__(256) void k_quality(QualityArgs A)
{
    __shared__ __attribute__((aligned(8))) uint32_t s_b[3][kQRows * kQLdsW];
    __shared__ unsigned long long s_part[4][2];
    const int pic = (int)blockIdx.z / 3, plane = (int)blockIdx.z - 3 * pic;
    const int W = plane ? A.W >> 1 : A.W, H = plane ? A.H >> 1 : A.H;
    const int bx0 = (int)blockIdx.x * kQTileBX, by0 = (int)blockIdx.y * kQTileBY;
    if (4 * bx0 >= W || 4 * by0 >= H) return;  // (the whole workgroup: the grid is the luma plane's)
    const uint8_t *src, *rec;
    if (A.tab) {
        src = A.tab[6 * (size_t)pic + plane];
        rec = A.tab[6 * (size_t)pic + 3 + plane];
    }
    else {
        src = plane == 0 ? A.one[0] : plane == 1 ? A.one[1] : A.one[2];
        rec = plane == 0 ? A.one[3] : plane == 1 ? A.one[4] : A.one[5];
    }
    // the window measured: the plane's top-left ww x wh samples (the plane itself without a display size)
    const bool windowed = A.dW != 0;
    const int ww = windowed ? (plane ? A.dW >> 1 : A.dW) : W, wh = windowed ? (plane ? A.dH >> 1 : A.dH) : H;
    const int t = (int)threadIdx.x;
    uint2 va[2][4], vb[2][4];
    int at[2];
    bool own[2];
    HL_Q_UNROLL
    for (int j = 0; j < 2; ++j) {
        const int i = t + 256 * j;
        at[j] = -1;
        own[j] = false;
        HL_Q_UNROLL
        for (int r = 0; r < 4; ++r) va[j][r] = vb[j][r] = make_uint2(0u, 0u);
        if (i < kQStrips) {
            ptrdiff_t off;
            at[j] = q_strip(i, bx0, by0, W, H, &off, &own[j]);
            if (off >= 0) {
                HL_Q_UNROLL
                for (int r = 0; r < 4; ++r) {
                    va[j][r] = *reinterpret_cast<const uint2*>(src + off + (ptrdiff_t)r * W);
                    vb[j][r] = *reinterpret_cast<const uint2*>(rec + off + (ptrdiff_t)r * W);
                }
                if (windowed) {  // what lies outside the window is zero in both pictures: every sum is the window's
                    int x, y;
                    q_strip_xy(i, bx0, by0, &x, &y);
                    HL_Q_UNROLL
                    for (int r = 0; r < 4; ++r) {
                        uint32_t lo, hi;
                        q_mask(x, y + r, ww, wh, &lo, &hi);
                        va[j][r].x &= lo;
                        va[j][r].y &= hi;
                        vb[j][r].x &= lo;
                        vb[j][r].y &= hi;
                    }
                }
            }
        }
    }
    uint32_t sse = 0;  // (a tile's is below 2^30)
    HL_Q_UNROLL
    for (int j = 0; j < 2; ++j)
        if (at[j] >= 0) {
            const uint32_t a0[4] = {va[j][0].x, va[j][1].x, va[j][2].x, va[j][3].x}, b0[4] = {vb[j][0].x, vb[j][1].x, vb[j][2].x, vb[j][3].x};
            const uint32_t a1[4] = {va[j][0].y, va[j][1].y, va[j][2].y, va[j][3].y}, b1[4] = {vb[j][0].y, vb[j][1].y, vb[j][2].y, vb[j][3].y};
            uint32_t p[3], q[3];
            q_block(a0, b0, p);
            q_block(a1, b1, q);
            HL_Q_UNROLL
            for (int k = 0; k < 3; ++k) *reinterpret_cast<uint2*>(&s_b[k][at[j]]) = make_uint2(p[k], q[k]);  // (at is even)
            if (own[j]) sse += q_sse(p[1], p[2]) + q_sse(q[1], q[2]);
        }
    __syncthreads();
    long long ssim = 0;
    HL_Q_UNROLL
    for (int j = 0; j < 2; ++j) {
        const int w = t + 256 * j, wx = w & (kQTileBX - 1), wy = w / kQTileBX;
        if (bx0 + wx <= ww / 4 - 2 && by0 + wy <= wh / 4 - 2) ssim += q_window_at(s_b[0], s_b[1], s_b[2], wx, wy);
    }
    if (plane == 0 && t < 32) {
        const int mbw = W >> 4, mbx = (bx0 >> 2) + (t & 15), mby = (by0 >> 2) + (t >> 4);
        if (mbx < mbw && mby < (H >> 4)) A.mb[(size_t)pic * (size_t)(mbw * (H >> 4)) + (size_t)mby * mbw + mbx] = q_mb_sse(s_b[1], s_b[2], t & 15, t >> 4);
    }
    unsigned long long e = sse, q = (unsigned long long)ssim;
    HL_Q_UNROLL
    for (int d = 32; d; d >>= 1) {
        e += __shfl_xor(e, d);
        q += __shfl_xor(q, d);
    }
    if ((t & 63) == 0) {
        s_part[t >> 6][0] = e;
        s_part[t >> 6][1] = q;
    }
    __syncthreads();
    if (t == 0) {
        unsigned long long* o = A.sums + 6 * (size_t)pic + 2 * plane;
        atomicAdd(o, s_part[0][0] + s_part[1][0] + s_part[2][0] + s_part[3][0]);
        atomicAdd(o + 1, s_part[0][1] + s_part[1][1] + s_part[2][1] + s_part[3][1]);
    }
}

// `pictures` pictures on `stream`; A.sums and A.mb are those of the first
inline hipError_t launch_quality(const QualityArgs& A, int pictures, hipStream_t stream)
{
    if (pictures < 1 || pictures > 65535 / 3 || A.W <= 0 || A.H <= 0 || (A.W & 15) || (A.H & 15) || (A.H + 31) / 32 > 65535 || !A.sums || !A.mb)
        return hipErrorInvalidValue;
    if ((A.dW || A.dH) && (((A.dW | A.dH) & 1) || A.dW <= 0 || A.dW > A.W || A.dH <= 0 || A.dH > A.H)) return hipErrorInvalidValue;
    for (int c = 0; c < 6 && !A.tab; ++c)
        if (!A.one[c]) return hipErrorInvalidValue;
    const dim3 grid((A.W + 4 * kQTileBX - 1) / (4 * kQTileBX), (A.H + 4 * kQTileBY - 1) / (4 * kQTileBY), 3 * pictures);
    k_quality<<<grid, 256, 0, stream>>>(A);
    return hipGetLastError();
}
#endif

}  // namespace hl
