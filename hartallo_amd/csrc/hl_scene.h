// hl_scene.h -- scene-cut analysis of the input frames (hl_amd_set_scenecut).
// No reference interface: the reference takes its picture types from gop_size
// and hl_frame_t.encoding alone; this analysis only chooses the encoding the
// caller would have passed.
//
// Frame k is compared with the previous input frame of the stream, luma only,
// on the picture's 16x16 macroblocks:
//   intra[mb] = sum |p - m| over the 256 samples, m = (sum p + 128) >> 8
//   inter[mb] = min over (dx, dy) in [-R, R]^2 of SAD16x16(cur MB, prev at
//               +(dx, dy)); only displacements whose block lies wholly inside
//               the picture take part ((0, 0) always does); R = 0..16
//   P = sum min(inter, intra), I = sum intra (64 bits, per frame)
// Everything is integer sums and minima: no result depends on order or ties.
//
// k_scene: one workgroup of 256 lanes (4 waves) takes a strip of kScStrip = 4
// macroblocks of one macroblock row (grid x), of one row (grid y), of one
// frame (grid z).  It stages, as 4-byte words in LDS,
//   s_cur  the strip's current samples, [MB][16 rows][4 words] (1 KiB), and
//   s_win  the previous frame's window of the strip: 16 + 2R rows of
//          kScWinW = 24 words (16 * 4 + 2 * 16 columns, from 16 columns left
//          of the strip whatever R is, so every row starts word-aligned),
//          row stride kScStride = 25 words (4.7 KiB at R = 16).
// Every lane issues its up to six global loads (five window words, one
// current word) before the first LDS store.  Words outside the picture are
// not loaded (zero is stored); the displacements that would read them are
// masked (sc_valid).
//
// Wave w owns macroblock w of the strip; its lanes take the (2R + 1)^2
// displacements, dx fastest, 64 at a time.  The current block is the same for
// every lane: its 64 words are read once from LDS at wave-uniform addresses
// (broadcast) and held in registers.  Per row of the block a lane reads the 5
// window words its 16 misaligned samples span, forms the 4 words with
// __builtin_amdgcn_alignbyte and accumulates with __builtin_amdgcn_sad_u8.
// LDS banks (ds_read_b32: 32 banks, per 32-lane half): lanes with consecutive
// dx of one dy read overlapping words -- four consecutive lanes the same word
// (a broadcast), the next four the next word -- and the next dy's lanes start
// 25 words on, an odd stride: at R = 8 a half's 32 lanes cover two rows of 5
// or 6 consecutive words each, 25 banks apart; at R = 16 one row of 9.  Both
// are conflict-free.  The minimum over a macroblock's displacements is a DPP
// row minimum and four readlanes; intra is sixteen row SADs against the mean
// byte replicated in a word.  Lane 0 of a wave writes the macroblock's two
// values; the workgroup adds its partial sums into the frame's two 64-bit
// sums with integer atomicAdd (exact in any order).
//
// Host and device run the same per-macroblock code (the CPU suite builds it
// into tests/emu/libhl_scene_emu.so).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define HL_SC_HD __host__ __device__ __forceinline__
#define HL_SC_UNROLL _Pragma("unroll")
#else
#define HL_SC_HD inline
#define HL_SC_UNROLL
#endif

namespace hl {

constexpr int kScStrip = 4;                                // macroblocks of a workgroup's strip (one wave each)
constexpr int kScMaxR = 16;                                // largest search range
constexpr int kScWinW = (16 * kScStrip + 2 * kScMaxR) / 4;  // window words per row
constexpr int kScStride = kScWinW + 1;                     // ... and the row stride (odd: see the bank note above)
constexpr int kScWinRows = 16 + 2 * kScMaxR;

// sum of the four |a.byte - b.byte|, plus acc
HL_SC_HD uint32_t sc_sad4(uint32_t a, uint32_t b, uint32_t acc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sad_u8(a, b, acc);
#else
    for (int i = 0; i < 4; ++i) {
        const int d = (int)((a >> (8 * i)) & 255) - (int)((b >> (8 * i)) & 255);
        acc += (uint32_t)(d < 0 ? -d : d);
    }
    return acc;
#endif
}

// the 4 bytes from byte sh (0..3) of the little-endian pair lo, hi
HL_SC_HD uint32_t sc_align(uint32_t hi, uint32_t lo, unsigned sh)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbyte(hi, lo, sh);
#else
    return sh ? (lo >> (8 * sh)) | (hi << (32 - 8 * sh)) : lo;
#endif
}

// does the block of macroblock (mbx, mby) displaced by (dx, dy) lie wholly inside the W x H picture?
HL_SC_HD bool sc_valid(int mbx, int mby, int dx, int dy, int W, int H)
{
    const int x = 16 * mbx + dx, y = 16 * mby + dy;
    return x >= 0 && x + 16 <= W && y >= 0 && y + 16 <= H;
}

// Window word i (< kScWinW * (16 + 2R)) of the strip that starts at macroblock
// (mbx0, mby): its index in s_win, and in *off its byte offset in the W x H
// plane, or -1 when it lies outside the picture (words are wholly in or out:
// W is a multiple of 16).
HL_SC_HD int sc_win_word(int i, int mbx0, int mby, int R, int W, int H, ptrdiff_t* off)
{
    const int r = i / kScWinW, c = i - r * kScWinW;
    const int gy = 16 * mby - R + r, gx = 16 * mbx0 - 16 + 4 * c;
    *off = gy >= 0 && gy < H && gx >= 0 && gx < W ? (ptrdiff_t)gy * W + gx : (ptrdiff_t)-1;
    return r * kScStride + c;
}

// Current word i (< 64 * kScStrip; word i & 15 of row i >> 4 of the strip):
// its index in s_cur ([MB][row][word]) and its byte offset in the plane or -1
// (a macroblock right of the picture).
HL_SC_HD int sc_cur_word(int i, int mbx0, int mby, int W, ptrdiff_t* off)
{
    const int row = i >> 4, cw = i & 15;
    const int gx = 16 * mbx0 + 4 * cw;
    *off = gx < W ? (ptrdiff_t)(16 * mby + row) * W + gx : (ptrdiff_t)-1;
    return (cw >> 2) * 64 + row * 4 + (cw & 3);
}

// SAD of the strip's macroblock mb (its 64 words cur) against the window at
// displacement (dx, dy), |dx|, |dy| <= R.  The caller keeps sc_valid.
HL_SC_HD uint32_t sc_sad16(const uint32_t* cur, const uint32_t* win, int mb, int dx, int dy, int R)
{
    const int bx = 16 + 16 * mb + dx;  // the block's first column in the window, 0..80
    const unsigned sh = (unsigned)bx & 3u;
    const uint32_t* p = win + (R + dy) * kScStride + (bx >> 2);
    uint32_t acc = 0;
    HL_SC_UNROLL
    for (int r = 0; r < 16; ++r, p += kScStride) {
        const uint32_t a0 = p[0], a1 = p[1], a2 = p[2], a3 = p[3], a4 = p[4];  // (a4: the pad word of the row when sh = 0, unused then)
        acc = sc_sad4(cur[4 * r + 0], sc_align(a1, a0, sh), acc);
        acc = sc_sad4(cur[4 * r + 1], sc_align(a2, a1, sh), acc);
        acc = sc_sad4(cur[4 * r + 2], sc_align(a3, a2, sh), acc);
        acc = sc_sad4(cur[4 * r + 3], sc_align(a4, a3, sh), acc);
    }
    return acc;
}

// sum |p - m| of a macroblock's 64 words, m = (sum p + 128) >> 8
HL_SC_HD uint32_t sc_intra(const uint32_t* cur)
{
    uint32_t s = 0;
    HL_SC_UNROLL
    for (int i = 0; i < 64; ++i) s = sc_sad4(cur[i], 0u, s);
    const uint32_t m = ((s + 128u) >> 8) * 0x01010101u;
    uint32_t acc = 0;
    HL_SC_UNROLL
    for (int r = 0; r < 16; ++r) {
        uint32_t row = 0;
        HL_SC_UNROLL
        for (int c = 0; c < 4; ++c) row = sc_sad4(cur[4 * r + c], m, row);
        acc += row;
    }
    return acc;
}

// One frame pair on the host, strip by strip as the kernel's workgroups take
// it (the same staging indices, the same per-macroblock code): mb[2 a] =
// inter, mb[2 a + 1] = intra of macroblock a; sums[0] += P, sums[1] += I.
inline void scene_frame_host(const uint8_t* cur, const uint8_t* prev, int W, int H, int R, uint32_t* mb, uint64_t* sums)
{
    const int mbw = W >> 4, mbh = H >> 4, side = 2 * R + 1;
    uint32_t s_cur[64 * kScStrip], s_win[kScWinRows * kScStride];
    for (int mby = 0; mby < mbh; ++mby)
        for (int mbx0 = 0; mbx0 < mbw; mbx0 += kScStrip) {
            memset(s_win, 0xA5, sizeof(s_win));  // (what the kernel leaves unwritten: the pad words)
            for (int i = 0; i < kScWinW * (16 + 2 * R); ++i) {
                ptrdiff_t off;
                const int at = sc_win_word(i, mbx0, mby, R, W, H, &off);
                uint32_t v = 0;
                if (off >= 0) memcpy(&v, prev + off, 4);
                s_win[at] = v;
            }
            for (int i = 0; i < 64 * kScStrip; ++i) {
                ptrdiff_t off;
                const int at = sc_cur_word(i, mbx0, mby, W, &off);
                uint32_t v = 0;
                if (off >= 0) memcpy(&v, cur + off, 4);
                s_cur[at] = v;
            }
            for (int w = 0; w < kScStrip && mbx0 + w < mbw; ++w) {
                const uint32_t* c = s_cur + 64 * w;
                uint32_t best = 0xFFFFFFFFu;
                for (int d = 0; d < side * side; ++d) {
                    const int dy = d / side - R, dx = d % side - R;
                    if (!sc_valid(mbx0 + w, mby, dx, dy, W, H)) continue;
                    const uint32_t s = sc_sad16(c, s_win, w, dx, dy, R);
                    if (s < best) best = s;
                }
                const uint32_t intra = sc_intra(c);
                const size_t a = (size_t)mby * mbw + mbx0 + w;
                mb[2 * a] = best;
                mb[2 * a + 1] = intra;
                sums[0] += best < intra ? best : intra;
                sums[1] += intra;
            }
        }
}

#if defined(__HIPCC__)
// One launch for every frame of a call (grid z).
struct SceneArgs {
    const uint8_t* const* tab;  // [f0 + frames] luma planes of the call's frames (device memory), 4-byte aligned, dense
    const uint8_t* prev0;       // the frame before the call's first (the carried-over luma), or null: frame 0 is not analysed
    uint32_t* mb;               // [frame][MB][2] inter, intra
    unsigned long long* sums;   // [frame][2] P, I (zeroed before the launch)
    int32_t W, H, R, f0;        // f0: the call's frame of grid z = 0
};

template <int CTRL>
__device__ __forceinline__ uint32_t sc_dpp(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}

// minimum over the wave (every lane active); the result is uniform
__device__ __forceinline__ uint32_t sc_wave_min(uint32_t x)
{
    x = min(x, sc_dpp<0x128>(x));  // row_ror 8, 4, 2, 1: the minimum of every 16-lane row
    x = min(x, sc_dpp<0x124>(x));
    x = min(x, sc_dpp<0x122>(x));
    x = min(x, sc_dpp<0x121>(x));
    const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)x, 0), b = (uint32_t)__builtin_amdgcn_readlane((int)x, 16);
    const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)x, 32), d = (uint32_t)__builtin_amdgcn_readlane((int)x, 48);
    return min(min(a, b), min(c, d));
}

__global__ __launch_bounds__(256) void k_scene(SceneArgs A)
{
    __shared__ uint32_t s_cur[64 * kScStrip];
    __shared__ uint32_t s_win[kScWinRows * kScStride];
    __shared__ uint32_t s_part[kScStrip][2];
    const int f = A.f0 + (int)blockIdx.z;
    const uint8_t* prev = f ? A.tab[f - 1] : A.prev0;
    if (!prev) return;  // (the whole workgroup: a frame without a previous input frame)
    const uint8_t* cur = A.tab[f];
    const int W = A.W, H = A.H, R = A.R, mbw = W >> 4;
    const int mbx0 = (int)blockIdx.x * kScStrip, mby = (int)blockIdx.y;
    const int t = (int)threadIdx.x;
    constexpr int kLoads = (kScWinW * kScWinRows + 255) / 256;
    const int nwin = kScWinW * (16 + 2 * R);
    uint32_t v[kLoads], at[kLoads];
    for (int j = 0; j < kLoads; ++j) {
        const int i = t + 256 * j;
        v[j] = 0;
        at[j] = 0xFFFFFFFFu;
        if (i < nwin) {
            ptrdiff_t off;
            at[j] = (uint32_t)sc_win_word(i, mbx0, mby, R, W, H, &off);
            if (off >= 0) v[j] = *reinterpret_cast<const uint32_t*>(prev + off);
        }
    }
    uint32_t cv = 0;
    ptrdiff_t coff;
    const int cat = sc_cur_word(t, mbx0, mby, W, &coff);
    if (coff >= 0) cv = *reinterpret_cast<const uint32_t*>(cur + coff);
    for (int j = 0; j < kLoads; ++j)
        if (at[j] != 0xFFFFFFFFu) s_win[at[j]] = v[j];
    s_cur[cat] = cv;
    __syncthreads();

    const int wave = t >> 6, lane = t & 63, mbx = mbx0 + wave;
    uint32_t both = 0, intra = 0;
    if (mbx < mbw) {  // (wave-uniform)
        uint32_t c[64];
        HL_SC_UNROLL
        for (int i = 0; i < 64; ++i) c[i] = s_cur[64 * wave + i];
        const int side = 2 * R + 1, nd = side * side;
        uint32_t best = 0xFFFFFFFFu;
        for (int d0 = 0; d0 < nd; d0 += 64) {
            const int d = d0 + lane, q = d / side;
            const int dy = q - R, dx = d - q * side - R;
            if (d < nd && sc_valid(mbx, mby, dx, dy, W, H)) best = min(best, sc_sad16(c, s_win, wave, dx, dy, R));
        }
        best = sc_wave_min(best);
        intra = sc_intra(c);
        both = min(best, intra);
        if (lane == 0) {
            uint32_t* o = A.mb + 2 * ((size_t)blockIdx.z * (size_t)(mbw * (H >> 4)) + (size_t)mby * mbw + mbx);
            o[0] = best;
            o[1] = intra;
        }
    }
    if (lane == 0) {
        s_part[wave][0] = both;
        s_part[wave][1] = intra;
    }
    __syncthreads();
    if (t == 0) {
        unsigned long long p = 0, i = 0;
        for (int w = 0; w < kScStrip; ++w) {
            p += s_part[w][0];
            i += s_part[w][1];
        }
        atomicAdd(A.sums + 2 * (size_t)blockIdx.z, p);
        atomicAdd(A.sums + 2 * (size_t)blockIdx.z + 1, i);
    }
}

// `frames` frames from the call's frame A.f0 on `stream`; A.mb and A.sums are
// those of frame A.f0
inline hipError_t launch_scene(const SceneArgs& A, int frames, hipStream_t stream)
{
    if (frames < 1 || frames > 65535 || A.f0 < 0 || A.W <= 0 || A.H <= 0 || (A.W & 15) || (A.H & 15) || (A.H >> 4) > 65535 || A.R < 0 ||
        A.R > kScMaxR || !A.tab || !A.mb || !A.sums)
        return hipErrorInvalidValue;
    const dim3 grid(((A.W >> 4) + kScStrip - 1) / kScStrip, A.H >> 4, frames);
    k_scene<<<grid, 256, 0, stream>>>(A);
    return hipGetLastError();
}
#endif

}  // namespace hl
