// hl_pyramid.h -- the input planes of the lower spatial layers, derived from
// the top layer's frame (hl_amd_encode_au / hl_amd_encode_aus_batch).  No
// reference interface: the reference's caller scales every layer itself
// (test_encoder.c:100-111 reads one file per layer).
//
// The filter is the one every SVC workload of this project is made with
// (hartallo_amd.synth._down2): level k+1 = the 2x2 box average of level k,
// (a + b + c + d + 2) >> 2, every plane on its own, rounded at every level.
// It is not the 2^K x 2^K average: the rows 1 1 1 1 / 0 0 0 0 / 1 1 1 0 /
// 0 0 0 0 give 1 staged (1 1 / 1 0 after level 1, then (3 + 2) >> 2 = 1) and
// (7 + 8) >> 4 = 0 direct.
//
// One lane owns a span of 8 columns x 2^K rows of a top plane (K = layers - 1
// levels, 1..3) and reduces it wholly in registers: 2^K loads of 8 bytes, then
// per level 1 / 2 / 3 stores of 4 / 2 / 1 bytes per row.  Consecutive lanes
// own consecutive spans of a row, so a wave's loads of one sample row are one
// contiguous 512-byte run and its stores of a level's row are contiguous too.
// Every layer is a multiple of 16 in both dimensions (hl_amd_add_layer), so
// every top plane -- luma (16 << K) * m, chroma (8 << K) * m -- tiles exactly
// into spans: there are no partial spans, only partial waves.  The planes are
// dense (stride = width).  Host and device run the same pyr_span (the CPU
// suite builds it into tests/emu/libhl_pyr_emu.so).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define HL_PYR_HD __host__ __device__ __forceinline__
#else
#define HL_PYR_HD inline
#endif

namespace hl {

// Two rows of up to 8 samples (little-endian bytes of a word) -> their up to
// 4 box averages, packed.  Byte pairs are summed in 16-bit fields (at most
// 4 * 255 + 2 = 1022: no carry between fields); absent samples are zero and
// give zero.
HL_PYR_HD uint32_t pyr_down(uint64_t r0, uint64_t r1)
{
    const uint64_t m = 0x00FF00FF00FF00FFull;
    const uint64_t s = (r0 & m) + ((r0 >> 8) & m) + (r1 & m) + ((r1 >> 8) & m) + 0x0002000200020002ull;
    const uint64_t q = (s >> 2) & m;  // samples in bytes 0, 2, 4, 6
    const uint32_t lo = (uint32_t)q, hi = (uint32_t)(q >> 32);
    return ((lo | (lo >> 8)) & 0xFFFFu) | (((hi | (hi >> 8)) & 0xFFFFu) << 16);
}

// 8 samples of a row.  On the device the address is 8-byte aligned (the
// planes are, and widths are multiples of 8): one 8-byte load.
HL_PYR_HD uint64_t pyr_load8(const uint8_t* p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return *reinterpret_cast<const uint64_t*>(p);
#else
    uint64_t v;
    memcpy(&v, p, 8);
    return v;
#endif
}

// Span (sx, sy) of a top plane of width W: columns [8 sx, 8 sx + 8), rows
// [sy << K, (sy + 1) << K).  dst[j] = the plane of level j + 1, width
// W >> (j + 1).  The caller keeps 8 sx < W and (sy + 1) << K <= the height.
template <int K>
HL_PYR_HD void pyr_span(const uint8_t* src, int W, int sx, int sy, uint8_t* const* dst)
{
    static_assert(K >= 1 && K <= 3, "1..3 levels (4 layers at most)");
    constexpr int R = 1 << K;
    const uint8_t* p = src + (size_t)sy * R * W + 8 * sx;
    uint64_t r[R];
    for (int i = 0; i < R; ++i) r[i] = pyr_load8(p + (size_t)i * W);
    uint32_t a[R / 2];
    uint8_t* d1 = dst[0] + (size_t)sy * (R / 2) * (W >> 1) + 4 * sx;
    for (int i = 0; i < R / 2; ++i) {
        a[i] = pyr_down(r[2 * i], r[2 * i + 1]);
        memcpy(d1 + (size_t)i * (W >> 1), &a[i], 4);
    }
    if constexpr (K >= 2) {
        uint32_t b[R / 4];
        uint8_t* d2 = dst[1] + (size_t)sy * (R / 4) * (W >> 2) + 2 * sx;
        for (int i = 0; i < R / 4; ++i) {
            b[i] = pyr_down(a[2 * i], a[2 * i + 1]);
            const uint16_t v = (uint16_t)b[i];
            memcpy(d2 + (size_t)i * (W >> 2), &v, 2);
        }
        if constexpr (K >= 3) dst[2][(size_t)sy * (W >> 3) + sx] = (uint8_t)pyr_down(b[0], b[1]);
    }
}

// Every span of one plane (the host's loop; the kernel's lanes take one each)
template <int K>
inline void pyr_plane(const uint8_t* src, int W, int H, uint8_t* const* dst)
{
    for (int sy = 0; sy < (H >> K); ++sy)
        for (int sx = 0; sx < (W >> 3); ++sx) pyr_span<K>(src, W, sx, sy, dst);
}

#if defined(__HIPCC__)
// One launch for the three planes (grid y) of every frame (grid z).
struct PyrArgs {
    const uint8_t* src[3];      // the top planes of the one frame, when tab is null
    const uint8_t* const* tab;  // else [3 * frames] top planes, frame by frame (device memory)
    uint8_t* dst[3][3];         // [level - 1][plane] of frame 0
    size_t fstride[3];          // [level - 1] bytes from a frame's planes to the next frame's
    int32_t W, H;               // top luma size
};

template <int K>
__global__ __launch_bounds__(256) void k_pyramid(PyrArgs A)
{
    const int c = blockIdx.y, f = blockIdx.z;
    const int W = c ? A.W >> 1 : A.W, H = c ? A.H >> 1 : A.H;
    const int sw = W >> 3, n = sw * (H >> K);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;  // tail lanes, and the chroma planes' share of a grid sized for luma
    const uint8_t* src = A.tab ? A.tab[3 * f + c] : A.src[c];
    uint8_t* dst[3];
    for (int j = 0; j < K; ++j) dst[j] = A.dst[j][c] + A.fstride[j] * f;
    pyr_span<K>(src, W, i % sw, i / sw, dst);
}

// levels 1..K of `frames` frames on `stream`; W, H: the top luma size
inline hipError_t launch_pyramid(const PyrArgs& A, int K, int frames, hipStream_t stream)
{
    if (K < 1 || K > 3 || frames < 1 || frames > 65535 || A.W <= 0 || A.H <= 0 || (A.W & ((16 << K) - 1)) || (A.H & ((16 << K) - 1)))
        return hipErrorInvalidValue;
    const dim3 grid(((A.W >> 3) * (A.H >> K) + 255) / 256, 3, frames);
    if (K == 1) k_pyramid<1><<<grid, 256, 0, stream>>>(A);
    else if (K == 2) k_pyramid<2><<<grid, 256, 0, stream>>>(A);
    else k_pyramid<3><<<grid, 256, 0, stream>>>(A);
    return hipGetLastError();
}
#endif

}  // namespace hl
