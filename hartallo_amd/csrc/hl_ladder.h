// hl_ladder.h -- one source fanned out to several encoders
// (hl_amd_encode_ladder_frame / hl_amd_encode_ladder_frames): k_scale_fan
// between one frame ingest at the source size (hl_ingest.h) and the unchanged
// per-encoder coding paths.  No reference interface: the reference has no
// scaler (hl_scale.h).
//
// A ladder is up to 8 renditions ("rungs") of one source size: rung r scales
// sw x sh to its display size dw_r x dh_r inside its coded size W_r x H_r.  The
// arithmetic is hl_scale.h's, called and not copied (sk_tile, sk_reduce,
// sk_output, sk_div): every rung is the direct area filter of the source,
// never a cascade of another rung.  A rung of the source's own size takes one
// tap of weight 1 per axis and D = 1 -- the identity -- and still gets the
// edge replication beyond its display size.
//
// k_scale_fan: k_scale's workgroup (256 lanes, an output tile of 64 x 16
// samples of one plane), one launch for frames x rungs x planes.  Grid x: the
// tile, up to the largest luma tile count of any rung; y: the plane; z: frame *
// count + r, so that the rungs of one frame are neighbours in the dispatch
// order and re-read the frame from cache (the expectation; DESIGN.md 6.15
// measured no gain from it: the kernel is bound by its byte loads).  A
// workgroup beyond its rung's or plane's tile count leaves at once
// (block-uniform).  The rungs' SkParm and destinations travel in the kernel
// argument and are selected by the uniform r: scalar loads, no scratch.  The
// frames' source planes are a device table (SkFrame, the destinations unused),
// as k_scale's.  Dynamic LDS: the largest sk_lds_bytes(lrows) of the launch's
// rungs (at most 33,024 bytes).  Host and device run the same block selection
// (ld_block) and the same per-lane functions (the CPU suite builds ld_frames
// into tests/emu/libhl_ladder_emu.so).
#pragma once
#include "hl_scale.h"

namespace hl {

constexpr int kLdMaxRungs = 8;

// a rung: its scale, and plane c of frame k of the launch at dst[c] + k * stride
struct LdRung {
    SkParm parm;
    uint8_t* dst[3];
    size_t stride;
};

// One launch (or the host's loop) for every frame and rung.
struct LdArgs {
    SkFrame one;         // the one frame, when tab is null (its dst is not used)
    const SkFrame* tab;  // else the launch's frames (device memory; dst not used)
    int32_t count;       // rungs
    LdRung rung[kLdMaxRungs];
};

// the launch's grid x (the largest luma tile count of its rungs) and dynamic LDS bytes
inline int ld_grid_x(const LdArgs& A)
{
    int m = 0;
    for (int r = 0; r < A.count; ++r) {
        const int t = sk_tiles_x(A.rung[r].parm, 0) * sk_tiles_y(A.rung[r].parm, 0);
        m = t > m ? t : m;
    }
    return m;
}
inline size_t ld_lds_bytes(const LdArgs& A)
{
    int m = 0;
    for (int r = 0; r < A.count; ++r) m = A.rung[r].parm.lrows > m ? A.rung[r].parm.lrows : m;
    return sk_lds_bytes(m);
}

// what launch_ladder takes: 1 to 8 rungs of one source, each as sk_parm derives it
inline bool ld_args_ok(const LdArgs& A)
{
    if (A.count < 1 || A.count > kLdMaxRungs) return false;
    for (int r = 0; r < A.count; ++r) {
        const SkParm& P = A.rung[r].parm;
        SkParm Q;
        if (!sk_parm(P.sw, P.sh, P.sp, P.dw, P.dh, P.W, P.H, &Q) || memcmp(&P, &Q, sizeof(Q)) != 0 || P.lrows > kSkTileH * kSkMaxRatio + 1) return false;
        if (P.sw != A.rung[0].parm.sw || P.sh != A.rung[0].parm.sh || P.sp != A.rung[0].parm.sp) return false;
        for (int c = 0; c < 3; ++c)
            if (!A.rung[r].dst[c]) return false;
    }
    return true;
}

// Workgroup (x, c, z) of a launch: its frame k and rung r, whether it has a
// tile at all, the tile, and the planes it reads and writes.  Uniform.
struct LdBlock {
    int32_t k, r;
    bool on;
    SkTile T;
    const uint8_t* src;
    uint8_t* dst;
};
HL_SK_HD LdBlock ld_block(const LdArgs& A, int x, int c, int z)
{
    LdBlock B;
    B.k = z / A.count;
    B.r = z - B.k * A.count;
    const LdRung& R = A.rung[B.r];
    B.on = x < sk_tiles_x(R.parm, c) * sk_tiles_y(R.parm, c);  // another rung, or luma, has more tiles
    B.src = nullptr;
    B.dst = nullptr;
    B.T = SkTile{};
    if (!B.on) return B;
    const SkFrame F = A.tab ? A.tab[B.k] : A.one;
    B.src = c == 0 ? F.src[0] : c == 1 ? F.src[1] : F.src[2];  // (no indexing by the plane: that would live in scratch)
    B.dst = (c == 0 ? R.dst[0] : c == 1 ? R.dst[1] : R.dst[2]) + (size_t)B.k * R.stride;
    B.T = sk_tile(R.parm, c, x);
    return B;
}

// Every frame, rung, plane and tile of one launch, workgroups and lanes in the
// kernel's order (the host's loop); lds: ld_lds_bytes(A)
inline void ld_frames(const LdArgs& A, int frames, uint32_t* lds)
{
    const int gx = ld_grid_x(A);
    for (int z = 0; z < frames * A.count; ++z)
        for (int c = 0; c < 3; ++c)
            for (int x = 0; x < gx; ++x) {
                const LdBlock B = ld_block(A, x, c, z);
                if (!B.on) continue;
                const SkParm& P = A.rung[B.r].parm;
                for (int lane = 0; lane < kSkLanes; ++lane) sk_reduce(B.src, P, B.T, lds, lane & 63, lane >> 6, 4);
                for (int lane = 0; lane < kSkLanes; ++lane) sk_output(B.dst, P, B.T, lds, lane & 15, lane >> 4);
            }
}

#if defined(__HIPCC__)
// frames that one launch can hold (grid z = frames * count)
inline int ld_max_frames(int count) { return 65535 / count; }

// `frames` frames on `stream`
hipError_t launch_ladder(const LdArgs& A, int frames, hipStream_t stream);

#if defined(HL_LADDER_KERNELS)  // hl_ladder.hip: the one translation unit that holds the kernel
__global__ __launch_bounds__(kSkLanes) void k_scale_fan(LdArgs A)
{
    extern __shared__ __align__(16) uint32_t ld_lds[];
    const LdBlock B = ld_block(A, blockIdx.x, blockIdx.y, blockIdx.z);
    if (!B.on) return;
    const SkParm P = A.rung[B.r].parm;  // (uniform: scalar registers)
    sk_reduce(B.src, P, B.T, ld_lds, threadIdx.x & 63, threadIdx.x >> 6, 4);
    __syncthreads();
    sk_output(B.dst, P, B.T, ld_lds, threadIdx.x & 15, threadIdx.x >> 4);
}

hipError_t launch_ladder(const LdArgs& A, int frames, hipStream_t stream)
{
    if (!ld_args_ok(A) || frames < 1 || frames > ld_max_frames(A.count)) return hipErrorInvalidValue;
    const dim3 grid(ld_grid_x(A), 3, frames * A.count);
    k_scale_fan<<<grid, kSkLanes, ld_lds_bytes(A), stream>>>(A);
    return hipGetLastError();
}
#endif  // HL_LADDER_KERNELS
#endif

}  // namespace hl
