// hl_unit_cand.hip -- TEST INFRASTRUCTURE.  GPU unit kernel for the candidate
// slot of the partition search (hl_mbcore.h put_cand, CandSlot): the device
// path forms a candidate's two plane offsets from the per-phase table the MB
// start leaves in LDS (Shared::qoff) and its memo key part from the clamped
// displacement; tests/test_gpu_unit_cand.py compares every field with the
// host formula restated there, on a virtual picture (no plane is read).
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../hartallo_amd/csrc/hl_coop.h"
#include "../../hartallo_amd/csrc/hl_quad.h"
#include "../../hartallo_amd/csrc/hl_filters.h"
#include "../../hartallo_amd/csrc/hl_mbcore.h"

using namespace hl;

// in: n cases of {xL, yL, xo, yo, mvx, mvy, point}; out: n slots of {off1, off2, mvx, mvy, pad}
__global__ __launch_bounds__(64) void k_unit_cand(int W, int H, int pstride, int plsz, const int* in, int n, int* out)
{
    __shared__ Shared S;
    __shared__ FrameArgs F;
    const int tid = threadIdx.x;
    if (tid == 0) {
        F.W = W;
        F.H = H;
        F.pstride = pstride;
        F.plsz = plsz;
    }
    __syncthreads();
    if (tid < 16) {  // the phase table as mb_begin fills it
        const uint32_t q = qpel_entry(tid);
        const int o1 = (int)(q & 3) * F.plsz + (int)((q >> 3) & 1) * F.pstride + (int)((q >> 2) & 1);
        S.qoff[tid] = make_int2(o1, (q & 16) ? (int)((q >> 5) & 3) * F.plsz + (int)((q >> 8) & 1) * F.pstride + (int)((q >> 7) & 1) : o1);
    }
    __syncthreads();
    Ctx c{F, S, tid, 64, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int base = 0; base < n; base += kMaxCand) {  // a step's worth of slots at a time, lane = slot
        const int k = base + tid;
        if (tid < kMaxCand && k < n) {
            const int* e = in + 7 * k;
            c.xL = e[0];
            c.yL = e[1];
            put_cand(c, e[2], e[3], 0, 0, tid, e[4], e[5], e[6], true);
        }
        __syncthreads();
        if (tid < kMaxCand && k < n) {
            const CandSlot cs = S.wc[0][tid];
            int* o = out + 5 * k;
            o[0] = cs.off1;
            o[1] = cs.off2;
            o[2] = cs.mvx;
            o[3] = cs.mvy;
            o[4] = cs.pad;
        }
        __syncthreads();
    }
}

extern "C" int unit_cand(int W, int H, int pstride, int plsz, const int* h_in, int n, int* h_out)
{
    int *d_in = nullptr, *d_out = nullptr;
    if (hipMalloc(&d_in, (size_t)n * 7 * sizeof(int)) != hipSuccess) return 1;
    if (hipMalloc(&d_out, (size_t)n * 5 * sizeof(int)) != hipSuccess) return 2;
    int rc = 0;
    if (hipMemcpy(d_in, h_in, (size_t)n * 7 * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) rc = 3;
    if (!rc) {
        k_unit_cand<<<1, 64>>>(W, H, pstride, plsz, d_in, n, d_out);
        if (hipDeviceSynchronize() != hipSuccess) rc = 4;
    }
    if (!rc && hipMemcpy(h_out, d_out, (size_t)n * 5 * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) rc = 5;
    hipFree(d_in);
    hipFree(d_out);
    return rc;
}
