// hl_unit_rec.hip -- TEST INFRASTRUCTURE.  GPU unit kernel for the candidate
// record of an evaluation pass and the selection that reads it (hl_mbcore.h
// CandRec, rec_store, sel_load, sel_minima, sel_take): one wave writes a
// pass's records into both parities through the writers' store and its slots
// through put_cand, in the layout the search generates them in (lane 16 j + i
// = point i of step j, candidates numbered in lane order), reads them back
// through the selection's loader, runs the one-row minimum and takes every
// step's winner; tests/test_gpu_cand_record.py compares all of it with the
// inputs restated there.
#include <hip/hip_runtime.h>
#include <string.h>

#include "../../hartallo_amd/csrc/hl_coop.h"
#include "../../hartallo_amd/csrc/hl_quad.h"
#include "../../hartallo_amd/csrc/hl_filters.h"
#include "../../hartallo_amd/csrc/hl_mbcore.h"

using namespace hl;

constexpr int kCandIn = 10;                               // cost low, cost high, bits, dist, cbp, single, last, mvx, mvy, -
constexpr int kCaseIn = 2 + 2 * kMaxCand * kCandIn;       // gen low, gen high, then both parities' candidates
constexpr int kLaneOut = 6;                               // cost low, cost high, bd, meta, mv, ci
constexpr int kTakeOut = 8;                               // cost low, cost high, single, dist, cbp, mv x, mv y, point
constexpr int kParOut = 64 * kLaneOut + kMaxSeg * 3 + kMaxSeg * kTakeOut;  // lanes, (minimum low, high, lane) per step, takes
constexpr int kCaseOut = 2 * kParOut;

__global__ __launch_bounds__(64) void k_unit_rec(const int* in, int n, int* out)
{
#if defined(__HIP_DEVICE_COMPILE__)  // (the selection's functions exist in the device pass only)
    __shared__ Shared S;
    __shared__ FrameArgs F;
    const int tid = threadIdx.x;
    if (tid == 0) {  // a virtual picture: put_cand forms offsets, no plane is read
        F.W = 4096;
        F.H = 2304;
        F.pstride = 4224;
        F.plsz = 4224 * 2384;
    }
    __syncthreads();
    if (tid < 16) {  // the phase table as mb_begin fills it
        const uint32_t q = qpel_entry(tid);
        const int o1 = (int)(q & 3) * F.plsz + (int)((q >> 3) & 1) * F.pstride + (int)((q >> 2) & 1);
        S.qoff[tid] = make_int2(o1, (q & 16) ? (int)((q >> 5) & 3) * F.plsz + (int)((q >> 8) & 1) * F.pstride + (int)((q >> 7) & 1) : o1);
    }
    __syncthreads();
    Ctx c{F, S, tid, 64, 0, 0, 0, 2048, 1152, 0, 0, 0};
    for (int k = 0; k < n; ++k) {
        const int* e = in + (size_t)k * kCaseIn;
        const unsigned long long gen = (unsigned long long)(unsigned)e[0] | (unsigned long long)(unsigned)e[1] << 32;  // uniform
        const bool en = (gen >> tid) & 1;
        const int ci = en ? lanes_below(gen) : 0;  // < kMaxCand: the host checks the mask
        if (en) {
#pragma unroll
            for (int par = 0; par < 2; ++par) {  // both parities, different values
                const int* v = e + 2 + (par * kMaxCand + ci) * kCandIn;
                const double cost = __builtin_bit_cast(double, (unsigned long long)(unsigned)v[0] | (unsigned long long)(unsigned)v[1] << 32);
                rec_store(S.cd[par][ci], cost, rec_bd(v[2], v[3]), rec_meta(v[4], v[5], v[6]));
            }
        }
        __syncthreads();
#pragma unroll
        for (int par = 0; par < 2; ++par) {
            int* o = out + (size_t)k * kCaseOut + par * kParOut;
            if (en) {  // the pass's slots hold the parity's MVs (the search writes them per pass)
                const int* v = e + 2 + (par * kMaxCand + ci) * kCandIn;
                put_cand(c, 0, 0, 16, 16, ci, v[7], v[8], tid & 15, true);
            }
            __syncthreads();
            const SelRec pv = sel_load(S, par, 0, gen, tid);
            const unsigned long long cb = __builtin_bit_cast(unsigned long long, pv.cost);
            o[tid * kLaneOut + 0] = (int)(unsigned)cb;
            o[tid * kLaneOut + 1] = (int)(cb >> 32);
            o[tid * kLaneOut + 2] = (int)pv.bd;
            o[tid * kLaneOut + 3] = (int)pv.meta;
            o[tid * kLaneOut + 4] = (int)pv.mv;
            o[tid * kLaneOut + 5] = pv.ci;
            double sm[kMaxSeg];
            int sb[kMaxSeg];
            sel_minima(pv, sm, sb);
            int* om = o + 64 * kLaneOut;
            int* ot = om + kMaxSeg * 3;
#pragma unroll
            for (int j = 0; j < kMaxSeg; ++j) {
                const unsigned long long mb = __builtin_bit_cast(unsigned long long, sm[j]);
                Best b;
                b.cost = -1.0;
                b.dist = b.single = b.cbp = b.mv[0] = b.mv[1] = -1;
                int pt = -1;
                if (sb[j] >= 0) pt = sel_take(pv, sb[j], sm[j], b);  // (uniform)
                if (tid == 0) {
                    om[3 * j + 0] = (int)(unsigned)mb;
                    om[3 * j + 1] = (int)(mb >> 32);
                    om[3 * j + 2] = sb[j];
                    const unsigned long long tb = __builtin_bit_cast(unsigned long long, b.cost);
                    int* t = ot + j * kTakeOut;
                    t[0] = (int)(unsigned)tb;
                    t[1] = (int)(tb >> 32);
                    t[2] = b.single;
                    t[3] = b.dist;
                    t[4] = b.cbp;
                    t[5] = b.mv[0];
                    t[6] = b.mv[1];
                    t[7] = pt;
                }
            }
            __syncthreads();
        }
    }
#endif
}

// h_in: n cases of kCaseIn words; h_out: n cases of kCaseOut words.
// Returns 0, or 10 for a mask with more than kMaxCand lanes (nothing runs).
extern "C" int unit_rec(const int* h_in, int n, int* h_out)
{
    for (int k = 0; k < n; ++k)
        if (__builtin_popcount((unsigned)h_in[(size_t)k * kCaseIn]) + __builtin_popcount((unsigned)h_in[(size_t)k * kCaseIn + 1]) > kMaxCand) return 10;
    int *d_in = nullptr, *d_out = nullptr;
    if (hipMalloc(&d_in, (size_t)n * kCaseIn * sizeof(int)) != hipSuccess) return 1;
    if (hipMalloc(&d_out, (size_t)n * kCaseOut * sizeof(int)) != hipSuccess) {
        (void)hipFree(d_in);
        return 2;
    }
    int rc = 0;
    if (hipMemcpy(d_in, h_in, (size_t)n * kCaseIn * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) rc = 3;
    if (!rc) {
        k_unit_rec<<<1, 64>>>(d_in, n, d_out);
        if (hipDeviceSynchronize() != hipSuccess) rc = 4;
    }
    if (!rc && hipMemcpy(h_out, d_out, (size_t)n * kCaseOut * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) rc = 5;
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    return rc;
}

extern "C" int unit_rec_case_in(void) { return kCaseIn; }
extern "C" int unit_rec_case_out(void) { return kCaseOut; }
