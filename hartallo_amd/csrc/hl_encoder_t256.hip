// hl_encoder_t256.hip -- k_pipeline again, built with 256-lane workgroups
// (HL_MB_THREADS=256), for long runs of pictures.
//
// A macroblock decision is one dependent chain that every wave of the
// workgroup executes alike, and the eight waves of the 512-lane workgroup
// hold the CU's whole register file.  Four waves per macroblock leave room
// for a second workgroup on the CU: each decision takes longer, two of them
// overlap.  That pays only while the run supplies enough ready macroblocks
// for twice the workgroups, so the launcher (hl_encoder.hip,
// pipeline_build_choice) picks this build per run.  This translation unit
// compiles hl_encoder.hip's kernel section inside a namespace of its own (its
// headers' types and inline functions become hl_t256::hl::..., no clash with
// the product's); the argument structs are the same layout in both builds.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <future>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#define HL_MB_THREADS 256
#define HL_KERNELS_ONLY 1
namespace hl_t256 {
#include "hl_encoder.hip"
}

// Launches the 256-lane k_pipeline on `stream` with the product's PipeArgs
// (psz = its size, checked against this build's).
extern "C" __attribute__((visibility("hidden"))) hipError_t hl_t256_launch_pipeline(const void* args, size_t psz, int mbw, int mbh,
                                                                                      int workgroups, hipStream_t stream)
{
    if (psz != sizeof(hl_t256::hl::PipeArgs)) return hipErrorInvalidValue;
    hl_t256::hl::PipeArgs P;
    memcpy(&P, args, psz);
    hl_t256::k_pipeline<<<workgroups, hl_t256::hl::kMbThreads, 0, stream>>>(P, mbw, mbh);
    return hipGetLastError();
}

// Resident workgroups per CU of this build's k_pipeline.  For 256-thread
// blocks the occupancy query can report one workgroup more than the CU holds;
// LDS (two Shared images) and the 256 VGPRs per wave both cap it at 2.  The
// run has no grid barrier and claim_next needs no co-residency, so a grid
// smaller than the residency is only slower.
extern "C" __attribute__((visibility("hidden"))) hipError_t hl_t256_pipeline_occupancy(int* per_cu)
{
    int n = 0;
    const hipError_t r = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, hl_t256::k_pipeline, hl_t256::hl::kMbThreads, 0);
    *per_cu = std::min(n, 2);
    return r;
}
