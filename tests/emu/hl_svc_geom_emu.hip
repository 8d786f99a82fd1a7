// hl_svc_geom_emu.hip -- TEST INFRASTRUCTURE.  Host exports of the per-layer
// constants of the enhancement-layer kernel (hartallo_amd/csrc/hl_svc.h
// svc_geom) and of one Intra_Base luma sample (svc_resample), for
// tests/test_emu_svc_display.py: which layer sizes take the reproduced
// reference quirk of the Intra_Base sample array (svc_ref_array_sample), and
// that every other size runs the plain G.8.6.2 interpolation.
#include <hip/hip_runtime.h>

#include "../../hartallo_amd/csrc/hl_svc.h"
#include "../../hartallo_amd/csrc/hl_writer.h"

using namespace hl;

// SvcGeom::rsa_bytes of a W x H layer over its dyadic reference layer
extern "C" int32_t svc_geom_emu_rsa_bytes(int32_t W, int32_t H)
{
    if (W < 32 || H < 32 || (W & 31) || (H & 31)) return -1;
    return svc_geom(W, H, W / 2, H / 2, stream_level_idc(W, H)).rsa_bytes;
}

// The Intra_Base luma prediction of a whole W x H layer from the dense
// (W / 2) x (H / 2) reference-layer plane, as k_svc_mb's lanes compute it;
// plain != 0: with the quirk switched off (rsa_bytes = 0)
extern "C" int32_t svc_geom_emu_intra_base(int32_t W, int32_t H, const uint8_t* ref, int32_t plain, uint8_t* out)
{
    if (W < 32 || H < 32 || (W & 31) || (H & 31) || !ref || !out) return -1;
    SvcGeom g = svc_geom(W, H, W / 2, H / 2, stream_level_idc(W, H));
    if (plain) g.rsa_bytes = 0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) out[(size_t)y * W + x] = (uint8_t)svc_resample(g, ref, 0, x >> 4, y >> 4, x & 15, y & 15);
    return 0;
}
