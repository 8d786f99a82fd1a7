// hl_emu_ctl.hip -- TEST INFRASTRUCTURE.  The translation unit of the host
// emulation (tests/emu/libhl_emu.so): hl_emu_memo.hip (hl_emu.hip plus the
// memo's exports) as it is, plus the per-frame encoding type and live
// settings of hl_amd_encode_ex (include/hartallo_amd.h), so that their
// semantics are tested on the CPU against reference-made goldens.
#include "hl_emu_memo.hip"

// emu_encode_frame with the frame's hl_frame_t.encoding (0 AUTO, 1 INTRA,
// 2 INTER, 3 LOSSLESS, 4 RAW) and the hl_codec_t settings at the time of its
// call, which stay until the next change.  Returns the bytes, or minus the
// product's error code for a refused frame (-7 not implemented, -1 invalid
// parameter), the encoder left as it was.
extern "C" long emu_encode_frame_ex(void* h, const uint8_t* y, const uint8_t* u, const uint8_t* v, uint8_t* out, long cap, int encoding,
                                    int me_range, int deblock, int early_term, int gop)
{
    EmuEnc* e = (EmuEnc*)h;
    if (encoding < 0 || encoding > 2) return -7;
    if (early_term && (e->W < 32 || e->H < 32)) return -1;  // rdo.c:895-896, as the product's create
    e->me_range = me_range < 1 ? 1 : (me_range > 64 ? 64 : me_range);  // rdo.c:847
    e->deblock = deblock;  // the pass and the slice header's disable_deblocking_filter_idc (SPS / PPS were written at create)
    e->early_term = early_term;
    e->gop = gop;  // read only where the counter reloads (hl_codec_264.c:709, 717)
    // hl_codec_264.c:705-718: a counter that has run out gives an IDR whatever
    // is asked; INTRA elsewhere forces one and reloads the counter from
    // gop_size -- which is what emu_encode_frame does with a spent counter
    if (encoding == 1) e->gop_left = 0;
    return emu_encode_frame(h, y, u, v, out, cap);
}
