// hl_rec_emu.hip -- TEST INFRASTRUCTURE.  Host exports of the candidate
// record's pack and unpack functions (hl_mbcore.h CandRec, rec_*), the same
// ones the kernels, the emulator and the selection use;
// tests/test_cand_record.py checks every field at both ends of its range.
#include <hip/hip_runtime.h>

#include "../../hartallo_amd/csrc/hl_mbcore.h"

using namespace hl;

// in: {bits, dist, cbp, single, last}; rec: the record as it lies in memory
// (four 32-bit words: cost low, cost high, bd, meta), written by the
// writers' rec_store; out: the five fields unpacked from the stored record
extern "C" void rec_roundtrip(const int* in, double cost, uint32_t* rec, int* out)
{
    CandRec r;
    rec_store(r, cost, rec_bd(in[0], in[1]), rec_meta(in[2], in[3], in[4]));
    memcpy(rec, &r, sizeof r);
    out[0] = rec_bits(r.bd);
    out[1] = rec_dist(r.bd);
    out[2] = rec_cbp(r.meta);
    out[3] = rec_single(r.meta);
    out[4] = rec_last(r.meta);
}

extern "C" int rec_sizeof(void) { return (int)sizeof(CandRec); }
extern "C" int rec_lds_bytes(void) { return (int)sizeof(Shared::cd); }
