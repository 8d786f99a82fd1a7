// Test-only host build of the pop's pure parts (hartallo_amd/csrc/hl_sched.h):
// the priority key, the choice among a wave's keys, the head-advance rule
// and the slot / claim / head transitions pop_task runs, exported one by one
// (tests/test_pop_select.py drives them in a protocol model).
#include "../../hartallo_amd/csrc/hl_sched.h"

extern "C" int32_t sched_emu_spread(void) { return hl::kPopSpread; }
extern "C" int32_t sched_emu_look(void) { return hl::kPopLook; }
extern "C" int32_t sched_emu_oversub(void) { return hl::kPopOversub; }
extern "C" int32_t sched_emu_stand_back(void) { return hl::kPopStandBack; }

extern "C" int32_t sched_emu_key(int32_t mbw, int32_t mbh, int32_t x, int32_t y, int32_t hop, int32_t j, int32_t own)
{
    return hl::sched_key(mbw, mbh, x, y, hop, j, own);
}
extern "C" int32_t sched_emu_key_oldest(int32_t r) { return hl::sched_key_oldest(r); }

// What a wave does with its 64 lanes' best keys (has[l] = 0: lane l has no
// entry): the packed maximum, the lanes within the spread, the chosen lane.
// Returns the lane, -1 with no entry at all, or -2 when the popper stands
// back this round (must = 0 only); *within_out = the lanes within the
// spread, *count_out = sched_spread_count.
extern "C" int32_t sched_emu_choose(const int32_t* keys, const int32_t* has, int32_t spread, uint32_t seq, int32_t poppers, int32_t must,
                                    uint64_t* within_out, int32_t* count_out)
{
    int32_t packed[64], best = -1;
    for (int l = 0; l < 64; ++l) {
        packed[l] = has[l] ? hl::sched_pack(keys[l], l) : -1;
        if (packed[l] > best) best = packed[l];
    }
    if (best < 0) return -1;
    uint64_t within = 0;
    for (int l = 0; l < 64; ++l)
        if (hl::sched_within(packed[l], best, spread)) within |= 1ull << l;
    if (within_out) *within_out = within;
    if (count_out) *count_out = hl::sched_spread_count(within, poppers);
    const int lane = hl::sched_choose(within, hl::sched_packed_lane(best), seq, poppers, must != 0);
    return lane < 0 ? -2 : lane;
}
extern "C" int32_t sched_emu_in_lane(uint32_t seq, int32_t m, int32_t c) { return hl::sched_in_lane(seq, m, c); }
extern "C" uint32_t sched_emu_seq_next(uint32_t seq) { return hl::sched_seq_next(seq); }

extern "C" int32_t sched_emu_head_target(int32_t h, int32_t t, int32_t p0, const int32_t* v, int32_t n, int32_t own)
{
    return hl::sched_head_target(h, t, p0, v, n, own);
}
extern "C" int32_t sched_emu_take_slot(int32_t* slot, int32_t v) { return hl::sched_take_slot(slot, v) ? 1 : 0; }
extern "C" int32_t sched_emu_claim_task(int32_t* claim) { return hl::sched_claim_task(claim) ? 1 : 0; }
extern "C" void sched_emu_advance_head(int32_t* head, int32_t to) { hl::sched_advance_head(head, to); }
