// hl_sched.h -- the pure parts of the pipelined run's pop (pop_task in
// hl_encoder.hip): the priority key, the choice among a wave's keys, the
// head-advance rule and the slot / claim / head transitions.  Host and
// device share them: the kernel calls them per lane and per wave, the host
// build (tests/emu/hl_sched_emu.cpp, tests/sanitize/pop_tsan.cpp) runs the
// same functions in a protocol model and under ThreadSanitizer.
//
// The ready queue of (picture f, sub-queue q) is P.queue[(f * kSubQ + q) *
// nmb + pos]: 0 = not yet written, a + 1 = MB address a ready, -(a + 1) =
// taken.  A push moves `tail` by fetch-add and stores a + 1 with release.  A
// pop CASes the slot word itself a + 1 -> -(a + 1), then the task's claim
// word 0 -> 1 (workgroup 0's claim_next may hold the task already: the slot
// is spent either way).  `head` is a hint with one invariant: every slot
// below it is taken.  Whoever sees taken slots at the head moves it past
// them (a maximum: it never moves back).  A popper looks at the slots of the
// head's aligned group (kPopLook words), so two poppers that see several
// ready entries can take different ones, and nobody waits for a slot: one
// that is still 0 is skipped.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HL_SCHED_HD __host__ __device__ __forceinline__
#else
#define HL_SCHED_HD inline
#endif

namespace hl {

// entries within this many wavefront steps of the best visible one are
// candidates of a pop when several workgroups pop at once (the own-band
// preference is worth 30)
#ifndef HL_POP_SPREAD
#define HL_POP_SPREAD 30
#endif
constexpr int kPopSpread = HL_POP_SPREAD;
// slots of a queue a pop reads: the head's aligned pair (one 8-byte load), or group of four (two)
#ifndef HL_POP_LOOK
#define HL_POP_LOOK 2
#endif
constexpr int kPopLook = HL_POP_LOOK;
// With more poppers present than entries within the spread, a popper tries
// only if its k (sequence modulo poppers) falls below entries * this (>= 1)
// and stands back otherwise (a round without a CAS), at most kPopStandBack
// rounds in a row: the others' CASes on the few ready slot words are what a
// lost round costs (every popper trying in every round, k modulo
// min(entries, poppers), measured 5.5 % slower at 120 pictures).
#ifndef HL_POP_OVERSUB
#define HL_POP_OVERSUB 4
#endif
constexpr int kPopOversub = HL_POP_OVERSUB;
static_assert(kPopOversub >= 1, "HL_POP_OVERSUB: tries per entry and round, at least one");
constexpr int kPopStandBack = 8;
constexpr int kSchedKeyBias = 1 << 16;  // keeps packed keys positive (|key| < 2^16: 128 pictures of hop <= 64, 2^12 MB rows)

// Priority of ready MB (x, y) of the j-th picture of the window: the longest
// remaining dependency path to the end of the run in wavefront steps, a
// picture boundary counting hop steps; own = the preference for the
// workgroup's own sub-queue.
HL_SCHED_HD int sched_key(int mbw, int mbh, int x, int y, int hop, int j, int own)
{
    return (mbw - 1 - x) + 2 * (mbh - 1 - y) - hop * j + own;
}
// hop < 0 (oldest picture first): the r-th picture of the window in window
// order; its sub-queues tie (the lowest lane is the first of them), and the
// next picture is further than any spread away.
HL_SCHED_HD int sched_key_oldest(int r) { return -256 * r; }

// A lane's key with its lane: the wave's maximum is the best key, ties to the lowest lane.
HL_SCHED_HD int sched_pack(int key, int lane) { return ((key + kSchedKeyBias) << 6) | (63 - lane); }
HL_SCHED_HD int sched_packed_key(int p) { return (p >> 6) - kSchedKeyBias; }
HL_SCHED_HD int sched_packed_lane(int p) { return 63 - (p & 63); }
// packed key p (< 0: the lane has no entry) within `spread` of the wave's best
HL_SCHED_HD bool sched_within(int p, int best, int spread) { return p >= 0 && (p >> 6) >= (best >> 6) - spread; }

// index of the k-th set bit of m (k < popcount(m))
HL_SCHED_HD int sched_kth_bit(uint64_t m, int k)
{
    for (int i = 0; i < k; ++i) m &= m - 1;
    return __builtin_ctzll(m);
}

// A workgroup's sequence: blockIdx first (neighbouring workgroups differ by
// one), another value after every lost attempt.
HL_SCHED_HD uint32_t sched_seq_next(uint32_t seq) { return seq * 1664525u + 1013904223u; }
HL_SCHED_HD uint32_t sched_seq_value(uint32_t seq) { return seq ^ (seq >> 16); }

// candidates a pop chooses among: the lanes within the spread, at most one per popper present
HL_SCHED_HD int sched_spread_count(uint64_t within, int poppers)
{
    const int n = __builtin_popcountll(within);
    return n < poppers ? n : (poppers > 1 ? poppers : 1);
}
// The lane whose entry this pop tries, or -1: stand back this round.  k =
// sequence modulo poppers present; with n lanes within the spread the popper
// stands back if k >= n * kPopOversub, unless `must` (it has stood back
// kPopStandBack rounds); else it tries the (k modulo n)-th lane within the
// spread, counted from the best lane upwards (cyclically).  One popper
// present: k = 0, the best lane, and no standing back.  A pop starts its
// sequence at blockIdx, so with p poppers present the workgroups whose
// blockIdx modulo p is n * kPopOversub or more stand back in the first round
// of every pop (and then take a helper task if one is queued): a fixed bias
// towards low workgroup numbers for the first try, not for the task.
HL_SCHED_HD int sched_choose(uint64_t within, int best_lane, uint32_t seq, int poppers, bool must)
{
    const int n = __builtin_popcountll(within);
    int k = (int)(sched_seq_value(seq) % (uint32_t)(poppers > 1 ? poppers : 1));
    if (k >= n * kPopOversub && !must) return -1;
    k %= n;
    const uint64_t rot = best_lane ? (within >> best_lane) | (within << (64 - best_lane)) : within;
    return (best_lane + sched_kth_bit(rot, k)) & 63;
}
// which of the chosen lane's c entries within the spread (slot order), so
// that poppers with equal k still differ; m = sched_spread_count.  m == 1:
// the caller takes the lane's best entry.
HL_SCHED_HD int sched_in_lane(uint32_t seq, int m, int c) { return (int)((sched_seq_value(seq) / (uint32_t)m) % (uint32_t)c); }

// Head-advance rule.  v[0..n) are the slot words at queue positions p0 ..
// p0 + n - 1 as one read saw them, h the head (p0 <= h) and t the tail of
// the same read; own = the position this popper has just taken, or -1.
// Returns the head's new value: past every consecutive taken slot from h.
HL_SCHED_HD int sched_head_target(int h, int t, int p0, const int32_t* v, int n, int own)
{
    int to = h;
    for (int s = 0; s < n; ++s) {
        const int p = p0 + s;
        if (p == to && p < t && (v[s] < 0 || p == own)) ++to;
    }
    return to;
}

// Transitions over plain words.  Device: relaxed agent-scope atomics (the
// popper's acquire fence follows the pop, hl_pipeline.h).  Host (the model
// and the ThreadSanitizer program): the same transitions with acquire /
// release on the operation itself, since ThreadSanitizer does not model fences.
HL_SCHED_HD bool sched_cas(int32_t* w, int32_t expect, int32_t desired)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicCAS(w, expect, desired) == expect;
#else
    return __atomic_compare_exchange_n(w, &expect, desired, false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE);
#endif
}
// slot word v = a + 1 > 0 as read: true if this popper took the entry
HL_SCHED_HD bool sched_take_slot(int32_t* slot, int32_t v) { return sched_cas(slot, v, -v); }
// the task's claim word: false if workgroup 0 holds the task already
HL_SCHED_HD bool sched_claim_task(int32_t* claim) { return sched_cas(claim, 0, 1); }
// moves the head to `to` unless it is already there or further
HL_SCHED_HD void sched_advance_head(int32_t* head, int32_t to)
{
#if defined(__HIP_DEVICE_COMPILE__)
    atomicMax(head, to);
#else
    int32_t cur = __atomic_load_n(head, __ATOMIC_RELAXED);
    while (cur < to && !__atomic_compare_exchange_n(head, &cur, to, false, __ATOMIC_ACQ_REL, __ATOMIC_RELAXED)) {
    }
#endif
}

}  // namespace hl
