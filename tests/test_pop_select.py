"""The pipelined run's pop (hartallo_amd/csrc/hl_sched.h) through its host
build, tests/emu/libhl_sched_emu.so: the functions pop_task itself calls.

1. One popper present chooses the entry of maximal key, ties to the lowest
   lane, over random sets of up to 256 queue heads (64 lanes x 4); the key is
   restated here: (mbw-1-x) + 2 (mbh-1-y) - hop j + own.  With hop < 0 the
   first non-empty queue in window order.
2. With p poppers present every k < p chooses an entry within the spread of
   the best one, and distinct k choose distinct entries while entries within
   the spread remain.  With more poppers than entries (kPopOversub > 0) a
   popper whose k is entries * kPopOversub or more stands back for the round,
   unless it has stood back kPopStandBack rounds.
3. A discrete-event model of the protocol on the exported slot / claim / head
   transitions and emu_task_deps / emu_task_succ, every memory step of a pop
   round and of a push interleaved at random with the other workers' steps
   (heads and tails read, slots read, head maxima, slot CAS, claim CAS, head
   maximum; tail fetch-add, slot store): every task runs exactly once, the
   run completes, every head ends at its tail, and no popper ever waits: a
   worker that polls a word for another's write is recorded, and only
   claim_next's worker ever is; slots seen unwritten are met and skipped.  A variant that
   never moves a head is caught: the model can fail.
"""
import ctypes
import os
import random
import subprocess

import pytest

from hl_testlib import emu_lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(HERE, "emu", "libhl_sched_emu.so")
SUBQ, SCAN, HOP = 4, 4, 18  # hl_encoder.hip: kSubQ, kScan; the launcher's hop
LOOK = 4  # (set from the library: kPopLook)
i32p = ctypes.POINTER(ctypes.c_int32)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", ROOT, "tests/emu/libhl_sched_emu.so"], check=True, capture_output=True)
    so = ctypes.CDLL(LIB)
    so.sched_emu_key.argtypes = [ctypes.c_int32] * 7
    so.sched_emu_key_oldest.argtypes = [ctypes.c_int32]
    so.sched_emu_choose.argtypes = [i32p, i32p, ctypes.c_int32, ctypes.c_uint32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint64), i32p]
    so.sched_emu_in_lane.argtypes = [ctypes.c_uint32, ctypes.c_int32, ctypes.c_int32]
    so.sched_emu_seq_next.argtypes = [ctypes.c_uint32]
    so.sched_emu_seq_next.restype = ctypes.c_uint32
    so.sched_emu_head_target.argtypes = [ctypes.c_int32] * 3 + [i32p, ctypes.c_int32, ctypes.c_int32]
    so.sched_emu_take_slot.argtypes = [i32p, ctypes.c_int32]
    so.sched_emu_claim_task.argtypes = [i32p]
    so.sched_emu_advance_head.argtypes = [i32p, ctypes.c_int32]
    global LOOK
    LOOK = so.sched_emu_look()
    return so


@pytest.fixture(scope="module")
def deps_lib():
    so = emu_lib()
    so.emu_task_deps.argtypes = [ctypes.c_int] * 6 + [ctypes.POINTER(ctypes.c_int)]
    so.emu_task_succ.argtypes = [ctypes.c_int] * 7 + [ctypes.POINTER(ctypes.c_int)]
    return so


def _choose(lib, keys, has, seq, poppers, spread=None, must=True):
    """The chosen lane (-1: no entry, -2: stands back), the lanes within the spread, sched_spread_count."""
    k = (ctypes.c_int32 * 64)(*keys)
    h = (ctypes.c_int32 * 64)(*[1 if b else 0 for b in has])
    within, count = ctypes.c_uint64(0), ctypes.c_int32(0)
    lane = lib.sched_emu_choose(k, h, lib.sched_emu_spread() if spread is None else spread, seq, poppers, 1 if must else 0, ctypes.byref(within), ctypes.byref(count))
    return lane, within.value, count.value


def _random_heads(lib, rng, oldest_first):
    """Up to 256 heads: entry e = lane + 64 i is sub-queue e % 4 of the (e // 4)-th
    picture of the window.  Returns per lane its best key the way a lane
    forms it (first of equal keys) and, for the check, every (key, e)."""
    mbw, mbh, hop, ownq = rng.randrange(1, 121), rng.randrange(1, 69), rng.choice([15, 18, 21]), rng.randrange(SUBQ)
    fill = rng.choice([0.02, 0.2, 0.7, 1.0])
    best = [None] * 64
    entries = []
    for lane in range(64):
        for i in range(SCAN):
            if rng.random() >= fill:
                continue
            e = lane + 64 * i
            x, y, j = rng.randrange(mbw), rng.randrange(mbh), e // SUBQ
            own = 30 if e % SUBQ == ownq else 0
            if oldest_first:
                key = lib.sched_emu_key_oldest(e // SUBQ)
                assert key == -256 * (e // SUBQ)
            else:
                key = lib.sched_emu_key(mbw, mbh, x, y, hop, j, own)
                assert key == (mbw - 1 - x) + 2 * (mbh - 1 - y) - hop * j + own
            entries.append((key, e))
            if best[lane] is None or key > best[lane]:
                best[lane] = key
    return best, entries


@pytest.mark.parametrize("oldest_first", [False, True], ids=["hop18", "oldest_first"])
def test_one_popper_chooses_as_before(lib, oldest_first):
    rng = random.Random(7 + oldest_first)
    for _ in range(300):
        best, entries = _random_heads(lib, rng, oldest_first)
        lane, _, count = _choose(lib, [b or 0 for b in best], [b is not None for b in best], rng.randrange(1 << 32), 1, must=False)
        if not entries:
            assert lane == -1
            continue
        assert count == 1
        if oldest_first:  # the first non-empty queue in window order
            assert lane == min(e for _, e in entries) % 64
        else:  # the maximal key, ties to the lowest lane
            top = max(k for k, _ in entries)
            assert lane == min(e % 64 for k, e in entries if k == top)


@pytest.mark.parametrize("poppers", [2, 3, 5, 17, 64, 300])
def test_spread_stays_within_and_covers(lib, poppers):
    rng = random.Random(poppers)
    spread = lib.sched_emu_spread()
    for _ in range(60):
        best, entries = _random_heads(lib, rng, False)
        if not entries:
            continue
        has = [b is not None for b in best]
        top = max(b for b in best if b is not None)
        inside = [l for l in range(64) if has[l] and best[l] >= top - spread]
        chosen = []
        oversub = lib.sched_emu_oversub()
        for k in range(poppers if poppers <= 64 else 80):
            lane, within, count = _choose(lib, [b or 0 for b in best], has, k, poppers)
            assert within == sum(1 << l for l in inside) and count == min(len(inside), poppers)
            assert lane in inside
            chosen.append(lane)
            free = _choose(lib, [b or 0 for b in best], has, k, poppers, must=False)[0]
            if oversub > 0 and k >= len(inside) * oversub:
                assert free == -2  # more poppers than entries: this one stands back
            else:
                assert free == lane
        m = min(len(inside), poppers)
        assert len(set(chosen[:m])) == m  # distinct k, distinct entries, while entries within the spread remain
        assert chosen[0] == min(l for l in inside if best[l] == top)  # k = 0: the best one
        # equal k: the entries of the lane in turn
        for c in (1, 2, 3, 16):
            assert [lib.sched_emu_in_lane(m * r + m - 1, m, c) for r in range(2 * c)] == [r % c for r in range(2 * c)]


def test_head_target_rule(lib):
    def target(h, t, p0, v, own=-1):
        return lib.sched_emu_head_target(h, t, p0, (ctypes.c_int32 * len(v))(*v), len(v), own)
    assert target(0, 0, 0, [0, 0, 0, 0]) == 0
    assert target(4, 8, 4, [-5, -6, 7, -8]) == 6          # stops at the first ready slot
    assert target(5, 8, 4, [0, -6, -7, -8]) == 8          # from the head, to the tail
    assert target(5, 7, 4, [0, -6, -7, -8]) == 7          # never past the tail
    assert target(4, 8, 4, [0, -6, -7, -8]) == 4          # a slot not yet written stops it
    assert target(4, 8, 4, [5, -6, 7, 0], own=4) == 6     # the popper's own slot counts as taken
    assert target(4, 8, 4, [5, 6, -7, 0], own=5) == 4     # not past a ready slot below it
    assert target(1, 3, -2, [0, 0, 0, -2]) == 2           # a group that starts in the row before


# --- 3. the protocol model -------------------------------------------------

class _Run:
    def __init__(self, lib, dl, mbw, mbh, R, nf, workers, seed, advance=True, in_order=False, oldest_first=False):
        self.lib, self.mbw, self.mbh, self.nf, self.workers = lib, mbw, mbh, nf, workers
        self.rng = random.Random(seed)
        self.advance, self.in_order, self.oldest_first = advance, in_order, oldest_first
        self.nmb = nmb = mbw * mbh
        out = (ctypes.c_int * (3 * 512))()
        trip = lambda n: [(out[3 * i], out[3 * i + 1], out[3 * i + 2]) for i in range(n)]
        tasks = [(f, x, y) for f in range(nf) for y in range(mbh) for x in range(mbw)]
        self.succ = {t: trip(dl.emu_task_succ(*t, mbw, mbh, R, nf, out)) for t in tasks}
        self.cnt = {t: dl.emu_task_deps(*t, mbw, mbh, R, out) for t in tasks}
        self.order = tasks  # run order: picture, then raster address
        nq = nf * SUBQ
        self.queue = (ctypes.c_int32 * (nq * nmb + 4))()  # (+4: a head's group may end past the last row, as in the kernel's allocation)
        self.head = (ctypes.c_int32 * nq)()
        self.tail = (ctypes.c_int32 * nq)()
        self.claim = (ctypes.c_int32 * (nf * nmb))()
        self.queue[0], self.tail[0] = 1, 1
        self.ran = {}
        self.done = set()
        self.version = 0  # any write to the shared words
        self.skipped_unwritten = self.lost = self.advances = 0
        self.waited = set()  # workers that ever polled a word for another worker's write
        # a worker: its pending steps (generators), or None while parked after an empty round
        self.gen = [self._worker(w) for w in range(workers)]
        self.parked_at = [None] * workers
        self.in_pop = [not (in_order and w == 0) for w in range(workers)]  # inside pop_task (P.poppers)

    def _ptr(self, arr, i):
        return ctypes.cast(ctypes.byref(arr, 4 * i), i32p)

    def _push(self, s):
        f, x, y = s
        a = y * self.mbw + x
        q = f * SUBQ + x * SUBQ // self.mbw
        pos = self.tail[q]
        self.tail[q] = pos + 1  # the fetch-add
        self.version += 1
        yield
        self.queue[q * self.nmb + pos] = a + 1  # the slot's release store
        self.version += 1
        yield

    def _task(self, w, t):
        assert t not in self.ran, f"task {t} ran twice"
        self.ran[t] = w
        self.in_pop[w] = False
        for _ in range(self.rng.randrange(0, 4)):  # the decision
            yield
        for s in self.succ[t]:
            self.cnt[s] -= 1
            self.version += 1
            yield
            if self.cnt[s] == 0:
                yield from self._push(s)
        self.done.add(t)  # (the kernel's pops end when the last task has finished: `oldest`)
        self.version += 1
        self.in_pop[w] = not (self.in_order and w == 0)

    def _worker(self, w):
        lib, nmb = self.lib, self.nmb
        if w == 0 and self.in_order:  # claim_next: run order, then the dependencies
            for t in self.order:
                f, x, y = t
                if not lib.sched_emu_claim_task(self._ptr(self.claim, f * nmb + y * self.mbw + x)):
                    continue
                self.version += 1
                yield
                while self.cnt[t]:
                    yield "blocked"
                yield from self._task(w, t)
            return
        seq, stood_back = w, 0
        while True:
            # heads and tails, then (later) the slots of each head's group
            nq = self.nf * SUBQ
            hs, ts = list(self.head), list(self.tail)
            yield
            poppers = sum(self.in_pop)
            look = []
            for q in range(nq):
                if hs[q] < ts[q]:
                    g = (q * nmb + hs[q]) & ~(LOOK - 1)
                    p0 = g - q * nmb
                    v = [self.queue[g + s] if hs[q] <= p0 + s < ts[q] else 0 for s in range(LOOK)]
                    self.skipped_unwritten += sum(1 for s in range(LOOK) if hs[q] <= p0 + s < ts[q] and v[s] == 0)
                    look.append((q, p0, v))
            yield
            # taken slots at a head: the maxima
            for q, p0, v in look:
                to = lib.sched_emu_head_target(hs[q], ts[q], p0, (ctypes.c_int32 * LOOK)(*v), LOOK, -1)
                if to > hs[q] and self.advance:
                    lib.sched_emu_advance_head(self._ptr(self.head, q), to)
                    self.version += 1
                    self.advances += 1
                    yield
            # keys: lane = queue index (picture-major, as entry e of the kernel's first 64)
            own_q = w % SUBQ
            keys, has, ent = [0] * 64, [False] * 64, {}
            for q, p0, v in look:
                for s in range(LOOK):
                    if v[s] > 0:
                        a = v[s] - 1
                        key = (lib.sched_emu_key_oldest(q // SUBQ) if self.oldest_first else
                               lib.sched_emu_key(self.mbw, self.mbh, a % self.mbw, a // self.mbw, HOP, q // SUBQ, 30 if q % SUBQ == own_q else 0))
                        ent.setdefault(q, []).append((key, p0 + s, v[s]))
                        if not has[q] or key > keys[q]:
                            keys[q], has[q] = key, True
            if not ent:
                # an empty round (the heads moved first): the end of the run, or another scan (here: once a word has changed)
                if len(self.done) == len(self.order):
                    return
                self.parked_at[w] = self.version
                yield "empty"
                continue
            lane, _, m = _choose(lib, keys, has, seq, poppers, must=stood_back >= lib.sched_emu_stand_back())
            if lane == -2:  # more poppers than entries: no attempt this round, and no wait either (the next round follows)
                stood_back += 1
                seq = lib.sched_emu_seq_next(seq)
                yield
                continue
            stood_back = 0
            top = max(k for k, h in zip(keys, has) if h)
            cands = [e for e in ent[lane] if e[0] >= top - lib.sched_emu_spread()]
            key, pos, v = max(ent[lane], key=lambda e: (e[0], -e[1])) if m == 1 else cands[lib.sched_emu_in_lane(seq, m, len(cands))]
            won = lib.sched_emu_take_slot(self._ptr(self.queue, lane * nmb + pos), v)
            yield
            if won:
                self.version += 1
                f, a = lane // SUBQ, v - 1
                got = lib.sched_emu_claim_task(self._ptr(self.claim, f * nmb + a))
                yield
                q, p0, vv = next(l for l in look if l[0] == lane)
                to = lib.sched_emu_head_target(hs[q], ts[q], p0, (ctypes.c_int32 * LOOK)(*vv), LOOK, pos)
                if to > hs[q] and self.advance:
                    lib.sched_emu_advance_head(self._ptr(self.head, q), to)
                    self.version += 1
                    yield
                if got:
                    yield from self._task(w, (f, a % self.mbw, a // self.mbw))
                    continue
            self.lost += 1
            seq = lib.sched_emu_seq_next(seq)

    def run(self):
        """True when every task ran; False when no worker can take a step
        any more (or far too many steps were taken)."""
        live = list(range(self.workers))
        for _ in range(400 * len(self.order) * self.workers + 10000):
            if not live:
                return len(self.done) == len(self.order)
            ready = [w for w in live if self.parked_at[w] is None or self.parked_at[w] != self.version]
            if not ready:
                return False  # every worker idle and no word can change any more
            w = self.rng.choice(ready)
            self.parked_at[w] = None
            try:
                r = next(self.gen[w])
                if r == "blocked":
                    self.waited.add(w)
                    self.parked_at[w] = self.version
            except StopIteration:
                live.remove(w)
        return False

    def check_end(self):
        assert sorted(self.ran) == sorted(self.order)
        # no popper ever waits: only claim_next (worker 0 of the in-order variant) polls a word
        assert self.waited <= ({0} if self.in_order else set()), self.waited
        for q in range(self.nf * SUBQ):
            assert all(self.queue[q * self.nmb + p] < 0 for p in range(self.head[q])), "a head passed a slot nobody took"
            if not self.in_order:
                assert self.head[q] == self.tail[q], (q, self.head[q], self.tail[q])


GEOMETRIES = [(6, 5), (8, 3), (3, 6), (1, 1)]  # (1, 1): fewer MBs than sub-queue heads


@pytest.mark.parametrize("workers", [1, 2, 3, 6, 40])
@pytest.mark.parametrize("mbw,mbh", GEOMETRIES)
def test_protocol_model(lib, deps_lib, mbw, mbh, workers):
    skipped = 0
    for R in range(3):
        for seed in range(6):
            run = _Run(lib, deps_lib, mbw, mbh, R, 3, workers, seed)
            assert run.run(), (mbw, mbh, R, workers, seed, len(run.ran))
            run.check_end()
            skipped += run.skipped_unwritten
    print(f"{mbw}x{mbh}, {workers} workers: slots seen unwritten and skipped {skipped}")
    if workers > 1 and mbw * mbh > 1:
        # the case the old pop spun on (tail moved, slot not yet stored) was met, and skipped
        assert skipped > 0


@pytest.mark.parametrize("workers", [2, 6])
def test_protocol_model_with_the_in_order_workgroup(lib, deps_lib, workers):
    # worker 0 claims in run order (claim_next): poppers then meet entries whose claim word is held
    blocked = False
    for seed in range(6):
        run = _Run(lib, deps_lib, 6, 5, 2, 3, workers, seed, in_order=True)
        assert run.run(), (workers, seed)
        run.check_end()
        blocked = blocked or 0 in run.waited
    assert blocked  # (the check can see a wait: claim_next's was met)


def test_protocol_model_oldest_first(lib, deps_lib):
    for seed in range(6):
        run = _Run(lib, deps_lib, 8, 3, 1, 3, 6, seed, oldest_first=True)
        assert run.run(), seed
        run.check_end()


def test_protocol_model_catches_a_head_that_never_moves(lib, deps_lib):
    # a head left on taken slots hides the entries behind its group
    for workers in (1, 6):
        assert not any(_Run(lib, deps_lib, 6, 5, 0, 3, workers, seed, advance=False).run() for seed in range(6))
