"""The candidate record and the selection that reads it, on the GPU
(hl_mbcore.h CandRec, rec_store, sel_load, sel_minima, sel_take): a 64-lane
unit kernel (tests/gpu_unit/hl_unit_rec.hip) writes up to kMaxCand records
into both parities through the writers' store, in the layout the search
generates a pass in (lane 16 j + i = point i of step j, candidates numbered
in lane order), reads them back through the selection's loader, runs the
one-row minimum and takes each step's winner.  Everything is compared with
the inputs restated here: costs with ties, 0.0 and the largest double; the
first lane of equal costs wins; the four step rows are kept apart; an absent
step gives lane -1; every field at both ends of its range.  Tolerance: none."""
import ctypes
import os
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_unit", "libhl_unit_rec.so")
KMAX, NSEG = 32, 4
DMAX = 1.7976931348623157e308
CAND_IN, LANE_OUT, TAKE_OUT = 10, 6, 8
CASE_IN = 2 + 2 * KMAX * CAND_IN
PAR_OUT = 64 * LANE_OUT + NSEG * 3 + NSEG * TAKE_OUT
HI = {"bits": (1 << 15) - 1, "dist": (1 << 17) - 1, "cbp": 0xFFFF, "single": 224, "last": 15}
LO = {"bits": 0, "dist": 0, "cbp": 0, "single": 0, "last": -1}


def _dwords(x):
    return struct.unpack("<ii", struct.pack("<d", x))


def _mask(rows):
    """rows: per step row, the enabled points (lanes of the row)."""
    m = 0
    for j, pts in enumerate(rows):
        for p in pts:
            m |= 1 << (16 * j + p)
    return m


def _cand(rng, cost, ends=None):
    """One candidate: (cost, bits, dist, cbp, single, last, mvx, mvy)."""
    if ends is not None:
        f = [ends[k] for k in ("bits", "dist", "cbp", "single", "last")]
    else:
        f = [int(rng.integers(LO[k], HI[k] + 1)) for k in ("bits", "dist", "cbp", "single", "last")]
    return (cost, *f, int(rng.integers(-2048, 2048)), int(rng.integers(-2048, 2048)))


def _cases():
    rng = np.random.default_rng(2609)
    full9 = list(range(9))
    cases = []  # (mask, [cands of parity 0], [cands of parity 1])

    def add(rows, costs0, costs1, ends0=None, ends1=None):
        m = _mask(rows)
        n = bin(m).count("1")
        assert n <= KMAX and len(costs0) == n and len(costs1) == n
        cases.append((m, [_cand(rng, c, ends0) for c in costs0], [_cand(rng, c, ends1) for c in costs1]))

    # the MVP/(0,0) step and three full continuations (2 + 9 + 5 + 9 = 25): distinct costs; every field at its ends
    rows = [[0, 1], full9, list(range(5)), full9]
    add(rows, [float(x) for x in rng.permutation(25) + 1], [float(x) for x in rng.permutation(25) + 100], HI, LO)
    # ties inside a row (the first lane wins), 0.0, and a row whose only costs are the largest double
    add(rows, [5.0, 5.0] + [7.0, 3.0, 9.0, 3.0, 3.0, 8.0, 7.0, 9.0, 4.0] + [0.0, 1.0, 0.0, 2.0, 0.0] + [DMAX] * 9,
        [DMAX, 0.0] + [DMAX] * 8 + [6.0] + [2.5] * 5 + [1e300, 1e-300, 1e-300, 5e-324, 5e-324, 1.0, 2.0, 3.0, 4.0])
    # the same smallest cost in every row: each row reports its own first lane
    add([[3, 5], [8], [0, 4], [2, 6, 7]], [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0], [2.0, 1.0, 1.0, 3.0, 1.0, 9.0, 1.0, 1.0])
    # absent steps: rows 1 and 3 empty; then only row 2; then only lane 63's neighbour rows
    add([full9, [], list(range(5)), []], [float(x) for x in range(14, 0, -1)], [DMAX] * 13 + [0.0])
    add([[], [], [2], []], [4.0], [DMAX])
    add([[], [], [], [15]], [0.0], [3.0])
    # kMaxCand records: two rows of 16, and 8 in each of the four rows; minima at the rows' last lanes
    add([list(range(16)), list(range(16))], [float(40 - i) for i in range(32)], [1.0] * 31 + [0.5])
    add([list(range(0, 16, 2))] * 4, [float(x) for x in rng.permutation(32)], [float(x % 3) for x in rng.permutation(32)], LO, HI)
    # sparse points of continued steps (visited points and the window's edge leave gaps)
    for _ in range(6):
        rows = [sorted(rng.choice(9, size=int(rng.integers(0, 9)), replace=False).tolist()) for _ in range(NSEG)]
        n = sum(len(r) for r in rows)
        add(rows, [float(x) for x in rng.integers(0, 6, size=n)], [float(x) * 0.25 for x in rng.integers(0, 1000, size=n)])
    return cases


def _expect(mask, cands):
    """What one parity of a case must give: per-lane loads, minima, takes."""
    lanes, ci = [], 0
    for lane in range(64):
        if (mask >> lane) & 1:
            cost, bits, dist, cbp, single, last, mvx, mvy = cands[ci]
            lanes.append((cost, bits | dist << 15, cbp | single << 16 | (last + 1) << 24, (mvx & 0xFFFF) | (mvy & 0xFFFF) << 16, ci))
            ci += 1
        else:
            lanes.append((DMAX, None, None, None, KMAX))
    minima, takes = [], []
    for j in range(NSEG):
        row = [(lanes[l][0], l) for l in range(16 * j, 16 * j + 16) if (mask >> l) & 1]
        if not row:
            minima.append((DMAX, -1))
            takes.append(None)
            continue
        m = min(c for c, _ in row)
        win = next(l for c, l in row if c == m)  # the sequential strict-< scan: the first of equal costs
        minima.append((m, win))
        cost, bits, dist, cbp, single, last, mvx, mvy = cands[lanes[win][4]]
        takes.append((m, single, dist, cbp, mvx, mvy, win & 15))
    return lanes, minima, takes


def test_records_selection_and_take(gpu):
    lib = ctypes.CDLL(LIB)
    assert lib.unit_rec_case_in() == CASE_IN and lib.unit_rec_case_out() == 2 * PAR_OUT
    cases = _cases()
    n = len(cases)
    a = np.zeros((n, CASE_IN), dtype=np.int32)
    for k, (mask, c0, c1) in enumerate(cases):
        a[k, 0:2] = np.array([mask & 0xFFFFFFFF, mask >> 32], dtype=np.uint32).view(np.int32)
        for par, cands in enumerate((c0, c1)):
            for ci, (cost, bits, dist, cbp, single, last, mvx, mvy) in enumerate(cands):
                a[k, 2 + (par * KMAX + ci) * CAND_IN:][:9] = [*_dwords(cost), bits, dist, cbp, single, last, mvx, mvy]
    out = np.full((n, 2, PAR_OUT), -7, dtype=np.int32)
    rc = lib.unit_rec(a.ctypes.data_as(ctypes.c_void_p), n, out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    u32 = lambda v: int(v) & 0xFFFFFFFF  # noqa: E731
    for k, (mask, c0, c1) in enumerate(cases):
        for par, cands in enumerate((c0, c1)):
            o = out[k, par]
            lanes, minima, takes = _expect(mask, cands)
            where = f"case {k} (mask {mask:#018x}) parity {par}"
            for lane, (cost, bd, meta, mv, ci) in enumerate(lanes):
                g = o[lane * LANE_OUT:(lane + 1) * LANE_OUT]
                assert (int(g[0]), int(g[1])) == _dwords(cost) and int(g[5]) == ci, f"{where} lane {lane}: cost / candidate"
                if bd is not None:
                    assert (u32(g[2]), u32(g[3]), u32(g[4])) == (bd, meta, mv), f"{where} lane {lane}: record words"
            om = o[64 * LANE_OUT:]
            ot = om[NSEG * 3:]
            for j in range(NSEG):
                m, win = minima[j]
                assert (int(om[3 * j]), int(om[3 * j + 1]), int(om[3 * j + 2])) == (*_dwords(m), win), f"{where} step {j}: minimum"
                t = [int(x) for x in ot[j * TAKE_OUT:(j + 1) * TAKE_OUT]]
                if takes[j] is None:
                    assert t == [*_dwords(-1.0), -1, -1, -1, -1, -1, -1], f"{where} step {j}: nothing to take"
                else:
                    cost, single, dist, cbp, mvx, mvy, pt = takes[j]
                    assert t == [*_dwords(cost), single, dist, cbp, mvx, mvy, pt], f"{where} step {j}: take"
    # vacuity guards: the properties named above are among the cases
    exp = [_expect(m, c) for m, c0, c1 in cases for c in (c0, c1)]
    assert any(win == -1 for _, mi, _ in exp for _, win in mi)  # an absent step
    assert any(m == 0.0 for _, mi, _ in exp for m, win in mi if win >= 0)
    assert any(m == DMAX for _, mi, _ in exp for m, win in mi if win >= 0)  # the largest double as a real cost
    assert any(bin(m).count("1") == KMAX for m, _, _ in cases)
    ties = 0
    for (m, c0, c1), par in ((c, p) for c in cases for p in (0, 1)):
        lanes, minima, _ = _expect(m, (c0, c1)[par])
        for j, (mn, win) in enumerate(minima):
            ties += win >= 0 and sum(1 for l in range(16 * j, 16 * j + 16) if (m >> l) & 1 and lanes[l][0] == mn) > 1
    assert ties >= 4
    assert all(any(len({mi[j][1] >= 0 for _, mi, _ in exp}) == 2 for _ in (0,)) for j in range(NSEG))  # every row both held and absent


def test_mask_with_too_many_lanes_is_refused():
    """The wrapper's own guard (host only: nothing is launched)."""
    lib = ctypes.CDLL(LIB)
    a = np.zeros((1, CASE_IN), dtype=np.int32)
    a[0, 0] = -1
    a[0, 1] = 1
    out = np.zeros((1, 2, PAR_OUT), dtype=np.int32)
    assert lib.unit_rec(a.ctypes.data_as(ctypes.c_void_p), 1, out.ctypes.data_as(ctypes.c_void_p)) == 10
