"""The candidate slot of the partition search on the GPU (hl_mbcore.h
put_cand, CandSlot): the device path forms a candidate's two plane offsets
from the per-phase table the MB start leaves in LDS and the memo key part
from its clamped displacement; the quads that miss the memo read exactly
these two offsets.  Every field against the host formula restated here, on a
virtual 4096x2304 picture (no plane is read): all 16 quarter-pel phases,
origins clamped at each picture edge, and displacements outside +-1024,
which no golden stream reaches (the memo's bypass).  Tolerance: none."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gpu_unit", "libhl_unit_cand.so")
W, H, PAD = 4096, 2304, 40
PSTRIDE = (W + 2 * PAD + 63) & ~63
PLSZ = PSTRIDE * (H + 2 * PAD)
# kQpelTab (8.4.2.2.1 as interpol.h computes it): plane1, dx1, dy1, plane2 (-1: none), dx2, dy2 per phase (mvy & 3) << 2 | (mvx & 3)
QPEL = [(0, 0, 0, -1, 0, 0), (0, 0, 0, 1, 0, 0), (1, 0, 0, -1, 0, 0), (0, 1, 0, 1, 0, 0),
        (0, 0, 0, 2, 0, 0), (1, 0, 0, 2, 0, 0), (1, 0, 0, 3, 0, 0), (1, 0, 0, 2, 1, 0),
        (2, 0, 0, -1, 0, 0), (2, 0, 0, 3, 0, 0), (3, 0, 0, -1, 0, 0), (3, 0, 0, 2, 1, 0),
        (0, 0, 1, 2, 0, 0), (2, 0, 0, 1, 0, 1), (3, 0, 0, 1, 0, 1), (2, 1, 0, 1, 0, 1)]


def _clip3(lo, hi, v):
    return lo if v < lo else (hi if v > hi else v)


def _expect(xl, yl, xo, yo, mvx, mvy, pt):
    ph = ((mvy & 3) << 2) | (mvx & 3)
    p1, dx1, dy1, p2, dx2, dy2 = QPEL[ph]
    x = _clip3(-17, W + 17, xl + xo + (mvx >> 2)) + PAD
    y = _clip3(-17, H + 17, yl + yo + (mvy >> 2)) + PAD
    off1 = p1 * PLSZ + (y + dy1) * PSTRIDE + x + dx1
    off2 = off1 if p2 < 0 else p2 * PLSZ + (y + dy2) * PSTRIDE + x + dx2
    dx, dy = x - PAD - (xl + xo), y - PAD - (yl + yo)  # the clamped displacement: the memo key's candidate part
    fit = -1024 <= dx <= 1023 and -1024 <= dy <= 1023
    kbase = (1 << 26) | (ph << 22) | ((dy & 0x7FF) << 11) | (dx & 0x7FF) if fit else 0
    return [off1, off2, mvx, mvy, pt | (kbase << 4)]


def _cases():
    rng = np.random.default_rng(88)
    cases = []
    origins = [(0, 0), (W - 16, 0), (0, H - 16), (W - 16, H - 16), (1920, 1088), (2048, 1152)]
    for ph in range(16):  # every phase at every origin, small displacements both ways
        for k, (xl, yl) in enumerate(origins):
            ix, iy = int(rng.integers(-20, 21)), int(rng.integers(-20, 21))
            cases.append((xl, yl, 4 * (k & 3), 4 * ((k >> 1) & 3), 4 * ix + (ph & 3), 4 * iy + (ph >> 2), ph % 9))
    for xl, yl in origins:  # windows over the [-17, W + 17] x [-17, H + 17] clamp
        for ix, iy in ((-40, 3), (5, -33), (60, 60), (-17, -17), (-18, -18), (33, 17), (34, 18)):
            cases.append((xl, yl, 8, 4, 4 * ix + 1, 4 * iy + 2, 4))
    for ix, iy in ((1023, 0), (1024, 0), (-1024, 5), (-1025, 5), (0, 1024), (3, -1025), (1500, -1500), (-2040, 1100)):
        for ph in (0, 5, 15):  # displacements at and beyond the key's +-1024 (inside the picture: no clamp)
            cases.append((2048, 1152, 4, 12, 4 * ix + (ph & 3), 4 * iy + (ph >> 2), 8))
    return cases


def test_slot_matches_host_formula(gpu):
    lib = ctypes.CDLL(LIB)
    cases = _cases()
    n = len(cases)
    a = np.array(cases, dtype=np.int32)
    out = np.zeros((n, 5), dtype=np.int32)
    rc = lib.unit_cand(W, H, PSTRIDE, PLSZ, a.ctypes.data_as(ctypes.c_void_p), n, out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    want = np.array([_expect(*c) for c in cases], dtype=np.int64).astype(np.int32)
    bad = np.nonzero((out != want).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} of {n} slots differ; first: case {cases[bad[0]]} got {out[bad[0]].tolist()} want {want[bad[0]].tolist()}"
    # vacuity guards: the bypass, the clamp and every phase are among the cases
    keyed = (want[:, 4].astype(np.int64) & 0xFFFFFFFF) >> 4
    assert (keyed == 0).any() and (keyed != 0).any()
    assert len({(c[5] & 3) << 2 | (c[4] & 3) for c in cases}) == 16
    assert any(_clip3(-17, W + 17, c[0] + c[2] + (c[4] >> 2)) != c[0] + c[2] + (c[4] >> 2) for c in cases)
