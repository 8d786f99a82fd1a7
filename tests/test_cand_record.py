"""The candidate record of an evaluation pass (hl_mbcore.h CandRec): a
candidate's cost, bits, distortion, Single_ctr sum, coded-block pattern and
last counter in 16 bytes, bd = bits | dist << 15 and meta = cbp | single << 16
| (last + 1) << 24.  The pack and unpack functions the kernels, the emulator
and the selection share, through a host library of their own
(tests/emu/hl_rec_emu.hip): every field at both ends of its range, together
and one at a time; the round trip exact, the stored words as the layout
says, no field reaching its neighbour.  Tolerance: none."""
import ctypes
import itertools
import os
import struct

import numpy as np
import pytest

LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu", "libhl_rec_emu.so")
# (low end, high end) of every field: bits < 2^15 and dist < 2^17 over a whole
# MB, cbp one bit per 4x4 block, single 16 blocks' counters of at most 14,
# last -1 (no block coded) .. 15
ENDS = {"bits": (0, (1 << 15) - 1), "dist": (0, (1 << 17) - 1), "cbp": (0, 0xFFFF), "single": (0, 224), "last": (-1, 15)}
NAMES = list(ENDS)
COSTS = (0.0, 1.0, 123456.789, 1.7976931348623157e308)


@pytest.fixture(scope="module")
def lib():
    so = ctypes.CDLL(LIB)
    so.rec_roundtrip.argtypes = [ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p]
    so.rec_roundtrip.restype = None
    return so


def _roundtrip(lib, fields, cost):
    a = np.array(fields, dtype=np.int32)
    rec = np.zeros(4, dtype=np.uint32)
    out = np.zeros(5, dtype=np.int32)
    lib.rec_roundtrip(a.ctypes.data, cost, rec.ctypes.data, out.ctypes.data)
    return [int(x) for x in rec], [int(x) for x in out]


def _words(fields, cost):
    bits, dist, cbp, single, last = fields
    lo, hi = struct.unpack("<II", struct.pack("<d", cost))
    return [lo, hi, bits | dist << 15, cbp | single << 16 | (last + 1) << 24]


def test_layout_is_one_16_byte_record(lib):
    assert lib.rec_sizeof() == 16
    assert lib.rec_lds_bytes() == 2 * 32 * 16  # both parities of kMaxCand records: 1 024 B


def test_every_combination_of_range_ends(lib):
    for k, combo in enumerate(itertools.product(*(ENDS[n] for n in NAMES))):
        cost = COSTS[k % len(COSTS)]
        rec, out = _roundtrip(lib, combo, cost)
        assert out == list(combo), f"fields {dict(zip(NAMES, combo))} came back as {dict(zip(NAMES, out))}"
        assert rec == _words(combo, cost), f"fields {dict(zip(NAMES, combo))}: stored words {[hex(w) for w in rec]}"


@pytest.mark.parametrize("name", NAMES)
def test_one_field_at_a_time(lib, name):
    """One field at its high end, all others at their low end, and the
    reverse: the others must read back untouched (no leak either way)."""
    i = NAMES.index(name)
    low = [ENDS[n][0] for n in NAMES]
    high = [ENDS[n][1] for n in NAMES]
    for base, other in ((low, high), (high, low)):
        f = list(base)
        f[i] = other[i]
        rec, out = _roundtrip(lib, f, 2.5)
        assert out == f, f"{name} alone at {f[i]}: {dict(zip(NAMES, out))}"
        assert rec == _words(f, 2.5)


def test_values_inside_the_ranges(lib):
    rng = np.random.default_rng(9)
    for _ in range(2000):
        f = [int(rng.integers(ENDS[n][0], ENDS[n][1] + 1)) for n in NAMES]
        cost = float(rng.random() * 1e6)
        rec, out = _roundtrip(lib, f, cost)
        assert out == f
        assert rec == _words(f, cost)
