"""The layer pyramid's per-span code (hartallo_amd/csrc/hl_pyramid.h pyr_span,
what every lane of k_pyramid runs) built for the host
(tests/emu/libhl_pyr_emu.so) against hartallo_amd.synth._down2 applied level
by level: the filter every SVC workload and golden of this project is made
with.  Exact equality on the three planes of every level."""
import ctypes
import os

import numpy as np
import pytest

from hartallo_amd import synth
from hl_testlib import ROOT

LIB = os.path.join(ROOT, "tests", "emu", "libhl_pyr_emu.so")

BASES = [(16, 16), (48, 16), (80, 48), (176, 144)]
# rows 1 1 1 1 / 0 0 0 0 / 1 1 1 0 / 0 0 0 0: 1 when rounded at every level, 0 as one 4x4 average
CRAFTED = np.array([[1, 1, 1, 1], [0, 0, 0, 0], [1, 1, 1, 0], [0, 0, 0, 0]], np.uint8)


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(LIB)
    lib.pyr_emu_plane.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p)]
    lib.pyr_emu_plane.restype = ctypes.c_int32
    return lib


def emu_levels(lib, plane, K):
    h, w = plane.shape
    src = np.ascontiguousarray(plane)
    out = [np.full((h >> (j + 1), w >> (j + 1)), 0xA5, np.uint8) for j in range(K)]
    ptrs = (ctypes.c_void_p * K)(*[o.ctypes.data for o in out])
    assert lib.pyr_emu_plane(src.ctypes.data, w, h, K, ptrs) == 0
    return out


def staged(plane, K):
    out = []
    for _ in range(K):
        plane = synth._down2(plane)
        out.append(plane)
    return out


def planes_of(kind, w, h, rng):
    shapes = [(h, w), (h // 2, w // 2), (h // 2, w // 2)]
    if kind == "random":
        return [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes]
    if kind == "all255":
        return [np.full(s, 255, np.uint8) for s in shapes]
    return [np.tile(CRAFTED, (s[0] // 4, s[1] // 4)) for s in shapes]


@pytest.mark.parametrize("kind", ["random", "all255", "crafted"])
@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("base", BASES, ids=lambda b: f"{b[0]}x{b[1]}")
def test_pyramid_matches_down2_staged(lib, base, K, kind):
    w, h = base[0] << K, base[1] << K
    rng = np.random.default_rng(1000 * K + base[0] + base[1])
    for c, p in enumerate(planes_of(kind, w, h, rng)):
        got, want = emu_levels(lib, p, K), staged(p, K)
        for j in range(K):
            assert got[j].shape == want[j].shape
            assert np.array_equal(got[j], want[j]), f"plane {c} level {j + 1}: {np.count_nonzero(got[j] != want[j])} samples differ"


def test_crafted_block_separates_staged_from_direct(lib):
    """The crafted block is 1 rounded level by level and 0 as one 4x4 average:
    a pyramid that averaged 2^K x 2^K samples at once would not pass."""
    p = np.tile(CRAFTED, (8, 8))
    lv = emu_levels(lib, p, 2)
    assert np.all(lv[1] == 1)
    direct = (p.astype(np.uint32).reshape(8, 4, 8, 4).sum(axis=(1, 3)) + 8) >> 4
    assert np.all(direct == 0)


def test_bad_geometry_refused(lib):
    p = np.zeros((16, 16), np.uint8)
    buf = np.zeros(256, np.uint8)
    out = (ctypes.c_void_p * 3)(*[buf.ctypes.data] * 3)
    assert lib.pyr_emu_plane(p.ctypes.data, 12, 16, 1, out) == -1  # width no multiple of 8
    assert lib.pyr_emu_plane(p.ctypes.data, 16, 12, 3, out) == -1  # height no multiple of 2^K
    assert lib.pyr_emu_plane(p.ctypes.data, 16, 16, 4, out) == -1  # more than 3 levels
