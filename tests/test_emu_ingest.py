"""The frame ingest's per-tile code (hartallo_amd/csrc/hl_ingest.h in_tile, what
every lane of k_ingest runs) built for the host (tests/emu/libhl_ingest_emu.so)
against the numpy model of its definition (tests/in_testlib.py, coefficients
derived there with fractions.Fraction).  Everything is integer: exact equality.
"""
import ctypes
import os

import numpy as np
import pytest

import in_testlib as it
from hl_testlib import ROOT

LIB = os.path.join(ROOT, "tests", "emu", "libhl_ingest_emu.so")

# 1040 x 32: one tile column wider and (more than) one tile row taller than a
# workgroup's 64 x 4 tiles of 16 x 2 samples (1024 x 8)
SIZES = [(16, 16), (48, 32), (176, 144), (1040, 32)]
TABLES = [(it.BT601, it.LIMITED), (it.BT601, it.FULL), (it.BT709, it.LIMITED), (it.BT709, it.FULL)]
CORNERS = [(r, g, b) for r in (0, 255) for g in (0, 255) for b in (0, 255)]


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(LIB)
    lib.in_emu_coef.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]
    lib.in_emu_frame.argtypes = [ctypes.c_int32] * 5 + [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64)] + [ctypes.c_void_p] * 3
    lib.in_emu_lanes.argtypes = [ctypes.POINTER(ctypes.c_int32)] * 2
    return lib


def emu(lib, fmt, planes, w, h, matrix=0, rng=0):
    """planes: 2-D uint8 arrays (possibly strided views) -> dense Y, U, V"""
    y = np.full((h, w), 0xEE, np.uint8)
    u = np.full((h // 2, w // 2), 0xEE, np.uint8)
    v = np.full((h // 2, w // 2), 0xEE, np.uint8)
    n = len(planes)
    ptrs = (ctypes.c_void_p * 3)(*[p.ctypes.data for p in planes])
    pitches = (ctypes.c_int64 * 3)(*[p.strides[0] for p in planes])
    assert all(p.strides[1] == 1 for p in planes) and n <= 3
    assert lib.in_emu_frame(fmt, matrix, rng, w, h, ptrs, pitches, y.ctypes.data, u.ctypes.data, v.ctypes.data) == 0
    return y, u, v


def same(got, want):
    for name, g, w in zip("YUV", got, want):
        assert g.shape == w.shape
        assert np.array_equal(g, w), f"{name}: {np.count_nonzero(g != w)} samples differ, first at {np.argwhere(g != w)[0].tolist()}"


@pytest.mark.parametrize("key", TABLES, ids=["601l", "601f", "709l", "709f"])
def test_coefficient_tables(lib, key):
    """the header's constexpr derivation, the Fraction derivation and the issue's literal tables agree"""
    out = (ctypes.c_int32 * 10)()
    assert lib.in_emu_coef(key[0], key[1], out) == 0
    got = (tuple(out[0:3]), tuple(out[3:6]), tuple(out[6:9]), out[9])
    assert got == it.TABLES[key]
    assert it.coefficients(*key) == it.TABLES[key]
    assert sum(got[1]) == 0 and sum(got[2]) == 0  # grey gives exactly 128
    assert lib.in_emu_coef(2, 0, out) == -1 and lib.in_emu_coef(0, 2, out) == -1


def test_workgroup_tile_is_what_the_sizes_cross(lib):
    x, y = ctypes.c_int32(), ctypes.c_int32()
    lib.in_emu_lanes(ctypes.byref(x), ctypes.byref(y))
    assert (16 * x.value, 2 * y.value) == (1024, 8)
    assert SIZES[-1][0] == 16 * x.value + 16 and SIZES[-1][1] >= 2 * y.value + 2


@pytest.mark.parametrize("pad", [0, 24], ids=["dense", "padded"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", ["i420", "nv12"])
def test_yuv_formats_are_identities(lib, fmt, size, pad):
    w, h = size
    rng = np.random.default_rng(w * 31 + h + pad)
    yuv = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((h, w), (h // 2, w // 2), (h // 2, w // 2))]
    outs = []
    for fill in (0xA5, 0x3C):
        planes = [it.padded(p, pad if p.shape[1] == w else pad // 2 if fmt == "i420" else pad, fill) for p in it.pack(it.FORMATS[fmt], yuv)]
        outs.append(emu(lib, it.FORMATS[fmt], planes, w, h))
        same(outs[-1], yuv)
    same(outs[0], outs[1])


@pytest.mark.parametrize("pad", [0, 20], ids=["dense", "padded"])
@pytest.mark.parametrize("key", TABLES, ids=["601l", "601f", "709l", "709f"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("fmt", ["rgb24", "rgba32", "rgbp"])
def test_rgb_noise_matches_the_model(lib, fmt, size, key, pad):
    w, h = size
    rng = np.random.default_rng(w * 17 + h + 5 * key[0] + key[1])
    rgb = [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(3)]
    want = it.rgb_to_i420(*rgb, *key)
    outs = []
    for fill in (0xA5, 0x3C):  # what lies between the rows reaches no output
        planes = [it.padded(p, pad, fill) for p in it.pack(it.FORMATS[fmt], rgb)]
        outs.append(emu(lib, it.FORMATS[fmt], planes, w, h, *key))
        same(outs[-1], want)
    same(outs[0], outs[1])


@pytest.mark.parametrize("key", TABLES, ids=["601l", "601f", "709l", "709f"])
@pytest.mark.parametrize("fmt", ["rgb24", "rgba32", "rgbp"])
def test_grey_gives_neutral_chroma(lib, fmt, key):
    w, h = 48, 32
    for g in (0, 1, 127, 255):
        rgb = [np.full((h, w), g, np.uint8)] * 3
        y, u, v = emu(lib, it.FORMATS[fmt], it.pack(it.FORMATS[fmt], rgb), w, h, *key)
        assert np.all(u == 128) and np.all(v == 128), (g, int(u[0, 0]), int(v[0, 0]))
        same((y, u, v), it.rgb_to_i420(*rgb, *key))
        lo, hi = (0, 255) if key[1] == it.FULL else (16, 235)
        assert int(y[0, 0]) == {0: lo, 255: hi}.get(g, int(y[0, 0]))


@pytest.mark.parametrize("key", TABLES, ids=["601l", "601f", "709l", "709f"])
@pytest.mark.parametrize("fmt", ["rgb24", "rgba32", "rgbp"])
def test_rgb_corners(lib, fmt, key):
    """the eight corners of the RGB cube as flat pictures, and a 2x2 checker of
    them (every block mixes four corners); pure blue and pure red in full
    range reach 256 before the min"""
    w, h = 48, 32
    for c in CORNERS:
        rgb = [np.full((h, w), x, np.uint8) for x in c]
        got = emu(lib, it.FORMATS[fmt], it.pack(it.FORMATS[fmt], rgb), w, h, *key)
        same(got, it.rgb_to_i420(*rgb, *key))
        if key[1] == it.FULL and c == (0, 0, 255):
            assert int(got[1][0, 0]) == 255  # 256 clipped by the min
        if key[1] == it.FULL and c == (255, 0, 0):
            assert int(got[2][0, 0]) == 255
        if key[1] == it.LIMITED:
            assert 16 <= int(got[1].min()) and int(got[1].max()) <= 240 and 16 <= int(got[2].min()) and int(got[2].max()) <= 240
    idx = (np.arange(h)[:, None] * 3 + np.arange(w)[None, :] * 5 + (np.arange(h)[:, None] // 2) * (np.arange(w)[None, :] // 2)) % 8
    rgb = [np.array([c[k] for c in CORNERS], np.uint8)[idx] for k in range(3)]
    same(emu(lib, it.FORMATS[fmt], it.pack(it.FORMATS[fmt], rgb), w, h, *key), it.rgb_to_i420(*rgb, *key))


def test_refused_descriptions(lib):
    p = np.zeros((16, 48), np.uint8)
    out = np.zeros(16 * 16, np.uint8)
    ptrs = (ctypes.c_void_p * 3)(p.ctypes.data, p.ctypes.data, p.ctypes.data)
    o = out.ctypes.data

    def call(fmt, w, h, pitches, planes=ptrs):
        return lib.in_emu_frame(fmt, 0, 0, w, h, planes, (ctypes.c_int64 * 3)(*pitches), o, o, o)

    assert call(it.RGB24, 16, 16, (48, 0, 0)) == 0
    assert call(5, 16, 16, (0, 0, 0)) == -1          # unknown format
    assert call(it.RGB24, 16, 16, (47, 0, 0)) == -1   # pitch below row bytes
    assert call(it.RGB24, 16, 16, (-48, 0, 0)) == -1  # negative pitch
    assert call(it.RGB24, 24, 16, (0, 0, 0)) == -1    # width no multiple of 16
    assert call(it.NV12, 16, 16, (0, 0, 0), (ctypes.c_void_p * 3)(p.ctypes.data, None, None)) == -1  # a plane the format needs
