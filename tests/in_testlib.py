"""Test support for the frame ingest (hartallo_amd/csrc/hl_ingest.h): a numpy
model of its definition -- the coefficients derived here with
fractions.Fraction from Kr, Kb and the range, without reading the header --
and helpers that lay frames out in memory.  TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

from fractions import Fraction
from math import floor

import numpy as np

I420, NV12, RGB24, RGBA32, RGBP = range(5)
FORMATS = {"i420": I420, "nv12": NV12, "rgb24": RGB24, "rgba32": RGBA32, "rgbp": RGBP}
BT601, BT709 = 0, 1
LIMITED, FULL = 0, 1
KR_KB = {BT601: (Fraction(299, 1000), Fraction(114, 1000)), BT709: (Fraction(2126, 10000), Fraction(722, 10000))}

# the four tables as the issue states them: y, u, v, off
TABLES = {
    (BT601, LIMITED): ((16829, 33039, 6416), (-9714, -19070, 28784), (28784, -24103, -4681), 16),
    (BT601, FULL): ((19595, 38470, 7471), (-11058, -21710, 32768), (32768, -27439, -5329), 0),
    (BT709, LIMITED): ((11966, 40254, 4064), (-6596, -22188, 28784), (28784, -26145, -2639), 16),
    (BT709, FULL): ((13933, 46871, 4732), (-7509, -25259, 32768), (32768, -29763, -3005), 0),
}


def rnd(x: Fraction) -> int:
    """round-half-up of an exact rational"""
    return floor(x + Fraction(1, 2))


def coefficients(matrix: int, rng: int):
    """(y, u, v, off) from Kr, Kb and the range, in exact rationals"""
    kr, kb = KR_KB[matrix]
    s = Fraction(1 << 16) if rng == FULL else Fraction(219 * (1 << 16), 255)
    c = Fraction(1 << 16) if rng == FULL else Fraction(224 * (1 << 16), 255)
    yr, yb = rnd(kr * s), rnd(kb * s)
    yg = rnd(s) - yr - yb
    ub = rnd(c / 2)
    ur = -rnd(kr / (2 * (1 - kb)) * c)
    ug = -(ur + ub)
    vr = rnd(c / 2)
    vb = -rnd(kb / (2 * (1 - kr)) * c)
    vg = -(vr + vb)
    return (yr, yg, yb), (ur, ug, ub), (vr, vg, vb), 0 if rng == FULL else 16


def rgb_to_i420(r, g, b, matrix=BT601, rng=LIMITED):
    """R, G, B planes (H, W) uint8 -> dense Y (H, W), U, V (H/2, W/2) uint8"""
    cy, cu, cv, off = coefficients(matrix, rng)
    R, G, B = (p.astype(np.int64) for p in (r, g, b))
    y = (cy[0] * R + cy[1] * G + cy[2] * B + (off << 16) + (1 << 15)) >> 16
    assert y.min() >= 0 and y.max() <= 255
    h, w = r.shape

    def s4(p):
        return p.reshape(h // 2, 2, w // 2, 2).sum(axis=(1, 3))

    SR, SG, SB = s4(R), s4(G), s4(B)
    out = [y.astype(np.uint8)]
    for c in (cu, cv):
        acc = c[0] * SR + c[1] * SG + c[2] * SB + (128 << 18) + (1 << 17)
        assert acc.min() >= 0 and acc.max() <= (1 << 26)  # 2^26 itself: pure blue or red in full range, 256 before the min
        out.append(np.minimum(255, acc >> 18).astype(np.uint8))
    return tuple(out)


def padded_buffer(plane: np.ndarray, pad: int, fill: int = 0xA5):
    """(buffer, pitch): `plane` (rows, bytes) laid out with `pad` bytes between
    the rows (filled with `fill`) and nothing after the last row."""
    rows, rb = plane.shape
    pitch = rb + pad
    buf = np.full(pitch * (rows - 1) + rb, fill, np.uint8)
    np.lib.stride_tricks.as_strided(buf, (rows, rb), (pitch, 1))[...] = plane
    return buf, pitch


def padded(plane: np.ndarray, pad: int, fill: int = 0xA5) -> np.ndarray:
    """`plane` as a strided view of its padded_buffer"""
    buf, pitch = padded_buffer(plane, pad, fill)
    return np.lib.stride_tricks.as_strided(buf, plane.shape, (pitch, 1))


def pack(fmt: int, planes):
    """The planes a format is made of, as dense (rows, bytes) arrays: from Y, U,
    V for I420 / NV12 and from R, G, B for the RGB formats (RGBA32: alpha noise)."""
    a, b, c = planes
    if fmt == I420:
        return [a, b, c]
    if fmt == NV12:
        return [a, np.stack([b, c], axis=-1).reshape(b.shape[0], -1)]
    if fmt == RGB24:
        return [np.stack([a, b, c], axis=-1).reshape(a.shape[0], -1)]
    if fmt == RGBA32:
        alpha = np.random.default_rng(a.shape[0] * 7 + a.shape[1]).integers(0, 256, a.shape, dtype=np.uint8)
        return [np.stack([a, b, c, alpha], axis=-1).reshape(a.shape[0], -1)]
    return [a, b, c]


def split(frame: np.ndarray, w: int, h: int):
    """a concatenated Y|U|V frame (hartallo_amd.synth) as three 2-D planes"""
    n = w * h
    return frame[:n].reshape(h, w), frame[n:n + n // 4].reshape(h // 2, w // 2), frame[n + n // 4:n * 3 // 2].reshape(h // 2, w // 2)
