"""Test support for the quality metric (hl_amd_set_quality): a
numpy model of the definition and the handle on the kernel's host build.
TEST INFRASTRUCTURE ONLY.

The model follows the definition, not the kernel: whole-plane block sums in
int64, window sums by adding four shifted block arrays, and the division in
Python integers ((num << 30) // den: a floor, num may be negative).
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from hl_testlib import ROOT

QUALITY_EMU_LIB = os.path.join(ROOT, "tests", "emu", "libhl_quality_emu.so")
C1, C2 = 416, 235963


def block_sums(a: np.ndarray, b: np.ndarray):
    """(s1, s2, ss, s12) per 4x4 block, int64 arrays of shape (h / 4, w / 4)."""
    h, w = a.shape
    assert b.shape == a.shape and h % 8 == 0 and w % 8 == 0 and a.dtype == np.uint8 and b.dtype == np.uint8
    A = a.astype(np.int64).reshape(h // 4, 4, w // 4, 4)
    B = b.astype(np.int64).reshape(h // 4, 4, w // 4, 4)
    return A.sum(axis=(1, 3)), B.sum(axis=(1, 3)), (A * A + B * B).sum(axis=(1, 3)), (A * B).sum(axis=(1, 3))


def window_terms(a: np.ndarray, b: np.ndarray):
    """(num, den) of every window, int64 arrays of shape (h / 4 - 1, w / 4 - 1)."""
    S1, S2, SS, S12 = (x[:-1, :-1] + x[:-1, 1:] + x[1:, :-1] + x[1:, 1:] for x in block_sums(a, b))
    var = 64 * SS - S1 * S1 - S2 * S2
    cov = 64 * S12 - S1 * S2
    return (2 * S1 * S2 + C1) * (2 * cov + C2), (S1 * S1 + S2 * S2 + C1) * (var + C2)


def plane_quality(a: np.ndarray, b: np.ndarray) -> dict:
    """The model on one plane pair (h x w uint8; a = source, b = reconstruction)."""
    h, w = a.shape
    s1, s2, ss, s12 = block_sums(a, b)
    num, den = window_terms(a, b)
    assert (den > 0).all()
    q = sum((int(n) << 30) // int(d) for n, d in zip(num.ravel().tolist(), den.ravel().tolist()))
    return {"sse": int((ss - 2 * s12).sum()), "samples": w * h, "ssim_q30": q, "windows": (w // 4 - 1) * (h // 4 - 1)}


def mb_sse(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """sum (a - b)^2 per 16x16 macroblock, uint32 (h / 16, w / 16)."""
    h, w = a.shape
    d = a.astype(np.int64) - b.astype(np.int64)
    return (d * d).reshape(h // 16, 16, w // 16, 16).sum(axis=(1, 3)).astype(np.uint32)


def planes(frame: np.ndarray, w: int, h: int):
    """(y, u, v) of a planar Y|U|V frame."""
    n = w * h
    return (np.ascontiguousarray(frame[:n]).reshape(h, w), np.ascontiguousarray(frame[n:n + n // 4]).reshape(h // 2, w // 2),
            np.ascontiguousarray(frame[n + n // 4:n + n // 2]).reshape(h // 2, w // 2))


def picture_quality(src: np.ndarray, rec: np.ndarray, w: int, h: int) -> dict:
    """The model on a picture (planar Y|U|V frames): the integers of
    hl_amd_quality_t as lists of three, and the luma SSE per macroblock."""
    per = [plane_quality(a, b) for a, b in zip(planes(src, w, h), planes(rec, w, h))]
    out = {k: [p[k] for p in per] for k in ("sse", "samples", "ssim_q30", "windows")}
    out["mb"] = mb_sse(planes(src, w, h)[0], planes(rec, w, h)[0])
    return out


def assert_quality(got: dict, mb: np.ndarray, want: dict, what=""):
    """got: Encoder.last_quality's dict, mb: Encoder.debug_quality_mb's array."""
    for k in ("sse", "samples", "ssim_q30", "windows"):
        assert list(got[k]) == want[k], (what, k, got[k], want[k])
    assert np.array_equal(mb, want["mb"]), (what, np.argwhere(mb != want["mb"])[:4])
    assert int(mb.astype(np.uint64).sum()) == want["sse"][0], what


def quality_emu_lib():
    lib = ctypes.CDLL(QUALITY_EMU_LIB)
    lib.quality_emu_plane.restype = ctypes.c_int32
    lib.quality_emu_plane.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint64),
                                      ctypes.POINTER(ctypes.c_int64), ctypes.c_void_p]
    lib.quality_emu_div30.restype = ctypes.c_int64
    lib.quality_emu_div30.argtypes = [ctypes.c_int64, ctypes.c_int64]
    return lib


def emu_plane(a: np.ndarray, b: np.ndarray, with_mb: bool = False):
    """(sse, ssim_q30[, mb]) from the host build of hl_quality.h."""
    h, w = a.shape
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    sse, q = ctypes.c_uint64(), ctypes.c_int64()
    mb = np.full((h // 16, w // 16), 0xDEADBEEF, np.uint32) if with_mb else None
    rc = quality_emu_lib().quality_emu_plane(a.ctypes.data, b.ctypes.data, w, h, ctypes.byref(sse), ctypes.byref(q),
                                             mb.ctypes.data if with_mb else None)
    assert rc == 0, rc
    return (sse.value, q.value, mb) if with_mb else (sse.value, q.value)
