"""Test support for the display size (hl_amd_set_display_size):
numpy models of the edge padding and of the quality metric over a window, an
exp-Golomb SPS parser, and the handle on the host build
(tests/emu/libhl_display_emu.so).  TEST INFRASTRUCTURE ONLY.

The models follow the definitions, not the kernels: the padding is
np.pad(..., mode="edge") of the planes in_testlib gives for the dw x dh frame;
the quality model crops both planes to the window and then sums.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

import in_testlib as it
from hl_testlib import ROOT
from q_testlib import C1, C2

DISPLAY_EMU_LIB = os.path.join(ROOT, "tests", "emu", "libhl_display_emu.so")


# ---- SPS ------------------------------------------------------------------------
def nals(stream: bytes):
    """the NAL units of an Annex B stream with 3-byte start codes, escaped as they are"""
    return stream.split(b"\x00\x00\x01")[1:]


def unescape(nal: bytes) -> bytes:
    out, zeros = bytearray(), 0
    for b in nal:
        if zeros >= 2 and b == 3:
            zeros = 0
            continue
        out.append(b)
        zeros = zeros + 1 if b == 0 else 0
    return bytes(out)


def needs_no_escape(nal: bytes) -> bool:
    """no 00 00 0[0-3] in the NAL as it is sent, other than an escape's own 00 00 03"""
    for i in range(len(nal) - 2):
        if nal[i] == 0 and nal[i + 1] == 0 and nal[i + 2] <= 3:
            if nal[i + 2] != 3 or (i + 3 < len(nal) and nal[i + 3] > 3):
                return False
    return True


class Bits:
    def __init__(self, data: bytes):
        self.bits = "".join(f"{b:08b}" for b in data)
        self.at = 0

    def u(self, n: int) -> int:
        v = int(self.bits[self.at:self.at + n], 2)
        self.at += n
        return v

    def ue(self) -> int:
        z = 0
        while self.u(1) == 0:
            z += 1
        return (1 << z) - 1 + (self.u(z) if z else 0)


def parse_sps(nal: bytes) -> dict:
    """Every field of a Baseline SPS as write_stream_headers writes it (7.3.2.1.1)."""
    b = Bits(unescape(nal))
    s = {"header": b.u(8), "profile_idc": b.u(8), "constraints": b.u(8), "level_idc": b.u(8)}
    for k in ("sps_id", "log2_max_frame_num_minus4", "poc_type", "max_num_ref_frames"):
        s[k] = b.ue()
    assert s["poc_type"] == 2
    s["gaps"] = b.u(1)
    s["width_mbs_minus1"], s["height_mbs_minus1"] = b.ue(), b.ue()
    s["frame_mbs_only"], s["direct_8x8"], s["cropping"] = b.u(1), b.u(1), b.u(1)
    s["crop"] = tuple(b.ue() for _ in range(4)) if s["cropping"] else None
    s["vui"] = b.u(1)
    rest = b.bits[b.at:]
    assert rest == "1" + "0" * (len(rest) - 1) and len(rest) <= 8, rest  # rbsp_trailing_bits
    return s


# ---- padding ----------------------------------------------------------------------
def pad_edge(planes, w: int, h: int):
    """dense (y, u, v) of a dw x dh frame padded to w x h by edge replication"""
    y, u, v = planes
    dh, dw = y.shape
    out = [np.pad(y, ((0, h - dh), (0, w - dw)), mode="edge")]
    for p in (u, v):
        out.append(np.pad(p, ((0, h // 2 - dh // 2), (0, w // 2 - dw // 2)), mode="edge"))
    return tuple(np.ascontiguousarray(p) for p in out)


def model_planes(fmt: int, content, key, w: int, h: int):
    """The coded w x h planes of a frame whose content (Y, U, V or R, G, B planes of
    the display size) is in format fmt: in_testlib's planes of the frame, padded."""
    if fmt in (it.I420, it.NV12):
        return pad_edge(content, w, h)
    return pad_edge(it.rgb_to_i420(*content, *key), w, h)


def content_planes(fmt: int, dw: int, dh: int, kind: str, seed: int):
    """(Y, U, V) or (R, G, B) planes of a dw x dh frame: noise, or a quiet frame
    whose last column and row (and the chroma's) differ strongly from their
    neighbours, so that a clamp one sample off shows."""
    rng = np.random.default_rng(seed)
    yuv = fmt in (it.I420, it.NV12)
    shapes = [(dh, dw), (dh // 2, dw // 2), (dh // 2, dw // 2)] if yuv else [(dh, dw)] * 3
    if kind == "noise":
        return tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in shapes)
    out = []
    for c, s in enumerate(shapes):
        p = rng.integers(100, 140, s, dtype=np.uint8)
        step = 1 if (yuv and c) else 2  # (an RGB or luma edge is a 2x2 block wide as far as chroma goes)
        p[:, -1] = 250 - 40 * c
        p[:, -1 - step:-1] = 5 + 30 * c
        p[-1, :] = 10 + 50 * c
        p[-1 - step:-1, :] = 240 - 20 * c
        p[-1, -1] = 77 + c
        out.append(p)
    return tuple(out)


def display_emu_lib():
    lib = ctypes.CDLL(DISPLAY_EMU_LIB)
    i32 = ctypes.c_int32
    lib.display_emu_frame.argtypes = [i32] * 7 + [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64)] + [ctypes.c_void_p] * 3
    lib.display_emu_frame.restype = i32
    lib.display_emu_tiles.argtypes = [i32] * 4 + [ctypes.POINTER(i32)] * 2
    lib.display_emu_edge_at.argtypes = [i32] * 5 + [ctypes.POINTER(i32)] * 2
    lib.display_emu_edge_at.restype = i32
    lib.display_emu_quality.argtypes = [ctypes.c_void_p, ctypes.c_void_p, i32, i32, i32, i32, ctypes.POINTER(ctypes.c_uint64),
                                        ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p]
    lib.display_emu_quality.restype = i32
    return lib


# ---- quality over a window ----------------------------------------------------------
def window_quality(a: np.ndarray, b: np.ndarray, ww: int, wh: int) -> dict:
    """The model on the top-left ww x wh samples of one plane pair: crop, then
    sum; the 8x8 windows (stride 4) are those wholly inside the crop."""
    A, B = a[:wh, :ww].astype(np.int64), b[:wh, :ww].astype(np.int64)
    sse = int(((A - B) ** 2).sum())
    nbx, nby = ww // 4, wh // 4
    q, n = 0, 0
    for by in range(nby - 1):
        for bx in range(nbx - 1):
            wa, wb = A[4 * by:4 * by + 8, 4 * bx:4 * bx + 8], B[4 * by:4 * by + 8, 4 * bx:4 * bx + 8]
            s1, s2, ss, s12 = int(wa.sum()), int(wb.sum()), int((wa * wa + wb * wb).sum()), int((wa * wb).sum())
            num = (2 * s1 * s2 + C1) * (2 * (64 * s12 - s1 * s2) + C2)
            den = (s1 * s1 + s2 * s2 + C1) * (64 * ss - s1 * s1 - s2 * s2 + C2)
            assert den > 0
            q += (num << 30) // den
            n += 1
    assert n == max(0, nbx - 1) * max(0, nby - 1)
    return {"sse": sse, "samples": ww * wh, "ssim_q30": q, "windows": n}


def window_mb_sse(a: np.ndarray, b: np.ndarray, ww: int, wh: int) -> np.ndarray:
    """sum (a - b)^2 over each 16x16 macroblock's part inside the window, uint32 (h / 16, w / 16)"""
    h, w = a.shape
    d = a.astype(np.int64) - b.astype(np.int64)
    d[wh:, :] = 0
    d[:, ww:] = 0
    return (d * d).reshape(h // 16, 16, w // 16, 16).sum(axis=(1, 3)).astype(np.uint32)


def picture_window_quality(src, rec, dw: int, dh: int) -> dict:
    """src, rec: (y, u, v) planes of the coded size; the integers of
    hl_amd_quality_t over the display rectangle as lists of three, and the luma
    SSE of each macroblock's display part."""
    per = [window_quality(a, b, dw >> (c > 0), dh >> (c > 0)) for c, (a, b) in enumerate(zip(src, rec))]
    out = {k: [p[k] for p in per] for k in ("sse", "samples", "ssim_q30", "windows")}
    out["mb"] = window_mb_sse(src[0], rec[0], dw, dh)
    return out
