"""Test support for the access unit's display size (hl_amd_set_au_display_size,
DESIGN.md 6.13): the fixture of tests/golden/make_svc_display_golden.py and its
input, an exp-Golomb parser of the subset SPS, the numpy models (in_testlib's
planes, np.pad(mode="edge"), synth._down2 level by level) and the handle on the
host build of the wide-margin ingest (tests/emu/libhl_svc_display_emu.so).
TEST INFRASTRUCTURE ONLY.
"""
from __future__ import annotations

import ctypes
import functools
import json
import os

import numpy as np

import dp_testlib as dp
import in_testlib as it
from hl_testlib import ROOT

from hartallo_amd import synth

GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
GOLD = json.load(open(os.path.join(GOLDEN_DIR, "svc_display_golden.json")))
SVC_GOLD = json.load(open(os.path.join(GOLDEN_DIR, "svc_golden.json")))
EMU_LIB = os.path.join(ROOT, "tests", "emu", "libhl_svc_display_emu.so")
PYR_EMU_LIB = os.path.join(ROOT, "tests", "emu", "libhl_pyr_emu.so")


# ---- sizes --------------------------------------------------------------------------
def legal(layers: int, w: int, h: int, dw: int, dh: int) -> bool:
    """the issue's rule for the top layer's display size dw x dh in the top coded size w x h"""
    k = layers - 1
    return (dw % (2 << k) == 0 and dh % (2 << k) == 0 and w - (16 << k) < dw <= w and h - (16 << k) < dh <= h)


def legal_values(layers: int, w: int):
    """every legal display width (or height) of a top coded width (height) w"""
    k = layers - 1
    return [d for d in range(2 << k, w + 1, 2 << k) if d > w - (16 << k)]


# ---- headers --------------------------------------------------------------------------
def nal_type(nal: bytes) -> int:
    return nal[0] & 31


def parse_subset_sps(nal: bytes) -> dict:
    """Every field of a subset SPS as put_subset_sps writes it (7.3.2.1.1 with the
    High-profile fields of profile_idc 83, then G.7.3.2.1.4)."""
    b = dp.Bits(dp.unescape(nal))
    s = {"header": b.u(8), "profile_idc": b.u(8), "constraints": b.u(8), "level_idc": b.u(8), "sps_id": b.ue()}
    assert s["profile_idc"] == 83
    for k in ("chroma_format_idc", "bit_depth_luma_minus8", "bit_depth_chroma_minus8"):
        s[k] = b.ue()
    s["qpprime"], s["scaling_matrix"] = b.u(1), b.u(1)
    assert s["chroma_format_idc"] == 1 and s["scaling_matrix"] == 0
    for k in ("log2_max_frame_num_minus4", "poc_type", "max_num_ref_frames"):
        s[k] = b.ue()
    assert s["poc_type"] == 2
    s["gaps"] = b.u(1)
    s["width_mbs_minus1"], s["height_mbs_minus1"] = b.ue(), b.ue()
    s["frame_mbs_only"], s["direct_8x8"], s["cropping"] = b.u(1), b.u(1), b.u(1)
    s["crop"] = tuple(b.ue() for _ in range(4)) if s["cropping"] else None
    s["vui"] = b.u(1)
    s["svc_ext"] = (b.u(1), b.u(2), b.u(1), b.u(2), b.u(1), b.u(1))  # ildfc present, ess idc, phase x, phase y, tcoeff pred, slice hdr restriction
    s["svc_vui"], s["ext2"] = b.u(1), b.u(1)
    rest = b.bits[b.at:]
    assert rest == "1" + "0" * (len(rest) - 1) and len(rest) <= 8, rest  # rbsp_trailing_bits
    return s


def split_headers(hdr: bytes, layers: int):
    """(SPS 0, [subset SPS 1..], [PPS 0..]) of svc_stream_headers' bytes"""
    n = dp.nals(hdr)
    assert [nal_type(x) for x in n] == [7] + [15] * (layers - 1) + [8] * layers, [nal_type(x) for x in n]
    return n[0], n[1:layers], n[layers:]


# ---- the fixture's input ----------------------------------------------------------------
def planes_of(frame: np.ndarray, w: int, h: int):
    return it.split(frame, w, h)


def down(planes):
    return tuple(synth._down2(p) for p in planes)


def pyramid(top, layers: int):
    """[layer 0, ..., the top layer] as (y, u, v) from the top layer's planes: synth._down2 level by level"""
    out = [tuple(top)]
    for _ in range(layers - 1):
        out.insert(0, down(out[0]))
    return out


def flat(planes) -> np.ndarray:
    return np.concatenate([np.ascontiguousarray(p).ravel() for p in planes])


@functools.lru_cache(maxsize=None)
def workload(name: str):
    """The fixture's input: per access unit the display-size (y, u, v) of the top
    layer (synth.clip at the coded top size, cropped) and the padded pyramid
    [layer 0, ..., top] of coded-size (y, u, v).  Shared; not to be changed."""
    g = GOLD[name]
    L, dw, dh = g["layers"], g["display_width"], g["display_height"]
    W, H = g["w0"] << (L - 1), g["h0"] << (L - 1)
    clip = synth.clip(W, H, g["frames"], g["seed"])
    shown, layers = [], []
    for i in range(g["frames"]):
        y, u, v = planes_of(clip[i], W, H)
        s = (np.ascontiguousarray(y[:dh, :dw]), np.ascontiguousarray(u[:dh // 2, :dw // 2]), np.ascontiguousarray(v[:dh // 2, :dw // 2]))
        for p in s:
            p.setflags(write=False)
        shown.append(s)
        layers.append(pyramid(dp.pad_edge(s, W, H), L))
    return shown, layers


def stream(name: str) -> bytes:
    return open(os.path.join(GOLDEN_DIR, GOLD[name]["stream"]), "rb").read()


def rgb_of(shown):
    """R, G, B planes of the display size made from a (y, u, v) frame: colourful, deterministic"""
    y, u, v = shown
    return y, np.repeat(np.repeat(u, 2, axis=0), 2, axis=1), np.repeat(np.repeat(v, 2, axis=0), 2, axis=1)


def frame_content(fmt: int, shown):
    """the content planes in_testlib.pack takes for a frame of format fmt showing `shown`"""
    return shown if fmt in (it.I420, it.NV12) else rgb_of(shown)


# ---- host builds --------------------------------------------------------------------------
def emu_lib():
    lib = ctypes.CDLL(EMU_LIB)
    i32 = ctypes.c_int32
    lib.svcd_emu_frame.argtypes = [i32] * 8 + [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64)] + [ctypes.c_void_p] * 3
    lib.svcd_emu_frame.restype = i32
    lib.svcd_emu_tiles.argtypes = [i32] * 5 + [ctypes.POINTER(i32)] * 2
    lib.svcd_emu_tiles.restype = i32
    lib.svcd_emu_edge_all.argtypes = [i32] * 5 + [ctypes.c_void_p] * 2
    lib.svcd_emu_edge_all.restype = i32
    return lib


def emu_frame(lib, fmt, planes, w, h, dw, dh, max_margin, key=(0, 0)):
    y = np.full((h, w), 0xEE, np.uint8)
    u = np.full((h // 2, w // 2), 0xEE, np.uint8)
    v = np.full((h // 2, w // 2), 0xEE, np.uint8)
    ptrs = (ctypes.c_void_p * 3)(*[p.ctypes.data for p in planes])
    pitches = (ctypes.c_int64 * 3)(*[p.strides[0] for p in planes])
    assert all(p.strides[1] == 1 for p in planes)
    rc = lib.svcd_emu_frame(fmt, key[0], key[1], w, h, dw, dh, max_margin, ptrs, pitches, y.ctypes.data, u.ctypes.data, v.ctypes.data)
    assert rc == 0, rc
    return y, u, v


def emu_pyramid(planes, layers: int):
    """[layer 0, ..., top] from the top planes through libhl_pyr_emu (k_pyramid's per-span code)"""
    lib = ctypes.CDLL(PYR_EMU_LIB)
    lib.pyr_emu_plane.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_void_p)]
    lib.pyr_emu_plane.restype = ctypes.c_int32
    K = layers - 1
    levels = [[None] * 3 for _ in range(K)]
    for c, p in enumerate(planes):
        p = np.ascontiguousarray(p)
        h, w = p.shape
        outs = [np.empty((h >> (j + 1), w >> (j + 1)), np.uint8) for j in range(K)]
        assert lib.pyr_emu_plane(p.ctypes.data, w, h, K, (ctypes.c_void_p * K)(*[o.ctypes.data for o in outs])) == 0
        for j in range(K):
            levels[j][c] = outs[j]
    return [tuple(levels[j]) for j in range(K - 1, -1, -1)] + [tuple(planes)]
