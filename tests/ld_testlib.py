"""Test support for the rendition ladder (hl_amd_encode_ladder_frame(s),
DESIGN.md 6.15): the ladders the tests share and the handle on the host build
(tests/emu/libhl_ladder_emu.so).  The model is sk_testlib's: rung r's planes
are sk.model_planes(fmt, content, key, disp_r, coded_r).  TEST INFRASTRUCTURE
ONLY.
"""
from __future__ import annotations

import ctypes
import functools
import os

import numpy as np

import in_testlib as it
from hl_testlib import ROOT

LADDER_EMU_LIB = os.path.join(ROOT, "tests", "emu", "libhl_ladder_emu.so")

# name -> (source, [(display, coded) per rung]); all ratios <= 8, all sizes even
LADDERS = {
    # the smallest mixed case: the identity, 2:1 (must equal synth._down2), 48/17 and 32/9 with edges on both sides
    "L1": ((96, 64), [((96, 64), (96, 64)), ((48, 32), (48, 32)), ((34, 18), (48, 32))]),
    # an identity rung with padding and odd chroma
    "L2": ((150, 102), [((150, 102), (160, 112)), ((50, 34), (64, 48)), ((72, 48), (80, 48))]),
    # very different tap counts and LDS sizes in one launch (the second rung: nine taps)
    "L3": ((382, 254), [((192, 128), (192, 128)), ((48, 32), (48, 32))]),
    # wide: the rungs have different tile-column counts, surplus workgroups in x leave
    "L4": ((1538, 26), [((1026, 18), (1040, 32)), ((770, 18), (784, 32))]),
    # count = 1: must equal the per-encoder call
    "L5": ((72, 48), [((48, 32), (48, 32))]),
}


def sizes_array(rungs):
    flat = [v for disp, coded in rungs for v in (*disp, *coded)]
    return (ctypes.c_int32 * len(flat))(*flat)


@functools.lru_cache(maxsize=None)
def ladder_emu_lib():
    lib = ctypes.CDLL(LADDER_EMU_LIB)
    i32, pi32 = ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)
    lib.ladder_emu_frames.argtypes = [i32] * 6 + [pi32, i32, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_void_p)]
    lib.ladder_emu_frames.restype = i32
    lib.ladder_emu_geometry.argtypes = [i32, i32, i32, pi32, pi32]
    lib.ladder_emu_geometry.restype = i32
    lib.ladder_emu_block.argtypes = [i32, i32, i32, pi32, i32, i32, i32, pi32]
    lib.ladder_emu_block.restype = i32
    return lib


def emu_ladder(fmt: int, contents, key, pads, fill, src, rungs):
    """the frames `contents` (each the planes of a frame of the source size), laid
    out with pads[c] bytes between the rows (filled with `fill`), through the host
    build: per rung a list of (y, u, v) per frame"""
    n = len(contents)
    bufs = [[it.padded_buffer(p, pad, fill) for p, pad in zip(it.pack(fmt, c), pads)] for c in contents]
    planes = (ctypes.c_void_p * (3 * n))()
    pitches = (ctypes.c_int64 * (3 * n))()
    for i, fb in enumerate(bufs):
        for c, ((b, pitch), pad) in enumerate(zip(fb, pads)):
            planes[3 * i + c] = b.ctypes.data
            pitches[3 * i + c] = 0 if pad == 0 else pitch
    outs = [np.full(n * w * h * 3 // 2, 0xEE, np.uint8) for _, (w, h) in rungs]
    optr = (ctypes.c_void_p * len(rungs))(*[o.ctypes.data for o in outs])
    rc = ladder_emu_lib().ladder_emu_frames(fmt, key[0], key[1], *src, len(rungs), sizes_array(rungs), n, planes, pitches, optr)
    assert rc == 0, rc
    res = []
    for o, (_, (w, h)) in zip(outs, rungs):
        fb, ny, nc = w * h * 3 // 2, w * h, w * h // 4
        res.append([(o[i * fb:i * fb + ny].reshape(h, w), o[i * fb + ny:i * fb + ny + nc].reshape(h // 2, w // 2),
                     o[i * fb + ny + nc:(i + 1) * fb].reshape(h // 2, w // 2)) for i in range(n)])
    return res
