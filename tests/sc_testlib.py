"""Test support for scene-cut detection (hl_amd_set_scenecut): a
numpy model of the analysis and of the planner, and the clips the tests share.
TEST INFRASTRUCTURE ONLY.

The model follows the definition, not the kernel: per displacement one
whole-frame absolute difference, block sums per macroblock, a running minimum
over the displacements whose block lies inside the picture.
"""
from __future__ import annotations

import ctypes
import functools
import os

import numpy as np

from hl_testlib import ROOT
from hartallo_amd import synth

SCENE_EMU_LIB = os.path.join(ROOT, "tests", "emu", "libhl_scene_emu.so")
AUTO, INTRA, INTER, LOSSLESS, RAW = 0, 1, 2, 3, 4
DEFAULT_THR, DEFAULT_GAP, DEFAULT_RANGE = 192, 1, 8


def mb_costs(cur: np.ndarray, prev: np.ndarray, R: int):
    """(inter, intra) per macroblock, uint32 arrays of shape (mbh, mbw), of the
    luma frame cur (h x w uint8) against prev."""
    h, w = cur.shape
    assert prev.shape == cur.shape and h % 16 == 0 and w % 16 == 0 and 0 <= R <= 16
    mbh, mbw = h // 16, w // 16
    blocks = cur.reshape(mbh, 16, mbw, 16).astype(np.int64)
    mean = (blocks.sum(axis=(1, 3)) + 128) >> 8
    intra = np.abs(blocks - mean[:, None, :, None]).sum(axis=(1, 3)).astype(np.uint32)
    pad = np.zeros((h + 2 * R, w + 2 * R), np.uint8)
    pad[R:R + h, R:R + w] = prev
    x0, y0 = 16 * np.arange(mbw), 16 * np.arange(mbh)
    inter = np.full((mbh, mbw), 0xFFFFFFFF, np.uint32)
    for dy in range(-R, R + 1):
        oky = (y0 + dy >= 0) & (y0 + dy + 16 <= h)
        for dx in range(-R, R + 1):
            okx = (x0 + dx >= 0) & (x0 + dx + 16 <= w)
            p = pad[R + dy:R + dy + h, R + dx:R + dx + w]
            d = np.maximum(cur, p) - np.minimum(cur, p)
            sad = d.reshape(mbh, 16, mbw, 16).sum(axis=(1, 3), dtype=np.uint32)
            sad[~(oky[:, None] & okx[None, :])] = 0xFFFFFFFF
            np.minimum(inter, sad, out=inter)
    return inter, intra


def frame_sums(inter: np.ndarray, intra: np.ndarray):
    """(P, I) as Python integers."""
    return int(np.minimum(inter, intra).astype(np.uint64).sum()), int(intra.astype(np.uint64).sum())


def is_cut(P: int, I: int, thr: int) -> bool:
    assert 1 <= thr <= 256
    return I > 0 and 256 * P >= thr * I


def luma(frame: np.ndarray, w: int, h: int) -> np.ndarray:
    return np.ascontiguousarray(frame[:w * h]).reshape(h, w)


def analyse(frames, w: int, h: int, R: int, prev=None):
    """Per frame of the clip (planar Y|U|V rows) None (not analysed) or
    (P, I, inter, intra); prev: the luma frame before the first, if any."""
    out = []
    for f in frames:
        y = luma(f, w, h)
        if prev is None:
            out.append(None)
        else:
            inter, intra = mb_costs(y, prev, R)
            out.append(frame_sums(inter, intra) + (inter, intra))
        prev = y
    return out


def plan(stats, thr: int, min_gap: int, gop_size: int, encodings=None, gop_left: int = 0, since_idr: int = 0):
    """The planner on a call's frames: stats as analyse() returns them.
    Returns (turned, idr): per frame whether the detector turned it into an
    IDR, and whether it is coded as one (GOP counter, caller or detector)."""
    turned, idr = [], []
    for k, s in enumerate(stats):
        enc = encodings[k] if encodings else AUTO
        t = s is not None and is_cut(s[0], s[1], thr) and since_idr >= min_gap and enc == AUTO
        i = gop_left <= 0 or enc == INTRA or t
        if i:
            gop_left = gop_size
        gop_left -= 1
        since_idr = 1 if i else since_idr + 1
        turned.append(t)
        idr.append(i)
    return turned, idr


@functools.lru_cache(maxsize=None)
def ab_clip(w: int, h: int, kind: str = "ab8") -> np.ndarray:
    """The clips of two contents (synth.clip seeds 5 and 9, 8 frames each):
    "ab8"  A[0:4] + B[0:4]            one cut, at frame 4
    "aba"  A[0:4] + B[0:3] + [A[6]]   cuts at frames 4 and 7
    "alt"  A0 B0 A1 B1 ... (9 frames) a cut at every frame
    Shared and read-only."""
    A, B = synth.clip(w, h, 8, 5), synth.clip(w, h, 8, 9)
    if kind == "ab8":
        c = np.concatenate([A[0:4], B[0:4]])
    elif kind == "aba":
        c = np.concatenate([A[0:4], B[0:3], A[6:7]])
    else:
        assert kind == "alt"
        c = np.stack([(A, B)[i & 1][i >> 1] for i in range(9)])
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def ab_stats(w: int, h: int, kind: str, R: int):
    """analyse() of ab_clip(w, h, kind), computed once."""
    return analyse(ab_clip(w, h, kind), w, h, R)


def scene_emu_lib():
    lib = ctypes.CDLL(SCENE_EMU_LIB)
    lib.scene_emu_frame.restype = ctypes.c_int32
    lib.scene_emu_frame.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                                    ctypes.c_void_p]
    return lib


def emu_costs(cur: np.ndarray, prev: np.ndarray, R: int):
    """(inter, intra, P, I) from the host build of hl_scene.h."""
    h, w = cur.shape
    cur, prev = np.ascontiguousarray(cur), np.ascontiguousarray(prev)
    mb = np.zeros((h // 16, w // 16, 2), np.uint32)
    sums = np.zeros(2, np.uint64)
    rc = scene_emu_lib().scene_emu_frame(cur.ctypes.data, prev.ctypes.data, w, h, R, mb.ctypes.data, sums.ctypes.data)
    assert rc == 0, rc
    return mb[:, :, 0], mb[:, :, 1], int(sums[0]), int(sums[1])
