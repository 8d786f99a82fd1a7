"""Test support for the per-frame encoding type and live settings
(hl_amd_frame_ctl_t, include/hartallo_amd.h): the golden configurations
tests/golden/make_frame_ctl_golden.py encodes with the reference through
oracle/_ref/ref_enc_sched (tests/refdrive/ref_sched_harness.c), and the
schedule format those drivers share.  TEST INFRASTRUCTURE ONLY.

A schedule is TYPES, one letter per frame (A = AUTO, I = INTRA, P = INTER,
R = RAW, L = LOSSLESS; frames beyond its end are A; "-" = all A), plus
CHANGES, "frame:key=value" items separated by ';' ("-" = none) applied to the
hl_codec_t right before that frame's call (keys me_range, deblock,
early_term, gop, qp).
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from hl_testlib import GOLDEN, ROOT, _planes, emu_lib
from hartallo_amd import synth

REF_ENC_SCHED = os.path.join(ROOT, "oracle", "_ref", "ref_enc_sched")
DROP_IN_SCHED = os.path.join(ROOT, "oracle", "_ref", "drop_in_sched")
FC_GOLDEN_JSON = os.path.join(GOLDEN, "fc_golden.json")

ENCODING = {"A": 0, "I": 1, "P": 2, "L": 3, "R": 4}  # HL_VIDEO_ENCODING_TYPE_T (hl_types.h:262-274)

# 176x144 and 480x272 (several column bands of the pipelined scheduler), QP 28,
# me_range 16, deblocking on, early termination off, synth.clip seed 7
_BASE = dict(qp=28, me_range=16, deblock=1, early_term=0, seed=7, types="-", changes="-")
FC_CONFIGS = [
    dict(_BASE, name="fc_qcif_idr3", width=176, height=144, frames=8, gop=30, types="AAAIAAAA"),
    dict(_BASE, name="fc_qcif_gop3_idr4", width=176, height=144, frames=8, gop=3, types="AAAAIAAA"),
    dict(_BASE, name="fc_qcif_settings", width=176, height=144, frames=8, gop=30, changes="3:me_range=4;5:deblock=0;6:early_term=1"),
    dict(_BASE, name="fc_qcif_gop3to5", width=176, height=144, frames=10, gop=3, changes="1:gop=5"),
    dict(_BASE, name="fc_rc_qcif_idr", width=176, height=144, frames=8, gop=5, types="AAIAAAIA", rc_bitrate=100000, rc_basicunit=-1,
         rc_qp_min=-1, rc_qp_max=-1, fps_num=1, fps_den=15),
    dict(_BASE, name="fc_w480_mixed", width=480, height=272, frames=6, gop=30, types="AAAIAA", changes="2:me_range=4;4:deblock=0"),
    # the other direction of every change: me_range rising past its predecessor's (the motion window reaches further
    # into the reference picture than the run's guaranteed reach), deblocking off then on again, early termination on
    dict(_BASE, name="fc_w480_rising", width=480, height=272, frames=7, gop=30, types="AAAAAIA",
         changes="1:me_range=2;2:deblock=0;3:me_range=32;4:deblock=1;5:early_term=1;6:me_range=8"),
]
FC_BY_NAME = {c["name"]: c for c in FC_CONFIGS}

# Schedules the reference codes exactly like another one (the generator asserts
# it and stores the MD5): INTRA asked on the frame that is the GOP's IDR
# anyway; INTER asked while the GOP counter has run out (hl_codec_264.c:706-711
# still gives the IDR); a qp changed after the first frame (captured once,
# hl_codec_264.c:465).
FC_IDENTITIES = [
    dict(_BASE, name="id_gop3_intra_on_idr", width=176, height=144, frames=8, gop=3, types="AAAIAAAA"),
    dict(_BASE, name="id_inter_on_first", width=176, height=144, frames=8, gop=30, types="PAAAAAAA"),
    dict(_BASE, name="id_qp_change", width=176, height=144, frames=8, gop=30, changes="1:qp=35"),
]


def fc_input(cfg) -> np.ndarray:
    return synth.clip(cfg["width"], cfg["height"], cfg["frames"], cfg["seed"])


def fc_schedule(cfg):
    """Per frame (encoding, me_range, deblock, early_term, gop_size): the
    hl_frame_t.encoding and hl_codec_t values at that frame's call.  A qp
    change is not part of it (the reference ignores it)."""
    cur = dict(me_range=cfg["me_range"], deblock=cfg["deblock"], early_term=cfg["early_term"], gop=cfg["gop"])
    items = [] if cfg["changes"] == "-" else cfg["changes"].split(";")
    out = []
    for f in range(cfg["frames"]):
        for it in items:
            fr, kv = it.split(":")
            k, v = kv.split("=")
            if int(fr) == f and k != "qp":
                assert k in cur, k
                cur[k] = int(v)
        t = cfg["types"]
        enc = ENCODING[t[f]] if t != "-" and f < len(t) else 0
        out.append((enc, cur["me_range"], cur["deblock"], cur["early_term"], cur["gop"]))
    return out


def fc_frame_ctls(cfg):
    """The schedule as hartallo_amd.FrameCtl objects."""
    from hartallo_amd import FrameCtl

    return [FrameCtl(*s) for s in fc_schedule(cfg)]


def rc_args(cfg):
    """set_rate_control arguments of a rate-controlled configuration, or None."""
    if "rc_bitrate" not in cfg:
        return None
    return (cfg["rc_bitrate"], cfg["fps_num"], cfg["fps_den"], cfg["rc_basicunit"], cfg["rc_qp_min"], cfg["rc_qp_max"])


def ref_sched_command(binary, cfg, inp, out):
    """Command line and environment of ref_enc_sched / drop_in_sched."""
    env = dict(os.environ)
    for k in ("HL_REF_RC_BITRATE", "HL_REF_RC_BASICUNIT", "HL_REF_RC_QP_MIN", "HL_REF_RC_QP_MAX", "HL_REF_MAX_REF_FRAME", "HL_AMD_LOOKAHEAD"):
        env.pop(k, None)
    if "rc_bitrate" in cfg:
        env.update(HL_REF_RC_BITRATE=str(cfg["rc_bitrate"]), HL_REF_RC_BASICUNIT=str(cfg["rc_basicunit"]),
                   HL_REF_RC_QP_MIN=str(cfg["rc_qp_min"]), HL_REF_RC_QP_MAX=str(cfg["rc_qp_max"]))
    cmd = [binary] + [str(cfg[k]) for k in ("width", "height", "frames", "qp", "me_range", "deblock", "gop", "early_term")] + [
        inp, out, cfg["types"], cfg["changes"]]
    return cmd, env


class EmuCtlEncoder:
    """The host build of the kernel logic through emu_encode_frame_ex."""

    def __init__(self, cfg):
        lib = emu_lib()
        lib.emu_encode_frame_ex.restype = ctypes.c_long
        lib.emu_encode_frame_ex.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_long] + [ctypes.c_int] * 5
        self.lib, self.w, self.h = lib, cfg["width"], cfg["height"]
        self.h_ = lib.emu_create(self.w, self.h, cfg["qp"], cfg["me_range"], cfg["deblock"], cfg["gop"], cfg["early_term"])
        assert self.h_
        if rc_args(cfg):
            assert lib.emu_set_rc(ctypes.c_void_p(self.h_), *rc_args(cfg)) == 0
        self.out = np.zeros(self.w * self.h * 4 + (1 << 20), np.uint8)

    def encode(self, frame, ctl=None):
        """Bytes of the frame, or the (negative) refusal code."""
        y, u, v = _planes(frame, self.w, self.h)
        args = [ctypes.c_void_p(self.h_), y.ctypes.data, u.ctypes.data, v.ctypes.data, self.out.ctypes.data, self.out.size]
        n = self.lib.emu_encode_frame(*args) if ctl is None else self.lib.emu_encode_frame_ex(*args, *ctl)
        return self.out[:n].tobytes() if n > 0 else n

    def last_qp(self):
        return self.lib.emu_last_qp(ctypes.c_void_p(self.h_))

    def recon(self):
        from hl_testlib import _recon

        return _recon(lambda p: self.lib.emu_recon(ctypes.c_void_p(self.h_), p), self.w, self.h)

    def __del__(self):
        if getattr(self, "h_", None):
            self.lib.emu_destroy(ctypes.c_void_p(self.h_))
