"""Per-frame encoding type and live settings (hl_amd_frame_ctl_t,
include/hartallo_amd.h) on the CPU: the host build of the kernel logic with
the product's writer and rate control, through emu_encode_frame_ex, against
streams the reference itself made from the same schedules
(tests/golden/make_frame_ctl_golden.py, oracle/_ref/ref_enc_sched).  The GPU
is checked by test_gpu_frame_ctl.py."""
import json
import os
import subprocess
import sys
import tempfile

import pytest

from fc_testlib import (FC_BY_NAME, FC_CONFIGS, FC_GOLDEN_JSON, FC_IDENTITIES, REF_ENC_SCHED, EmuCtlEncoder, fc_input, fc_schedule)
from hl_testlib import GOLDEN, ROOT, first_diff, md5

GOLD = json.load(open(FC_GOLDEN_JSON))


def emu_stream(cfg, check=None):
    """The configuration's schedule through emu_encode_frame_ex; check: the
    golden entry whose per-frame recon MD5 (and QP, under rate control) to
    compare."""
    clip, sched = fc_input(cfg), fc_schedule(cfg)
    enc = EmuCtlEncoder(cfg)
    out = b""
    for f in range(cfg["frames"]):
        b = enc.encode(clip[f], sched[f])
        assert isinstance(b, bytes), f"{cfg['name']}: frame {f} refused ({b})"
        out += b
        if check:
            assert md5(enc.recon()) == check["recon_md5"][f], f"{cfg['name']}: recon of frame {f}"
            assert enc.last_qp() == check["slice_qp"][f], f"{cfg['name']}: QP of frame {f}"
    return out


@pytest.mark.parametrize("cfg", FC_CONFIGS, ids=[c["name"] for c in FC_CONFIGS])
def test_schedule_matches_reference(cfg):
    ref = open(os.path.join(GOLDEN, cfg["name"] + ".264"), "rb").read()
    assert md5(ref) == GOLD[cfg["name"]]["stream_md5"]
    out = emu_stream(cfg, GOLD[cfg["name"]])
    assert out == ref, f"{cfg['name']}: first differing byte {first_diff(out, ref)}"


@pytest.mark.parametrize("cfg", FC_IDENTITIES, ids=[c["name"] for c in FC_IDENTITIES])
def test_identity_schedules(cfg):
    """INTRA asked on the GOP's own IDR, INTER asked while the GOP counter has
    run out, and a qp changed after the first frame: the reference's stream is
    that of the plain schedule (asserted by the generator), and so is this."""
    g = GOLD["identities"][cfg["name"]]
    out = emu_stream(cfg, g)
    assert md5(out) == g["stream_md5"]
    plain = dict(cfg, types="-", changes="-")
    enc, clip = EmuCtlEncoder(plain), fc_input(plain)
    assert out == b"".join(enc.encode(clip[f]) for f in range(plain["frames"])), "differs from the calls without a ctl"


@pytest.mark.parametrize("encoding", [3, 4, 99], ids=["lossless", "raw", "unknown"])
def test_refused_types_leave_the_stream_alone(encoding):
    """RAW, LOSSLESS and unknown types are refused (no reference behaviour to
    match) and the stream goes on as if the refused call had not happened."""
    cfg = FC_BY_NAME["fc_qcif_idr3"]
    clip, sched = fc_input(cfg), fc_schedule(cfg)
    enc = EmuCtlEncoder(cfg)
    out = b""
    for f in range(cfg["frames"]):
        if f in (0, 2, 3):  # before the first frame, before a P picture, before the forced IDR
            assert enc.encode(clip[f], (encoding,) + sched[f][1:]) == -7
        out += enc.encode(clip[f], sched[f])
    assert md5(out) == GOLD[cfg["name"]]["stream_md5"]


def test_early_term_refused_on_small_picture():
    cfg = dict(FC_BY_NAME["fc_qcif_idr3"], width=32, height=16, frames=3)
    clip = fc_input(cfg)
    enc, plain = EmuCtlEncoder(cfg), EmuCtlEncoder(cfg)
    a = enc.encode(clip[0], (0, 16, 1, 0, 30))
    assert enc.encode(clip[1], (0, 16, 1, 1, 30)) == -1  # rdo.c:895-896 reads around the MB quadrants
    a += enc.encode(clip[1], (0, 16, 1, 0, 30))
    assert a == plain.encode(clip[0]) + plain.encode(clip[1])


def test_hl_codec_mirror_forwards_encoding_and_settings():
    """hl_codec.py's hl_codec_encode hands hl_frame_video_t.encoding and the
    codec's current settings to Encoder.encode as a FrameCtl."""
    import numpy as np

    from hartallo_amd import FrameCtl, hl_codec as hc

    seen = []

    class Fake:
        def encode(self, y, u, v, ctl=None):
            seen.append(ctl)
            return type("R", (), {"type": 1, "data": b"x", "hdr": b""})()

    codec = hc.hl_codec_create(hc.hl_codec_plugin_find(hc.HL_CODEC_TYPE_H264))
    codec.width, codec.height, codec._enc = 32, 32, Fake()
    codec.me_range, codec.deblock_flag, codec.me_early_term_flag, codec.gop_size = 8, 1, 0, 12
    frame, res = hc.hl_frame_video_create(), hc.hl_codec_result_create()
    assert frame.encoding == hc.HL_VIDEO_ENCODING_TYPE_AUTO
    hc.hl_frame_video_fill(frame, 32, 32, np.zeros(32 * 32 * 3 // 2, np.uint8))
    assert hc.hl_codec_encode(codec, frame, res) == 0
    frame.encoding = hc.HL_VIDEO_ENCODING_TYPE_INTRA
    codec.me_range, codec.deblock_flag, codec.gop_size, codec.qp = 4, 0, 5, 40
    assert hc.hl_codec_encode(codec, frame, res) == 0
    assert seen == [FrameCtl(0, 8, 1, 0, 12), FrameCtl(1, 4, 0, 0, 5)]


REF = "/root/reference"


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "include")), reason="reference sources are only in the build container")
def test_plugin_compiles_against_reference_headers():
    """integration/hl_codec_264_gfx950.c, which now reads hl_frame_video_t.encoding
    and the live hl_codec_t fields and calls hl_amd_encode_ex, against the
    reference's own headers, without a warning of its own."""
    prelude = os.path.join(ROOT, "oracle", "_ref", "prelude.h")
    plugin = os.path.join(ROOT, "integration", "hl_codec_264_gfx950.c")
    cmd = ["gcc", "-fsyntax-only", "-Wall", "-Wextra", "-Werror=incompatible-pointer-types", "-Werror=int-conversion",
           "-Werror=implicit-function-declaration", "-D_GNU_SOURCE", "-include", "limits.h", "-include", prelude,
           "-I" + os.path.join(REF, "include"), "-I" + os.path.join(ROOT, "include"), plugin]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "hl_codec_264_gfx950" not in r.stderr, r.stderr
    src = open(plugin).read()
    assert "hl_amd_encode_ex" in src and "f->encoding" in src


def test_goldens_regenerate_identically():
    if not os.path.exists(REF_ENC_SCHED):
        pytest.skip("reference build not present (oracle/_ref/ref_enc_sched)")
    with tempfile.TemporaryDirectory() as td:
        subprocess.run([sys.executable, os.path.join(GOLDEN, "make_frame_ctl_golden.py"), td], check=True, stdout=subprocess.DEVNULL)
        assert json.load(open(os.path.join(td, "fc_golden.json"))) == GOLD
        for cfg in FC_CONFIGS:
            a = open(os.path.join(td, cfg["name"] + ".264"), "rb").read()
            assert a == open(os.path.join(GOLDEN, cfg["name"] + ".264"), "rb").read(), cfg["name"]
