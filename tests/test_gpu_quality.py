"""Per-picture quality on the GPU (hl_amd_set_quality): with
the feature on, every entry point of the AVC path still produces the
reference's stream (the goldens), and k_quality's sums and per-macroblock SSE
equal the numpy model (q_testlib) applied to the input frame and the
reconstruction the encoder hands out.  The goldens pin that reconstruction to
the reference's, so these are the reference encoder's own PSNR and SSIM."""
import functools
import json
import math
import os

import numpy as np
import pytest

from hl_testlib import GOLDEN, GOLDEN_CONFIGS, GOLDEN_RC_CONFIGS, _planes, first_diff, golden_input
from q_testlib import assert_quality, picture_quality

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(GOLDEN, "golden.json")))
NAMES = ["tiny_32x16_qp26", "qcif_ippp_qp28_db", "qcif_qp0_me1", "w480_h272_qp28_me16"]
CFG = {c[0]: c for c in GOLDEN_CONFIGS + GOLDEN_RC_CONFIGS}
INVALID_PARAMETER, INVALID_STATE = 1, 3


@functools.lru_cache(maxsize=None)
def clip_of(name):
    c = golden_input(CFG[name])
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def golden_stream(name):
    return open(os.path.join(GOLDEN, name + ".264"), "rb").read()


def make_encoder(name, quality=True):
    from hartallo_amd import Encoder

    cfg = CFG[name]
    _, w, h, n, qp, mer, db, gop, seed = cfg[:9]
    enc = Encoder(w, h, qp, mer, db, gop, 0)
    if len(cfg) > 9:
        br, bu, qmin, qmax = cfg[9:]
        enc.set_rate_control(br, GOLD[name]["fps_num"], GOLD[name]["fps_den"], bu, qmin, qmax)
    if quality:
        enc.set_quality(True)
    return enc


def on_device(clip, w, h, shift=0):
    """The clip in device memory and each frame's (y, u, v) pointers; `shift`
    bytes into the allocation (for planes that are not 8-byte aligned)."""
    import torch

    flat = np.concatenate([np.zeros(shift, np.uint8), np.array(clip).ravel()])
    dev = torch.from_numpy(flat).cuda()
    n, fb = w * h, w * h * 3 // 2
    base = dev.data_ptr() + shift
    return dev, [(base + fb * i, base + fb * i + n, base + fb * i + n + n // 4) for i in range(len(clip))]


def same(got, ref, what):
    assert got == ref, f"{what}: first differing byte {first_diff(got, ref)} of {len(got)} / {len(ref)}"


def check_picture(enc, k, frame, w, h, what, recon=None):
    """Picture k of the last call against the model on (frame, debug_recon(k))."""
    rec = enc.debug_recon(k) if recon is None else recon
    assert rec is not None, what
    want = picture_quality(frame, rec, w, h)
    got = enc.last_quality(k)
    assert_quality(got, enc.debug_quality_mb(k), want, what)
    for c, p in enumerate("yuv"):
        sse, n = want["sse"][c], want["samples"][c]
        assert got["psnr_" + p] == (math.inf if sse == 0 else pytest.approx(10 * math.log10(255 * 255 * n / sse), abs=1e-9)), what
        assert got["ssim_" + p] == pytest.approx(want["ssim_q30"][c] / (1 << 30) / want["windows"][c], abs=1e-12), what
    return got


def expect_code(code, fn, *a):
    from hartallo_amd import HlAmdError

    with pytest.raises(HlAmdError) as e:
        fn(*a)
    assert e.value.code == code, e.value


@pytest.mark.parametrize("mode", ["per_call", "device", "batch", "lookahead3"])
@pytest.mark.parametrize("name", NAMES)
def test_golden_stream_and_model(gpu, name, mode):
    _, w, h, n = CFG[name][:4]
    clip, ref = clip_of(name), golden_stream(name)
    enc = make_encoder(name)
    what = f"{name} {mode}"
    out = b""
    if mode == "per_call":
        for f in range(n):
            out += enc.encode(*_planes(clip[f], w, h)).annexb()
            check_picture(enc, 0, clip[f], w, h, f"{what} frame {f}")
            expect_code(INVALID_PARAMETER, enc.last_quality, -1)
            expect_code(INVALID_STATE, enc.last_quality, 1)
    elif mode == "device":
        dev, ptrs = on_device(clip, w, h)
        for f in range(n):
            out += enc.encode_device(*ptrs[f]).annexb()
            check_picture(enc, 0, clip[f], w, h, f"{what} frame {f}")
    elif mode == "batch":
        dev, ptrs = on_device(clip, w, h)
        out = b"".join(r.annexb() for r in enc.encode_batch_device(ptrs))
        for f in range(n):
            check_picture(enc, f, clip[f], w, h, f"{what} frame {f}")
        expect_code(INVALID_STATE, enc.last_quality, n)
    else:
        enc.set_lookahead(3)
        coded = 0  # frames the queue has coded so far
        for f in range(n):
            r = enc.encode(*_planes(clip[f], w, h))
            out += r.annexb() if r.type else b""
            if f % 3 == 2:  # this call coded frames f - 2 .. f
                for k in range(3):
                    check_picture(enc, k, clip[f - 2 + k], w, h, f"{what} frame {f - 2 + k}")
                coded = f + 1
        while (r := enc.flush()).type:
            out += r.annexb()
            if coded < n:  # the first flush coded the rest
                for k in range(n - coded):
                    check_picture(enc, k, clip[coded + k], w, h, f"{what} flushed frame {coded + k}")
                coded = n
    same(out, ref, what)
    if name == "qcif_qp0_me1":  # near-lossless: a tiny SSE, PSNR far above anything a lossy QP gives
        q = enc.last_quality(0)
        assert q["psnr_y"] > 55 and q["ssim_y"] > 0.999, q
    enc.close()


def test_two_streams(gpu):
    """hl_amd_encode_streams: every encoder its own setting and results."""
    from hartallo_amd import Encoder

    name = "qcif_ippp_qp28_db"
    _, w, h, n = CFG[name][:4]
    clip = clip_of(name)
    a, b, off = make_encoder(name), make_encoder(name), make_encoder(name, quality=False)
    dev, ptrs = on_device(clip, w, h)
    rev = clip[::-1]
    dev2, ptrs2 = on_device(rev, w, h)
    res = Encoder.encode_streams_device([a, b, off], [ptrs, ptrs2, ptrs])
    same(b"".join(r.annexb() for r in res[0]), golden_stream(name), "stream 0")
    same(b"".join(r.annexb() for r in res[2]), golden_stream(name), "stream 2 (feature off)")
    for f in range(n):
        check_picture(a, f, clip[f], w, h, f"stream 0 frame {f}")
        check_picture(b, f, rev[f], w, h, f"stream 1 frame {f}")
        expect_code(INVALID_STATE, off.last_quality, f)


def test_rate_controlled_golden(gpu):
    name = "rc_qcif_60k_qp20_36"
    _, w, h, n = CFG[name][:4]
    clip = clip_of(name)
    enc = make_encoder(name)
    out = b""
    for f in range(n):
        out += enc.encode(*_planes(clip[f], w, h)).annexb()
        assert enc.last_qp() == GOLD[name]["slice_qp"][f]
        check_picture(enc, 0, clip[f], w, h, f"{name} frame {f}")
    same(out, golden_stream(name), name)
    # ... and as one batch (a run of one picture each under rate control)
    enc = make_encoder(name)
    dev, ptrs = on_device(clip, w, h)
    same(b"".join(r.annexb() for r in enc.encode_batch_device(ptrs)), golden_stream(name), name + " batch")
    check_picture(enc, n - 1, clip[n - 1], w, h, f"{name} batch, last frame")
    assert enc.last_quality(0)["sse"][0] > 0


def test_fallback_runs_are_measured(gpu, monkeypatch):
    """A run that is re-encoded picture by picture keeps its pictures in the
    run buffers: they are measured there."""
    name = "qcif_ippp_qp28_db"
    _, w, h, n = CFG[name][:4]
    clip = clip_of(name)
    monkeypatch.setenv("HL_AMD_FORCE_FALLBACK", "1")
    enc = make_encoder(name)
    dev, ptrs = on_device(clip, w, h)
    same(b"".join(r.annexb() for r in enc.encode_batch_device(ptrs)), golden_stream(name), "forced fallback")
    assert enc.last_batch_stats()["fallbacks"] >= 1
    for f in range(n):
        check_picture(enc, f, clip[f], w, h, f"fallback frame {f}")


def test_batch_longer_than_a_run_group(gpu):
    """130 pictures at 32x16: two groups (128 + 2); the second reuses the run
    buffers, and the first group's pictures were measured before that.  The
    reference values: the same clip coded per call."""
    from hartallo_amd import synth

    w, h, n = 32, 16, 130
    _, _, _, _, qp, mer, db, gop, _ = CFG["tiny_32x16_qp26"]
    clip = np.concatenate([synth.clip(w, h, 65, 21), synth.clip(w, h, 65, 22)])
    from hartallo_amd import Encoder

    one = Encoder(w, h, qp, mer, db, gop, 0)
    one.set_quality(True)
    want, stream = [], b""
    for f in range(n):
        stream += one.encode(*_planes(clip[f], w, h)).annexb()
        want.append(picture_quality(clip[f], np.concatenate(one.recon()), w, h))
    enc = Encoder(w, h, qp, mer, db, gop, 0)
    enc.set_quality(True)
    dev, ptrs = on_device(clip, w, h)
    same(b"".join(r.annexb() for r in enc.encode_batch_device(ptrs)), stream, "130-picture batch against per-call")
    for f in range(n):
        assert_quality(enc.last_quality(f), enc.debug_quality_mb(f), want[f], f"picture {f} of 130")
    expect_code(INVALID_STATE, enc.last_quality, n)
    assert enc.bench_quality(2) > 0  # (the last launch can be repeated alone)
    expect_code(INVALID_STATE, enc.last_quality, 0)  # ... which spends its sums


def test_feature_off_and_switching(gpu):
    name = "qcif_ippp_qp28_db"
    _, w, h, n = CFG[name][:4]
    clip = clip_of(name)
    enc = make_encoder(name, quality=False)
    out = enc.encode(*_planes(clip[0], w, h)).annexb()
    expect_code(INVALID_STATE, enc.last_quality, 0)
    expect_code(INVALID_STATE, enc.debug_quality_mb, 0)
    expect_code(INVALID_STATE, enc.bench_quality, 1)
    enc.set_quality(True)  # between any two encode calls
    expect_code(INVALID_STATE, enc.last_quality, 0)  # (the last call was not measured)
    out += enc.encode(*_planes(clip[1], w, h)).annexb()
    check_picture(enc, 0, clip[1], w, h, "switched on at frame 1")
    enc.set_quality(False)
    expect_code(INVALID_STATE, enc.last_quality, 0)
    for f in range(2, n):
        out += enc.encode(*_planes(clip[f], w, h)).annexb()
    same(out, golden_stream(name), "switched on and off")
    la = make_encoder(name, quality=False)
    la.set_lookahead(3)
    la.encode(*_planes(clip[0], w, h))
    expect_code(INVALID_STATE, la.set_quality, True)  # while look-ahead frames are queued


def test_unaligned_device_plane_is_refused(gpu):
    name = "qcif_ippp_qp28_db"
    _, w, h, n = CFG[name][:4]
    clip = clip_of(name)
    enc = make_encoder(name)
    dev, ptrs = on_device(clip, w, h)
    dev4, ptrs4 = on_device(clip, w, h, shift=4)
    assert ptrs[0][0] % 8 == 0 and ptrs4[0][0] % 8 == 4
    out = b"".join(enc.encode_device(*ptrs[f]).annexb() for f in range(2))
    expect_code(INVALID_PARAMETER, enc.encode_device, *ptrs4[2])
    expect_code(INVALID_STATE, enc.last_quality, 0)  # a refused call leaves no results
    expect_code(INVALID_PARAMETER, enc.encode_batch_device, [ptrs[2], (ptrs[3][0], ptrs4[3][1], ptrs[3][2])])
    out += b"".join(r.annexb() for r in enc.encode_batch_device(ptrs[2:]))  # the next call continues the stream
    same(out, golden_stream(name), "after the refusals")
    for k in range(n - 2):
        check_picture(enc, k, clip[2 + k], w, h, f"frame {2 + k} after the refusals")
