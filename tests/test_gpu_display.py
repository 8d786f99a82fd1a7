"""The display size on the GPU (hl_amd_set_display_size):
with cropping every slice NAL stays the reference's for the padded picture and
only the SPS changes; frames of the display size are padded on the GPU exactly
as np.pad(mode="edge") pads the model's planes (k_ingest on the full tiles,
k_ingest_edge on the others) and then coded as those planes; quality covers the
display rectangle; refusals leave the stream as it was."""
import functools
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import dp_testlib as dp
import in_testlib as it
import q_testlib as qt
from hartallo_amd import synth
from hl_testlib import GOLDEN, GOLDEN_CONFIGS, GOLDEN_ET_CONFIGS, GOLDEN_RC_CONFIGS, ROOT, first_diff, golden_input

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(GOLDEN, "golden.json")))
REF_DEC = os.path.join(ROOT, "oracle", "_ref", "ref_dec")
QCIF_CROPPED_SPS = "27 42 e0 0b 95 a0 b1 36 49 90"  # 176x144, display 170x134
FORMATS = ["i420", "nv12", "rgb24", "rgba32", "rgbp"]
KEY = (it.BT709, it.LIMITED)
# coded size, display size (test_emu_display.py: odd chroma, one dimension only, the edge column in the second workgroup column)
SHAPES = [(48, 32, 34, 18), (48, 32, 46, 30), (48, 32, 48, 18), (48, 32, 34, 32), (176, 144, 162, 130), (1040, 32, 1026, 18)]
N = 5  # frames of a clip: with a GOP of 3 an IDR, two P, an IDR, a P


def same(got, ref, what):
    assert got == ref, f"{what}: first differing byte {first_diff(got, ref)} of {len(got)} / {len(ref)}"


def golden_cfg(name):
    return next(c for c in GOLDEN_CONFIGS + GOLDEN_ET_CONFIGS + GOLDEN_RC_CONFIGS if c[0] == name)


def golden_encoder(name, display=None):
    from hartallo_amd import Encoder

    cfg = golden_cfg(name)
    _, w, h, n, qp, me, db, gop, seed = cfg[:9]
    enc = Encoder(w, h, qp, me, db, gop, GOLD[name].get("early_term", 0))
    if len(cfg) > 9:
        enc.set_rate_control(cfg[9], GOLD[name]["fps_num"], GOLD[name]["fps_den"], cfg[10], cfg[11], cfg[12])
    if display:
        enc.set_display_size(*display)
        assert enc.display_size == display
    return enc


def make_encoder(w, h, display=None, gop=3, quality=False, scenecut=False):
    from hartallo_amd import Encoder

    enc = Encoder(w, h, 28, 8, 1, gop, 0)
    enc.set_colour(*KEY)
    if display:
        enc.set_display_size(*display)
    if quality:
        enc.set_quality(True)
    if scenecut:
        enc.set_scenecut(192, 1, 8)
    return enc


def planar_ptrs(frames):
    """dense (y, u, v) frames in device memory: the tensor and the pointers encode_batch_device takes"""
    import torch

    flat = np.stack([np.concatenate([np.ascontiguousarray(p).ravel() for p in f]) for f in frames])
    dev = torch.from_numpy(flat).cuda()
    torch.cuda.synchronize()
    ny = frames[0][0].size
    return dev, [(dev[i].data_ptr(), dev[i].data_ptr() + ny, dev[i].data_ptr() + ny + ny // 4) for i in range(len(frames))]


def lookahead(enc, k, calls):
    """the calls (each returns a result) under a look-ahead of k, then the flush"""
    enc.set_lookahead(k)
    out = b""
    for call in calls:
        r = call()
        out += r.annexb() if r.type else b""
    while (r := enc.flush()).type:
        out += r.annexb()
    return out


# ---- parity with the reference under cropping -------------------------------------
@pytest.mark.parametrize("mode", ["encode", "batch"])
@pytest.mark.parametrize("name", ["qcif_ippp_qp28_db", "et_qcif_ippp_qp28", "rc_qcif_100k_gop5"])
def test_cropping_changes_the_sps_only(gpu, name, mode, tmp_path):
    """(the rate-controlled golden: the rate controller reads slice bits only)"""
    from hartallo_amd import stream_headers

    cfg = golden_cfg(name)
    w, h, n, qp = cfg[1], cfg[2], cfg[3], cfg[4]
    display = (w - 6, h - 10)
    clip = golden_input(cfg)
    ref = open(os.path.join(GOLDEN, name + ".264"), "rb").read()
    plain, cropped = stream_headers(w, h, qp), stream_headers(w, h, qp, 1, *display)
    assert ref.startswith(plain + b"\x00\x00\x01") and dp.nals(cropped)[1] == dp.nals(plain)[1]
    assert dp.nals(cropped)[0].hex(" ") == QCIF_CROPPED_SPS and (w, h) == (176, 144)
    enc = golden_encoder(name, display)
    frames = [it.split(clip[f], w, h) for f in range(n)]
    if mode == "encode":
        res = [enc.encode(*f) for f in frames]
    else:
        dev, ptrs = planar_ptrs(frames)
        res = enc.encode_batch_device(ptrs)
    enc.close()
    assert res[0].hdr == cropped and all(not r.hdr for r in res[1:])
    got = b"".join(r.annexb() for r in res)
    same(got[len(cropped):], ref[len(plain):], f"{name} {mode}: the slices")  # every slice NAL is the golden's
    if os.path.exists(REF_DEC) and "decoded_md5" in GOLD[name]:  # the reference's decoder parses the cropping fields and ignores them
        src, out = tmp_path / "s.264", tmp_path / "d.yuv"
        src.write_bytes(got)
        r = subprocess.run([REF_DEC, str(src), str(out)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        info = json.loads(r.stdout.strip().splitlines()[-1])
        assert info["errors"] == 0 and (info["width"], info["height"]) == (w, h), info
        d = np.fromfile(out, np.uint8).reshape(-1, w * h * 3 // 2)
        assert [hashlib.md5(p.tobytes()).hexdigest() for p in d] == GOLD[name]["decoded_md5"]


def test_the_setters_work_in_either_order(gpu):
    from hartallo_amd import Encoder, stream_headers

    w, h = 176, 144
    y, u, v = next(iter(synth.frames(w, h, 1, 3)))
    hdrs = []
    for order in (0, 1):
        enc = Encoder(w, h, 30, 8, 1, 3, 0)
        for step in ((0, 1) if order == 0 else (1, 0)):
            enc.set_max_ref_frame(4) if step == 0 else enc.set_display_size(170, 134)
        hdrs.append(enc.encode(y, u, v).hdr)
        enc.close()
    assert hdrs[0] == hdrs[1] == stream_headers(w, h, 30, 4, 170, 134)
    enc = Encoder(w, h, 30, 8, 1, 3, 0)
    enc.set_display_size(170, 134)
    enc.set_display_size(w, h)  # back to none: today's bytes
    assert enc.display_size == (w, h) and enc.encode(y, u, v).hdr == stream_headers(w, h, 30)
    enc.close()


# ---- ingest ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clip_planes(w, h, dw, dh, yuv, n=N, seeds=(21, 22, 23)):
    """n frames of (Y, U, V) or (R, G, B) planes of the display size, cut out of synth.frames of the coded size.  Shared, read-only."""
    if yuv:
        out = [(y[:dh, :dw].copy(), u[:dh // 2, :dw // 2].copy(), v[:dh // 2, :dw // 2].copy()) for y, u, v in synth.frames(w, h, n, 7)]
    else:
        chans = [[y[:dh, :dw].copy() for y, _, _ in synth.frames(w, h, n, s)] for s in seeds]
        out = [tuple(chans[c][f] for c in range(3)) for f in range(n)]
    for f in out:
        for p in f:
            p.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def model_clip(w, h, dw, dh, fmt):
    return [dp.model_planes(fmt, f, KEY, w, h) for f in clip_planes(w, h, dw, dh, fmt in (it.I420, it.NV12))]


def pads_for(fmt, dw, pitched):
    """bytes between the rows, per plane: pitched -> at least 8, and every pitch a
    multiple of 4 (device frames); else dense where the row bytes are such multiples"""
    out = []
    for c in range(it_planes(fmt)):
        rb = row_bytes(fmt, c, dw)
        out.append(((-rb) % 4) + (8 if pitched else 0))
    return tuple(out)


def it_planes(fmt):
    return {it.I420: 3, it.NV12: 2, it.RGB24: 1, it.RGBA32: 1, it.RGBP: 3}[fmt]


def row_bytes(fmt, c, dw):
    return {it.I420: dw // 2 if c else dw, it.NV12: dw, it.RGB24: 3 * dw, it.RGBA32: 4 * dw, it.RGBP: dw}[fmt]


def host_frame(fmt, planes, pads, fill=0xA5):
    from hartallo_amd import Frame

    bufs = [it.padded_buffer(p, pad, fill) for p, pad in zip(it.pack(fmt, planes), pads)]
    return Frame(fmt, [b.ctypes.data for b, _ in bufs], [pitch for _, pitch in bufs], False, bufs)


def device_frame(fmt, planes, pads, fill=0xA5, dense_as_zero=False):
    import torch

    from hartallo_amd import Frame

    bufs = [it.padded_buffer(p, pad, fill) for p, pad in zip(it.pack(fmt, planes), pads)]
    dev = [torch.from_numpy(b).cuda() for b, _ in bufs]
    torch.cuda.synchronize()
    return Frame(fmt, [d.data_ptr() for d in dev], [0 if dense_as_zero and pad == 0 else pitch for (_, pitch), pad in zip(bufs, pads)], True, dev)


def check_input(enc, k, want, what):
    got = enc.last_input(k)
    for name, g, m in zip("YUV", got, want):
        assert g.shape == m.shape and np.array_equal(g, m), f"{what}: {name} of picture {k}: {np.count_nonzero(g != m)} samples differ"


@functools.lru_cache(maxsize=None)
def reference_stream(w, h, dw, dh, fmt):
    """a fresh encoder with the same display size fed the model's planes through encode"""
    ref = make_encoder(w, h, (dw, dh))
    out = [ref.encode(*f).annexb() for f in model_clip(w, h, dw, dh, fmt)]
    ref.close()
    return out


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[2]}x{s[3]}in{s[0]}x{s[1]}")
def test_frames_of_the_display_size_are_padded_and_coded_as_the_model(gpu, shape, fmt):
    w, h, dw, dh = shape
    F = it.FORMATS[fmt]
    clip, model, want = clip_planes(w, h, dw, dh, F in (it.I420, it.NV12)), model_clip(w, h, dw, dh, F), reference_stream(w, h, dw, dh, F)
    what = f"{fmt} {dw}x{dh} in {w}x{h}"
    pitched = pads_for(F, dw, True)
    dense = pads_for(F, dw, False)  # (all zero where the row bytes are multiples of 4)
    # one frame per call: from the host (any pitch: 6 more bytes a row, and dense), and from the device
    enc = make_encoder(w, h, (dw, dh))
    for k in range(N):
        if k % 3 == 0:
            f = host_frame(F, clip[k], tuple(6 for _ in pitched))
        elif k % 3 == 1:
            f = host_frame(F, clip[k], tuple(0 for _ in pitched))
        else:
            f = device_frame(F, clip[k], pitched)
            assert all(p % 4 == 0 for p in f.pitches)
        got = enc.encode_frame(f).annexb()
        check_input(enc, 0, model[k], f"{what} frame {k}")
        same(got, want[k], f"{what} frame {k}")
    assert enc.bench_ingest(2) > 0  # (every launch of the last call can be repeated alone)
    enc.close()
    # one call for the clip, from device memory: pitched and (row bytes permitting) dense frames
    enc = make_encoder(w, h, (dw, dh))
    frames = [device_frame(F, clip[k], dense if k & 1 else pitched, dense_as_zero=True) for k in range(N)]
    got = enc.encode_frames_device(frames)
    for k in range(N):
        check_input(enc, k, model[k], f"{what} frames")
        same(got[k].annexb(), want[k], f"{what} frames, picture {k}")
    assert enc.bench_ingest(2) > 0
    enc.close()
    # a look-ahead of 3 with a flush (5 frames: two are left to the flush)
    enc = make_encoder(w, h, (dw, dh))
    frames = [host_frame(F, clip[k], tuple(2 for _ in pitched)) if k & 1 else device_frame(F, clip[k], pitched) for k in range(N)]
    same(lookahead(enc, 3, [functools.partial(enc.encode_frame, f) for f in frames]), b"".join(want), what + " lookahead3")
    enc.close()


def test_two_padding_fills_and_a_dense_i420_device_frame(gpu):
    """what lies between the rows reaches no output; a dense I420 device frame of a
    display size below the coded size is converted like any other (it is forwarded
    only when the display size is the coded size)"""
    w, h, dw, dh = 48, 32, 40, 18  # (dense rows of 40 and 20 bytes: multiples of 4)
    clip, model = clip_planes(w, h, dw, dh, True), model_clip(w, h, dw, dh, it.I420)
    enc = make_encoder(w, h, (dw, dh))
    outs = []
    for fill in (0xA5, 0x3C):
        enc.encode_frame(device_frame(it.NV12, clip[0], (8, 8), fill))
        outs.append(enc.last_input(0))
        check_input(enc, 0, model[0], f"fill {fill:#x}")
    enc.encode_frame(device_frame(it.I420, clip[1], (0, 0, 0), dense_as_zero=True))
    check_input(enc, 0, model[1], "dense I420")
    enc.close()


def test_scene_cuts_read_the_padded_planes(gpu):
    """content that changes at frame 4: picture types, scene statistics and bytes
    are those of the planar call on the padded model planes, and the statistics
    those of the analysis' model (sc_testlib) on them: k_scene reads the
    replicated edges"""
    from sc_testlib import analyse, plan

    w, h, dw, dh = 64, 48, 50, 34
    clip = clip_planes(w, h, dw, dh, False, 4) + clip_planes(w, h, dw, dh, False, 4, (31, 32, 33))
    model = [dp.model_planes(it.RGB24, f, KEY, w, h) for f in clip]
    flat = [np.concatenate([np.ascontiguousarray(p).ravel() for p in f]) for f in model]
    turned, idr = plan(analyse(flat, w, h, 8), 192, 1, 30)
    assert turned[4] and idr == [True, False, False, False, True, False, False, False]  # the clip has the cut the test is about
    enc, ref = make_encoder(w, h, (dw, dh), gop=30, scenecut=True), make_encoder(w, h, (dw, dh), gop=30, scenecut=True)
    got = enc.encode_frames_device([device_frame(it.RGBA32, f, (8,)) for f in clip])
    dev, ptrs = planar_ptrs(model)
    want = ref.encode_batch_device(ptrs)
    for k in range(8):
        same(got[k].annexb(), want[k].annexb(), f"picture {k}")
        assert enc.last_scene_stats(k) == ref.last_scene_stats(k) and enc.last_scene_stats(k)["turned"] == turned[k]
        assert (got[k].data[0] & 31 == 5) == idr[k]
    enc.close(), ref.close()


# ---- quality -------------------------------------------------------------------------
def check_quality(enc, k, src, dw, dh, what):
    w, h = enc.width, enc.height
    rec = qt.planes(enc.debug_recon(k), w, h)
    want = dp.picture_window_quality(src, rec, dw, dh)
    got, mb = enc.last_quality(k), enc.debug_quality_mb(k)
    for key in ("sse", "samples", "ssim_q30", "windows"):
        assert list(got[key]) == want[key], (what, k, key, got[key], want[key])
    assert np.array_equal(mb, want["mb"]), (what, k)
    assert int(mb.astype(np.uint64).sum()) == want["sse"][0], (what, k)
    assert want["samples"] == [dw * dh, dw * dh // 4, dw * dh // 4]


@pytest.mark.parametrize("shape", [(48, 32, 34, 18), (176, 144, 162, 130), (288, 48, 274, 34)], ids=lambda s: f"{s[2]}x{s[3]}in{s[0]}x{s[1]}")
def test_quality_covers_the_display_rectangle(gpu, shape):
    """(the last shape: the luma window ends in the second tile of 256 x 32 samples, in both directions)"""
    w, h, dw, dh = shape
    model = model_clip(w, h, dw, dh, it.I420)
    what = f"{dw}x{dh} in {w}x{h}"
    # per call: the plain entry point with planes the caller padded
    enc = make_encoder(w, h, (dw, dh), quality=True)
    for k in range(3):
        enc.encode(*model[k])
        check_quality(enc, 0, model[k], dw, dh, what + " encode")
    enc.close()
    # batched: the frame call pads, quality sees the padded planes' display part
    enc = make_encoder(w, h, (dw, dh), quality=True)
    clip = clip_planes(w, h, dw, dh, True)
    enc.encode_frames_device([device_frame(it.NV12, f, pads_for(it.NV12, dw, True)) for f in clip])
    for k in range(N):
        check_quality(enc, k, model[k], dw, dh, what + " frames")
    assert enc.bench_quality(2) > 0
    enc.close()
    # through the look-ahead: measured when the queue is coded
    enc = make_encoder(w, h, (dw, dh), quality=True)
    enc.set_lookahead(3)
    for k in range(3):
        r = enc.encode_frame(host_frame(it.I420, clip[k], (6, 6, 6)))
    assert r.type
    for k in range(3):
        check_quality(enc, k, model[k], dw, dh, what + " lookahead")
    enc.close()
    # without a display size: today's numbers on the same clip
    enc = make_encoder(w, h, None, quality=True)
    for k in range(2):
        enc.encode(*model[k])
        flat = np.concatenate([np.ascontiguousarray(p).ravel() for p in model[k]])
        qt.assert_quality(enc.last_quality(0), enc.debug_quality_mb(0), qt.picture_quality(flat, enc.debug_recon(0), w, h), what + " no display size")
    enc.close()


# ---- refusals ------------------------------------------------------------------------
def test_refusals_leave_the_stream_as_it_was(gpu):
    from hartallo_amd import Frame, HlAmdError, SvcEncoder
    from hartallo_amd import _lib as L

    w, h, dw, dh = 48, 32, 34, 18
    clip, model = clip_planes(w, h, dw, dh, False, 12), [dp.model_planes(it.RGB24, f, KEY, w, h) for f in clip_planes(w, h, dw, dh, False, 12)]
    ref = make_encoder(w, h, (dw, dh))
    want = [ref.encode(*m).annexb() for m in model]
    ref.close()
    enc = make_encoder(w, h)
    k = 0

    def refused(code, call):
        with pytest.raises(HlAmdError) as e:
            call()
        assert e.value.code == code, (e.value.code, code)

    def next_frame_continues():
        nonlocal k
        same(enc.encode_frame(host_frame(it.RGB24, clip[k], (6,))).annexb(), want[k], f"frame {k} after a refusal")
        check_input(enc, 0, model[k], f"frame {k}")
        k += 1

    # odd, too small, too large: refused, and the setting stays what it was
    for bad in ((33, 18), (34, 17), (32, 18), (34, 16), (50, 18), (34, 34), (0, 0), (-34, 18)):
        refused(1, lambda: enc.set_display_size(*bad))
        assert enc.display_size == (w, h)
    enc.set_display_size(dw, dh)
    next_frame_continues()
    # after the first picture
    refused(3, lambda: enc.set_display_size(w, h))
    refused(3, lambda: enc.set_display_size(dw + 2, dh))
    assert enc.display_size == (dw, dh)
    next_frame_continues()
    rb = 3 * dw  # 102: no multiple of 4
    good_dev = device_frame(it.RGB24, clip[0], (2,))
    coded_planes = tuple(np.ascontiguousarray(np.pad(p, ((0, h - dh), (0, w - dw)), mode="edge")) for p in clip[0])

    def mutated(frame, **kw):
        f = Frame(frame.format, frame.planes, frame.pitches, frame.on_device, frame.source)
        for key, val in kw.items():
            setattr(f, key, val)
        return f

    cases = [
        (1, lambda: enc.encode_frame(mutated(good_dev, pitches=(rb + 4,)))),       # a device pitch that is no multiple of 4 (106)
        (1, lambda: enc.encode_frame(mutated(good_dev, pitches=(0,)))),            # a dense device frame of 34 samples: 102 bytes a row
        (1, lambda: enc.encode_frames_device([good_dev, mutated(good_dev, pitches=(rb,))])),
        (1, lambda: enc.encode_frame(mutated(good_dev, pitches=(rb - 2,)))),       # a pitch below the display size's row bytes
        (4, lambda: enc.encode_frame(Frame.from_array(np.stack(coded_planes, axis=-1)))),  # a frame of the coded size (Python's check)
        (4, lambda: enc.encode_frames_device([Frame.from_array(np.stack(coded_planes, axis=-1))])),
    ]
    for code, call in cases:
        refused(code, call)
        next_frame_continues()
    enc.close()

    # look-ahead: frames queued
    enc = make_encoder(w, h)
    enc.set_lookahead(2)
    assert enc.encode(*model[0]).type == 0
    refused(3, lambda: enc.set_display_size(dw, dh))
    enc.close()

    # spatial layers are not served, in either order; the access units go on as those of an encoder that was not disturbed
    top = list(synth.frames(2 * w, 2 * h, 2, 5))
    svc, svc_ref = SvcEncoder(w, h, 2, 28, 8, 1, 3), SvcEncoder(w, h, 2, 28, 8, 1, 3)
    aus = [svc_ref.encode_au(*f).annexb() for f in top]
    svc_ref.close()
    refused(7, lambda: svc.set_display_size(dw, dh))
    same(svc.encode_au(*top[0]).annexb(), aus[0], "access unit 0")
    refused(7, lambda: svc.set_display_size(dw, dh))
    same(svc.encode_au(*top[1]).annexb(), aus[1], "access unit 1")
    svc.close()
    enc = make_encoder(w, h, (dw, dh))
    assert enc.lib.hl_amd_add_layer(enc._h, w, h) == L.HL_AMD_ERROR_NOT_IMPLEMENTED
    k = 0
    next_frame_continues()  # (still an AVC encoder with its display size)
    enc.close()
