"""Frame ingest on the GPU (hl_amd_encode_frame / hl_amd_encode_frames,
k_ingest): pitched I420 and NV12 repacks of the reference
goldens' inputs must give the goldens byte for byte through every entry point;
RGB frames must be converted exactly as the numpy model converts them
(in_testlib) and then coded exactly as the planar calls code the model's
planes; scene cuts, quality, refusals and the torch device-tensor path."""
import functools
import json
import os

import numpy as np
import pytest

import in_testlib as it
from hartallo_amd import synth
from hl_testlib import GOLDEN, GOLDEN_CONFIGS, GOLDEN_ET_CONFIGS, GOLDEN_RC_CONFIGS, first_diff, golden_input
from sc_testlib import analyse, plan

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(GOLDEN, "golden.json")))
GOLDENS = ["tiny_32x16_qp26", "et_w64_h32_qp36", "qcif_gop3_qp20_me4", "qcif_ippp_qp28_db", "rc_qcif_100k_gop5"]
TABLES = [(it.BT601, it.LIMITED), (it.BT601, it.FULL), (it.BT709, it.LIMITED), (it.BT709, it.FULL)]
TABLE_IDS = ["601l", "601f", "709l", "709f"]
TILE_CROSSING = (1040, 32)  # one tile column and row beyond a workgroup's 1024 x 8 samples (test_emu_ingest.py)


def golden_cfg(name):
    return next(c for c in GOLDEN_CONFIGS + GOLDEN_ET_CONFIGS + GOLDEN_RC_CONFIGS if c[0] == name)


def golden_encoder(name):
    from hartallo_amd import Encoder

    cfg = golden_cfg(name)
    _, w, h, n, qp, me, db, gop, seed = cfg[:9]
    enc = Encoder(w, h, qp, me, db, gop, GOLD[name].get("early_term", 0))
    if len(cfg) > 9:
        enc.set_rate_control(cfg[9], GOLD[name]["fps_num"], GOLD[name]["fps_den"], cfg[10], cfg[11], cfg[12])
    return enc


def same(got, ref, what):
    assert got == ref, f"{what}: first differing byte {first_diff(got, ref)} of {len(got)} / {len(ref)}"


def host_frame(fmt, planes, pads, fill=0xA5):
    """planes (dense 2-D arrays) laid out with pads[c] bytes between the rows, as a Frame on the host"""
    from hartallo_amd import Frame

    bufs = [it.padded_buffer(p, pad, fill) for p, pad in zip(it.pack(fmt, planes), pads)]
    return Frame(fmt, [b.ctypes.data for b, _ in bufs], [pitch for _, pitch in bufs], False, bufs)


def device_frame(fmt, planes, pads, fill=0xA5):
    """the same layout in device memory"""
    import torch

    from hartallo_amd import Frame

    bufs = [it.padded_buffer(p, pad, fill) for p, pad in zip(it.pack(fmt, planes), pads)]
    dev = [torch.from_numpy(b).cuda() for b, _ in bufs]
    torch.cuda.synchronize()
    return Frame(fmt, [d.data_ptr() for d in dev], [pitch for _, pitch in bufs], True, dev)


def planar_ptrs(frames):
    """dense (y, u, v) frames in device memory: the tensor and the pointers encode_batch_device takes"""
    import torch

    flat = np.stack([np.concatenate([p.ravel() for p in f]) for f in frames])
    dev = torch.from_numpy(flat).cuda()
    torch.cuda.synchronize()
    ny = frames[0][0].size
    return dev, [(dev[i].data_ptr(), dev[i].data_ptr() + ny, dev[i].data_ptr() + ny + ny // 4) for i in range(len(frames))]


def code_frames(enc, mode, frames, ctls=None):
    """a list of Frames through one entry point of the frame calls"""
    if mode == "frame":
        return b"".join(enc.encode_frame(f, ctls[i] if ctls else None).annexb() for i, f in enumerate(frames))
    if mode == "frames":
        return b"".join(r.annexb() for r in enc.encode_frames_device(frames, ctls))
    assert mode.startswith("lookahead")
    enc.set_lookahead(int(mode[9:]))
    out = b""
    for i, f in enumerate(frames):
        r = enc.encode_frame(f, ctls[i] if ctls else None)
        out += r.annexb() if r.type else b""
    while (r := enc.flush()).type:
        out += r.annexb()
    return out


def code_planar(enc, mode, frames):
    """dense (y, u, v) frames through the calls that exist without the feature"""
    if mode == "frame":
        return b"".join(enc.encode(*f).annexb() for f in frames)
    if mode == "frames":
        dev, ptrs = planar_ptrs(frames)
        return b"".join(r.annexb() for r in enc.encode_batch_device(ptrs))
    enc.set_lookahead(int(mode[9:]))
    out = b""
    for f in frames:
        r = enc.encode(*f)
        out += r.annexb() if r.type else b""
    while (r := enc.flush()).type:
        out += r.annexb()
    return out


# ---- golden identity ----------------------------------------------------------
@pytest.mark.parametrize("path", ["frame_host", "frame_device", "frames", "lookahead3"])
@pytest.mark.parametrize("form", ["i420_pitched", "nv12_pitched"])
@pytest.mark.parametrize("name", GOLDENS)
def test_repacked_golden_inputs_give_the_goldens(gpu, name, form, path):
    cfg = golden_cfg(name)
    w, h, n = cfg[1], cfg[2], cfg[3]
    clip = golden_input(cfg)
    ref = open(os.path.join(GOLDEN, name + ".264"), "rb").read()
    fmt, pads = (it.I420, (24, 12, 12)) if form == "i420_pitched" else (it.NV12, (8, 8))
    make = device_frame if path in ("frame_device", "frames") else host_frame
    frames = [make(fmt, it.split(clip[f], w, h), pads) for f in range(n)]
    assert frames[0].pitches[0] == w + pads[0] and frames[0].pitches[1] == (w // 2 + 12 if fmt == it.I420 else w + 8)
    enc = golden_encoder(name)
    mode = {"frame_host": "frame", "frame_device": "frame"}.get(path, path)
    same(code_frames(enc, mode, frames), ref, f"{name} {form} {path}")
    if mode != "lookahead3":
        y, u, v = enc.last_input(n - 1 if mode == "frames" else 0)
        want = it.split(clip[n - 1], w, h)
        assert np.array_equal(y, want[0]) and np.array_equal(u, want[1]) and np.array_equal(v, want[2])
        assert enc.bench_ingest(2) > 0  # (the launch can be repeated alone)
    enc.close()


@pytest.mark.parametrize("name", ["tiny_32x16_qp26", "qcif_gop3_qp20_me4"])
def test_dense_i420_device_frames_are_forwarded(gpu, name):
    from hartallo_amd import HlAmdError

    cfg = golden_cfg(name)
    w, h, n = cfg[1], cfg[2], cfg[3]
    clip = golden_input(cfg)
    ref = open(os.path.join(GOLDEN, name + ".264"), "rb").read()
    # pitch 0 and pitch = row bytes both say dense
    frames = [device_frame(it.I420, it.split(clip[f], w, h), (0, 0, 0)) for f in range(n)]
    for f in frames[::2]:
        f.pitches = (0, 0, 0)
    enc = golden_encoder(name)
    same(code_frames(enc, "frames", frames), ref, f"{name} forwarded")
    with pytest.raises(HlAmdError) as e:
        enc.bench_ingest(2)  # nothing was launched
    assert e.value.code == 3
    with pytest.raises(HlAmdError) as e:
        enc.last_input(0)  # the planes are the caller's
    assert e.value.code == 3
    enc.close()
    # a call that mixes forwarded frames with others converts only the others
    mixed = [f if i & 1 else device_frame(it.NV12, it.split(clip[i], w, h), (8, 8)) for i, f in enumerate(frames)]
    enc = golden_encoder(name)
    same(code_frames(enc, "frames", mixed), ref, f"{name} mixed")
    with pytest.raises(HlAmdError):
        enc.last_input(1)
    assert np.array_equal(enc.last_input(0)[0], it.split(clip[0], w, h)[0])
    assert enc.bench_ingest(2) > 0
    enc.close()


def test_forwarded_frames_need_no_alignment_when_they_are_queued(gpu):
    """dense I420 device frames at odd addresses, scene-cut detection and
    quality on: refused where those kernels would read the caller's planes (as
    encode_device refuses them), taken by encode_frame with look-ahead, where
    the queue's copy is what they read (as encode takes any host frame)"""
    import torch

    from hartallo_amd import Frame, HlAmdError

    w, h, n = 48, 32, 4
    ny, fb = w * h, w * h * 3 // 2
    model = rgb_model(w, h, n, (it.BT601, it.LIMITED))
    buf = np.zeros((n, fb + 8), np.uint8)  # a row is a multiple of 8 bytes: every frame starts 1 byte past one
    for i, f in enumerate(model):
        buf[i, 1:1 + fb] = np.concatenate([p.ravel() for p in f])
    dev = torch.from_numpy(buf).cuda()
    torch.cuda.synchronize()
    frames = []
    for i in range(n):
        p = dev[i].data_ptr() + 1
        frames.append(Frame(it.I420, (p, p + ny, p + ny + ny // 4), (0, 0, 0), True, dev))
    assert all(f.planes[0] & 7 == 1 for f in frames)

    def encoder():
        enc = rgb_encoder(w, h, gop=30)
        enc.set_scenecut(192, 1, 8)
        enc.set_quality(True)
        return enc

    ref = encoder()
    want_frames = [ref.encode(*f).annexb() for f in model]
    ref.close()
    ref = encoder()
    want = code_planar(ref, "lookahead2", model)
    ref.close()
    enc = encoder()
    same(enc.encode_frame(host_frame(it.I420, model[0], (24, 12, 12))).annexb(), want_frames[0], "frame 0")
    for call in (lambda: enc.encode_frame(frames[1]), lambda: enc.encode_frames_device(frames[1:])):
        with pytest.raises(HlAmdError) as e:
            call()
        assert e.value.code == 1
    same(enc.encode_frame(host_frame(it.I420, model[1], (24, 12, 12))).annexb(), want_frames[1], "frame 1 after the refusals")
    enc.close()
    enc = encoder()
    same(code_frames(enc, "lookahead2", frames), want, "queued")
    enc.close()


# ---- RGB -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rgb_clip(w, h, n, seeds=(21, 22, 23)):
    """n frames of (R, G, B) planes: the lumas of synth.frames of three seeds.  Shared, read-only."""
    chans = [[y for y, _, _ in synth.frames(w, h, n, s)] for s in seeds]
    out = [tuple(chans[c][f] for c in range(3)) for f in range(n)]
    for f in out:
        for p in f:
            p.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def rgb_model(w, h, n, key, seeds=(21, 22, 23)):
    return [it.rgb_to_i420(*f, *key) for f in rgb_clip(w, h, n, seeds)]


def check_input(enc, k, want, what):
    got = enc.last_input(k)
    for name, g, m in zip("YUV", got, want):
        assert np.array_equal(g, m), f"{what}: {name} of picture {k}: {np.count_nonzero(g != m)} samples differ"


def rgb_encoder(w, h, key=None, gop=3):
    from hartallo_amd import Encoder

    enc = Encoder(w, h, 28, 8, 1, gop, 0)
    if key is not None:
        enc.set_colour(*key)
    return enc


@pytest.mark.parametrize("key", TABLES, ids=TABLE_IDS)
@pytest.mark.parametrize("fmt", ["rgb24", "rgba32", "rgbp"])
@pytest.mark.parametrize("size", [(48, 32, 4), (176, 144, 3)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_rgb_is_converted_as_the_model_and_coded_as_its_planes(gpu, size, fmt, key):
    w, h, n = size
    clip, model = rgb_clip(w, h, n), rgb_model(w, h, n, key)
    F = it.FORMATS[fmt]
    pads = {it.RGB24: (12,), it.RGBA32: (16,), it.RGBP: (8, 8, 8)}[F]
    what = f"{w}x{h} {fmt} {key}"
    # one frame per call, from the host
    enc, ref = rgb_encoder(w, h, key), rgb_encoder(w, h)
    for k in range(n):
        got = enc.encode_frame(host_frame(F, clip[k], pads)).annexb()
        check_input(enc, 0, model[k], what + " frame")
        same(got, ref.encode(*model[k]).annexb(), f"{what} frame {k}")
    enc.close(), ref.close()
    # one call for the clip, from device memory
    enc, ref = rgb_encoder(w, h, key), rgb_encoder(w, h)
    got = code_frames(enc, "frames", [device_frame(F, clip[k], pads) for k in range(n)])
    for k in range(n):
        check_input(enc, k, model[k], what + " frames")
    same(got, code_planar(ref, "frames", model), what + " frames")
    assert enc.bench_ingest(2) > 0
    enc.close(), ref.close()
    # look-ahead of 2 with a flush (n = 3: one frame is left to the flush)
    enc, ref = rgb_encoder(w, h, key), rgb_encoder(w, h)
    frames = [host_frame(F, clip[k], pads) if k & 1 else device_frame(F, clip[k], pads) for k in range(n)]
    same(code_frames(enc, "lookahead2", frames), code_planar(ref, "lookahead2", model), what + " lookahead2")
    enc.close(), ref.close()


def test_rgb_at_the_tile_crossing_size(gpu):
    w, h = TILE_CROSSING
    key = (it.BT709, it.LIMITED)
    clip, model = rgb_clip(w, h, 2), rgb_model(w, h, 2, key)
    for fmt, pads in ((it.RGB24, (0,)), (it.RGBA32, (4,)), (it.RGBP, (16, 16, 16))):
        enc, ref = rgb_encoder(w, h, key), rgb_encoder(w, h)
        got = code_frames(enc, "frames", [device_frame(fmt, f, pads) for f in clip])
        for k in range(2):
            check_input(enc, k, model[k], f"{w}x{h} format {fmt}")
        same(got, code_planar(ref, "frames", model), f"{w}x{h} format {fmt}")
        enc.close(), ref.close()


def test_rgb_host_frames_in_strided_views(gpu):
    """a cropped view of a larger interleaved image, and planes taken out of a taller planar stack"""
    from hartallo_amd import Frame

    w, h, n = 48, 32, 4
    clip, model = rgb_clip(w, h, n), rgb_model(w, h, n, (it.BT601, it.LIMITED))
    enc, ref = rgb_encoder(w, h), rgb_encoder(w, h)
    rng = np.random.default_rng(3)
    for k in range(n):
        if k & 1:
            big = rng.integers(0, 256, (h + 9, w + 20, 3), dtype=np.uint8)
            view = big[5:5 + h, 7:7 + w]
            view[...] = np.stack(clip[k], axis=-1)
        else:
            big = rng.integers(0, 256, (5, h + 4, w + 8), dtype=np.uint8)
            view = big[0:5:2, 2:2 + h, 8:8 + w]
            view[...] = np.stack(clip[k])
        f = Frame.from_array(view)
        assert not f.on_device and f.pitches[0] == (3 * (w + 20) if k & 1 else w + 8)
        got = enc.encode_frame(f).annexb()
        check_input(enc, 0, model[k], f"view {k}")
        same(got, ref.encode(*model[k]).annexb(), f"view {k}")
    enc.close(), ref.close()


def test_rgb_torch_device_tensors(gpu):
    import torch

    from hartallo_amd import Frame

    assert torch.cuda.is_available(), "a gpu test: torch must see the device the encoder runs on"
    w, h, n = 48, 32, 4
    key = (it.BT709, it.FULL)
    clip, model = rgb_clip(w, h, n), rgb_model(w, h, n, key)
    hwc = torch.from_numpy(np.stack([np.stack(f, axis=-1) for f in clip])).cuda()    # (n, H, W, 3)
    chw = torch.from_numpy(np.stack([np.stack(f) for f in clip])).cuda()             # (n, 3, H, W)
    wide = torch.zeros((n, h, w + 16, 4), dtype=torch.uint8, device="cuda")           # RGBA, cropped below
    wide[:, :, 4:4 + w, :3] = hwc
    torch.cuda.synchronize()
    ref = rgb_encoder(w, h)
    want = code_planar(ref, "frames", model)
    ref.close()
    for what, frames in (("HWC", [Frame.from_array(hwc[k]) for k in range(n)]), ("CHW", [Frame.from_array(chw[k]) for k in range(n)]),
                         ("cropped RGBA", [Frame.from_array(wide[k, :, 4:4 + w]) for k in range(n)])):
        assert all(f.on_device for f in frames)
        enc = rgb_encoder(w, h, key)
        got = code_frames(enc, "frames", frames)
        for k in range(n):
            check_input(enc, k, model[k], what)
        same(got, want, what)
        enc.close()


# ---- scene cuts, quality, set_colour -------------------------------------------
def test_scene_cuts_and_quality_follow_the_converted_planes(gpu):
    """RGB content that changes at frame 4: picture types, scene statistics,
    quality sums and bytes are those of the planar call on the model's planes"""
    w, h = 64, 48
    key = (it.BT601, it.LIMITED)
    clip = rgb_clip(w, h, 4) + rgb_clip(w, h, 4, (31, 32, 33))
    model = rgb_model(w, h, 4, key) + rgb_model(w, h, 4, key, (31, 32, 33))
    flat = [np.concatenate([p.ravel() for p in f]) for f in model]
    turned, idr = plan(analyse(flat, w, h, 8), 192, 1, 30)
    assert turned[4] and idr == [True, False, False, False, True, False, False, False]  # the clip has the cut the test is about
    encs = []
    for _ in range(2):
        enc = rgb_encoder(w, h, key, gop=30)
        enc.set_scenecut(192, 1, 8)
        enc.set_quality(True)
        encs.append(enc)
    enc, ref = encs
    got = enc.encode_frames_device([device_frame(it.RGBP, f, (8, 8, 8)) for f in clip])
    dev, ptrs = planar_ptrs(model)
    want = ref.encode_batch_device(ptrs)
    for k in range(8):
        same(got[k].annexb(), want[k].annexb(), f"picture {k}")
        assert (got[k].data[0] & 31 == 5) == idr[k]
        assert enc.last_scene_stats(k) == ref.last_scene_stats(k) and enc.last_scene_stats(k)["turned"] == turned[k]
        assert enc.last_quality(k) == ref.last_quality(k)
        check_input(enc, k, model[k], "scene clip")
    # the next frame, alone and from the host: compared with the batch's last frame
    f = host_frame(it.RGB24, clip[0], (12,))
    same(enc.encode_frame(f).annexb(), ref.encode(*model[0]).annexb(), "frame after the batch")
    assert enc.last_scene_stats(0) == ref.last_scene_stats(0) and enc.last_scene_stats(0)["turned"]
    assert enc.last_quality(0) == ref.last_quality(0)
    enc.close(), ref.close()


def test_set_colour_changes_the_following_frames_only(gpu):
    w, h, n = 48, 32, 4
    clip = rgb_clip(w, h, n)
    keys = [(it.BT601, it.LIMITED), (it.BT709, it.FULL), (it.BT709, it.FULL), (it.BT601, it.FULL)]
    model = [rgb_model(w, h, n, keys[k])[k] for k in range(n)]
    enc, ref = rgb_encoder(w, h), rgb_encoder(w, h)
    for k in range(n):
        if k and keys[k] != keys[k - 1]:
            enc.set_colour(*keys[k])
        got = enc.encode_frame(host_frame(it.RGB24, clip[k], (0,))).annexb()
        check_input(enc, 0, model[k], f"frame {k} with {keys[k]}")
        same(got, ref.encode(*model[k]).annexb(), f"frame {k}")
    # I420 and NV12 are copies whatever the colour setting is
    yuv = rgb_model(w, h, n, keys[0])[0]
    same(enc.encode_frame(host_frame(it.NV12, yuv, (8, 8))).annexb(), ref.encode(*yuv).annexb(), "NV12 under BT.601 full")
    enc.close(), ref.close()


# ---- refusals --------------------------------------------------------------------
def test_refusals_leave_the_stream_as_it_was(gpu):
    from hartallo_amd import Frame, FrameCtl, HlAmdError, SvcEncoder
    from hartallo_amd import _lib as L

    w, h, n = 48, 32, 4
    clip, model = rgb_clip(w, h, 13), rgb_model(w, h, 13, (it.BT601, it.LIMITED))  # one frame after each of the 11 refusals, one before, one after
    ref = rgb_encoder(w, h)
    want = [ref.encode(*m).annexb() for m in model]
    ref.close()
    enc = rgb_encoder(w, h)
    good_host = host_frame(it.RGB24, clip[0], (12,))
    good_dev = device_frame(it.RGB24, clip[0], (12,))

    def refused(code, call):
        with pytest.raises(HlAmdError) as e:
            call()
        assert e.value.code == code, (e.value.code, code)
        for probe in (lambda: enc.last_input(0), lambda: enc.bench_ingest(1)):  # a refused call leaves nothing to show
            with pytest.raises(HlAmdError) as e:
                probe()
            assert e.value.code == 3

    def mutated(frame, **kw):
        f = Frame(frame.format, frame.planes, frame.pitches, frame.on_device, frame.source)
        for k, v in kw.items():
            setattr(f, k, v)
        return f

    with pytest.raises(HlAmdError) as e:
        enc.last_input(0)  # before any frame call
    assert e.value.code == 3
    k = 0

    def next_frame_continues():
        nonlocal k
        same(enc.encode_frame(host_frame(it.RGB24, clip[k], (12,))).annexb(), want[k], f"frame {k} after a refusal")
        check_input(enc, 0, model[k], f"frame {k}")
        k += 1

    next_frame_continues()
    rgb_row = 3 * w
    cases = [
        (1, lambda: enc.encode_frame(mutated(good_host, format=9))),                                   # unknown format
        (1, lambda: enc.encode_frame(mutated(good_host, planes=(0,)))),                                # a null plane
        (1, lambda: enc.encode_frame(mutated(good_host, pitches=(rgb_row - 1,)))),                     # pitch below row bytes
        (1, lambda: enc.encode_frame(mutated(good_host, pitches=(-rgb_row,)))),                        # negative pitch
        (1, lambda: enc.encode_frame(mutated(good_dev, planes=(good_dev.planes[0] + 1,)))),            # misaligned device plane
        (1, lambda: enc.encode_frame(mutated(good_dev, pitches=(rgb_row + 6,)))),                      # misaligned device pitch
        (1, lambda: enc.encode_frame(mutated(host_frame(it.NV12, model[0], (8, 8)), planes=(good_host.planes[0], 0)))),  # NV12 without UV
        (1, lambda: enc.encode_frames_device([good_dev, good_host])),                                   # a host frame in the device call
        (1, lambda: enc.encode_frames_device([good_dev, mutated(good_dev, pitches=(rgb_row - 4,))])),   # any frame of a call
        (7, lambda: enc.encode_frame(good_host, FrameCtl(L.HL_AMD_ENCODING_RAW, 8, 1, 0, 3))),          # the ctl, as in the _ex calls
        (7, lambda: enc.encode_frames_device([good_dev], [FrameCtl(L.HL_AMD_ENCODING_LOSSLESS, 8, 1, 0, 3)])),
    ]
    for code, call in cases:
        refused(code, call)
        next_frame_continues()
    for bad in ((2, 0), (0, 2), (-1, 0)):
        with pytest.raises(HlAmdError) as e:
            enc.set_colour(*bad)
        assert e.value.code == 1
    next_frame_continues()  # (still BT.601 limited)
    assert k == len(cases) + 2 <= len(want)
    enc.close()

    # look-ahead: frames queued
    enc = rgb_encoder(w, h)
    enc.set_lookahead(3)
    assert enc.encode_frame(good_host).type == 0
    for call in (lambda: enc.encode_frames_device([good_dev]), lambda: enc.set_colour(it.BT709, it.FULL)):
        with pytest.raises(HlAmdError) as e:
            call()
        assert e.value.code == 3
    with pytest.raises(HlAmdError) as e:
        enc.last_input(0)  # with look-ahead on
    assert e.value.code == 3
    assert enc.encode_frame(host_frame(it.RGB24, clip[1], (12,))).type == 0
    out = b""
    while (r := enc.flush()).type:
        out += r.annexb()
    same(out, want[0] + want[1], "look-ahead after the refusals")
    enc.close()

    # spatial layers are not served; the access units go on as those of an encoder that was not disturbed
    top = list(synth.frames(2 * w, 2 * h, 3, 5))
    svc, svc_ref = SvcEncoder(w, h, 2, 28, 8, 1, 3), SvcEncoder(w, h, 2, 28, 8, 1, 3)
    aus = [svc_ref.encode_au(*f).annexb() for f in top]
    svc_ref.close()
    same(svc.encode_au(*top[0]).annexb(), aus[0], "access unit 0")
    for a, call in enumerate((lambda: svc.encode_frame(good_host), lambda: svc.encode_frames_device([good_dev])), 1):
        with pytest.raises(HlAmdError) as e:
            call()
        assert e.value.code == 7
        same(svc.encode_au(*top[a]).annexb(), aus[a], f"access unit {a} after a refusal")
    svc.close()

    # any other encode call: nothing of a frame call is left to show
    enc = rgb_encoder(w, h)
    enc.encode_frame(good_host)
    enc.last_input(0)
    enc.encode(*model[1])
    with pytest.raises(HlAmdError) as e:
        enc.last_input(0)
    assert e.value.code == 3
    enc.close()
