"""The area downscaler on the GPU (hl_amd_set_source_size):
frames of a source size above the display size are converted by k_ingest,
scaled by k_scale exactly as sk_testlib's model scales them, padded by edge
replication and then coded as those planes -- per frame, per call, through the
look-ahead, across a change of the source size, with scene cuts and quality on;
with the feature off the path is the one before it; refusals leave the stream
as it was."""
import functools
import json
import os

import numpy as np
import pytest

import in_testlib as it
import sk_testlib as sk
from hartallo_amd import synth
from hl_testlib import GOLDEN, GOLDEN_CONFIGS, first_diff, golden_input

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(GOLDEN, "golden.json")))
KEY = (it.BT709, it.LIMITED)
N = 5  # frames of a clip: with a GOP of 3 an IDR, two P, an IDR, a P
FORMS = {"nv12": it.NV12, "rgb24": it.RGB24, "i420": it.I420}
ALL_FORMATS = ["i420", "nv12", "rgb24", "rgba32", "rgbp"]


def same(got, ref, what):
    assert got == ref, f"{what}: first differing byte {first_diff(got, ref)} of {len(got)} / {len(ref)}"


def make_encoder(coded, disp=None, source=None, gop=3, quality=False, scenecut=False):
    from hartallo_amd import Encoder

    enc = Encoder(*coded, 28, 8, 1, gop, 0)
    enc.set_colour(*KEY)
    if disp and tuple(disp) != tuple(coded):
        enc.set_display_size(*disp)
    if source:
        enc.set_source_size(*source)
        assert enc.source_size == tuple(source)
    if quality:
        enc.set_quality(True)
    if scenecut:
        enc.set_scenecut(192, 1, 8)
    return enc


def yuv(F):
    return F in (it.I420, it.NV12)


@functools.lru_cache(maxsize=None)
def model_clip(shape, F, n=N, seeds=(21, 22, 23)):
    src, disp, coded = shape
    return [sk.model_planes(F, f, KEY, disp, coded) for f in sk.clip_planes(*src, yuv(F), n, seeds)]


@functools.lru_cache(maxsize=None)
def reference_stream(shape, F):
    """a fresh encoder with the same display size fed the model's planes through encode"""
    _, disp, coded = shape
    ref = make_encoder(coded, disp)
    out = [ref.encode(*f).annexb() for f in model_clip(shape, F)]
    ref.close()
    return out


def check_input(enc, k, want, what):
    got = enc.last_input(k)
    for name, g, m in zip("YUV", got, want):
        assert g.shape == m.shape and np.array_equal(g, m), f"{what}: {name} of picture {k}: {np.count_nonzero(g != m)} samples differ"


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


# ---- per frame ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("shape", sk.SHAPES, ids=sk.shape_id)
def test_a_frame_is_scaled_as_the_model_and_coded_as_its_planes(gpu, shape, form):
    """NV12 and I420 pitched, RGB24 as dense as the 4-byte rule allows; from the host (two pitches) and from device memory"""
    src, disp, coded = shape
    F = FORMS[form]
    clip, model, want = sk.clip_planes(*src, yuv(F)), model_clip(shape, F), reference_stream(shape, F)
    what = f"{form} {sk.shape_id(shape)}"
    dev_pads = sk.pads_for(F, src[0], 0 if F == it.RGB24 else 8)
    enc = make_encoder(coded, disp, src)
    for k in range(N):
        if k % 3 == 0:
            f = sk.host_frame(F, clip[k], tuple(6 for _ in dev_pads))
        elif k % 3 == 1:
            f = sk.device_frame(F, clip[k], dev_pads)
            assert all(p % 4 == 0 for p in f.pitches)
        else:
            f = sk.host_frame(F, clip[k], tuple(0 for _ in dev_pads))
        got = enc.encode_frame(f).annexb()
        check_input(enc, 0, model[k], f"{what} frame {k}")
        same(got, want[k], f"{what} frame {k}")
    assert enc.bench_scale(2) > 0 and enc.bench_ingest(2) > 0  # (each stage's launches can be repeated alone)
    check_input(enc, 0, model[N - 1], f"{what} after the repetitions")
    enc.close()


# ---- one call for the clip, and the look-ahead ---------------------------------------------------
@pytest.mark.parametrize("fmt", ALL_FORMATS)
@pytest.mark.parametrize("shape", [sk.SHAPES[2], sk.SHAPES[7]], ids=sk.shape_id)
def test_frames_calls_and_the_lookahead(gpu, shape, fmt):
    src, disp, coded = shape
    F = it.FORMATS[fmt]
    clip, model, want = sk.clip_planes(*src, yuv(F)), model_clip(shape, F), reference_stream(shape, F)
    what = f"{fmt} {sk.shape_id(shape)}"
    pads = sk.pads_for(F, src[0])
    enc = make_encoder(coded, disp, src)
    got = enc.encode_frames_device([sk.device_frame(F, clip[k], pads, 0xA5 if k & 1 else 0x3C) for k in range(N)])
    for k in range(N):
        check_input(enc, k, model[k], f"{what} frames")
        same(got[k].annexb(), want[k], f"{what} frames, picture {k}")
    assert enc.bench_scale(2) > 0 and enc.bench_ingest(2) > 0
    enc.close()
    # a look-ahead of 3 with a flush (5 frames: two are left to the flush)
    enc = make_encoder(coded, disp, src)
    frames = [sk.host_frame(F, clip[k], tuple(2 for _ in pads)) if k & 1 else sk.device_frame(F, clip[k], pads) for k in range(N)]
    same(lookahead(enc, 3, [functools.partial(enc.encode_frame, f) for f in frames]), b"".join(want), what + " lookahead3")
    enc.close()


def test_mixed_formats_in_one_call(gpu):
    """one ingest launch per format, one scale launch for the call"""
    shape = sk.SHAPES[2]
    src, disp, coded = shape
    fmts = [it.NV12, it.RGB24, it.I420, it.NV12, it.RGBP]
    frames = [sk.device_frame(F, sk.clip_planes(*src, yuv(F))[k], sk.pads_for(F, src[0])) for k, F in enumerate(fmts)]
    enc = make_encoder(coded, disp, src, gop=1)
    ref = make_encoder(coded, disp, gop=1)
    got = enc.encode_frames_device(frames)
    for k, F in enumerate(fmts):
        check_input(enc, k, model_clip(shape, F)[k], f"mixed, picture {k}")
        same(got[k].annexb(), ref.encode(*model_clip(shape, F)[k]).annexb(), f"mixed, picture {k}")
    enc.close(), ref.close()


# ---- CIF to QCIF is the SVC layers' filter ----------------------------------------------------------
def test_cif_to_qcif_is_down2(gpu):
    clip = sk.clip_planes(352, 288, True)
    enc, ref = make_encoder((176, 144), None, (352, 288)), make_encoder((176, 144))
    for k in range(N):
        small = tuple(synth._down2(p) for p in clip[k])
        got = enc.encode_frame(sk.device_frame(it.NV12, clip[k], (8, 8))).annexb()
        check_input(enc, 0, small, f"frame {k}")
        same(got, ref.encode(*small).annexb(), f"frame {k}")
    enc.close(), ref.close()


# ---- a source that changes its resolution -------------------------------------------------------------
def test_the_source_size_changes_mid_stream(gpu):
    a, b = sk.SHAPES[0], sk.SHAPES[1]  # 96x64, then 72x48, into 48x32
    coded = a[2]
    model = model_clip(a, it.NV12)[:3] + model_clip(b, it.NV12)[3:]
    ref = make_encoder(coded)
    want = [ref.encode(*m).annexb() for m in model]
    ref.close()
    enc = make_encoder(coded, None, a[0])
    for k in range(N):
        if k == 3:
            enc.set_source_size(*b[0])
            assert enc.source_size == b[0]
        shape = a if k < 3 else b
        f = sk.device_frame(it.NV12, sk.clip_planes(*shape[0], True)[k], (8, 8))
        got = enc.encode_frame(f).annexb()
        check_input(enc, 0, model[k], f"frame {k}")
        same(got, want[k], f"frame {k}")
    # and back to none: a dense I420 device frame of the coded size is forwarded again
    enc.set_source_size(*coded)
    assert enc.source_size == coded
    enc.close()


# ---- scene cuts and quality ------------------------------------------------------------------------------
def test_scene_cuts_and_quality_read_the_scaled_planes(gpu):
    """content that changes at frame 4: picture types, scene statistics, quality
    sums and bytes are those of the planar call on the model's planes"""
    from sc_testlib import analyse, plan

    shape = ((150, 102), (50, 34), (64, 48))  # 3:1 into a display size below the coded size
    src, disp, coded = shape
    clip = list(sk.clip_planes(*src, False, 4)) + list(sk.clip_planes(*src, False, 4, (31, 32, 33)))
    model = model_clip(shape, it.RGB24, 4) + model_clip(shape, it.RGB24, 4, (31, 32, 33))
    flat = [np.concatenate([np.ascontiguousarray(p).ravel() for p in f]) for f in model]
    turned, idr = plan(analyse(flat, *coded, 8), 192, 1, 30)
    assert turned[4] and idr == [True, False, False, False, True, False, False, False]  # the clip has the cut the test is about
    enc = make_encoder(coded, disp, src, gop=30, quality=True, scenecut=True)
    ref = make_encoder(coded, disp, gop=30, quality=True, scenecut=True)
    got = enc.encode_frames_device([sk.device_frame(it.RGBA32, f, (8,)) for f in clip])
    dev, ptrs = planar_ptrs(model)
    want = ref.encode_batch_device(ptrs)
    for k in range(8):
        same(got[k].annexb(), want[k].annexb(), f"picture {k}")
        assert (got[k].data[0] & 31 == 5) == idr[k]
        assert enc.last_scene_stats(k) == ref.last_scene_stats(k) and enc.last_scene_stats(k)["turned"] == turned[k]
        assert enc.last_quality(k) == ref.last_quality(k)
        check_input(enc, k, model[k], "scene clip")
    enc.close(), ref.close()


# ---- the feature off -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["never_set", "set_to_the_display_size", "set_and_taken_back"])
def test_without_a_source_size_nothing_changes(gpu, how):
    from hartallo_amd import Encoder, HlAmdError

    name = "qcif_ippp_qp28_db"
    cfg = next(c for c in GOLDEN_CONFIGS if c[0] == name)
    _, w, h, n, qp, me, db, gop, seed = cfg[:9]
    clip = golden_input(cfg)
    ref = open(os.path.join(GOLDEN, name + ".264"), "rb").read()

    def encoder():
        enc = Encoder(w, h, qp, me, db, gop, GOLD[name].get("early_term", 0))
        if how == "set_to_the_display_size":
            enc.set_source_size(w, h)
        elif how == "set_and_taken_back":
            enc.set_source_size(2 * w, 2 * h)
            enc.set_source_size(w, h)
        assert enc.source_size == (w, h) == enc.display_size
        return enc

    enc = encoder()
    frames = [sk.device_frame(it.NV12, it.split(clip[f], w, h), (8, 8)) for f in range(n)]
    same(b"".join(r.annexb() for r in enc.encode_frames_device(frames)), ref, f"{name} {how}")
    assert np.array_equal(enc.last_input(n - 1)[0], it.split(clip[n - 1], w, h)[0])
    with pytest.raises(HlAmdError) as e:
        enc.bench_scale(2)  # nothing was scaled
    assert e.value.code == 3
    enc.close()
    # dense I420 device frames are still forwarded: no copy, no kernel
    enc = encoder()
    frames = [sk.device_frame(it.I420, it.split(clip[f], w, h), (0, 0, 0)) for f in range(n)]
    same(b"".join(r.annexb() for r in enc.encode_frames_device(frames)), ref, f"{name} {how} forwarded")
    for call in (lambda: enc.last_input(0), lambda: enc.bench_ingest(2), lambda: enc.bench_scale(2)):
        with pytest.raises(HlAmdError) as e:
            call()
        assert e.value.code == 3
    enc.close()


# ---- refusals ---------------------------------------------------------------------------------------------------
def test_refusals_leave_the_stream_as_it_was(gpu):
    from hartallo_amd import Frame, HlAmdError, SvcEncoder
    from hartallo_amd import _lib as L

    shape = sk.SHAPES[2]  # 50x34 -> 34x18 in 48x32
    src, disp, coded = shape
    clip = sk.clip_planes(*src, False, 16)
    model = model_clip(shape, it.RGB24, 16)
    ref = make_encoder(coded, disp)
    want = [ref.encode(*m).annexb() for m in model]
    ref.close()
    enc = make_encoder(coded, disp)
    k = 0

    def refused(code, call):
        with pytest.raises(HlAmdError) as e:
            call()
        assert e.value.code == code, (e.value.code, code)

    def next_frame_continues():
        nonlocal k
        same(enc.encode_frame(sk.host_frame(it.RGB24, clip[k], (6,))).annexb(), want[k], f"frame {k} after a refusal")
        check_input(enc, 0, model[k], f"frame {k}")
        k += 1

    # odd, below the display size, above 8x, above 4096: refused, and the setting stays what it was
    for bad in ((49, 34), (50, 33), (32, 18), (34, 16), (274, 34), (50, 146), (0, 0), (-50, 34), (4098, 34), (50, 4098), (1 << 30, 1 << 30)):
        refused(L.HL_AMD_ERROR_INVALID_PARAMETER, lambda: enc.set_source_size(*bad))
        assert enc.source_size == disp
    enc.set_source_size(272, 144)  # the limits themselves: 8 x 34, 8 x 18
    assert enc.source_size == (272, 144)
    enc.set_source_size(*src)
    next_frame_continues()
    for bad in ((49, 34), (32, 18), (274, 34)):
        refused(L.HL_AMD_ERROR_INVALID_PARAMETER, lambda: enc.set_source_size(*bad))
        assert enc.source_size == src
        next_frame_continues()
    # the display size comes first
    refused(L.HL_AMD_ERROR_INVALID_STATE, lambda: enc.set_display_size(*disp))
    next_frame_continues()
    good_dev = sk.device_frame(it.RGB24, clip[0], (2,))
    rb = 3 * src[0]  # 150: no multiple of 4

    def mutated(frame, **kw):
        f = Frame(frame.format, frame.planes, frame.pitches, frame.on_device, frame.source)
        for key, val in kw.items():
            setattr(f, key, val)
        return f

    disp_planes = tuple(np.ascontiguousarray(p[:disp[1], :disp[0]]) for p in clip[0])
    y50 = sk.device_frame(it.I420, sk.clip_planes(*src, True)[0], (0, 0, 0))
    cases = [
        (L.HL_AMD_ERROR_INVALID_FORMAT, lambda: enc.encode_frame(Frame.from_array(np.stack(disp_planes, axis=-1)))),  # a frame of the display size (Python's check)
        (L.HL_AMD_ERROR_INVALID_FORMAT, lambda: enc.encode_frames_device([Frame.from_array(np.stack(disp_planes, axis=-1))])),
        (L.HL_AMD_ERROR_INVALID_PARAMETER, lambda: enc.encode_frame(mutated(y50, pitches=(0, 0, 0)))),  # a dense device frame of width 50: 50 and 25 bytes a row
        (L.HL_AMD_ERROR_INVALID_PARAMETER, lambda: enc.encode_frames_device([good_dev, mutated(good_dev, pitches=(0,))])),  # 150 bytes a row
        (L.HL_AMD_ERROR_INVALID_PARAMETER, lambda: enc.encode_frame(mutated(good_dev, pitches=(3 * disp[0] + 2,)))),  # a pitch for the display size: below the source's row bytes
        (L.HL_AMD_ERROR_INVALID_PARAMETER, lambda: enc.encode_frame(mutated(good_dev, pitches=(rb - 2,)))),
    ]
    for code, call in cases:
        refused(code, call)
        next_frame_continues()
    assert enc.lib.hl_amd_add_layer(enc._h, *coded) == L.HL_AMD_ERROR_NOT_IMPLEMENTED
    next_frame_continues()  # (still an AVC encoder with its source size)
    enc.close()

    # look-ahead: frames queued
    enc = make_encoder(coded, disp)
    enc.set_lookahead(2)
    assert enc.encode(*model[0]).type == 0
    refused(L.HL_AMD_ERROR_INVALID_STATE, lambda: enc.set_source_size(*src))
    assert enc.source_size == disp
    enc.close()

    # spatial layers are not served; the access units go on as those of an encoder that was not disturbed
    w, h = coded
    top = list(synth.frames(2 * w, 2 * h, 2, 5))
    svc, svc_ref = SvcEncoder(w, h, 2, 28, 8, 1, 3), SvcEncoder(w, h, 2, 28, 8, 1, 3)
    aus = [svc_ref.encode_au(*f).annexb() for f in top]
    svc_ref.close()
    refused(L.HL_AMD_ERROR_NOT_IMPLEMENTED, lambda: svc.set_source_size(2 * w, 2 * h))
    same(svc.encode_au(*top[0]).annexb(), aus[0], "access unit 0")
    refused(L.HL_AMD_ERROR_NOT_IMPLEMENTED, lambda: svc.set_source_size(w, h))
    same(svc.encode_au(*top[1]).annexb(), aus[1], "access unit 1")
    svc.close()
