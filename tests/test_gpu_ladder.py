"""The rendition ladder on the GPU (hl_amd_encode_ladder_frame(s), DESIGN.md
6.15): one frame call feeds several encoders of one common source size -- the
frames are converted once by k_ingest, k_scale_fan writes every rung's planes
exactly as sk_testlib's model scales them, and every rung's stream is, byte for
byte, that of a fresh encoder of the same sizes fed the same frames alone: per
frame, per call, with its own ctl, quality, scene cuts and rate control, across
plain calls in between and a change of the source size; every refusal leaves
every stream as it was; with no ladder call made the path is the one before."""
import functools
import json
import os

import numpy as np
import pytest

import in_testlib as it
import ld_testlib as ld
import sk_testlib as sk
from hartallo_amd import synth
from hl_testlib import GOLDEN, GOLDEN_CONFIGS, first_diff, golden_input

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(GOLDEN, "golden.json")))
KEY = (it.BT709, it.LIMITED)
N = 5  # frames of a clip: with a GOP of 3 an IDR, two P, an IDR, a P
FORMS = {"nv12": it.NV12, "rgb24": it.RGB24, "i420": it.I420}
NR = 20  # frames of the refusals' clip: one ladder call after every refusal
ALL_FORMATS = ["i420", "nv12", "rgb24", "rgba32", "rgbp"]


def same(got, ref, what):
    assert got == ref, f"{what}: first differing byte {first_diff(got, ref)} of {len(got)} / {len(ref)}"


def make_encoder(coded, disp=None, source=None, gop=3, quality=False, scenecut=False, key=KEY):
    from hartallo_amd import Encoder

    enc = Encoder(*coded, 28, 8, 1, gop, 0)
    enc.set_colour(*key)
    if disp and tuple(disp) != tuple(coded):
        enc.set_display_size(*disp)
    if source:
        enc.set_source_size(*source)  # (the display size itself: an identity rung, no source size)
        assert enc.source_size == tuple(source)
    if quality:
        enc.set_quality(True)
    if scenecut:
        enc.set_scenecut(192, 1, 8)
    return enc


def rung_encoders(src, rungs, **kw):
    return [make_encoder(coded, disp, src, **kw) for disp, coded in rungs]


def close(*groups):
    for g in groups:
        for e in g:
            e.close()


def yuv(F):
    return F in (it.I420, it.NV12)


@functools.lru_cache(maxsize=None)
def model_clip(src, disp, coded, F, n=N, seeds=(21, 22, 23)):
    return [sk.model_planes(F, f, KEY, disp, coded) for f in sk.clip_planes(*src, yuv(F), n, seeds)]


def check_input(enc, k, want, what):
    got = enc.last_input(k)
    for name, g, m in zip("YUV", got, want):
        assert g.shape == m.shape and np.array_equal(g, m), f"{what}: {name} of picture {k}: {np.count_nonzero(g != m)} samples differ"


def mixed_frame(F, planes, k, width):
    """host frames of two pitches and device frames across a clip"""
    dev_pads = sk.pads_for(F, width, 0 if F == it.RGB24 else 8)
    if k % 3 == 0:
        return sk.host_frame(F, planes, tuple(6 for _ in dev_pads))
    if k % 3 == 1:
        f = sk.device_frame(F, planes, dev_pads)
        assert all(p % 4 == 0 for p in f.pitches)
        return f
    return sk.host_frame(F, planes, tuple(0 for _ in dev_pads))


def ctl(encoding=0, gop=3):
    from hartallo_amd import FrameCtl

    return FrameCtl(encoding, 8, 1, 0, gop)


def is_idr(result):
    return result.data[0] & 31 == 5


# ---- per frame ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("name", sorted(ld.LADDERS))
def test_a_frame_feeds_every_rung_as_the_model_and_as_the_lone_encoder(gpu, name, form):
    from hartallo_amd import Encoder

    src, rungs = ld.LADDERS[name]
    F = FORMS[form]
    clip = sk.clip_planes(*src, yuv(F))
    encs, lone = rung_encoders(src, rungs), rung_encoders(src, rungs)
    down2 = make_encoder((48, 32)) if name == "L1" else None  # L1's 2:1 rung: the SVC layers' 2x2 box of the clip
    for k in range(N):
        got = Encoder.encode_ladder_frame(encs, mixed_frame(F, clip[k], k, src[0]))
        assert len(got) == len(rungs)
        for r, (disp, coded) in enumerate(rungs):
            what = f"{name} {form} rung {r} frame {k}"
            check_input(encs[r], 0, model_clip(src, disp, coded, F)[k], what)
            same(got[r].annexb(), lone[r].encode_frame(mixed_frame(F, clip[k], k, src[0])).annexb(), what)
        if down2:
            i420 = clip[k] if yuv(F) else it.rgb_to_i420(*clip[k], *KEY)
            same(got[1].annexb(), down2.encode(*(synth._down2(p) for p in i420)).annexb(), f"{name} {form} frame {k}: the 2:1 rung against _down2")
    assert encs[0].bench_ladder(2) > 0 and encs[0].bench_ingest(2) > 0  # (each stage's launches can be repeated alone)
    for r, (disp, coded) in enumerate(rungs):
        check_input(encs[r], 0, model_clip(src, disp, coded, F)[N - 1], f"{name} {form} rung {r} after the repetitions")
    close(encs, lone, [down2] if down2 else [])


# ---- one call for the clip ------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ALL_FORMATS)
@pytest.mark.parametrize("name", ["L1", "L2", "L4"])
def test_a_frames_call_feeds_every_rung(gpu, name, fmt):
    from hartallo_amd import Encoder

    src, rungs = ld.LADDERS[name]
    F = it.FORMATS[fmt]
    clip = sk.clip_planes(*src, yuv(F))
    pads = sk.pads_for(F, src[0])
    frames = [sk.device_frame(F, clip[k], pads, 0xA5 if k & 1 else 0x3C) for k in range(N)]
    encs, lone = rung_encoders(src, rungs), rung_encoders(src, rungs)
    got = Encoder.encode_ladder_frames_device(encs, frames)
    for r, (disp, coded) in enumerate(rungs):
        want = lone[r].encode_frames_device(frames)
        for k in range(N):
            check_input(encs[r], k, model_clip(src, disp, coded, F)[k], f"{name} {fmt} rung {r}")
            same(got[r][k].annexb(), want[k].annexb(), f"{name} {fmt} rung {r} picture {k}")
    assert encs[0].bench_ladder(2) > 0 and encs[0].bench_ingest(2) > 0
    close(encs, lone)


def test_mixed_formats_in_one_call(gpu):
    """one ingest launch per format, one fan-out launch for the call"""
    from hartallo_amd import Encoder

    src, rungs = ld.LADDERS["L1"]
    fmts = [it.NV12, it.RGB24, it.I420, it.RGBA32, it.RGBP]
    frames = [sk.device_frame(F, sk.clip_planes(*src, yuv(F))[k], sk.pads_for(F, src[0])) for k, F in enumerate(fmts)]
    encs, lone = rung_encoders(src, rungs), rung_encoders(src, rungs)
    got = Encoder.encode_ladder_frames_device(encs, frames)
    for r, (disp, coded) in enumerate(rungs):
        want = lone[r].encode_frames_device(frames)
        for k, F in enumerate(fmts):
            check_input(encs[r], k, model_clip(src, disp, coded, F)[k], f"mixed, rung {r}")
            same(got[r][k].annexb(), want[k].annexb(), f"mixed, rung {r} picture {k}")
    close(encs, lone)


# ---- every rung keeps its own state ------------------------------------------------------------
def test_every_rung_has_its_own_ctl(gpu):
    """a forced IDR at frame 2 on one rung only, another gop_size on another"""
    from hartallo_amd import Encoder
    from hartallo_amd import _lib as L

    src, rungs = ld.LADDERS["L1"]
    clip = sk.clip_planes(*src, True)
    frames = [sk.device_frame(it.NV12, clip[k], (8, 8)) for k in range(N)]
    ctls = [[ctl(L.HL_AMD_ENCODING_INTRA if k == 2 else L.HL_AMD_ENCODING_AUTO) for k in range(N)], [ctl(gop=2) for _ in range(N)], [ctl() for _ in range(N)]]
    encs, lone = rung_encoders(src, rungs), rung_encoders(src, rungs)
    got = Encoder.encode_ladder_frames_device(encs, frames, ctl=ctls)
    for r in range(3):
        want = lone[r].encode_frames_device(frames, ctl=ctls[r])
        for k in range(N):
            same(got[r][k].annexb(), want[k].annexb(), f"rung {r} picture {k}")
    assert [is_idr(x) for x in got[0]] == [True, False, True, False, False]
    assert [is_idr(x) for x in got[1]] == [True, False, True, False, True]
    assert [is_idr(x) for x in got[2]] == [True, False, False, True, False]
    # and through the single-frame call: the streams go on, every rung with its own ctl
    f = sk.host_frame(it.NV12, clip[0], (6, 6))
    one = [ctl(), ctl(gop=2), ctl(L.HL_AMD_ENCODING_INTRA)]
    got = Encoder.encode_ladder_frame(encs, f, ctl=one)
    for r in range(3):
        same(got[r].annexb(), lone[r].encode_frame(f, one[r]).annexb(), f"rung {r}, the sixth frame")
    assert [is_idr(x) for x in got] == [True, False, True]  # the GOP's end, inside a GOP of 2, forced
    close(encs, lone)


def test_quality_on_one_rung_and_scene_cuts_on_another(gpu):
    """content that changes at frame 4: statistics and bytes are the lone encoders'"""
    from hartallo_amd import Encoder

    src, rungs = ld.LADDERS["L2"]
    clip = list(sk.clip_planes(*src, False, 4)) + list(sk.clip_planes(*src, False, 4, (31, 32, 33)))
    frames = [sk.device_frame(it.RGBA32, f, (8,)) for f in clip]

    def encoders():
        return [make_encoder(coded, disp, src, gop=30, quality=(r == 0), scenecut=(r == 1)) for r, (disp, coded) in enumerate(rungs)]

    encs, lone = encoders(), encoders()
    got = Encoder.encode_ladder_frames_device(encs, frames)
    want = [lone[r].encode_frames_device(frames) for r in range(3)]
    for r in range(3):
        for k in range(8):
            same(got[r][k].annexb(), want[r][k].annexb(), f"rung {r} picture {k}")
    for k in range(8):
        assert encs[0].last_quality(k) == lone[0].last_quality(k)
        assert encs[1].last_scene_stats(k) == lone[1].last_scene_stats(k)
    assert lone[1].last_scene_stats(4)["turned"]  # the clip has the cut the test is about
    assert [is_idr(x) for x in got[1]] == [True, False, False, False, True, False, False, False]
    assert [is_idr(x) for x in got[2]] == [True] + [False] * 7  # (no detector on this rung)
    close(encs, lone)


def test_rate_control_on_one_rung(gpu):
    from hartallo_amd import Encoder

    src, rungs = ld.LADDERS["L1"]
    clip = sk.clip_planes(*src, True)
    encs, lone = rung_encoders(src, rungs), rung_encoders(src, rungs)
    encs[1].set_rate_control(48000)
    lone[1].set_rate_control(48000)
    for k in range(N):
        got = Encoder.encode_ladder_frame(encs, mixed_frame(it.NV12, clip[k], k, src[0]))
        for r in range(3):
            same(got[r].annexb(), lone[r].encode_frame(mixed_frame(it.NV12, clip[k], k, src[0])).annexb(), f"rung {r} frame {k}")
            assert encs[r].last_qp() == lone[r].last_qp()
    close(encs, lone)


# ---- continuation -----------------------------------------------------------------------------------
def test_plain_calls_between_ladder_calls(gpu):
    """a ladder call, a plain encode_frame on one rung's encoder with its own source size, another ladder call"""
    from hartallo_amd import Encoder

    src, rungs = ld.LADDERS["L1"]
    clip = sk.clip_planes(*src, False)
    frame = [sk.host_frame(it.RGB24, clip[k], (6,)) for k in range(N)]
    encs, lone = rung_encoders(src, rungs), rung_encoders(src, rungs)
    fed = ([0, 2, 3, 4], [0, 1, 2, 3, 4], [0, 2, 3, 4])  # the frames every stream sees
    want = [[lone[r].encode_frame(frame[k]).annexb() for k in fed[r]] for r in range(3)]
    got = [[], [], []]
    for r, x in enumerate(Encoder.encode_ladder_frame(encs, frame[0])):
        got[r].append(x.annexb())
    got[1].append(encs[1].encode_frame(frame[1]).annexb())
    check_input(encs[1], 0, model_clip(src, *rungs[1], it.RGB24)[1], "the plain call")
    for r, x in enumerate(Encoder.encode_ladder_frame(encs, frame[2])):
        got[r].append(x.annexb())
    dev = [sk.device_frame(it.RGB24, clip[k], (0,)) for k in (3, 4)]
    for r, xs in enumerate(Encoder.encode_ladder_frames_device(encs, dev)):
        got[r] += [x.annexb() for x in xs]
    for r in range(3):
        for i, k in enumerate(fed[r]):
            same(got[r][i], want[r][i], f"rung {r} frame {k}")
        check_input(encs[r], 1, model_clip(src, *rungs[r], it.RGB24)[4], f"rung {r}")
    close(encs, lone)


def test_the_common_source_size_changes_between_calls(gpu):
    from hartallo_amd import Encoder

    a, b = (96, 64), (72, 48)
    rungs = [((48, 32), (48, 32)), ((34, 18), (48, 32))]
    encs, lone = rung_encoders(a, rungs), rung_encoders(a, rungs)
    for k in range(N):
        if k == 3:
            for e in encs + lone:
                e.set_source_size(*b)
        src = a if k < 3 else b
        f = sk.device_frame(it.NV12, sk.clip_planes(*src, True)[k], (8, 8))
        got = Encoder.encode_ladder_frame(encs, f)
        for r, (disp, coded) in enumerate(rungs):
            check_input(encs[r], 0, model_clip(src, disp, coded, it.NV12)[k], f"rung {r} frame {k}")
            same(got[r].annexb(), lone[r].encode_frame(f).annexb(), f"rung {r} frame {k}")
    close(encs, lone)


# ---- refusals -------------------------------------------------------------------------------------------
def test_refusals_leave_every_stream_as_it_was(gpu):
    from hartallo_amd import Encoder, Frame, HlAmdError, SvcEncoder
    from hartallo_amd import _lib as L

    src, rungs = ld.LADDERS["L2"]  # 150 wide: dense rows of 150, 75 and 450 bytes are no multiples of 4
    rungs = rungs + [((24, 16), (32, 16))]  # and a rung under 32 rows: no early termination there
    clip = sk.clip_planes(*src, False, NR)
    frame = [sk.host_frame(it.RGB24, clip[k], (6,)) for k in range(NR)]
    lone = rung_encoders(src, rungs)
    want = [[e.encode_frame(f).annexb() for f in frame] for e in lone]
    close(lone)
    encs = rung_encoders(src, rungs)
    k = 0

    def refused(code, call):
        with pytest.raises(HlAmdError) as e:
            call()
        assert e.value.code == code, (e.value.code, code)

    def next_call_continues():
        nonlocal k
        got = Encoder.encode_ladder_frame(encs, frame[k])
        for r, (disp, coded) in enumerate(rungs):
            same(got[r].annexb(), want[r][k], f"rung {r} frame {k} after a refusal")
            check_input(encs[r], 0, model_clip(src, disp, coded, it.RGB24, NR)[k], f"rung {r} frame {k}")
        k += 1

    next_call_continues()
    small = ((50, 34), (64, 48))
    extra = [make_encoder(small[1], small[0], src) for _ in range(5)]
    other_size = make_encoder(small[1], small[0], (100, 68))
    other_colour = make_encoder(small[1], small[0], src, key=(it.BT601, it.LIMITED))
    svc = SvcEncoder(48, 32, 2, 28, 8, 1, 3)
    queued = make_encoder(small[1], small[0], src)
    queued.set_lookahead(2)
    assert queued.encode_frame(frame[0]).type == 0
    ahead = make_encoder(small[1], small[0], src)
    ahead.set_lookahead(2)  # look-ahead on, nothing queued: the n-frame call takes it, the single-frame call does not
    dev = sk.device_frame(it.RGB24, clip[0], (2,))
    dense = Frame(dev.format, dev.planes, (0,), True, dev.source)  # 450 bytes a row
    y150 = sk.device_frame(it.I420, sk.clip_planes(*src, True)[0], (0, 0, 0))  # 150 and 75 bytes a row
    early = [[ctl()] for _ in rungs[:-1]] + [[L.FrameCtl(0, 8, 1, 1, 3)]]
    P, S, NI = L.HL_AMD_ERROR_INVALID_PARAMETER, L.HL_AMD_ERROR_INVALID_STATE, L.HL_AMD_ERROR_NOT_IMPLEMENTED
    cases = [
        (P, lambda: Encoder.encode_ladder_frame([], frame[0])),
        (P, lambda: Encoder.encode_ladder_frames_device([], [dev])),
        (P, lambda: Encoder.encode_ladder_frame(encs + extra, frame[0])),  # nine
        (P, lambda: Encoder.encode_ladder_frames_device(encs + extra, [dev])),
        (P, lambda: Encoder.encode_ladder_frame(encs[:3] + [encs[1]], frame[0])),  # a duplicate
        (P, lambda: Encoder.encode_ladder_frame(encs + [other_size], frame[0])),
        (P, lambda: Encoder.encode_ladder_frames_device(encs + [other_size], [dev])),
        (P, lambda: Encoder.encode_ladder_frame(encs + [other_colour], frame[0])),
        (NI, lambda: Encoder.encode_ladder_frame(encs + [svc], frame[0])),
        (NI, lambda: Encoder.encode_ladder_frames_device(encs + [svc], [dev])),
        (S, lambda: Encoder.encode_ladder_frame(encs + [queued], frame[0])),
        (S, lambda: Encoder.encode_ladder_frames_device(encs + [queued], [dev])),
        (S, lambda: Encoder.encode_ladder_frame(encs + [ahead], frame[0])),
        (P, lambda: Encoder.encode_ladder_frames_device(encs, [dev, frame[0]])),  # a host frame in the n-frame call
        (P, lambda: Encoder.encode_ladder_frame(encs, dense)),
        (P, lambda: Encoder.encode_ladder_frames_device(encs, [dev, dense])),
        (P, lambda: Encoder.encode_ladder_frame(encs, y150)),
        (P, lambda: Encoder.encode_ladder_frame(encs, frame[0], ctl=[c[0] for c in early])),  # a bad ctl on the last rung only
        (P, lambda: Encoder.encode_ladder_frames_device(encs, [dev], ctl=early)),
    ]
    assert len(cases) <= NR
    for code, call in cases[:-2]:
        refused(code, call)
        next_call_continues()
    for code, call in cases[-2:]:
        refused(code, call)
        with pytest.raises(HlAmdError) as e:  # nothing was converted
            encs[0].last_input(0)
        assert e.value.code == S
        with pytest.raises(HlAmdError) as e:
            encs[0].bench_ladder(2)
        assert e.value.code == S
    next_call_continues()
    close(encs, extra, [other_size, other_colour, svc, queued, ahead])


# ---- the feature off -----------------------------------------------------------------------------------------
def test_without_a_ladder_call_nothing_changes(gpu):
    from hartallo_amd import Encoder, HlAmdError

    name = "qcif_ippp_qp28_db"
    cfg = next(c for c in GOLDEN_CONFIGS if c[0] == name)
    _, w, h, n, qp, me, db, gop, seed = cfg[:9]
    clip = golden_input(cfg)
    ref = open(os.path.join(GOLDEN, name + ".264"), "rb").read()
    enc = Encoder(w, h, qp, me, db, gop, GOLD[name].get("early_term", 0))
    assert enc.source_size == (w, h) == enc.display_size
    frames = [sk.device_frame(it.NV12, it.split(clip[f], w, h), (8, 8)) for f in range(n)]
    same(b"".join(r.annexb() for r in enc.encode_frames_device(frames)), ref, name)
    assert np.array_equal(enc.last_input(n - 1)[0], it.split(clip[n - 1], w, h)[0])
    for call in (lambda: enc.bench_scale(2), lambda: enc.bench_ladder(2)):  # nothing was scaled
        with pytest.raises(HlAmdError) as e:
            call()
        assert e.value.code == 3
    enc.close()
    # dense I420 device frames are still forwarded: no copy, no kernel
    enc = Encoder(w, h, qp, me, db, gop, GOLD[name].get("early_term", 0))
    frames = [sk.device_frame(it.I420, it.split(clip[f], w, h), (0, 0, 0)) for f in range(n)]
    same(b"".join(r.annexb() for r in enc.encode_frames_device(frames)), ref, f"{name} forwarded")
    for call in (lambda: enc.last_input(0), lambda: enc.bench_ingest(2), lambda: enc.bench_scale(2), lambda: enc.bench_ladder(2)):
        with pytest.raises(HlAmdError) as e:
            call()
        assert e.value.code == 3
    enc.close()
