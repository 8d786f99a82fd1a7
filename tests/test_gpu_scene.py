"""Scene-cut detection on the GPU (hl_amd_set_scenecut):
k_scene's per-macroblock costs and frame sums against the numpy model
(sc_testlib), and the streams -- anchored to the reference through the CPU
oracle (a cut found at frame 4 of a GOP-30 stream is the oracle's GOP-4
stream), equal to the feature-off streams with INTRA passed where the model
names a cut, through every entry point that honours the setting."""
import functools
import os

import numpy as np
import pytest

from fc_testlib import FC_BY_NAME, rc_args
from hl_testlib import GOLDEN, GOLDEN_CONFIGS, OracleEncoder, _planes, first_diff, golden_input
from sc_testlib import AUTO, INTER, INTRA, RAW, ab_clip, ab_stats, analyse, is_cut, plan

pytestmark = pytest.mark.gpu

QP, ME, DB = 28, 16, 1


def make_encoder(w, h, gop=30, scenecut=(192, 1, 8)):
    from hartallo_amd import Encoder

    enc = Encoder(w, h, QP, ME, DB, gop, 0)
    if scenecut:
        enc.set_scenecut(*scenecut)
    return enc


def on_device(clip, w, h):
    """The clip in device memory and each frame's (y, u, v) pointers."""
    import torch

    dev = torch.from_numpy(np.array(clip)).cuda()  # (a copy: the shared clips are read-only)
    n = w * h
    return dev, [(dev[i].data_ptr(), dev[i].data_ptr() + n, dev[i].data_ptr() + n + n // 4) for i in range(len(clip))]


def ctl_list(encodings, gop=30):
    from hartallo_amd import FrameCtl

    return [FrameCtl(e, ME, DB, 0, gop) for e in encodings]


@functools.lru_cache(maxsize=None)
def oracle_stream(w, h, kind, gop, frames):
    o = OracleEncoder(w, h, QP, ME, DB, gop)
    return b"".join(o.encode(f) for f in ab_clip(w, h, kind)[:frames])


def code(enc, mode, clip, w, h, ctls=None):
    """The clip's stream through one entry point."""
    n = len(clip)
    if mode == "per_call":
        return b"".join(enc.encode(*_planes(clip[f], w, h), ctl=ctls[f] if ctls else None).annexb() for f in range(n))
    if mode.startswith("lookahead"):
        enc.set_lookahead(int(mode[9:]))
        out = b""
        for f in range(n):
            r = enc.encode(*_planes(clip[f], w, h), ctl=ctls[f] if ctls else None)
            out += r.annexb() if r.type else b""
        while (r := enc.flush()).type:
            out += r.annexb()
        return out
    dev, ptrs = on_device(clip, w, h)
    if mode == "device":
        return b"".join(enc.encode_device(*ptrs[f], ctl=ctls[f] if ctls else None).annexb() for f in range(n))
    assert mode == "batch"
    return b"".join(r.annexb() for r in enc.encode_batch_device(ptrs, ctl=ctls))


def same(got, ref, what):
    assert got == ref, f"{what}: first differing byte {first_diff(got, ref)} of {len(got)} / {len(ref)}"


def check_frame(enc, k, want, what):
    """Picture k of the last call against the model's (P, I, inter, intra) or None."""
    from hartallo_amd import HlAmdError

    st = enc.last_scene_stats(k)
    if want is None:
        assert not st["analysed"] and not st["turned"] and st["P"] == st["I"] == 0, (what, st)
        with pytest.raises(HlAmdError) as e:
            enc.debug_scene_mb(k)
        assert e.value.code == 3
        return
    inter, intra = enc.debug_scene_mb(k)
    assert np.array_equal(intra, want[3]), what
    assert np.array_equal(inter, want[2]), (what, np.argwhere(inter != want[2])[:4])
    assert st["analysed"] and (st["P"], st["I"]) == want[:2], (what, st, want[:2])


# ---- costs ------------------------------------------------------------------
@pytest.mark.parametrize("R", [0, 8, 16])
@pytest.mark.parametrize("size", [(48, 32), (176, 144), (1920, 32)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_costs_of_a_batch(gpu, size, R):
    w, h = size
    clip, stats = ab_clip(w, h, "aba")[:6], ab_stats(w, h, "aba", R)
    enc = make_encoder(w, h, scenecut=(192, 1, R))
    dev, ptrs = on_device(clip, w, h)
    enc.encode_batch_device(ptrs)
    for k in range(6):
        check_frame(enc, k, stats[k], f"{w}x{h} R={R} frame {k}")  # (frame 0 of a stream: not analysed)
    turned, _ = plan(stats[:6], 192, 1, 30)
    assert [enc.last_scene_stats(k)["turned"] for k in range(6)] == turned
    assert enc.bench_scene(2) > 0  # (the launch can be repeated alone)


@pytest.mark.parametrize("R", [0, 8, 16])
@pytest.mark.parametrize("size", [(48, 32), (176, 144), (1920, 32)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_costs_of_single_calls(gpu, size, R):
    w, h = size
    clip, stats = ab_clip(w, h, "aba")[:6], ab_stats(w, h, "aba", R)
    enc = make_encoder(w, h, scenecut=(192, 1, R))
    for k in range(6):
        enc.encode(*_planes(clip[k], w, h))
        check_frame(enc, 0, stats[k], f"{w}x{h} R={R} call {k}")


def test_second_batch_is_compared_with_the_first_batch_s_last_frame(gpu):
    w, h = 176, 144
    clip, stats = ab_clip(w, h, "aba"), ab_stats(w, h, "aba", 8)
    enc = make_encoder(w, h)
    dev, ptrs = on_device(clip, w, h)
    enc.encode_batch_device(ptrs[:4])
    enc.encode_batch_device(ptrs[4:])
    for k in range(4):
        check_frame(enc, k, stats[4 + k], f"second batch, frame {k}")
    assert [enc.last_scene_stats(k)["turned"] for k in range(4)] == [True, False, False, True]
    # switched off and on again: the next frame has no previous input frame
    enc.set_scenecut(0)
    enc.set_scenecut(192, 1, 8)
    enc.encode_device(*ptrs[4])
    check_frame(enc, 0, None, "first frame after the feature is switched on")


# ---- anchored to the reference through the oracle ---------------------------
@pytest.mark.parametrize("case", [(64, 48, "per_call"), (64, 48, "batch"), (64, 48, "lookahead3"), (176, 144, "batch")],
                         ids=lambda c: f"{c[0]}x{c[1]}_{c[2]}")
def test_cut_in_a_long_gop_is_the_oracle_s_short_gop(gpu, case):
    """A[0:4] + B[0:4], gop_size 30, the defaults: the detector's IDR at
    frame 4 gives the stream of the oracle with gop 4 (gop_size is in no
    header, and the two differ only from frame 8 on)."""
    w, h, mode = case
    turned, idr = plan(ab_stats(w, h, "ab8", 8), 192, 1, 30)
    assert idr == [True, False, False, False, True, False, False, False] and turned[4]
    enc = make_encoder(w, h)
    same(code(enc, mode, ab_clip(w, h, "ab8"), w, h), oracle_stream(w, h, "ab8", 4, 8), f"{w}x{h} {mode}")
    if mode == "batch":
        st = enc.last_batch_stats()
        assert st["runs"] == 1 and st["per_picture"] == st["fallbacks"] == 0, st
        assert [enc.last_scene_stats(k)["turned"] for k in range(8)] == turned


@pytest.mark.parametrize("gap", [3, 1])
def test_minimum_gap(gpu, gap):
    """Two contents in turn, a cut at every frame: min_gap 3 codes IDRs at 0,
    3 and 6 (the oracle's gop 3), min_gap 1 every frame (gop 1)."""
    w, h = 64, 48
    stats = ab_stats(w, h, "alt", 8)
    assert all(is_cut(s[0], s[1], 192) for s in stats[1:])
    turned, idr = plan(stats, 192, gap, 30)
    assert idr == [k % gap == 0 for k in range(9)]
    enc = make_encoder(w, h, scenecut=(192, gap, 8))
    same(code(enc, "batch", ab_clip(w, h, "alt"), w, h), oracle_stream(w, h, "alt", gap, 9), f"min_gap {gap}")
    assert [enc.last_scene_stats(k)["turned"] for k in range(9)] == turned


# ---- the caller's types ------------------------------------------------------
def test_inter_is_the_caller_s_veto(gpu):
    w, h = 64, 48
    clip, stats = ab_clip(w, h, "ab8"), ab_stats(w, h, "ab8", 8)
    ctls = ctl_list([INTER if k == 4 else AUTO for k in range(8)])
    on, off = make_encoder(w, h), make_encoder(w, h, scenecut=None)
    got = code(on, "batch", clip, w, h, ctls)
    same(got, code(off, "batch", clip, w, h, ctls), "INTER at the cut")
    assert got != oracle_stream(w, h, "ab8", 4, 8)  # (frame 4 is a P picture)
    st = on.last_scene_stats(4)
    assert st["analysed"] and not st["turned"] and is_cut(st["P"], st["I"], 192) and (st["P"], st["I"]) == stats[4][:2], st
    assert not any(on.last_scene_stats(k)["turned"] for k in range(8))


W2, H2 = 176, 144


@functools.lru_cache(maxsize=None)
def explicit_stream(kind):
    """The feature-off stream of the 176x144 clip with INTRA passed at the frames the model names (per call)."""
    stats = ab_stats(W2, H2, kind, 8)
    turned, _ = plan(stats, 192, 1, 30)
    assert any(turned)
    ctls = ctl_list([INTRA if t else AUTO for t in turned])
    return code(make_encoder(W2, H2, scenecut=None), "per_call", ab_clip(W2, H2, kind), W2, H2, ctls)


@pytest.mark.parametrize("mode", ["per_call", "device", "batch", "lookahead3"])
def test_equals_explicit_intra(gpu, mode):
    same(code(make_encoder(W2, H2), mode, ab_clip(W2, H2, "ab8"), W2, H2), explicit_stream("ab8"), mode)


def test_equals_explicit_intra_with_auto_ctls(gpu):
    """AUTO ctls with the settings unchanged are the null ctl."""
    same(code(make_encoder(W2, H2), "batch", ab_clip(W2, H2, "ab8"), W2, H2, ctl_list([AUTO] * 8)), explicit_stream("ab8"), "AUTO ctls")


def test_two_streams_one_with_the_feature(gpu):
    from hartallo_amd import Encoder

    clips = [ab_clip(W2, H2, "ab8"), ab_clip(W2, H2, "aba")]
    devs, ptrs = zip(*[on_device(c, W2, H2) for c in clips])
    encs = [make_encoder(W2, H2), make_encoder(W2, H2, scenecut=None)]
    res = Encoder.encode_streams_device(encs, list(ptrs))
    same(b"".join(r.annexb() for r in res[0]), explicit_stream("ab8"), "the stream with the feature")
    plain = code(make_encoder(W2, H2, scenecut=None), "batch", clips[1], W2, H2)
    same(b"".join(r.annexb() for r in res[1]), plain, "the stream without it")
    assert encs[0].last_scene_stats(4)["turned"]
    from hartallo_amd import HlAmdError

    with pytest.raises(HlAmdError) as e:
        encs[1].last_scene_stats(4)
    assert e.value.code == 3


def test_batch_longer_than_a_run_is_analysed_once(gpu):
    """132 pictures: two pipelined runs (128 + 4), one analysis up front.  The
    clip repeats A0..A3 B0..B3, so every fourth frame is a cut -- frame 128,
    the second run's first picture, among them."""
    w, h = 48, 32
    clip = np.concatenate([ab_clip(w, h, "ab8")] * 17)[:132]
    stats = analyse(clip, w, h, 8)
    turned, _ = plan(stats, 192, 1, 30)
    assert turned == [k > 0 and k % 4 == 0 for k in range(132)]
    on, off = make_encoder(w, h), make_encoder(w, h, scenecut=None)
    got = code(on, "batch", clip, w, h)
    assert on.last_batch_stats()["runs"] == 2
    same(got, code(off, "batch", clip, w, h, ctl_list([INTRA if t else AUTO for t in turned])), "132 pictures")
    for k in (0, 1, 127, 128, 129, 131):
        check_frame(on, k, stats[k], f"frame {k}")
    assert [on.last_scene_stats(k)["turned"] for k in range(132)] == turned


@pytest.mark.parametrize("mode", ["per_call", "batch"])
def test_rate_control_sees_a_forced_idr(gpu, mode):
    """Under rate control (the parameters of fc_rc_qcif_idr) the detector's
    IDR is the caller's: the same bytes and the same QP per frame."""
    rc = rc_args(FC_BY_NAME["fc_rc_qcif_idr"])
    clip = ab_clip(W2, H2, "ab8")
    turned, _ = plan(ab_stats(W2, H2, "ab8", 8), 192, 1, 30)
    ctls = ctl_list([INTRA if t else AUTO for t in turned])
    on, off = make_encoder(W2, H2), make_encoder(W2, H2, scenecut=None)
    on.set_rate_control(*rc)
    off.set_rate_control(*rc)
    ref, qps = b"", []
    for f in range(8):
        ref += off.encode(*_planes(clip[f], W2, H2), ctl=ctls[f]).annexb()
        qps.append(off.last_qp())
    if mode == "per_call":
        got, got_qps = b"", []
        for f in range(8):
            got += on.encode(*_planes(clip[f], W2, H2)).annexb()
            got_qps.append(on.last_qp())
        assert got_qps == qps
    else:
        got = code(on, "batch", clip, W2, H2)
        assert on.last_batch_stats()["runs"] == 8  # (picture by picture, analysed once up front)
        assert on.last_qp() == qps[-1]
        assert [on.last_scene_stats(k)["turned"] for k in range(8)] == turned
    same(got, ref, f"rate control, {mode}")
    assert len(set(qps)) > 1  # (the controller did move the QP)


# ---- off means off -------------------------------------------------------------
@pytest.mark.parametrize("state", ["never_set", "set_then_off", "on"])
def test_golden_stream_unchanged(gpu, state):
    cfg = next(c for c in GOLDEN_CONFIGS if c[0] == "w480_h272_qp28_me16")
    name, w, h, n, qp, mer, db, gop, seed = cfg
    from hartallo_amd import Encoder, HlAmdError

    clip, ref = golden_input(cfg), open(os.path.join(GOLDEN, name + ".264"), "rb").read()
    enc = Encoder(w, h, qp, mer, db, gop, 0)
    if state != "never_set":
        enc.set_scenecut(192, 1, 8)
    if state == "set_then_off":
        enc.set_scenecut(0, 1, 8)
    dev, ptrs = on_device(clip, w, h)
    same(b"".join(r.annexb() for r in enc.encode_batch_device(ptrs)), ref, state)
    if state == "on":  # a plain synth.clip has no cut: the model finds none, and neither did the encoder
        stats = analyse(clip, w, h, 8)
        assert not any(s is not None and is_cut(s[0], s[1], 192) for s in stats)
        for k in range(n):
            st = enc.last_scene_stats(k)
            assert not st["turned"] and st["analysed"] == (k > 0)
            if k:
                assert (st["P"], st["I"]) == stats[k][:2]
    else:
        with pytest.raises(HlAmdError) as e:
            enc.last_scene_stats(0)
        assert e.value.code == 3


# ---- refusals ------------------------------------------------------------------
def test_refusals(gpu):
    from hartallo_amd import HlAmdError, SvcEncoder

    def refused(call, code_):
        with pytest.raises(HlAmdError) as e:
            call()
        assert e.value.code == code_

    w, h = 64, 48
    clip = ab_clip(w, h, "ab8")
    enc = make_encoder(w, h, scenecut=None)
    for bad in ((-1, 1, 8), (257, 1, 8), (192, 0, 8), (192, -3, 8), (192, 1, 17), (192, 1, -1), (0, 0, 8), (0, 1, 17)):
        refused(lambda: enc.set_scenecut(*bad), 1)
    for ok in ((1, 1, 0), (256, 1000, 16), (0, 1, 8)):
        enc.set_scenecut(*ok)
    # frames queued in the look-ahead
    enc.set_lookahead(3)
    enc.encode(*_planes(clip[0], w, h))
    refused(lambda: enc.set_scenecut(192, 1, 8), 3)
    assert enc.flush().type
    enc.set_scenecut(192, 1, 8)
    # layers
    svc = SvcEncoder(64, 48, 2, 30, 16, 1, 3, 0)
    refused(lambda: svc.set_scenecut(192, 1, 8), 7)
    refused(lambda: svc.set_scenecut(0, 1, 8), 7)
    svc.close()
    # a luma plane the kernel's 4-byte loads cannot take
    import torch

    buf = torch.zeros(w * h * 3 // 2 + 64, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr() + 1
    enc = make_encoder(w, h)
    refused(lambda: enc.encode_device(p, p + w * h, p + w * h * 5 // 4), 1)


def test_a_refused_call_moves_nothing(gpu):
    """A batch with a RAW frame is refused (NOT_IMPLEMENTED); the stream goes
    on as if the call had not been made: frame 3 is still compared with frame
    2, and the cut at frame 4 is still found."""
    from hartallo_amd import HlAmdError

    w, h = 64, 48
    clip = ab_clip(w, h, "ab8")
    dev, ptrs = on_device(clip, w, h)
    enc = make_encoder(w, h)
    out = b"".join(r.annexb() for r in enc.encode_batch_device(ptrs[:3]))
    with pytest.raises(HlAmdError) as e:
        enc.encode_batch_device(ptrs[5:8], ctl=ctl_list([AUTO, AUTO, RAW]))
    assert e.value.code == 7
    out += b"".join(r.annexb() for r in enc.encode_batch_device(ptrs[3:]))
    same(out, oracle_stream(w, h, "ab8", 4, 8), "after a refused call")
    stats = ab_stats(w, h, "ab8", 8)
    for k in range(5):
        check_frame(enc, k, stats[3 + k], f"frame {3 + k}")
    assert [enc.last_scene_stats(k)["turned"] for k in range(5)] == [False, True, False, False, False]
