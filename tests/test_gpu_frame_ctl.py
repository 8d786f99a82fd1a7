"""Per-frame encoding type and live settings (hl_amd_frame_ctl_t,
include/hartallo_amd.h) on the GPU: every golden the reference made from a
schedule (tests/golden/make_frame_ctl_golden.py) through each entry point
that takes a ctl -- per call from host and device memory, as one batch (one
pipelined run that holds the forced IDR and the changed settings), with
look-ahead, and two streams in shared runs -- byte for byte."""
import functools
import json
import os

import pytest

from fc_testlib import FC_BY_NAME, FC_CONFIGS, FC_GOLDEN_JSON, fc_frame_ctls, fc_input, rc_args
from hl_testlib import GOLDEN, GOLDEN_CONFIGS, _planes, first_diff, golden_input, md5

pytestmark = pytest.mark.gpu

GOLD = json.load(open(FC_GOLDEN_JSON))
IDS = [c["name"] for c in FC_CONFIGS]


def golden_stream(name):
    return open(os.path.join(GOLDEN, name + ".264"), "rb").read()


def make_encoder(cfg):
    from hartallo_amd import Encoder

    enc = Encoder(cfg["width"], cfg["height"], cfg["qp"], cfg["me_range"], cfg["deblock"], cfg["gop"], cfg["early_term"])
    if rc_args(cfg):
        enc.set_rate_control(*rc_args(cfg))
    return enc


def on_device(clip, w, h):
    """The clip in device memory and each frame's (y, u, v) pointers."""
    import torch

    dev = torch.from_numpy(clip).cuda()
    n = w * h
    return dev, [(dev[i].data_ptr(), dev[i].data_ptr() + n, dev[i].data_ptr() + n + n // 4) for i in range(len(clip))]


@functools.lru_cache(maxsize=None)
def per_call_stream(name):
    """(a) one encode(y, u, v, ctl) per frame; every frame's recon against the reference's."""
    import numpy as np

    cfg = FC_BY_NAME[name]
    clip, ctls, enc = fc_input(cfg), fc_frame_ctls(cfg), make_encoder(cfg)
    out = b""
    for f in range(cfg["frames"]):
        out += enc.encode(*_planes(clip[f], cfg["width"], cfg["height"]), ctl=ctls[f]).annexb()
        assert md5(np.concatenate(enc.recon())) == GOLD[name]["recon_md5"][f], f"{name}: recon of frame {f}"
        assert enc.last_qp() == GOLD[name]["slice_qp"][f], f"{name}: QP of frame {f}"
    return out


@pytest.mark.parametrize("name", IDS)
def test_per_call_host(gpu, name):
    out, ref = per_call_stream(name), golden_stream(name)
    assert out == ref, f"{name}: first differing byte {first_diff(out, ref)}"


@pytest.mark.parametrize("name", IDS)
def test_per_call_device(gpu, name):
    """(b) encode_device with a ctl per call."""
    cfg = FC_BY_NAME[name]
    dev, ptrs = on_device(fc_input(cfg), cfg["width"], cfg["height"])
    ctls, enc = fc_frame_ctls(cfg), make_encoder(cfg)
    out = b"".join(enc.encode_device(*ptrs[f], ctl=ctls[f]).annexb() for f in range(cfg["frames"]))
    ref = golden_stream(name)
    assert out == ref, f"{name}: first differing byte {first_diff(out, ref)}"


@pytest.mark.parametrize("name", IDS)
def test_batch_one_run(gpu, name):
    """(c) one encode_batch_device with the ctl list: the golden's and the
    per-call bytes, from a single pipelined launch -- the forced IDR and the
    changed settings do not split the run or send it to the per-picture path.
    (Under rate control a batch goes picture by picture: one run each.)"""
    cfg = FC_BY_NAME[name]
    dev, ptrs = on_device(fc_input(cfg), cfg["width"], cfg["height"])
    enc = make_encoder(cfg)
    out = b"".join(r.annexb() for r in enc.encode_batch_device(ptrs, ctl=fc_frame_ctls(cfg)))
    ref = golden_stream(name)
    assert out == ref, f"{name}: first differing byte {first_diff(out, ref)}"
    assert out == per_call_stream(name)
    st = enc.last_batch_stats()
    assert st["runs"] == (cfg["frames"] if rc_args(cfg) else 1), st
    assert st["per_picture"] == st["fallbacks"] == st["waits_gave_up"] == 0, st
    import numpy as np

    assert md5(np.concatenate(enc.recon())) == GOLD[name]["recon_md5"][-1]


@pytest.mark.parametrize("geometry", [(240, 2, 4), (8, 0, 2), (2, 0, 6), (1, 0, 8), (16, 2, 1)], ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("name", ["fc_w480_mixed", "fc_w480_rising"])
def test_batch_scheduler_geometries(gpu, name, geometry):
    """The run's bytes do not depend on its scheduling (workgroups, guaranteed
    reach, window) when neighbouring pictures differ in deblocking and
    me_range: with reach 0 every motion window beyond the task's own
    macroblock goes through reach_wait, with the searching picture's range."""
    cfg = FC_BY_NAME[name]
    dev, ptrs = on_device(fc_input(cfg), cfg["width"], cfg["height"])
    enc = make_encoder(cfg)
    enc.set_pipeline(*geometry)
    out = b"".join(r.annexb() for r in enc.encode_batch_device(ptrs, ctl=fc_frame_ctls(cfg)))
    ref = golden_stream(name)
    assert out == ref, f"{name}: first differing byte {first_diff(out, ref)}"
    st = enc.last_batch_stats()
    assert st["runs"] == 1 and st["per_picture"] == st["fallbacks"] == st["waits_gave_up"] == 0, st


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("name", IDS)
def test_lookahead(gpu, name, k):
    """(d) look-ahead k: every queued frame keeps its ctl; the bytes are those
    of separate calls (frame counts that are no multiple of k included)."""
    cfg = FC_BY_NAME[name]
    clip, ctls, enc = fc_input(cfg), fc_frame_ctls(cfg), make_encoder(cfg)
    enc.set_lookahead(k)
    out, got = b"", 0
    for f in range(cfg["frames"]):
        r = enc.encode(*_planes(clip[f], cfg["width"], cfg["height"]), ctl=ctls[f])
        if r.type:
            out += r.annexb()
            got += 1
    while (r := enc.flush()).type:
        out += r.annexb()
        got += 1
    assert got == cfg["frames"]
    ref = golden_stream(name)
    assert out == ref, f"{name} (look-ahead {k}): first differing byte {first_diff(out, ref)}"


def test_two_streams_shared_runs(gpu):
    """(e) two encoders with different schedules in one shared launch."""
    from hartallo_amd import Encoder

    cfgs = [FC_BY_NAME["fc_qcif_idr3"], FC_BY_NAME["fc_qcif_gop3_idr4"]]
    devs, ptrs = zip(*[on_device(fc_input(c), c["width"], c["height"]) for c in cfgs])
    encs = [make_encoder(c) for c in cfgs]
    res = Encoder.encode_streams_device(encs, list(ptrs), ctl=[fc_frame_ctls(c) for c in cfgs])
    for c, rs in zip(cfgs, res):
        out, ref = b"".join(r.annexb() for r in rs), golden_stream(c["name"])
        assert out == ref, f"{c['name']}: first differing byte {first_diff(out, ref)}"
    st = encs[0].last_batch_stats()
    assert st["runs"] == 1 and st["per_picture"] == st["fallbacks"] == st["waits_gave_up"] == 0, st


def test_no_ctl_and_auto_ctl_are_the_plain_calls(gpu):
    """(f) ctl=None next to AUTO ctls with the settings unchanged: the existing golden."""
    from hartallo_amd import FrameCtl

    cfg = next(c for c in GOLDEN_CONFIGS if c[0] == "qcif_ippp_qp28_db")
    name, w, h, n, qp, mer, db, gop, seed = cfg
    from hartallo_amd import Encoder

    clip, ref = golden_input(cfg), golden_stream(name)
    auto = FrameCtl(0, mer, db, 0, gop)
    enc = Encoder(w, h, qp, mer, db, gop, 0)
    out = b"".join(enc.encode(*_planes(clip[f], w, h), ctl=auto if f % 2 else None).annexb() for f in range(n))
    assert out == ref, f"per call: first differing byte {first_diff(out, ref)}"
    dev, ptrs = on_device(clip, w, h)
    enc = Encoder(w, h, qp, mer, db, gop, 0)
    out = b"".join(r.annexb() for r in enc.encode_batch_device(ptrs[:3]))
    out += b"".join(r.annexb() for r in enc.encode_batch_device(ptrs[3:], ctl=[auto] * (n - 3)))
    assert out == ref, f"batches: first differing byte {first_diff(out, ref)}"


@pytest.mark.parametrize("encoding", [3, 4, 99], ids=["lossless", "raw", "unknown"])
def test_refused_types_leave_the_stream_alone(gpu, encoding):
    """RAW, LOSSLESS and unknown types: HL_AMD_ERROR_NOT_IMPLEMENTED from
    every entry point, decided before anything is coded or queued; the next
    call continues the stream."""
    from hartallo_amd import FrameCtl, HlAmdError

    name = "fc_qcif_idr3"
    cfg = FC_BY_NAME[name]
    clip, ctls = fc_input(cfg), fc_frame_ctls(cfg)
    dev, ptrs = on_device(clip, cfg["width"], cfg["height"])
    bad = [FrameCtl(encoding, c.me_range, c.deblock, c.me_early_term, c.gop_size) for c in ctls]
    enc = make_encoder(cfg)
    out = b""

    def refused(call):
        with pytest.raises(HlAmdError) as e:
            call()
        assert e.value.code == 7

    refused(lambda: enc.encode(*_planes(clip[0], cfg["width"], cfg["height"]), ctl=bad[0]))
    out += enc.encode(*_planes(clip[0], cfg["width"], cfg["height"]), ctl=ctls[0]).annexb()
    refused(lambda: enc.encode_device(*ptrs[1], ctl=bad[1]))
    out += enc.encode_device(*ptrs[1], ctl=ctls[1]).annexb()
    refused(lambda: enc.encode_batch_device(ptrs[2:6], ctl=ctls[2:5] + bad[5:6]))  # the last one of the batch
    out += b"".join(r.annexb() for r in enc.encode_batch_device(ptrs[2:6], ctl=ctls[2:6]))
    refused(lambda: type(enc).encode_streams_device([enc], [ptrs[6:]], ctl=[bad[6:]]))
    out += b"".join(r.annexb() for r in type(enc).encode_streams_device([enc], [ptrs[6:]], ctl=[ctls[6:]])[0])
    ref = golden_stream(name)
    assert out == ref, f"first differing byte {first_diff(out, ref)}"
    # look-ahead: refused before the frame is queued
    enc = make_encoder(cfg)
    enc.set_lookahead(3)
    out = b""
    for f in range(cfg["frames"]):
        if f in (1, 3):
            refused(lambda: enc.encode(*_planes(clip[f], cfg["width"], cfg["height"]), ctl=bad[f]))
        r = enc.encode(*_planes(clip[f], cfg["width"], cfg["height"]), ctl=ctls[f])
        out += r.annexb() if r.type else b""
    while (r := enc.flush()).type:
        out += r.annexb()
    assert out == ref, f"look-ahead: first differing byte {first_diff(out, ref)}"


def test_bad_values_and_layers_refused(gpu):
    from hartallo_amd import Encoder, FrameCtl, HlAmdError, SvcEncoder, synth

    # early termination on a picture under 32x32 (rdo.c:895-896): INVALID_PARAMETER, stream unchanged
    w, h = 32, 16
    clip = synth.clip(w, h, 3, 7)
    enc, plain = Encoder(w, h, 28, 16, 1, 30, 0), Encoder(w, h, 28, 16, 1, 30, 0)
    a = enc.encode(*_planes(clip[0], w, h), ctl=FrameCtl(0, 16, 1, 0, 30)).annexb()
    with pytest.raises(HlAmdError) as e:
        enc.encode(*_planes(clip[1], w, h), ctl=FrameCtl(0, 16, 1, 1, 30))
    assert e.value.code == 1
    a += enc.encode(*_planes(clip[1], w, h), ctl=FrameCtl(0, 16, 1, 0, 30)).annexb()
    assert a == plain.encode(*_planes(clip[0], w, h)).annexb() + plain.encode(*_planes(clip[1], w, h)).annexb()
    # an encoder with layers: a forced IDR or a changed setting is not implemented
    svc = SvcEncoder(64, 48, 2, 30, 16, 1, 3, 0)
    base = synth.clip(64, 48, 1, 7)[0]
    for ctl in (FrameCtl(1, 16, 1, 0, 3), FrameCtl(0, 8, 1, 0, 3), FrameCtl(2, 16, 0, 0, 3), FrameCtl(0, 16, 1, 0, 5)):
        with pytest.raises(HlAmdError) as e:
            svc.encode(*_planes(base, 64, 48), ctl=ctl)
        assert e.value.code == 7, ctl
    svc.close()
