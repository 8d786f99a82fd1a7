"""The pipelined run's pop on the GPU (pop_task, hl_sched.h): runs in which
the hand-over is what is stressed, byte for byte against the same pictures
coded one call at a time (the lone-picture cases against the CPU oracle).

* Far more poppers than tasks: pictures of 1, 3 and 30 macroblocks, 40
  pictures with IDR pictures inside the run, every resident workgroup, both
  run builds (512 and 256 lanes).
* Few workgroups (1, 2, 3, 17), both builds: workgroup 0 claims in run order,
  so poppers meet entries whose task is held already.
* Several streams in one run: three streams of 30 macroblocks, eight of
  three (sub-queue = address % 4, windows of window / streams pictures).
* A lone picture and a two-picture run: the helper build's pop, where a
  loser takes a helper task.
Every run: fallbacks == 0 and waits_gave_up == 0; a forced build must be the
one that ran.  Tolerance: none.
"""
import functools

import numpy as np
import pytest
import torch

from hartallo_amd import Encoder, synth
from hl_testlib import OracleEncoder, first_diff

pytestmark = pytest.mark.gpu

QP, ME, DEBLOCK, GOP = 28, 16, 1, 8


@functools.lru_cache(maxsize=None)
def _clip(w, h, n, seed):
    return synth.clip(w, h, n, seed)


def _device_frames(clip, w, h):
    dev = torch.from_numpy(np.ascontiguousarray(clip)).cuda()
    torch.cuda.synchronize()
    n = w * h
    return dev, [(dev[i].data_ptr(), dev[i].data_ptr() + n, dev[i].data_ptr() + n + n // 4) for i in range(len(clip))]


def _no_giveups(enc):
    st = enc.last_batch_stats()
    assert st["fallbacks"] == 0 and st["waits_gave_up"] == 0, st
    return st


@functools.lru_cache(maxsize=None)
def _single_calls(w, h, n, seed):
    """The reference: the clip's pictures one call each (computed once)."""
    dev, ptrs = _device_frames(_clip(w, h, n, seed), w, h)
    enc = Encoder(w, h, QP, ME, DEBLOCK, GOP)
    out = []
    for p in ptrs:
        out.append(enc.encode_device(*p).annexb())
        _no_giveups(enc)
    enc.close()
    return tuple(out)


def _run(w, h, n, seed, build, geometry):
    """The first n pictures of the 40-picture clip as one batch."""
    dev, ptrs = _device_frames(_clip(w, h, 40, seed)[:n], w, h)
    enc = Encoder(w, h, QP, ME, DEBLOCK, GOP)
    if build:
        enc.set_pipeline_build(build)
    enc.set_pipeline(*geometry)
    res = enc.encode_batch_device(ptrs)
    st = _no_giveups(enc)
    assert st["runs"] >= 1 and st["per_picture"] == 0, st
    if build:
        assert enc.last_pipeline_build() == build
    enc.close()
    return [r.annexb() for r in res]


def _same(got, ref, what):
    assert len(got) == len(ref)
    for k, (a, b) in enumerate(zip(got, ref)):
        assert a == b, f"{what}: picture {k} differs from its single call at byte {first_diff(a, b)}"


@pytest.mark.parametrize("build", [1, 2], ids=["512-lane", "256-lane"])
@pytest.mark.parametrize("w,h", [(16, 16), (48, 16), (96, 80)])
def test_far_more_poppers_than_tasks(gpu, w, h, build):
    _same(_run(w, h, 40, 3, build, (0, 2, 64)), _single_calls(w, h, 40, 3), f"{w}x{h} build {build}")


@pytest.mark.parametrize("build", [1, 2], ids=["512-lane", "256-lane"])
@pytest.mark.parametrize("workgroups", [1, 2, 3, 17])
def test_few_workgroups(gpu, workgroups, build):
    _same(_run(96, 80, 12, 3, build, (workgroups, 2, 64)), _single_calls(96, 80, 40, 3)[:12], f"{workgroups} workgroups build {build}")


@pytest.mark.parametrize("streams,w,h", [(3, 96, 80), (8, 48, 16)])
def test_streams_share_a_run(gpu, streams, w, h):
    n = 10
    keep, ptrs = zip(*[_device_frames(_clip(w, h, 40, 3 + s)[:n], w, h) for s in range(streams)])
    encs = [Encoder(w, h, QP, ME, DEBLOCK, GOP) for _ in range(streams)]
    res = Encoder.encode_streams_device(encs, list(ptrs))
    st = _no_giveups(encs[0])
    assert st["runs"] >= 1 and st["per_picture"] == 0, st
    for s in range(streams):
        _same([r.annexb() for r in res[s]], _single_calls(w, h, 40, 3 + s)[:n], f"stream {s} of {streams}")
    for e in encs:
        e.close()


def test_lone_picture_and_two_picture_run(gpu):
    w, h = 96, 80
    clip = _clip(w, h, 40, 3)[:5]
    oracle = OracleEncoder(w, h, QP, ME, DEBLOCK, GOP)
    ref = [oracle.encode(f) for f in clip]
    dev, ptrs = _device_frames(clip, w, h)
    enc = Encoder(w, h, QP, ME, DEBLOCK, GOP)
    got = []
    for group in ([0], [1], [2, 3], [4]):  # an IDR alone, a P picture alone (its losers take helper tasks), two pictures, one more
        got += [r.annexb() for r in enc.encode_batch_device([ptrs[k] for k in group])]
        _no_giveups(enc)
    enc.close()
    for k, (a, b) in enumerate(zip(got, ref)):
        assert a == b, f"picture {k} differs from the oracle at byte {first_diff(a, b)}"
    _same(got, _single_calls(w, h, 40, 3)[:5], "lone pictures")
