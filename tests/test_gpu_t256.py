"""The 256-lane build of the pipelined kernel (hl_encoder_t256.hip, two
macroblocks per CU) against the 512-lane build and the reference.

Each case forces build 2 (256 lanes) and build 1 (512 lanes) on the same
input, in one batch of all its pictures, and asserts identical bytes and
reconstruction between the two and equality with the golden stream and
reconstruction MD5 the reference encoder produced (tests/golden/).  The cases
are the smallest at which a lane map of the 256-lane build can go wrong: two
macroblocks with every neighbour missing, early termination, QCIF (interior
and all four edge kinds, an IDR inside the run, a P macroblock's 16x16 step
in its third quad round) and 480x272 (more ready macroblocks than one XCD has
CUs).  Variants: the memo off (every pass computes all its rounds), few
workgroups with no guaranteed reach (long reach waits), two streams sharing
one run.
Tolerance: none.
"""
import json
import os

import numpy as np
import pytest
import torch

from hartallo_amd import Encoder
from hl_testlib import GOLDEN, GOLDEN_CONFIGS, GOLDEN_ET_CONFIGS, first_diff, golden_input, md5

pytestmark = pytest.mark.gpu

GOLD = json.load(open(os.path.join(GOLDEN, "golden.json")))
BY_NAME = {c[0]: c for c in GOLDEN_CONFIGS + GOLDEN_ET_CONFIGS}
CASES = ["tiny_32x16_qp26", "et_w64_h32_qp36", "qcif_ippp_qp28_db", "qcif_qp40_me16_gop4", "w480_h272_qp28_me16"]


def _device_frames(clip, w, h):
    dev = torch.from_numpy(np.ascontiguousarray(clip)).cuda()
    torch.cuda.synchronize()
    n = w * h
    return dev, [(dev[i].data_ptr(), dev[i].data_ptr() + n, dev[i].data_ptr() + n + n // 4) for i in range(len(clip))]


def _check_run(enc, build):
    assert enc.last_pipeline_build() == build
    st = enc.last_batch_stats()
    assert st["runs"] >= 1 and st["fallbacks"] == 0 and st["waits_gave_up"] == 0, st


def _encode(name, build, geometry=None, streams=1):
    """The case's pictures as one batch on the forced build: per stream the
    Annex-B bytes and the reconstruction of the last picture."""
    _, w, h, n, qp, mer, db, gop, _ = BY_NAME[name]
    et = GOLD[name].get("early_term", 0)
    dev, ptrs = _device_frames(golden_input(BY_NAME[name]), w, h)
    encs = [Encoder(w, h, qp, mer, db, gop, et) for _ in range(streams)]
    encs[0].set_pipeline_build(build)  # (a shared run follows encoder 0's setting)
    if geometry:
        encs[0].set_pipeline(*geometry)
    if streams == 1:
        res = [encs[0].encode_batch_device(ptrs)]
    else:
        res = Encoder.encode_streams_device(encs, [ptrs] * streams)
    _check_run(encs[0], build)
    out = [(b"".join(r.annexb() for r in rs), np.concatenate(e.recon())) for rs, e in zip(res, encs)]
    for e in encs:
        e.close()
    return out


def _compare(name, geometry=None, streams=1):
    n = BY_NAME[name][3]
    ref = open(os.path.join(GOLDEN, name + ".264"), "rb").read()
    t256 = _encode(name, 2, geometry, streams)
    t512 = _encode(name, 1, geometry, streams)
    for s in range(streams):
        (a, ra), (b, rb) = t256[s], t512[s]
        assert a == b, f"{name} stream {s}: builds differ at byte {first_diff(a, b)}"
        assert np.array_equal(ra, rb), f"{name} stream {s}: reconstructions of the two builds differ"
        assert a == ref, f"{name} stream {s}: differs from the reference at byte {first_diff(a, ref)}"
        assert md5(ra) == GOLD[name]["recon_md5"][n - 1]


@pytest.mark.parametrize("name", CASES)
def test_t256_equals_512_and_reference(gpu, name):
    _compare(name)


def test_t256_memo_off(gpu, monkeypatch):
    monkeypatch.setenv("HL_AMD_MEMO", "0")  # read at encoder creation
    _compare("qcif_ippp_qp28_db")


@pytest.mark.parametrize("name,geometry", [("qcif_qp40_me16_gop4", (3, 0, 64)), ("qcif_ippp_qp28_db", (1, 0, 8))],
                         ids=["3x0x64", "1x0x8"])
def test_t256_few_workgroups(gpu, name, geometry):
    _compare(name, geometry)


def test_t256_two_streams_share_a_run(gpu):
    _compare("qcif_qp40_me16_gop4", streams=2)
