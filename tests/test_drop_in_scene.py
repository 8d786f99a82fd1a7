"""Scene-cut detection through the reference's own API with the gfx950 plugin
installed (HL_AMD_SCENECUT, integration/hl_codec_264_gfx950.c):
oracle/_ref/drop_in_sched (tests/refdrive/drop_in_sched_harness.c) calls
hl_codec_encode with an all-AUTO schedule, the plugin's detector finds the cut,
and the stream is the CPU oracle's with the IDR where the cut is."""
import functools
import os
import subprocess
import tempfile

import pytest

from fc_testlib import DROP_IN_SCHED, ref_sched_command
from hl_testlib import OracleEncoder, first_diff
from sc_testlib import ab_clip, ab_stats, plan

pytestmark = pytest.mark.gpu

CFG = dict(name="sc_64x48", width=64, height=48, frames=8, qp=28, me_range=16, deblock=1, gop=30, early_term=0, types="-", changes="-")


@functools.lru_cache(maxsize=None)
def driver_reads_the_variable():
    """The plugin is compiled into the driver, and the driver is rebuilt only
    where the reference sources are: one that was built from a plugin older
    than HL_AMD_SCENECUT (its getenv literal is not in the binary) ignores the
    variable, and is not the driver of this plugin."""
    with open(DROP_IN_SCHED, "rb") as f:
        return b"HL_AMD_SCENECUT" in f.read()


def need_driver():
    if not os.path.exists(DROP_IN_SCHED):
        pytest.skip("oracle/_ref/drop_in_sched not built (make oracle, where the reference sources exist)")
    if not driver_reads_the_variable():
        pytest.skip("oracle/_ref/drop_in_sched holds a plugin from before HL_AMD_SCENECUT and cannot be rebuilt here "
                    "(make oracle, where the reference sources exist)")


def run(td, scenecut):
    inp, out = os.path.join(td, "in.yuv"), os.path.join(td, "out.264")
    ab_clip(CFG["width"], CFG["height"], "ab8").tofile(inp)
    cmd, env = ref_sched_command(DROP_IN_SCHED, CFG, inp, out)
    env.pop("HL_AMD_SCENECUT", None)
    if scenecut is not None:
        env["HL_AMD_SCENECUT"] = scenecut
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env)
    return r, (open(out, "rb").read() if os.path.exists(out) else b"")


def oracle(gop):
    o = OracleEncoder(CFG["width"], CFG["height"], CFG["qp"], CFG["me_range"], CFG["deblock"], gop)
    return b"".join(o.encode(f) for f in ab_clip(CFG["width"], CFG["height"], "ab8"))


@pytest.mark.parametrize("value", ["192", "192:1:8"])
def test_cut_found_behind_hl_codec_encode(gpu, value):
    need_driver()
    _, idr = plan(ab_stats(CFG["width"], CFG["height"], "ab8", 8), 192, 1, CFG["gop"])
    assert idr == [True, False, False, False, True, False, False, False]
    with tempfile.TemporaryDirectory() as td:
        r, got = run(td, value)
    assert r.returncode == 0, r.stderr
    ref = oracle(4)
    assert got == ref, f"first differing byte {first_diff(got, ref)}"


def test_without_the_variable_nothing_is_detected(gpu):
    need_driver()
    with tempfile.TemporaryDirectory() as td:
        r, got = run(td, None)
    assert r.returncode == 0, r.stderr
    ref = oracle(30)
    assert got == ref, f"first differing byte {first_diff(got, ref)}"


@pytest.mark.parametrize("value", ["", "abc", "192:", "192:1:8:2", "192;1", "300", "192:0", "192:1:17", "-5"])
def test_malformed_value_fails_the_open(gpu, value):
    need_driver()
    with tempfile.TemporaryDirectory() as td:
        r, got = run(td, value)
    assert r.returncode != 0
    assert "HL_ERROR_INVALID_PARAMETER" in r.stderr and "at frame 0" in r.stderr, r.stderr
