"""Per-picture quality through the reference's own API with the gfx950 plugin
installed (HL_AMD_QUALITY, integration/hl_codec_264_gfx950.c):
oracle/_ref/drop_in_sched (tests/refdrive/drop_in_sched_harness.c) calls
hl_codec_encode, the plugin reports every coded picture on stderr, and the
figures are the numpy model's (q_testlib) on the CPU oracle's reconstruction;
the stream is the oracle's, with and without the variable."""
import functools
import math
import os
import re
import subprocess
import tempfile

import pytest

from fc_testlib import DROP_IN_SCHED, ref_sched_command
from hl_testlib import OracleEncoder, first_diff
from hartallo_amd import synth
from q_testlib import picture_quality

pytestmark = pytest.mark.gpu

CFG = dict(name="q_64x48", width=64, height=48, frames=7, qp=28, me_range=16, deblock=1, gop=4, early_term=0, types="-", changes="-")
LINE = re.compile(r"^hl_codec_264_gfx950: quality picture (\d+) layer (\d+) psnr (\S+) (\S+) (\S+) ssim (\S+) (\S+) (\S+)$", re.M)


@functools.lru_cache(maxsize=None)
def driver_reads_the_variable():
    """The plugin is compiled into the driver, and the driver is rebuilt only
    where the reference sources are: one that was built from a plugin older
    than HL_AMD_QUALITY (its getenv literal is not in the binary) ignores the
    variable, and is not the driver of this plugin."""
    with open(DROP_IN_SCHED, "rb") as f:
        return b"HL_AMD_QUALITY" in f.read()


def need_driver():
    if not os.path.exists(DROP_IN_SCHED):
        pytest.skip("oracle/_ref/drop_in_sched not built (make oracle, where the reference sources exist)")
    if not driver_reads_the_variable():
        pytest.skip("oracle/_ref/drop_in_sched holds a plugin from before HL_AMD_QUALITY and cannot be rebuilt here "
                    "(make oracle, where the reference sources exist)")


@functools.lru_cache(maxsize=None)
def clip():
    c = synth.clip(CFG["width"], CFG["height"], CFG["frames"], 31)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def oracle():
    """(stream, the model's values per picture) of the CPU oracle."""
    w, h = CFG["width"], CFG["height"]
    o = OracleEncoder(w, h, CFG["qp"], CFG["me_range"], CFG["deblock"], CFG["gop"])
    stream, vals = b"", []
    for f in clip():
        stream += o.encode(f)
        vals.append(picture_quality(f, o.recon(), w, h))
    return stream, vals


def run(td, quality, lookahead=None):
    inp, out = os.path.join(td, "in.yuv"), os.path.join(td, "out.264")
    clip().tofile(inp)
    cmd, env = ref_sched_command(DROP_IN_SCHED, CFG, inp, out)
    env.pop("HL_AMD_QUALITY", None)
    env.pop("HL_AMD_SCENECUT", None)
    if quality is not None:
        env["HL_AMD_QUALITY"] = quality
    if lookahead:
        env["HL_AMD_LOOKAHEAD"] = str(lookahead)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env)
    return r, (open(out, "rb").read() if os.path.exists(out) else b"")


@pytest.mark.parametrize("lookahead", [None, 3], ids=["per_call", "lookahead3"])
def test_every_picture_is_reported(gpu, lookahead):
    need_driver()
    with tempfile.TemporaryDirectory() as td:
        r, got = run(td, "1", lookahead)
    assert r.returncode == 0, r.stderr
    ref, vals = oracle()
    assert got == ref, f"first differing byte {first_diff(got, ref)}"
    lines = LINE.findall(r.stderr)
    assert [(int(m[0]), int(m[1])) for m in lines] == [(k, 0) for k in range(CFG["frames"])], r.stderr
    for k, m in enumerate(lines):
        for c in range(3):
            sse, n = vals[k]["sse"][c], vals[k]["samples"][c]
            psnr = math.inf if sse == 0 else 10 * math.log10(255 * 255 * n / sse)
            assert float(m[2 + c]) == pytest.approx(psnr, abs=1e-6), (k, c, m)  # (printed with 6 decimals)
            ssim = vals[k]["ssim_q30"][c] / (1 << 30) / vals[k]["windows"][c]
            assert float(m[5 + c]) == pytest.approx(ssim, abs=1e-8), (k, c, m)  # (printed with 8)


@pytest.mark.parametrize("value", [None, "0"])
def test_without_the_variable_nothing_is_reported(gpu, value):
    need_driver()
    with tempfile.TemporaryDirectory() as td:
        r, got = run(td, value)
    assert r.returncode == 0, r.stderr
    assert got == oracle()[0] and not LINE.findall(r.stderr)
