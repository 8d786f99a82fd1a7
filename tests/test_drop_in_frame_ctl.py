"""hl_frame_t.encoding and the live hl_codec_t settings through the reference's
own API with the gfx950 plugin installed: oracle/_ref/drop_in_sched
(tests/refdrive/drop_in_sched_harness.c) makes the calls
oracle/_ref/ref_enc_sched made for the goldens -- hl_codec_encode with the
frame's encoding type set and the codec's fields changed between calls -- and
every frame is coded on the GPU.  The streams must be the reference's."""
import os
import subprocess
import tempfile

import pytest

from fc_testlib import DROP_IN_SCHED, FC_BY_NAME, FC_CONFIGS, fc_input, ref_sched_command
from hl_testlib import GOLDEN, first_diff

pytestmark = pytest.mark.gpu


def need_driver():
    if not os.path.exists(DROP_IN_SCHED):
        pytest.skip("oracle/_ref/drop_in_sched not built (make oracle, where the reference sources exist)")


def run(cfg, td, lookahead=None):
    inp, out = os.path.join(td, "in.yuv"), os.path.join(td, "out.264")
    fc_input(cfg).tofile(inp)
    cmd, env = ref_sched_command(DROP_IN_SCHED, cfg, inp, out)
    if lookahead:
        env["HL_AMD_LOOKAHEAD"] = str(lookahead)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env)
    return r, (open(out, "rb").read() if os.path.exists(out) else b"")


@pytest.mark.parametrize("lookahead", [None, 3], ids=["per_call", "lookahead3"])
@pytest.mark.parametrize("cfg", FC_CONFIGS, ids=[c["name"] for c in FC_CONFIGS])
def test_schedules_through_hl_codec_encode(gpu, cfg, lookahead):
    need_driver()
    with tempfile.TemporaryDirectory() as td:
        r, got = run(cfg, td, lookahead)
    assert r.returncode == 0, r.stderr
    ref = open(os.path.join(GOLDEN, cfg["name"] + ".264"), "rb").read()
    assert got == ref, f"{cfg['name']}: first differing byte {first_diff(got, ref)}"


@pytest.mark.parametrize("letter", ["R", "L"], ids=["raw", "lossless"])
def test_raw_and_lossless_refused(gpu, letter):
    """A RAW or LOSSLESS frame fails loudly with HL_ERROR_NOT_IMPLEMENTED
    instead of coming back as a P picture."""
    need_driver()
    cfg = dict(FC_BY_NAME["fc_qcif_idr3"], frames=3, types="AA" + letter)
    with tempfile.TemporaryDirectory() as td:
        r, _ = run(cfg, td)
    assert r.returncode != 0
    assert "HL_ERROR_NOT_IMPLEMENTED" in r.stderr and "at frame 2" in r.stderr, r.stderr
    assert "is not implemented" in r.stderr  # the plugin's own message


@pytest.mark.parametrize("types,changes", [("AI", "-"), ("-", "1:me_range=4")], ids=["forced_intra", "changed_setting"])
def test_svc_forced_type_or_changed_setting_refused(gpu, types, changes):
    need_driver()
    from hartallo_amd import synth

    L, w0, h0, n = 2, 64, 48, 2
    clips = synth.svc_clips(w0 << (L - 1), h0 << (L - 1), L, n, 7)
    with tempfile.TemporaryDirectory() as td:
        ins = []
        for l in range(L):
            ins.append(os.path.join(td, f"in{l}.yuv"))
            clips[l][:n].tofile(ins[-1])
        r = subprocess.run([DROP_IN_SCHED, "svc", str(L), str(w0), str(h0), str(n), "30", "16", "1", "3", "0", os.path.join(td, "out.264"),
                            types, changes] + ins, capture_output=True, text=True, timeout=240)
    assert r.returncode != 0
    assert "HL_ERROR_NOT_IMPLEMENTED" in r.stderr and "at frame 1" in r.stderr, r.stderr
