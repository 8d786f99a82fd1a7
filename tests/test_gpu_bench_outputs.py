"""bench.py as later measurements call it: a plain `--gpus 1 --steps N
--warmup W` run prints the headline line (with ms_per_step, the N timed
steps) and nothing that takes a run of its own, and --dump-outputs DIR
writes what the timed call returned for its last step.  The dumped frame is
checked against the reference encoder's MD5s of the same stream
(tests/golden/bench_golden.json): output for output, tolerance none."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from hl_testlib import GOLDEN

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(GOLDEN, "bench_golden.json")))["bench_1088p_s11"]


def _md5(a):
    return hashlib.md5(a.astype(np.uint8).tobytes()).hexdigest()


def test_plain_run_dumps_last_step(gpu, tmp_path):
    warmup, steps = 2, 3  # an IDR and a P picture to warm up, three timed P pictures in one pipelined launch
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE")}
    out = tmp_path / "dump"
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    line = json.loads(lines[0])
    assert line["steps"] == steps and line["warmup"] == warmup and line["full"] is False
    assert (line["unit"], line["higher_is_better"], line["dtype"]) == ("frames/s", True, "u8/int32")
    assert line["ms_per_step"] > 0 and abs(line["value"] * line["ms_per_step"] / 1e3 - 1) < 1e-3  # one stream: frames/s = 1 / step time
    p = line["pipeline"]  # the timed call: one clean pipelined run
    assert (p["runs"], p["per_picture"], p["fallbacks"], p["waits_gave_up"]) == (1, 0, 0, 0), p
    assert line["bitexact"] is None  # not checked: --full only, like the figures below
    for k in ("roofline", "planes_roofline", "cpu_baseline"):
        assert k not in line, k

    files = sorted(os.listdir(out))
    assert files == ["bitstream.npy", "frame_bytes.npy", "recon.npy"], files
    assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20
    arrs = {f[:-4]: np.load(out / f) for f in files}
    assert arrs["bitstream"].dtype == np.float32 and arrs["recon"].dtype == np.float32 and arrs["frame_bytes"].dtype == np.float64
    last = warmup + steps - 1
    assert _md5(arrs["bitstream"]) == GOLD["frame_md5"][last]
    assert _md5(arrs["recon"]) == GOLD["recon_md5"][last]
    assert arrs["recon"].size == GOLD["width"] * GOLD["height"] * 3 // 2
    # P pictures: start code + slice NAL, no headers
    assert arrs["frame_bytes"].tolist() == [b - 3 for b in GOLD["frame_bytes"][warmup:last + 1]]
