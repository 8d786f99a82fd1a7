"""Regenerates the per-frame-control goldens from the reference encoder itself.

Each configuration in tests/fc_testlib.FC_CONFIGS is synthesised with
hartallo_amd.synth (seeded) and encoded by oracle/_ref/ref_enc_sched
(tests/refdrive/ref_sched_harness.c: the reference's own library driven
through hl_codec_encode, with hl_frame_t.encoding set and hl_codec_t settings
changed between the calls as the configuration's schedule says), and stored as:
  fc_<name>.264     the reference's Annex-B output
  fc_golden.json    per configuration its parameters and schedule, the stream
                    MD5, the SliceQPY of every slice and the MD5 of the
                    reference's reconstructed picture after every frame
                    (golden.json's fields)
and, under "identities", the schedules the reference codes exactly like a
plainer one (fc_testlib.FC_IDENTITIES), asserted here and stored as MD5s.

Run where the reference sources exist:  python tests/golden/make_frame_ctl_golden.py [out_dir]
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

from fc_testlib import FC_CONFIGS, FC_IDENTITIES, REF_ENC_SCHED, fc_input, ref_sched_command  # noqa: E402
from hl_testlib import md5, slice_qps  # noqa: E402


def nal_types(stream: bytes) -> list:
    out, i = [], 0
    while (j := stream.find(b"\x00\x00\x01", i)) >= 0:
        i = j + 3
        out.append(stream[i] & 31)
    return out


def encode(cfg, td):
    """(stream, per-frame recon) of cfg through the reference."""
    inp = os.path.join(td, cfg["name"] + ".yuv")
    fc_input(cfg).tofile(inp)
    pre = os.path.join(td, cfg["name"])
    cmd, env = ref_sched_command(REF_ENC_SCHED, cfg, inp, pre)
    r = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True, env=env)
    if r.returncode:
        raise subprocess.CalledProcessError(r.returncode, cmd, stderr=r.stderr[-2000:])
    w, h = cfg["width"], cfg["height"]
    return open(pre + ".264", "rb").read(), np.fromfile(pre + ".rec.yuv", dtype=np.uint8).reshape(-1, w * h * 3 // 2)


def entry(cfg, stream, rec):
    return {**{k: v for k, v in cfg.items() if k != "name"}, "stream_md5": md5(stream), "stream_bytes": len(stream),
            "slice_qp": slice_qps(stream, cfg["qp"]), "nal_types": nal_types(stream), "recon_md5": [md5(r) for r in rec]}


def main():
    if not os.path.exists(REF_ENC_SCHED):
        sys.exit(f"{REF_ENC_SCHED} missing: run `make oracle` where the reference sources exist")
    out_dir = sys.argv[1] if len(sys.argv) > 1 else HERE
    table = {"identities": {}}
    with tempfile.TemporaryDirectory() as td:
        for cfg in FC_CONFIGS:
            stream, rec = encode(cfg, td)
            assert len(rec) == cfg["frames"]
            with open(os.path.join(out_dir, cfg["name"] + ".264"), "wb") as f:
                f.write(stream)
            table[cfg["name"]] = entry(cfg, stream, rec)
            print(f"{cfg['name']}: {len(stream)} bytes, NAL types {table[cfg['name']]['nal_types']}")
        for cfg in FC_IDENTITIES:
            plain = dict(cfg, name=cfg["name"] + "_plain", types="-", changes="-")
            a, ra = encode(cfg, td)
            b, rb = encode(plain, td)
            assert a == b and np.array_equal(ra, rb), f"{cfg['name']}: the reference codes it unlike the plain schedule"
            table["identities"][cfg["name"]] = entry(cfg, a, ra)
            print(f"{cfg['name']}: equals the plain schedule ({len(a)} bytes)")
    with open(os.path.join(out_dir, "fc_golden.json"), "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
