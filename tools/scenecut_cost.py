"""What scene-cut detection costs (hl_amd_set_scenecut), on one
MI355X at the bench geometry: 1920x1088, bench.py's clip, a 5-frame warm-up
call, then 20 frames as one encode_batch_device call.

  python tools/scenecut_cost.py [--parent parent/libhartallo_amd.so] > profiles/scenecut_cost.log

  (a) the parent commit's library (when given), three runs
  (b) this build, the feature off: the same bytes as (a), three runs
  (c) this build, the feature on at the defaults: the bench clip has no cut,
      so again the same bytes, and no picture is turned
  (d) the analysis launch of the 20-frame call alone, R = 8 and R = 16
  (e) a 20-frame clip whose content changes at frame 10 (two seeds), off and
      on: bytes and kernel time of the run, the size of picture 10

Every build and setting runs in a process of its own.  Development tool: it
asserts the byte identities and prints the times; it sets no bound on them.
"""
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, STEPS, RUNS, SEED, SEED2 = 5, 20, 3, 11, 12


def child(lib, mode):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from hartallo_amd import _lib

    _lib.load_library(os.path.abspath(lib))
    import bench
    from hartallo_amd import Encoder

    W, H = bench.W, bench.H
    ny = W * H
    if mode == "cut":
        clip = np.concatenate([bench.bench_clip(WARM + 10, SEED), bench.bench_clip(10, SEED2)])
    else:
        clip = bench.bench_clip(WARM + STEPS, SEED)
    dev = torch.from_numpy(clip).cuda()
    torch.cuda.synchronize()
    ptrs = [(dev[i].data_ptr(), dev[i].data_ptr() + ny, dev[i].data_ptr() + ny + ny // 4) for i in range(len(clip))]
    out = {"lib": os.path.relpath(lib, ROOT), "mode": mode, "runs": []}
    settings = {"base": [None] * RUNS, "on": [(192, 1, 8)] * RUNS + [(192, 1, 16)], "cut": [None, (192, 1, 8)]}[mode]
    for sc in settings:
        enc = Encoder(W, H, 28, 16, 1, 30)
        if sc:
            enc.set_scenecut(*sc)
        enc.set_timing(True)
        outs = [r.annexb() for r in enc.encode_batch_device(ptrs[:WARM])]
        torch.cuda.synchronize()
        t = time.perf_counter()
        enc.encode_batch_device(ptrs[WARM:], collect=False)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t) * 1e3
        res = enc.last_batch_results()
        outs += [r.annexb() for r in res]
        run = {"scenecut": sc, "call_ms": round(dt, 2), "kernel_ms": round(enc.timing_ms()[1], 2), "bytes": sum(map(len, outs)),
               "md5": hashlib.md5(b"".join(outs)).hexdigest(), "picture10_bytes": len(outs[WARM + 10])}
        if sc:
            st = [enc.last_scene_stats(k) for k in range(len(res))]
            run["turned"] = [k for k, s in enumerate(st) if s["turned"]]
            run["ratio_256P_over_I"] = [round(256 * s["P"] / s["I"], 1) for s in st if s["analysed"] and s["I"]]
            run["analysis_launch_ms"] = round(enc.bench_scene(20), 4)  # all frames of the call, one launch
            run["analysis_ms_per_frame"] = round(run["analysis_launch_ms"] / len(res), 4)
        out["runs"].append(run)
        enc.close()
    print(json.dumps(out), flush=True)


def run_child(lib, mode):
    r = subprocess.run([sys.executable, "-u", __file__, "--child", lib, mode], capture_output=True, text=True, timeout=600)
    if r.returncode:
        sys.stderr.write(r.stderr)
        sys.exit(r.returncode)  # (nothing more is started on the GPU after a failure)
    o = json.loads(r.stdout.strip().splitlines()[-1])
    for run in o["runs"]:
        print(f"  {o['lib']} {o['mode']}: {json.dumps(run)}", flush=True)
    return o["runs"]


def main():
    if len(sys.argv) > 3 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
        return
    here = os.path.join(ROOT, "hartallo_amd", "libhartallo_amd.so")
    parent = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--parent" else None
    print(f"scene-cut cost: {WARM}-frame warm-up call, then {STEPS} frames in one call, 1920x1088, bench clip seed {SEED}")
    a = None
    if parent:
        print("(a) the parent commit")
        a = run_child(parent, "base")
    print("(b) this build, the feature off")
    b = run_child(here, "base")
    print("(c) this build, the feature on (192, 1, 8); last line: range 16")
    c = run_child(here, "on")
    print("(e) content change at frame 10 of the timed call (seeds 11 | 12): off, then on")
    e = run_child(here, "cut")
    md5s = {r["md5"] for r in (a or []) + b + c}
    assert len(md5s) == 1, f"the streams differ: {md5s}"
    assert all(not r["turned"] for r in c), "a picture of the bench clip was turned"
    assert e[1]["turned"] == [10], e[1]["turned"]

    def stat(rs, key="call_ms"):
        v = sorted(r[key] for r in rs)
        return v[len(v) // 2], v[0], v[-1]

    print("summary (median, min, max of the timed call in ms):")
    if a:
        print(f"  (a) parent        {stat(a)}   kernel {stat(a, 'kernel_ms')}")
    print(f"  (b) off           {stat(b)}   kernel {stat(b, 'kernel_ms')}")
    print(f"  (c) on, R = 8     {stat(c[:RUNS])}   kernel {stat(c[:RUNS], 'kernel_ms')}")
    mb, mc = stat(b)[0], stat(c[:RUNS])[0]
    print(f"  (c) - (b) = {mc - mb:.2f} ms per call = {(mc - mb) / STEPS:.3f} ms per frame; "
          f"(d) the analysis launch alone: R = 8 {c[0]['analysis_launch_ms']} ms ({c[0]['analysis_ms_per_frame']} per frame), "
          f"R = 16 {c[RUNS]['analysis_launch_ms']} ms ({c[RUNS]['analysis_ms_per_frame']} per frame)")
    if a:
        sa = stat(a)
        print(f"  run-to-run spread of (a): {sa[2] - sa[1]:.2f} ms; (b) median - (a) median = {mb - sa[0]:.2f} ms")
    print(f"  (e) off: {e[0]['bytes']} bytes, kernel {e[0]['kernel_ms']} ms, picture 10 {e[0]['picture10_bytes']} bytes; "
          f"on: {e[1]['bytes']} bytes, kernel {e[1]['kernel_ms']} ms, picture 10 {e[1]['picture10_bytes']} bytes")


if __name__ == "__main__":
    main()
