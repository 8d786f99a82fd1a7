"""What the per-picture quality metric costs (hl_amd_set_quality, DESIGN.md
6.10), on one MI355X at the bench geometry: 1920x1088, bench.py's clip, a
5-frame warm-up call, then 120 frames as one encode_batch_device call.

  python tools/quality_cost.py [--parent parent/libhartallo_amd.so] > profiles/quality_cost.log

  (a) the parent commit's library (when given): the timed call, RUNS times
  (b) this build: the timed call with the feature off and on, alternating,
      RUNS times each; the same bytes as (a) every time
  (c) in the same process: k_quality alone on the 120 pictures of the last call
      (hl_amd_bench_quality; bytes moved = 2 x 1.5 W H per picture) beside
      k_planes alone (hl_amd_bench_planes)

Every library runs in a process of its own.  Development tool: it asserts the
byte identities and prints the times; it sets no bound on them.
"""
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, STEPS, RUNS, SEED = 5, 120, 4, 11


def child(lib, mode):
    sys.path.insert(0, ROOT)
    import torch

    from hartallo_amd import _lib

    _lib.load_library(os.path.abspath(lib))
    import bench
    from hartallo_amd import Encoder

    W, H = bench.W, bench.H
    ny = W * H
    clip = bench.bench_clip(WARM + STEPS, SEED)
    dev = torch.from_numpy(clip).cuda()
    torch.cuda.synchronize()
    ptrs = [(dev[i].data_ptr(), dev[i].data_ptr() + ny, dev[i].data_ptr() + ny + ny // 4) for i in range(len(clip))]
    out = {"lib": os.path.relpath(lib, ROOT), "mode": mode, "runs": []}
    settings = [False] * RUNS if mode == "base" else [False, True] * RUNS
    for on in settings:
        enc = Encoder(W, H, 28, 16, 1, 30)
        if on:
            enc.set_quality(True)
        enc.set_timing(True)
        outs = [r.annexb() for r in enc.encode_batch_device(ptrs[:WARM])]
        torch.cuda.synchronize()
        t = time.perf_counter()
        enc.encode_batch_device(ptrs[WARM:], collect=False)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t) * 1e3
        outs += [r.annexb() for r in enc.last_batch_results()]
        run = {"quality": on, "call_ms": round(dt, 2), "kernel_ms": round(enc.timing_ms()[1], 2), "bytes": sum(map(len, outs)),
               "md5": hashlib.md5(b"".join(outs)).hexdigest()}
        if on:
            q = [enc.last_quality(k) for k in range(STEPS)]
            run["psnr_y_mean"] = round(sum(x["psnr_y"] for x in q) / STEPS, 3)
            run["ssim_y_mean"] = round(sum(x["ssim_y"] for x in q) / STEPS, 5)
            ms = enc.bench_quality(20)  # the 120 pictures of the call, one launch
            run["quality_launch_ms"] = round(ms, 4)
            run["quality_ms_per_picture"] = round(ms / STEPS, 5)
            run["quality_TB_per_s"] = round(2 * 1.5 * W * H * STEPS / (ms * 1e-3) / 1e12, 3)
            pl = enc.bench_planes(50)  # one reference picture in, four planes out
            run["planes_launch_ms"] = round(pl, 4)
        out["runs"].append(run)
        enc.close()
    print(json.dumps(out), flush=True)


def run_child(lib, mode):
    r = subprocess.run([sys.executable, "-u", __file__, "--child", lib, mode], capture_output=True, text=True, timeout=900)
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
    print(f"quality cost: {WARM}-frame warm-up call, then {STEPS} frames in one call, 1920x1088, bench clip seed {SEED}")
    a = None
    if parent:
        print("(a) the parent commit")
        a = run_child(parent, "base")
    print("(b) this build, the feature off and on, alternating")
    b = run_child(here, "both")
    off, on = [r for r in b if not r["quality"]], [r for r in b if r["quality"]]
    md5s = {r["md5"] for r in (a or []) + b}
    assert len(md5s) == 1, f"the streams differ: {md5s}"

    def stat(rs, key="call_ms"):
        v = sorted(r[key] for r in rs)
        return round((v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2, 2), v[0], v[-1]

    print("summary (median, min, max of the timed call in ms):")
    if a:
        print(f"  (a) parent  {stat(a)}   kernel {stat(a, 'kernel_ms')}")
    print(f"  (b) off     {stat(off)}   kernel {stat(off, 'kernel_ms')}")
    print(f"  (b) on      {stat(on)}   kernel {stat(on, 'kernel_ms')}")
    so, sn = stat(off), stat(on)
    print(f"  feature-off spread (max - min): {so[2] - so[1]:.2f} ms; on - off (medians) = {sn[0] - so[0]:.2f} ms per call = "
          f"{(sn[0] - so[0]) / STEPS:.4f} ms per picture")
    if a:
        sa = stat(a)
        print(f"  parent spread: {sa[2] - sa[1]:.2f} ms; off median - parent median = {so[0] - sa[0]:.2f} ms")
    print(f"  (c) k_quality alone: {on[0]['quality_launch_ms']} ms per {STEPS}-picture launch = {on[0]['quality_ms_per_picture']} ms per picture, "
          f"{on[0]['quality_TB_per_s']} TB/s of source + reconstruction; k_planes alone: {on[0]['planes_launch_ms']} ms per launch")
    print(f"  mean luma PSNR {on[0]['psnr_y_mean']} dB, mean luma SSIM {on[0]['ssim_y_mean']}")


if __name__ == "__main__":
    main()
