"""What the rendition ladder's fan-out saves (hl_amd_encode_ladder_frames,
k_scale_fan), on one MI355X: a 3840x2160 device source, as
pitched NV12 and as RGBA32, into 1920x1080 in 1920x1088, 1280x720 and 854x480 in
864x480; a 5-frame call, then 60 frames.

  python tools/ladder_cost.py --parent parent/libhartallo_amd.so > profiles/ladder_cost.log

  (a) the parent commit's library: three encode_frames_device calls (one per
      rung) for the 5 frames, then three for the 60 frames, timed together
  (b) this build: one encode_ladder_frames_device call for the 5 frames, then
      one for the 60 frames, timed
      (a) and (b) alternate, RUNS processes each, every process both sources
  (c) in (b)'s processes, on a 16-frame call: the fan-out launch alone
      (hl_amd_bench_ladder) and its one ingest (hl_amd_bench_ingest) beside the
      sum of the three rungs' hl_amd_bench_scale and hl_amd_bench_ingest figures
      of three encode_frames_device calls on this build

The 4K frames are the top 1080 rows of bench.py's clip with every sample
repeated 2x2 (RGBA32: the luma, the luma moved by a few samples, 255).  Every
library runs in a process of its own.  Development tool: it asserts that (b)'s
three streams have the MD5s of (a)'s, and that (b)'s median is not above (a)'s
by more than (a)'s own spread (max - min) in this session; it sets no pass mark
on the gain.
"""
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, STEPS, RUNS, SEED = 5, 60, 3, 11
PAD, ALONE_FRAMES, DH = 64, 16, 1080
SOURCE = (3840, 2160)
# display, coded
RUNGS = [((1920, 1080), (1920, 1088)), ((1280, 720), (1280, 720)), ((854, 480), (864, 480))]


def child(lib, mode):
    sys.path.insert(0, ROOT)
    import torch

    from hartallo_amd import _lib

    _lib.load_library(os.path.abspath(lib))
    import bench
    from hartallo_amd import Encoder, Frame

    W, H = bench.W, bench.H
    ny = W * H
    n = WARM + STEPS
    sw, sh = SOURCE
    dev = torch.from_numpy(bench.bench_clip(n, SEED)).cuda()
    y = dev[:, :ny].view(n, H, W)[:, :DH]
    u = dev[:, ny:ny + ny // 4].view(n, H // 2, W // 2)[:, :DH // 2]
    v = dev[:, ny + ny // 4:].view(n, H // 2, W // 2)[:, :DH // 2]

    def encoders():
        out = []
        for disp, coded in RUNGS:
            e = Encoder(*coded, 28, 16, 1, 30)
            if disp != coded:
                e.set_display_size(*disp)
            e.set_source_size(sw, sh)
            out.append(e)
        return out

    out = {"lib": os.path.relpath(lib, ROOT), "mode": mode, "runs": [], "alone": []}
    for kind in ("nv12", "rgba32"):
        if kind == "nv12":
            ybuf = torch.zeros((n, sh, sw + PAD), dtype=torch.uint8, device="cuda")
            cbuf = torch.zeros((n, sh // 2, sw + PAD), dtype=torch.uint8, device="cuda")
            ybuf[:, :, :sw] = y.repeat_interleave(2, 1).repeat_interleave(2, 2)
            cbuf[:, :, 0:sw:2] = u.repeat_interleave(2, 1).repeat_interleave(2, 2)
            cbuf[:, :, 1:sw:2] = v.repeat_interleave(2, 1).repeat_interleave(2, 2)
            frames = [Frame.nv12(ybuf[i, :, :sw], cbuf[i, :, :sw]) for i in range(n)]
        else:
            y4 = y.repeat_interleave(2, 1).repeat_interleave(2, 2)
            rgba = torch.stack([y4, torch.roll(y4, 3, 2), torch.roll(y4, 5, 1), torch.full_like(y4, 255)], dim=-1).contiguous()
            del y4
            frames = [Frame.from_array(rgba[i]) for i in range(n)]
        torch.cuda.synchronize()
        encs = encoders()
        if mode == "ladder":
            res = Encoder.encode_ladder_frames_device(encs, frames[:WARM])
            torch.cuda.synchronize()
            t = time.perf_counter()
            Encoder.encode_ladder_frames_device(encs, frames[WARM:], collect=False)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t) * 1e3
        else:
            res = [e.encode_frames_device(frames[:WARM]) for e in encs]
            torch.cuda.synchronize()
            t = time.perf_counter()
            for e in encs:
                e.encode_frames_device(frames[WARM:], collect=False)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t) * 1e3
        md5 = [hashlib.md5(b"".join(x.annexb() for x in res[r] + e.last_batch_results())).hexdigest() for r, e in enumerate(encs)]
        out["runs"].append({"kind": kind, "call_ms": round(dt, 2), "md5": md5})
        for e in encs:
            e.close()
        if mode == "ladder":  # the launches alone, of a 16-frame call
            k = ALONE_FRAMES
            encs = encoders()
            Encoder.encode_ladder_frames_device(encs, frames[:k], collect=False)
            fan, fan_in = encs[0].bench_ladder(20) / k, encs[0].bench_ingest(20) / k
            for e in encs:
                e.close()
            encs = encoders()
            scale, ingest = [], []
            for e in encs:
                e.encode_frames_device(frames[:k], collect=False)
                scale.append(e.bench_scale(20) / k)
                ingest.append(e.bench_ingest(20) / k)
                e.close()
            out["alone"].append({"kind": kind, "fan_out_us_per_frame": round(fan * 1e3, 2), "one_ingest_us_per_frame": round(fan_in * 1e3, 2),
                                 "three_scales_us_per_frame": [round(s * 1e3, 2) for s in scale], "three_scales_sum_us": round(sum(scale) * 1e3, 2),
                                 "three_ingests_us_per_frame": [round(s * 1e3, 2) for s in ingest], "three_ingests_sum_us": round(sum(ingest) * 1e3, 2),
                                 "front_end_ladder_us": round((fan + fan_in) * 1e3, 2), "front_end_per_encoder_us": round((sum(scale) + sum(ingest)) * 1e3, 2)})
        del frames
        if kind == "nv12":
            del ybuf, cbuf
        else:
            del rgba
    print(json.dumps(out), flush=True)


def run_child(lib, mode):
    r = subprocess.run([sys.executable, "-u", __file__, "--child", lib, mode], capture_output=True, text=True, timeout=900)
    if r.returncode:
        sys.stderr.write(r.stderr)
        sys.exit(r.returncode)  # (nothing more is started on the GPU after a failure)
    o = json.loads(r.stdout.strip().splitlines()[-1])
    for run in o["runs"]:
        print(f"  {o['lib']} {o['mode']}: {json.dumps(run)}", flush=True)
    return o


def main():
    if len(sys.argv) > 3 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
        return
    here = os.path.join(ROOT, "hartallo_amd", "libhartallo_amd.so")
    if len(sys.argv) < 3 or sys.argv[1] != "--parent":
        sys.exit(__doc__)
    parent = sys.argv[2]
    print(f"ladder cost: source {SOURCE[0]}x{SOURCE[1]} -> {', '.join(f'{d[0]}x{d[1]} in {c[0]}x{c[1]}' for d, c in RUNGS)}; "
          f"a {WARM}-frame call, then {STEPS} frames (timed), bench clip seed {SEED}")
    print(f"(a) the parent commit: three encode_frames_device calls; (b) this build: one encode_ladder_frames_device call; alternating, {RUNS} processes each")
    a, b, alone = [], [], []
    for _ in range(RUNS):
        a += run_child(parent, "parent")["runs"]
        o = run_child(here, "ladder")
        b += o["runs"]
        alone += o["alone"]

    def stat(rs):
        vals = sorted(r["call_ms"] for r in rs)
        return round((vals[(len(vals) - 1) // 2] + vals[len(vals) // 2]) / 2, 2), vals[0], vals[-1]

    ok = True
    print("summary (median, min, max of the timed 60-frame call(s) in ms):")
    for kind in ("nv12", "rgba32"):
        ra, rb = [r for r in a if r["kind"] == kind], [r for r in b if r["kind"] == kind]
        md5s = {tuple(r["md5"]) for r in ra + rb}
        assert len(md5s) == 1, f"{kind}: the streams of (a) and (b) differ: {md5s}"
        sa, sb = stat(ra), stat(rb)
        spread = sa[2] - sa[1]
        print(f"  {kind}: the three streams' MD5s, (a) = (b): {list(md5s.pop())}")
        print(f"  {kind}: (a) three calls on the parent {sa}   (b) one ladder call {sb}")
        print(f"  {kind}: (b) median - (a) median = {sb[0] - sa[0]:+.2f} ms per 60 frames = {(sb[0] - sa[0]) / STEPS * 1e3:+.1f} us per source frame; "
              f"spread of (a) (max - min): {spread:.2f} ms")
        ok = ok and sb[0] <= sa[0] + spread
    print(f"(c) the launches alone, per source frame of a {ALONE_FRAMES}-frame call (this build):")
    for r in alone:
        print(f"  {json.dumps(r)}")
    assert ok, "(b)'s median is above (a)'s by more than (a)'s spread"
    print("ok: (b) is not above (a) by more than (a)'s spread")


if __name__ == "__main__":
    main()
