"""What the source size costs (hl_amd_set_source_size, k_scale),
on one MI355X at the bench geometry: 1920x1088 coded, bench.py's clip, a
5-frame warm-up call, then 120 frames as one call.

  python tools/scale_cost.py [--parent parent/libhartallo_amd.so] > profiles/scale_cost.log

  (a) the parent commit's library (when given): encode_frames_device of
      1088-row NV12 frames, pitch W + 64, RUNS times in a process of its own
  (b) this build: the same call, no source size, RUNS times in a process of its
      own like (a)
      with a parent (a) and (b) alternate, RUNS processes each
  (b2), (c), (d) alternate within one process, RUNS times each:
  (b2) this build: the same call as (b)
  (c) this build: display 1920x1080, source 3840x2160, pitched NV12 frames
  (d) as (c) with RGB24 frames
      (a), (b), (b2) give the same bytes.  The 4K frames are the top 1080 rows
      of the bench clip with every sample repeated 2x2, so (c) codes that
      1080-row clip (the 2x2 box gives it back) edge-padded to 1088 rows: not
      the 1088-row content of (a); (d)'s channels are the luma and the luma
      moved by a few samples.
  (e) in the same process, per geometry: the scale launches alone
      (hl_amd_bench_scale) and the ingest launches alone (hl_amd_bench_ingest)
      of a 16-frame call and of a one-frame call of pitched NV12 frames, and
      the coding time per picture of that 16-frame call (set_timing)

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
WARM, STEPS, RUNS, SEED = 5, 120, 3, 11
PAD, ALONE_FRAMES, DH = 64, 16, 1080
# source, display, coded
GEOMETRIES = [((3840, 2160), (1920, 1080), (1920, 1088)), ((2880, 1620), (1920, 1080), (1920, 1088)), ((1920, 1080), (854, 480), (864, 480))]


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
    dev = torch.from_numpy(bench.bench_clip(n, SEED)).cuda()
    y = dev[:, :ny].view(n, H, W)
    u = dev[:, ny:ny + ny // 4].view(n, H // 2, W // 2)
    v = dev[:, ny + ny // 4:].view(n, H // 2, W // 2)

    def nv12(k, sw, sh):
        """the first k frames' top 1080 rows resampled (nearest) to sw x sh, as NV12 with PAD bytes between the rows"""
        ry, rx = torch.arange(sh, device="cuda") * DH // sh, torch.arange(sw, device="cuda") * W // sw
        cy, cx = torch.arange(sh // 2, device="cuda") * (DH // 2) // (sh // 2), torch.arange(sw // 2, device="cuda") * (W // 2) // (sw // 2)
        ybuf = torch.zeros((k, sh, sw + PAD), dtype=torch.uint8, device="cuda")
        cbuf = torch.zeros((k, sh // 2, sw + PAD), dtype=torch.uint8, device="cuda")
        ybuf[:, :, :sw] = y[:k][:, ry][:, :, rx]
        cbuf[:, :, 0:sw:2] = u[:k][:, cy][:, :, cx]
        cbuf[:, :, 1:sw:2] = v[:k][:, cy][:, :, cx]
        return [Frame.nv12(ybuf[i, :, :sw], cbuf[i, :, :sw]) for i in range(k)]

    ybuf = torch.zeros((n, H, W + PAD), dtype=torch.uint8, device="cuda")
    cbuf = torch.zeros((n, H // 2, W + PAD), dtype=torch.uint8, device="cuda")
    ybuf[:, :, :W] = y
    cbuf[:, :, 0:W:2] = u
    cbuf[:, :, 1:W:2] = v
    frames = {"nv12_1088": [Frame.nv12(ybuf[i, :, :W], cbuf[i, :, :W]) for i in range(n)]}
    kinds = ["nv12_1088"] * RUNS
    if mode == "scale":
        frames["nv12_4k"] = nv12(n, 3840, 2160)
        y4 = y[:, :DH].repeat_interleave(2, 1).repeat_interleave(2, 2)
        rgb = torch.stack([y4, torch.roll(y4, 3, 2), torch.roll(y4, 5, 1)], dim=-1).contiguous()
        del y4
        frames["rgb24_4k"] = [Frame.from_array(rgb[i]) for i in range(n)]
        kinds = ["nv12_1088", "nv12_4k", "rgb24_4k"] * RUNS
    torch.cuda.synchronize()
    out = {"lib": os.path.relpath(lib, ROOT), "mode": mode, "runs": [], "alone": []}
    for kind in kinds:
        enc = Encoder(W, H, 28, 16, 1, 30)
        if kind.endswith("4k"):
            enc.set_display_size(W, DH)
            enc.set_source_size(3840, 2160)
        enc.set_timing(True)
        res = enc.encode_frames_device(frames[kind][:WARM])
        torch.cuda.synchronize()
        t = time.perf_counter()
        enc.encode_frames_device(frames[kind][WARM:], collect=False)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t) * 1e3
        res += enc.last_batch_results()
        out["runs"].append({"kind": kind, "call_ms": round(dt, 2), "kernel_ms": round(enc.timing_ms()[1], 2),
                            "bytes": sum(len(r.annexb()) for r in res), "md5": hashlib.md5(b"".join(r.annexb() for r in res)).hexdigest(),
                            "slices_md5": hashlib.md5(b"".join(r.data for r in res)).hexdigest()})
        enc.close()
    if mode == "scale":  # the scale and ingest launches alone, per geometry
        del frames, rgb
        k = ALONE_FRAMES
        for src, disp, coded in GEOMETRIES:
            fs = nv12(k, *src)
            torch.cuda.synchronize()
            enc = Encoder(*coded, 28, 16, 1, 30)
            if disp != coded:
                enc.set_display_size(*disp)
            enc.set_source_size(*src)
            enc.set_timing(True)
            enc.encode_frames_device(fs, collect=False)
            code_us = enc.timing_ms()[1] * 1e3 / k  # kernel time of the call per picture
            many, many_in = enc.bench_scale(20) / k, enc.bench_ingest(20) / k  # ms per frame inside a k-frame call
            enc.encode_frame(fs[0])
            one, one_in = enc.bench_scale(50), enc.bench_ingest(50)  # ms of a one-frame call
            nbytes = src[0] * src[1] * 3 // 2 + coded[0] * coded[1] * 3 // 2  # source planes read + coded planes written
            out["alone"].append({"source": src, "display": disp, "coded": coded, "scale_us_per_frame_in_16": round(many * 1e3, 2),
                                 "scale_us_one_frame": round(one * 1e3, 2), "scale_GBps_in_16": round(nbytes / many / 1e6, 1),
                                 "scale_GBps_one_frame": round(nbytes / one / 1e6, 1), "ingest_us_per_frame_in_16": round(many_in * 1e3, 2),
                                 "ingest_us_one_frame": round(one_in * 1e3, 2), "coding_us_per_picture": round(code_us, 1),
                                 "scale_share_of_coding_pct": round(100 * many * 1e3 / code_us, 2)})
            enc.close()
            del fs
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
    parent = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--parent" else None
    print(f"scale cost: {WARM}-frame warm-up call, then {STEPS} frames in one call, 1920x1088 coded, bench clip seed {SEED}")
    a, b = None, []
    if parent:
        print(f"(a) the parent commit, (b) this build with no source size: encode_frames_device of 1088-row pitched NV12 frames, "
              f"alternating, {RUNS} processes each")
        a = []
        for _ in range(RUNS):
            a += run_child(parent, "base")["runs"]
            b += run_child(here, "base")["runs"]
    else:
        print("(b) this build, encode_frames_device of 1088-row pitched NV12 frames, no source size, in a process of its own")
        b = run_child(here, "base")["runs"]
    print("(b2) the same call, (c) source 3840x2160 NV12 to display 1920x1080, (d) the same from RGB24: this build, alternating")
    o = run_child(here, "scale")
    by = {k: [r for r in o["runs"] if r["kind"] == k] for k in ("nv12_1088", "nv12_4k", "rgb24_4k")}
    md5s = {r["md5"] for r in (a or []) + b + by["nv12_1088"]}
    assert len(md5s) == 1, f"the streams of (a), (b), (b2) differ: {md5s}"
    assert len({r["md5"] for r in by["nv12_4k"]}) == 1 and len({r["md5"] for r in by["rgb24_4k"]}) == 1

    def stat(rs, key="call_ms"):
        vals = sorted(r[key] for r in rs)
        return round((vals[(len(vals) - 1) // 2] + vals[len(vals) // 2]) / 2, 2), vals[0], vals[-1]

    print(f"summary (median, min, max of the timed call in ms; (a), (b), (b2): one MD5, {md5s.pop()}):")
    rows = ([("(a) parent, NV12 1088", a)] if a else []) + [("(b) NV12 1088, own process", b)]
    rows += [("(b2) NV12 1088", by["nv12_1088"]), ("(c) 4K NV12 -> 1080", by["nv12_4k"]), ("(d) 4K RGB24 -> 1080", by["rgb24_4k"])]
    for name, rs in rows:
        print(f"  {name:30s} {stat(rs)}   kernel {stat(rs, 'kernel_ms')}")
    base, ref = (stat(a), "(a)") if a else (stat(b), "(b)")
    print(f"  spread of {ref} (max - min): {base[2] - base[1]:.2f} ms")
    for name, rs in rows[1:]:
        print(f"  {name} median - {ref} median = {stat(rs)[0] - base[0]:+.2f} ms per call = {(stat(rs)[0] - base[0]) / STEPS * 1e3:+.1f} us per picture")
    print("(e) the scale and ingest launches alone, pitched NV12 frames; GB/s = (source planes read + coded planes written) / scale time:")
    for r in o["alone"]:
        print(f"  {json.dumps(r)}")


if __name__ == "__main__":
    main()
