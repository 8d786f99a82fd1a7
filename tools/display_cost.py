"""What the display size costs (hl_amd_set_display_size, k_ingest_edge, the
quality window), on one MI355X at the bench geometry: 1920x1088
coded, bench.py's clip, a 5-frame warm-up call, then 120 frames as one call.

  python tools/display_cost.py [--parent parent/libhartallo_amd.so] > profiles/display_cost.log

The 1080-line clip is the top 1080 rows of bench.py's frames; "caller-padded"
frames are that clip edge-padded to 1088 rows by torch, which is also what the
encoder's own padding must give.

  (a) the parent commit's library (when given): encode_frames_device of
      caller-padded 1088-row pitched NV12 frames, RUNS times
  (b) this build: the same call, no display size, RUNS times in a process of its
      own like (a)
  (b2), (c), (d) alternate within one process, RUNS times each:
  (b2) this build: the same call as (b)
  (c) this build: display 1920x1080, pitched NV12 frames of 1080 rows
  (d) as (c) with RGB24 frames
      (a), (b), (b2) give the same bytes; (c)'s slices are theirs
  (e) in the same process: the ingest launch(es) alone (hl_amd_bench_ingest: a
      16-frame call and a one-frame call) per format for 1088-row frames without a
      display size and for 1080-row frames with one, and the quality launch
      alone (hl_amd_bench_quality, 16 pictures) with and without the window

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
    # the 1080-line clip edge-padded to 1088 rows, as pitched NV12
    ybuf = torch.zeros((n, H, W + PAD), dtype=torch.uint8, device="cuda")
    cbuf = torch.zeros((n, H // 2, W + PAD), dtype=torch.uint8, device="cuda")
    ybuf[:, :DH, :W] = y[:, :DH]
    ybuf[:, DH:, :W] = y[:, DH - 1:DH]
    cbuf[:, :DH // 2, 0:W:2] = u[:, :DH // 2]
    cbuf[:, :DH // 2, 1:W:2] = v[:, :DH // 2]
    cbuf[:, DH // 2:, :W] = cbuf[:, DH // 2 - 1:DH // 2, :W]
    frames = {"nv12_1088": [Frame.nv12(ybuf[i, :, :W], cbuf[i, :, :W]) for i in range(n)]}
    kinds = ["nv12_1088"] * RUNS
    if mode == "display":
        frames["nv12_1080"] = [Frame.nv12(ybuf[i, :DH, :W], cbuf[i, :DH // 2, :W]) for i in range(n)]
        # RGB content: the luma, and the luma moved by a few samples, as the three channels
        rgb = torch.stack([y, torch.roll(y, 3, 2), torch.roll(y, 5, 1)], dim=-1).contiguous()
        frames["rgb24_1080"] = [Frame.from_array(rgb[i, :DH]) for i in range(n)]
        kinds = ["nv12_1088", "nv12_1080", "rgb24_1080"] * RUNS
    torch.cuda.synchronize()
    out = {"lib": os.path.relpath(lib, ROOT), "mode": mode, "runs": [], "alone": [], "quality": []}
    for kind in kinds:
        enc = Encoder(W, H, 28, 16, 1, 30)
        if kind.endswith("1080"):
            enc.set_display_size(W, DH)
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
    if mode == "display":  # the ingest launches alone, per format and frame height; the quality launch alone
        k = ALONE_FRAMES
        rgba = torch.cat([rgb[:k], torch.zeros((k, H, W, 1), dtype=torch.uint8, device="cuda")], dim=-1).contiguous()
        rgbp = rgb[:k].permute(0, 3, 1, 2).contiguous()
        ubuf = torch.zeros((k, H // 2, W // 2 + PAD // 2), dtype=torch.uint8, device="cuda")
        vbuf = torch.zeros_like(ubuf)
        torch.cuda.synchronize()
        for rows in (H, DH):
            sets = {
                "i420_pitched": [Frame.i420(ybuf[i, :rows, :W], ubuf[i, :rows // 2, :W // 2], vbuf[i, :rows // 2, :W // 2]) for i in range(k)],
                "nv12_pitched": [Frame.nv12(ybuf[i, :rows, :W], cbuf[i, :rows // 2, :W]) for i in range(k)],
                "rgb24": [Frame.from_array(rgb[i, :rows]) for i in range(k)],
                "rgba32": [Frame.from_array(rgba[i, :rows]) for i in range(k)],
                "rgbp": [Frame.from_array(rgbp[i, :, :rows]) for i in range(k)],
            }
            for name, fs in sets.items():
                enc = Encoder(W, H, 28, 16, 1, 30)
                if rows != H:
                    enc.set_display_size(W, rows)
                enc.encode_frames_device(fs, collect=False)
                many = enc.bench_ingest(20) / k  # ms per frame inside a k-frame call
                enc.encode_frame(fs[0])
                one = enc.bench_ingest(50)       # ms of a one-frame call
                out["alone"].append({"format": name, "rows": rows, "us_per_frame_in_16": round(many * 1e3, 2), "us_one_frame": round(one * 1e3, 2)})
                enc.close()
        for rows in (H, DH):
            enc = Encoder(W, H, 28, 16, 1, 30)
            if rows != H:
                enc.set_display_size(W, rows)
            enc.set_quality(True)
            enc.encode_frames_device(frames["nv12_1088" if rows == H else "nv12_1080"][:k], collect=False)
            q = enc.last_quality(k - 1)
            ms = enc.bench_quality(20)
            out["quality"].append({"rows": rows, "pictures": k, "launch_us": round(ms * 1e3, 2), "us_per_picture": round(ms * 1e3 / k, 2),
                                   "samples_y": q["samples"][0], "psnr_y": round(q["psnr_y"], 3)})
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
    return o


def main():
    if len(sys.argv) > 3 and sys.argv[1] == "--child":
        child(sys.argv[2], sys.argv[3])
        return
    here = os.path.join(ROOT, "hartallo_amd", "libhartallo_amd.so")
    parent = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--parent" else None
    print(f"display cost: {WARM}-frame warm-up call, then {STEPS} frames in one call, 1920x1088 coded, bench clip seed {SEED}")
    a = None
    if parent:
        print("(a) the parent commit, encode_frames_device of caller-padded 1088-row NV12 frames")
        a = run_child(parent, "base")["runs"]
    print("(b) this build, the same call, no display size, in a process of its own like (a)")
    b = run_child(here, "base")["runs"]
    print("(b2) the same call, (c) display 1920x1080 with 1080-row NV12 frames, (d) with 1080-row RGB24 frames: this build, alternating")
    o = run_child(here, "display")
    by = {k: [r for r in o["runs"] if r["kind"] == k] for k in ("nv12_1088", "nv12_1080", "rgb24_1080")}
    md5s = {r["md5"] for r in (a or []) + b + by["nv12_1088"]}
    assert len(md5s) == 1, f"the streams of (a), (b), (b2) differ: {md5s}"
    slices = {r["slices_md5"] for r in b + by["nv12_1088"] + by["nv12_1080"]}
    assert len(slices) == 1, f"the slices of (c) are not those of (b) fed the edge-padded frames: {slices}"
    assert len({r["md5"] for r in by["nv12_1080"]}) == 1 and len({r["md5"] for r in by["rgb24_1080"]}) == 1
    assert {r["md5"] for r in by["nv12_1080"]} != md5s  # (the SPS differs)

    def stat(rs, key="call_ms"):
        vals = sorted(r[key] for r in rs)
        return round((vals[(len(vals) - 1) // 2] + vals[len(vals) // 2]) / 2, 2), vals[0], vals[-1]

    print(f"summary (median, min, max of the timed call in ms; (a), (b), (b2): one MD5, {md5s.pop()}; (c): their slices, {slices.pop()}):")
    rows = ([("(a) parent, NV12 1088", a)] if a else []) + [("(b) NV12 1088, own process", b), ("(b2) NV12 1088", by["nv12_1088"]),
                                                            ("(c) display 1080, NV12", by["nv12_1080"]), ("(d) display 1080, RGB24", by["rgb24_1080"])]
    for name, rs in rows:
        print(f"  {name:28s} {stat(rs)}   kernel {stat(rs, 'kernel_ms')}")
    base, ref = (stat(a), "(a)") if a else (stat(b), "(b)")
    print(f"  spread of {ref} (max - min): {base[2] - base[1]:.2f} ms")
    for name, rs in rows[1:]:
        print(f"  {name} median - {ref} median = {stat(rs)[0] - base[0]:+.2f} ms per call = {(stat(rs)[0] - base[0]) / STEPS * 1e3:+.1f} us per picture")
    cb = stat(by["nv12_1080"])[0] - stat(by["nv12_1088"])[0]
    print(f"  (c) median - (b2) median = {cb:+.2f} ms per call = {cb / STEPS * 1e3:+.1f} us per picture")
    print("(e) the ingest launches alone, per 1920-wide frame (rows 1088: k_ingest, no display size; rows 1080: k_ingest + k_ingest_edge):")
    for r in o["alone"]:
        print(f"  {json.dumps(r)}")
    print("    the quality launch alone (rows 1088: no window; rows 1080: the display window):")
    for r in o["quality"]:
        print(f"  {json.dumps(r)}")


if __name__ == "__main__":
    main()
