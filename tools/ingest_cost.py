"""What the frame ingest costs (hl_amd_encode_frames, k_ingest),
on one MI355X at the bench geometry: 1920x1088, bench.py's clip, a 5-frame
warm-up call, then 120 frames as one call.

  python tools/ingest_cost.py [--parent parent/libhartallo_amd.so] > profiles/ingest_cost.log

  (a) the parent commit's library (when given): encode_batch_device, RUNS times
  (b') this build: the same call, RUNS times in a process of its own like (a)
  (b) this build: the same call
  (c) this build: encode_frames_device with dense I420 frames (forwarded)
  (d) this build: encode_frames_device with pitched NV12 frames
  (e) this build: encode_frames_device with RGB24 frames
      (b) to (e) alternate within one process, RUNS times each; (a) to (d) give
      the same bytes every time
  (f) in the same process: k_ingest alone per format (hl_amd_bench_ingest: a
      16-frame launch and a one-frame launch) beside k_planes alone
      (hl_amd_bench_planes)

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
NV12_PAD, ALONE_FRAMES = 64, 16


def child(lib, mode):
    sys.path.insert(0, ROOT)
    import torch

    from hartallo_amd import _lib

    _lib.load_library(os.path.abspath(lib))
    import bench
    from hartallo_amd import Encoder

    W, H = bench.W, bench.H
    ny = W * H
    n = WARM + STEPS
    clip = bench.bench_clip(n, SEED)
    dev = torch.from_numpy(clip).cuda()
    torch.cuda.synchronize()
    ptrs = [(dev[i].data_ptr(), dev[i].data_ptr() + ny, dev[i].data_ptr() + ny + ny // 4) for i in range(n)]
    out = {"lib": os.path.relpath(lib, ROOT), "mode": mode, "runs": [], "alone": []}
    kinds = ["batch"] * RUNS if mode == "base" else ["batch", "i420_dense", "nv12_pitched", "rgb24"] * RUNS
    frames = {}
    if mode != "base":
        from hartallo_amd import Frame
        from hartallo_amd import _lib as L

        y = dev[:, :ny].view(n, H, W)
        u = dev[:, ny:ny + ny // 4].view(n, H // 2, W // 2)
        v = dev[:, ny + ny // 4:].view(n, H // 2, W // 2)
        frames["i420_dense"] = [Frame.i420(y[i], u[i], v[i]) for i in range(n)]
        ybuf = torch.zeros((n, H, W + NV12_PAD), dtype=torch.uint8, device="cuda")
        cbuf = torch.zeros((n, H // 2, W + NV12_PAD), dtype=torch.uint8, device="cuda")
        ybuf[:, :, :W] = y
        cbuf[:, :, 0:W:2] = u
        cbuf[:, :, 1:W:2] = v
        frames["nv12_pitched"] = [Frame.nv12(ybuf[i, :, :W], cbuf[i, :, :W]) for i in range(n)]
        # RGB content: the luma, and the luma moved by a few samples, as the three channels
        rgb = torch.stack([y, torch.roll(y, 3, 2), torch.roll(y, 5, 1)], dim=-1).contiguous()
        frames["rgb24"] = [Frame.from_array(rgb[i]) for i in range(n)]
        torch.cuda.synchronize()
    for kind in kinds:
        enc = Encoder(W, H, 28, 16, 1, 30)
        enc.set_timing(True)
        if kind == "batch":
            outs = [r.annexb() for r in enc.encode_batch_device(ptrs[:WARM])]
        else:
            outs = [r.annexb() for r in enc.encode_frames_device(frames[kind][:WARM])]
        torch.cuda.synchronize()
        t = time.perf_counter()
        if kind == "batch":
            enc.encode_batch_device(ptrs[WARM:], collect=False)
        else:
            enc.encode_frames_device(frames[kind][WARM:], collect=False)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t) * 1e3
        outs += [r.annexb() for r in enc.last_batch_results()]
        out["runs"].append({"kind": kind, "call_ms": round(dt, 2), "kernel_ms": round(enc.timing_ms()[1], 2), "bytes": sum(map(len, outs)),
                            "md5": hashlib.md5(b"".join(outs)).hexdigest()})
        enc.close()
    if mode != "base":  # k_ingest alone, per format
        k = ALONE_FRAMES
        rgba = torch.cat([rgb[:k], torch.zeros((k, H, W, 1), dtype=torch.uint8, device="cuda")], dim=-1).contiguous()
        rgbp = rgb[:k].permute(0, 3, 1, 2).contiguous()
        ubuf = torch.zeros((k, H // 2, W // 2 + NV12_PAD // 2), dtype=torch.uint8, device="cuda")
        vbuf = torch.zeros_like(ubuf)
        sets = {
            "i420_pitched": ([Frame.i420(ybuf[i, :, :W], ubuf[i, :, :W // 2], vbuf[i, :, :W // 2]) for i in range(k)], 1.5),
            "nv12_pitched": (frames["nv12_pitched"][:k], 1.5),
            "rgb24": (frames["rgb24"][:k], 3.0),
            "rgba32": ([Frame.from_array(rgba[i]) for i in range(k)], 4.0),
            "rgbp": ([Frame.from_array(rgbp[i]) for i in range(k)], 3.0),
        }
        torch.cuda.synchronize()
        for name, (fs, read) in sets.items():
            enc = Encoder(W, H, 28, 16, 1, 30)
            enc.encode_frames_device(fs, collect=False)
            many = enc.bench_ingest(20) / k  # ms per frame inside a k-frame launch
            enc.encode_frame(fs[0])
            one = enc.bench_ingest(50)       # ms of a one-frame launch
            planes = enc.bench_planes(50)
            moved = (read + 1.5) * W * H
            out["alone"].append({"format": name, "us_per_frame_in_16": round(many * 1e3, 2), "GB_per_s_in_16": round(moved / (many * 1e-3) / 1e9, 1),
                                 "us_one_frame_launch": round(one * 1e3, 2), "GB_per_s_one": round(moved / (one * 1e-3) / 1e9, 1),
                                 "k_planes_us": round(planes * 1e3, 2)})
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
    print(f"ingest cost: {WARM}-frame warm-up call, then {STEPS} frames in one call, 1920x1088, bench clip seed {SEED}")
    a = None
    if parent:
        print("(a) the parent commit, encode_batch_device")
        a = run_child(parent, "base")["runs"]
    print("(b') this build, encode_batch_device, in a process of its own like (a)")
    b1 = run_child(here, "base")["runs"]
    print("(b) encode_batch_device, (c) encode_frames dense I420, (d) pitched NV12, (e) RGB24: this build, alternating")
    o = run_child(here, "all")
    by = {k: [r for r in o["runs"] if r["kind"] == k] for k in ("batch", "i420_dense", "nv12_pitched", "rgb24")}
    md5s = {r["md5"] for r in (a or []) + b1 + by["batch"] + by["i420_dense"] + by["nv12_pitched"]}
    assert len(md5s) == 1, f"the streams of (a) to (d) differ: {md5s}"
    assert len({r["md5"] for r in by["rgb24"]}) == 1

    def stat(rs, key="call_ms"):
        v = sorted(r[key] for r in rs)
        return round((v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2, 2), v[0], v[-1]

    print(f"summary (median, min, max of the timed call in ms; (a) to (d): one MD5, {md5s.pop()}):")
    rows = ([("(a) parent batch", a)] if a else []) + [("(b') batch, own process", b1), ("(b) batch", by["batch"]), ("(c) frames, dense I420", by["i420_dense"]),
                                                       ("(d) frames, pitched NV12", by["nv12_pitched"]), ("(e) frames, RGB24", by["rgb24"])]
    for name, rs in rows:
        print(f"  {name:26s} {stat(rs)}   kernel {stat(rs, 'kernel_ms')}")
    base, ref = (stat(a), "(a)") if a else (stat(b1), "(b')")
    print(f"  spread of {ref} (max - min): {base[2] - base[1]:.2f} ms")
    for name, rs in rows[1:]:
        print(f"  {name} median - {ref} median = {stat(rs)[0] - base[0]:+.2f} ms per call = {(stat(rs)[0] - base[0]) / STEPS * 1e3:+.1f} us per picture")
    print(f"(f) k_ingest alone, per 1920x1088 frame (bytes moved = source rows + 1.5 W H written):")
    for r in o["alone"]:
        print(f"  {json.dumps(r)}")


if __name__ == "__main__":
    main()
