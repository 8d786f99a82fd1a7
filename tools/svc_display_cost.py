"""What the access unit's display size costs (hl_amd_set_au_display_size,
hl_amd_encode_au_frames, k_ingest_edge with wide margins), on
one MI355X at config 4's geometry: three dyadic layers up to 1920x1088, a
5-access-unit warm-up call, then 30 access units as one call, RUNS times each.

  python tools/svc_display_cost.py [--parent parent/libhartallo_amd.so] > profiles/svc_display_cost.log

The 1080-line clip is the top 1080 rows of synth.clip(1920, 1088); "caller-padded"
tops are that clip edge-padded to 1088 rows, which is also what the encoder's
own padding must give.

  (a) the parent commit's library (when given): encode_aus_batch_device of
      caller-padded 1088-row tops
  (b) this build: the same call, no display size, in a process of its own like (a)
  (b2), (c) alternate within one process:
  (b2) this build: the same call as (b)
  (c) this build: display 1920x1080, pitched NV12 frames of 1080 rows through
      encode_au_frames_device
      (a), (b), (b2) give the same bytes; (c)'s NAL units other than the SPS and
      subset SPSs are theirs
  (d) this build: 1280x720 in 1280x768 (layers 320x192, 640x384), pitched NV12
      frames through encode_au_frames_device, and (d0) the same clip
      caller-padded through encode_aus_batch_device
  (e) the ingest launches alone (hl_amd_bench_ingest, a 16-frame call and a
      one-frame call): margins of 8 rows (1920x1080) and of 48 rows (1280x720),
      and without a margin

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
WARM, STEPS, RUNS, SEED = 5, 30, 3, 41
PAD, ALONE_FRAMES = 64, 16
GEOM = {"1080": (480, 272, 1920, 1080), "720": (320, 192, 1280, 720)}  # base size, top display size (three layers)


def nals_but_sps(stream: bytes):
    return [x for x in stream.split(b"\x00\x00\x01")[1:] if (x[0] & 31) not in (7, 15)]


def child(lib, mode):
    sys.path.insert(0, ROOT)
    import torch

    from hartallo_amd import _lib

    _lib.load_library(os.path.abspath(lib))
    from hartallo_amd import Frame, SvcEncoder, synth

    n = WARM + STEPS
    out = {"lib": os.path.relpath(lib, ROOT), "mode": mode, "runs": [], "alone": []}
    data = {}
    for g, (w0, h0, dw, dh) in GEOM.items():
        if mode == "base" and g != "1080":
            continue
        W, H = w0 << 2, h0 << 2
        ny = W * H
        dev = torch.from_numpy(synth.clip(W, H, n, SEED)).cuda()
        y = dev[:, :ny].view(n, H, W)
        u = dev[:, ny:ny + ny // 4].view(n, H // 2, W // 2)
        v = dev[:, ny + ny // 4:].view(n, H // 2, W // 2)
        # the display rectangle edge-padded to the coded size: dense I420 tops, and pitched NV12 of the display size
        top = torch.empty((n, ny * 3 // 2), dtype=torch.uint8, device="cuda")
        ty, tu, tv = top[:, :ny].view(n, H, W), top[:, ny:ny + ny // 4].view(n, H // 2, W // 2), top[:, ny + ny // 4:].view(n, H // 2, W // 2)
        for t, s, a, b in ((ty, y, dh, dw), (tu, u, dh // 2, dw // 2), (tv, v, dh // 2, dw // 2)):
            t[:, :a, :b] = s[:, :a, :b]
            t[:, :a, b:] = s[:, :a, b - 1:b]
            t[:, a:, :] = t[:, a - 1:a, :]
        ybuf = torch.zeros((n, dh, dw + PAD), dtype=torch.uint8, device="cuda")
        cbuf = torch.zeros((n, dh // 2, dw + PAD), dtype=torch.uint8, device="cuda")
        ybuf[:, :, :dw] = y[:, :dh, :dw]
        cbuf[:, :, 0:dw:2] = u[:, :dh // 2, :dw // 2]
        cbuf[:, :, 1:dw:2] = v[:, :dh // 2, :dw // 2]
        p0 = top.data_ptr()
        data[g] = {
            "keep": (dev, top, ybuf, cbuf),
            "tops": [(p0 + i * (ny * 3 // 2), p0 + i * (ny * 3 // 2) + ny, p0 + i * (ny * 3 // 2) + ny + ny // 4) for i in range(n)],
            "nv12": [Frame.nv12(ybuf[i, :, :dw], cbuf[i, :, :dw]) for i in range(n)],
        }
    torch.cuda.synchronize()
    kinds = [("1080", "tops")] * RUNS if mode == "base" else [("1080", "tops"), ("1080", "nv12"), ("720", "tops"), ("720", "nv12")] * RUNS
    for g, kind in kinds:
        w0, h0, dw, dh = GEOM[g]
        enc = SvcEncoder(w0, h0, 3, 28, 16, 1, 30)
        if kind == "nv12":
            enc.set_au_display_size(dw, dh)
        src = data[g][kind]
        call = enc.encode_aus_batch_device if kind == "tops" else enc.encode_au_frames_device
        res = call(src[:WARM])
        torch.cuda.synchronize()
        t = time.perf_counter()
        res += call(src[WARM:])
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t) * 1e3
        stream = b"".join(r.annexb() for r in res)
        out["runs"].append({"kind": f"{g}_{kind}", "call_ms": round(dt, 2), "bytes": len(stream), "md5": hashlib.md5(stream).hexdigest(),
                            "slices_md5": hashlib.md5(b"\x00".join(nals_but_sps(stream))).hexdigest(), "unpinned": enc.unpinned()})
        enc.close()
    if mode == "display":  # the ingest launches alone
        k = ALONE_FRAMES
        for g, (w0, h0, dw, dh) in GEOM.items():
            W, H = w0 << 2, h0 << 2
            for rows, cols, what in ((dh, dw, f"margin {H - dh} rows"), (H, W, "no margin")):
                if rows == H:  # frames of the coded size: pitched NV12 views of fresh buffers
                    yb = torch.zeros((k, H, W + PAD), dtype=torch.uint8, device="cuda")
                    cb = torch.zeros((k, H // 2, W + PAD), dtype=torch.uint8, device="cuda")
                    fs = [Frame.nv12(yb[i, :, :W], cb[i, :, :W]) for i in range(k)]
                else:
                    fs = data[g]["nv12"][:k]
                torch.cuda.synchronize()
                enc = SvcEncoder(w0, h0, 3, 28, 16, 1, 30)
                enc.set_au_display_size(cols, rows)
                enc.encode_au_frames_device(fs)
                many = enc.bench_ingest(20) / k
                enc.encode_au_frame(fs[0])
                one = enc.bench_ingest(50)
                pyr = enc.bench_pyramid(50)
                out["alone"].append({"top": f"{W}x{H}", "frames": f"{cols}x{rows} nv12_pitched", "what": what,
                                     "us_per_frame_in_16": round(many * 1e3, 2), "us_one_frame": round(one * 1e3, 2),
                                     "pyramid_us": round(pyr * 1e3, 2)})
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
    print(f"svc display cost: {WARM}-access-unit warm-up call, then {STEPS} access units in one call, three layers, synth.clip seed {SEED}")
    a = None
    if parent:
        print("(a) the parent commit, encode_aus_batch_device of caller-padded 1920x1088 tops")
        a = run_child(parent, "base")["runs"]
    print("(b) this build, the same call, no display size, in a process of its own like (a)")
    b = run_child(here, "base")["runs"]
    print("(b2) the same call, (c) display 1920x1080 with NV12 frames, (d0) 1280x768 caller-padded, (d) display 1280x720 with NV12 frames: this build, alternating")
    o = run_child(here, "display")
    by = {k: [r for r in o["runs"] if r["kind"] == k] for k in ("1080_tops", "1080_nv12", "720_tops", "720_nv12")}
    md5s = {r["md5"] for r in (a or []) + b + by["1080_tops"]}
    assert len(md5s) == 1, f"the streams of (a), (b), (b2) differ: {md5s}"
    for g in ("1080", "720"):
        slices = {r["slices_md5"] for r in by[g + "_tops"] + by[g + "_nv12"]}
        assert len(slices) == 1, f"{g}: the slices of the frame call are not those of the caller-padded tops: {slices}"
        assert len({r["md5"] for r in by[g + "_nv12"]}) == 1 and {r["md5"] for r in by[g + "_nv12"]} != {r["md5"] for r in by[g + "_tops"]}

    def stat(rs, key="call_ms"):
        vals = sorted(r[key] for r in rs)
        return round((vals[(len(vals) - 1) // 2] + vals[len(vals) // 2]) / 2, 2), vals[0], vals[-1]

    print(f"summary (median, min, max of the timed call in ms; (a), (b), (b2): one MD5, {md5s.pop()}; (c), (d): the slices of (b2), (d0)):")
    rows = ([("(a) parent, tops 1088", a)] if a else []) + [("(b) tops 1088, own process", b), ("(b2) tops 1088", by["1080_tops"]),
                                                            ("(c) display 1080, NV12", by["1080_nv12"]), ("(d0) tops 1280x768", by["720_tops"]),
                                                            ("(d) display 720, NV12", by["720_nv12"])]
    for name, rs in rows:
        print(f"  {name:28s} {stat(rs)}   unpinned {sorted({r['unpinned'] for r in rs})}")
    base, ref = (stat(a), "(a)") if a else (stat(b), "(b)")
    print(f"  spread of {ref} (max - min): {base[2] - base[1]:.2f} ms")
    for name, rs in rows[1:4]:
        print(f"  {name} median - {ref} median = {stat(rs)[0] - base[0]:+.2f} ms per call = {(stat(rs)[0] - base[0]) / STEPS * 1e3:+.1f} us per access unit")
    for x, y0, n0 in (("1080_nv12", "1080_tops", "(c) median - (b2) median"), ("720_nv12", "720_tops", "(d) median - (d0) median")):
        d = stat(by[x])[0] - stat(by[y0])[0]
        print(f"  {n0} = {d:+.2f} ms per call = {d / STEPS * 1e3:+.1f} us per access unit")
    print("(e) the ingest launches alone (k_ingest + k_ingest_edge; without a margin k_ingest only), and k_pyramid alone:")
    for r in o["alone"]:
        print(f"  {json.dumps(r)}")


if __name__ == "__main__":
    main()
