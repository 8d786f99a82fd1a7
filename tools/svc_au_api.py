"""SVC access units from the top layer's frame alone against the per-layer
input a caller supplies today, on BASELINE config 4's geometry (480x272 /
960x544 / 1920x1088, tests/golden/svc_golden.json c4_svc3_480x272_s41):

  (a) layers   encode_layer once per layer and access unit, host planes of
               every layer (the caller scaled them);
  (b) au       encode_au, the host top frame only (k_pyramid derives the rest);
  (c) batch    encode_layers_batch_device (every layer resident in HBM)
               against encode_aus_batch_device (the top layer resident);
  (d) kernel   k_pyramid alone, HIP events around back-to-back launches, as
               bytes moved / time, next to k_planes' figure on a 1088p picture.

  python tools/svc_au_api.py [--aus 30] [--warmup 5] [--only a,b,c,d] [--lib PATH]

Wall time around calls that return the coded bytes (each ends in a device
synchronise).  The stream is the golden's 31 frames, then the same frames
again from frame 1: every access unit with a golden is checked against the
reference encoder's MD5, and every mode's whole stream against the others'.
--lib loads another build of the library (mode a needs only entry points
older builds have: run it several times on the build before this feature for
that build's run-to-run spread).  One JSON line per mode.
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAME = "c4_svc3_480x272_s41"


def md5(b) -> str:
    return hashlib.md5(b).hexdigest()


def _planes(f, w, h):
    n = w * h
    return f[:n], f[n:n + n // 4], f[n + n // 4:]


def _stats(ms):
    s = sorted(ms)
    return {"mean_ms": round(sum(ms) / len(ms), 3), "median_ms": round(s[len(s) // 2], 3), "min_ms": round(s[0], 3), "max_ms": round(s[-1], 3),
            "au_per_s": round(1e3 * len(ms) / sum(ms), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aus", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="a,b,c,d")
    ap.add_argument("--lib", default=None)
    args = ap.parse_args()
    only = set(args.only.split(","))

    from hartallo_amd import _lib

    if args.lib:
        _lib.load_library(os.path.abspath(args.lib))
    import torch

    from hartallo_amd import Encoder, SvcEncoder, synth

    g = json.load(open(os.path.join(ROOT, "tests", "golden", "svc_golden.json")))[NAME]
    L, w0, h0 = g["layers"], g["w0"], g["h0"]
    clips = synth.svc_clips(w0 << (L - 1), h0 << (L - 1), L, g["frames"], g["seed"])
    total = args.warmup + args.aus
    order = [i if i < g["frames"] else 1 + (i - g["frames"]) % (g["frames"] - 1) for i in range(total)]
    size = [(w0 << l, h0 << l) for l in range(L)]
    which = os.path.relpath(_lib.LOADED_PATH or _lib.LIB_PATH, ROOT)

    def new_encoder():
        return SvcEncoder(w0, h0, L, g["qp"], g["me_range"], g["deblock"], g["gop"], g["early_term"])

    def report(mode, path, aus, ms, extra=None):
        ok = all(md5(a) == g["au_md5"][i] for i, a in enumerate(aus[:g["frames"]]))
        line = {"mode": mode, "path": path, "lib": which, "aus_timed": len(ms), "warmup": args.warmup, "golden_md5_ok": ok,
                "golden_aus_checked": min(len(aus), g["frames"]), "stream_md5": md5(b"".join(aus))}
        line.update(_stats(ms))
        line.update(extra or {})
        print(json.dumps(line), flush=True)
        return line

    lines = {}
    if "a" in only:
        enc, aus, ms = new_encoder(), [], []
        for k, i in enumerate(order):
            t0 = time.perf_counter()
            au = b""
            for l in range(L):
                r = enc.encode_layer(l, *_planes(clips[l][i], *size[l]))
                if r.type & 2:
                    au += r.hdr
            au += b"\x00\x00\x01" + r.data
            if k >= args.warmup:
                ms.append(1e3 * (time.perf_counter() - t0))
            aus.append(au)
        enc.close()
        lines["a"] = report("a", "encode_layer x layers, host planes of every layer", aus, ms)
    if "b" in only:
        enc, aus, ms = new_encoder(), [], []
        for k, i in enumerate(order):
            t0 = time.perf_counter()
            au = enc.encode_au(*_planes(clips[L - 1][i], *size[L - 1])).annexb()
            if k >= args.warmup:
                ms.append(1e3 * (time.perf_counter() - t0))
            aus.append(au)
        lines["b"] = report("b", "encode_au, host top frame only", aus, ms)
        if "d" in only:
            fb = size[L - 1][0] * size[L - 1][1] * 3 // 2
            moved = fb + sum(fb >> (2 * j) for j in range(1, L))  # the top frame read, every lower level written
            pyr_ms = enc.bench_pyramid(200)
            av = Encoder(*size[L - 1], g["qp"], g["me_range"], g["deblock"], g["gop"])
            av.encode(*_planes(clips[L - 1][0], *size[L - 1]))
            planes_ms = av.bench_planes(50)
            W, H = size[L - 1]
            pbytes = W * H + 4 * (W + 80) * (H + 80)  # 1 B/px read, 4 B per padded pixel written (kPad = 40, as bench.py)
            av.close()
            print(json.dumps({"mode": "d", "kernel": "k_pyramid", "levels": L - 1, "top": list(size[L - 1]), "bytes_per_launch": moved,
                              "avg_launch_us": round(pyr_ms * 1e3, 2), "gb_per_s": round(moved / (pyr_ms / 1e3) / 1e9, 1),
                              "k_planes": {"picture": [W, H], "bytes_per_launch": pbytes, "avg_launch_us": round(planes_ms * 1e3, 2),
                                           "gb_per_s": round(pbytes / (planes_ms / 1e3) / 1e9, 1)},
                              "note": "200 (k_pyramid) / 50 (k_planes) back-to-back launches, HIP events on the encoder's stream"}), flush=True)
        enc.close()
    if "c" in only:
        dev = [torch.from_numpy(clips[l]).cuda() for l in range(L)]

        def ptrs(l, i):
            n = size[l][0] * size[l][1]
            p = dev[l][i].data_ptr()
            return p, p + n, p + n + n // 4

        for mode, path in (("c_layers", "encode_layers_batch_device, every layer resident"),
                           ("c_top", "encode_aus_batch_device, top layer resident")):
            enc, aus, ms = new_encoder(), [], []
            for lo, hi in ((0, args.warmup), (args.warmup, total)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if mode == "c_layers":
                    rs = enc.encode_layers_batch_device([[ptrs(l, i) for i in order[lo:hi]] for l in range(L)])
                else:
                    rs = enc.encode_aus_batch_device([ptrs(L - 1, i) for i in order[lo:hi]])
                dt = 1e3 * (time.perf_counter() - t0)
                if lo:
                    ms = [dt / (hi - lo)] * (hi - lo)
                aus += [r.annexb() for r in rs]
            st = enc.last_batch_stats()
            enc.close()
            lines[mode] = report(mode, path, aus, ms, {"call_ms": round(sum(ms), 2), "batch_stats": st})
    if len({v["stream_md5"] for v in lines.values()}) > 1:
        raise SystemExit("the modes' streams differ: " + json.dumps({k: v["stream_md5"] for k, v in lines.items()}))
    if any(not v["golden_md5_ok"] for v in lines.values()):
        raise SystemExit("an access unit differs from the reference encoder's MD5")


if __name__ == "__main__":
    main()
