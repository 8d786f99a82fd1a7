"""Spatial-SVC goldens for the access unit's display size
(tests/golden/svc_display_golden.json; hl_amd_set_au_display_size).

The reference knows no display size: it codes the coded sizes.  So each
workload is what a caller of a display size hands over -- hartallo_amd.synth.clip
at the top coded size, cropped to the display size and padded back with
np.pad(mode="edge"); every lower layer the 2x2 box average (synth._down2) of the
layer above -- encoded by oracle/_ref/ref_svc exactly as
tests/golden/make_svc_golden.py drives it.  A stream with a display size differs
from the reference's in its SPS and subset SPSs only, so the whole stream is
kept (<name>.264) and compared NAL unit by NAL unit.  Kept per workload: what
make_svc_golden.py keeps, plus the display size.

intra_in_p must be 0 (reference-layer intra macroblocks in P pictures lie
outside the pinned scope, hl_svc.h); the seeds below were chosen so that it is.

Run in the build container (needs oracle/_ref/ref_svc):
  python tests/golden/make_svc_display_golden.py [name ...]
"""
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from hartallo_amd import synth  # noqa: E402

REF_SVC = os.path.join(ROOT, "oracle", "_ref", "ref_svc")
OUT = os.path.join(HERE, "svc_display_golden.json")
MBR_STRIDE = 864  # oracle/mbrec.h

# name: (W0, H0, layers, display width, display height, frames, qp, me_range, deblock, gop, early_term, seed)
WORKLOADS = {
    "svcd3_64x48": (64, 48, 3, 200, 136, 5, 38, 8, 1, 3, 0, 29),  # top coded 256x192
    "svcd2_32x32": (32, 32, 2, 36, 44, 4, 40, 8, 0, 2, 0, 2),     # top coded 64x64
}
# The seeds: the padding is constant along its direction while the texture
# moves, so in a P picture intra prediction along the padding beats motion
# compensation at moderate QPs, and every seed of 1..30 at QP 26 and 34 leaves
# such macroblocks in a reference layer.  At these QPs the seeds 29, 38, 40, 47
# (svcd3_64x48, of 1..60) and 2, 12, 16, 22 (svcd2_32x32, of 1..30) leave none;
# the first of each is used.


def md5(b) -> str:
    return hashlib.md5(b).hexdigest()


def padded_clips(w0, h0, L, dw, dh, n, seed):
    """[clip of layer 0, ..., clip of the top layer], each (n, w_l * h_l * 3 / 2):
    the top layer is synth.clip cropped to dw x dh and edge-padded to the coded
    size, the others its _down2 pyramid."""
    W, H = w0 << (L - 1), h0 << (L - 1)
    top = synth.clip(W, H, n, seed)
    out = [[] for _ in range(L)]
    for f in range(n):
        ny = W * H
        y = top[f, :ny].reshape(H, W)[:dh, :dw]
        u = top[f, ny:ny + ny // 4].reshape(H // 2, W // 2)[:dh // 2, :dw // 2]
        v = top[f, ny + ny // 4:].reshape(H // 2, W // 2)[:dh // 2, :dw // 2]
        p = [np.pad(y, ((0, H - dh), (0, W - dw)), mode="edge"), np.pad(u, ((0, (H - dh) // 2), (0, (W - dw) // 2)), mode="edge"),
             np.pad(v, ((0, (H - dh) // 2), (0, (W - dw) // 2)), mode="edge")]
        for l in range(L - 1, -1, -1):
            out[l].append(np.concatenate([a.ravel() for a in p]))
            p = [synth._down2(a) for a in p]
    return [np.stack(c) for c in out]


def encode(name, seed=None, keep=True):
    w0, h0, L, dw, dh, n, qp, mer, db, gop, et, seed0 = WORKLOADS[name]
    seed = seed0 if seed is None else seed
    clips = padded_clips(w0, h0, L, dw, dh, n, seed)
    with tempfile.TemporaryDirectory() as td:
        ins = []
        for l in range(L):
            p = os.path.join(td, f"in{l}.yuv")
            clips[l].tofile(p)
            ins.append(p)
        pre = os.path.join(td, "o")
        r = subprocess.run([REF_SVC, str(L), str(w0), str(h0), str(n), str(qp), str(mer), str(db), str(gop), str(et), pre] + ins,
                           check=True, capture_output=True, text=True)
        info = json.loads(r.stdout.strip().splitlines()[-1])
        stream = open(pre + ".264", "rb").read()
        ends = [int(v) for v in open(pre + ".idx").read().split()]
        starts = [0] + ends[:-1]
        recon = []
        for l in range(L):
            fs = (w0 << l) * (h0 << l) * 3 // 2
            rec = np.fromfile(f"{pre}.L{l}.rec.yuv", np.uint8).reshape(-1, fs)
            recon.append([md5(rec[i].tobytes()) for i in range(rec.shape[0])])
        intra_in_p = 0  # intra MBs of reference layers (all but the top) in P pictures
        for l in range(L - 1):
            nmb = ((w0 << l) // 16) * ((h0 << l) // 16)
            recs = np.fromfile(f"{pre}.L{l}.mbs", np.int32).reshape(-1, nmb, MBR_STRIDE)
            for i in range(recs.shape[0]):
                if i % gop:
                    intra_in_p += int((recs[i, :, 0] & 1).sum())
        if keep:
            open(os.path.join(HERE, name + ".264"), "wb").write(stream)
    return {
        "w0": w0, "h0": h0, "layers": L, "display_width": dw, "display_height": dh, "frames": info["frames"], "qp": qp, "me_range": mer,
        "deblock": db, "gop": gop, "early_term": et, "seed": seed, "stream": name + ".264",
        "au_md5": [md5(stream[s:e]) for s, e in zip(starts, ends)],
        "au_bytes": [e - s for s, e in zip(starts, ends)],
        "recon_md5": recon, "intra_in_p": intra_in_p, "stream_md5": md5(stream),
    }


def main():
    names = sys.argv[1:] or list(WORKLOADS)
    data = json.load(open(OUT)) if os.path.exists(OUT) else {}
    for name in names:
        d = encode(name)
        assert d["intra_in_p"] == 0, f"{name}: seed {d['seed']} gives {d['intra_in_p']} intra macroblocks in P pictures of reference layers"
        data[name] = d
        print(name, d["frames"], "AUs", sum(d["au_bytes"]), "bytes, intra_in_p", d["intra_in_p"], flush=True)
    data = {k: data[k] for k in WORKLOADS if k in data}
    json.dump(data, open(OUT, "w"), indent=1)


if __name__ == "__main__":
    main()
