"""Frame rate of the 512-lane and the 256-lane build of the pipelined kernel
by run length, on bench.py's workload (1920x1088, QP 28, ME 16, deblocking,
GOP 30): the table behind the launcher's threshold (DESIGN.md §9.4,
hl_encoder.hip kT256MinPictures).

  python tools/run_length_sweep.py [--reps N] [--lengths 10,20,30,60,120]

One process; per run length the two builds alternate (hl_amd_set_pipeline_build
1 and 2), each timed call after a warm-up call of the same length on a fresh
encoder, the host clock around a call that ends in a device synchronise.  Every
stream is checked against the reference MD5s.  Development tool.
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lengths", default="10,20,30,60,120")
    args = ap.parse_args()
    lengths = [int(v) for v in args.lengths.split(",")]
    sys.path.insert(0, ROOT)
    import torch

    from hartallo_amd import Encoder, synth

    g = json.load(open(os.path.join(ROOT, "tests", "golden", "bench_golden.json")))["bench_1088p_s11"]
    W, H = g["width"], g["height"]
    nmax = 150  # the golden clip: synth.clip's content depends on its length
    clip = synth.clip(W, H, nmax, 11)
    dev = torch.from_numpy(clip).cuda()
    torch.cuda.synchronize()
    ny = W * H
    ptrs = [(dev[i].data_ptr(), dev[i].data_ptr() + ny, dev[i].data_ptr() + ny + ny // 4) for i in range(nmax)]
    ok = True
    for n in lengths:
        warm = min(n, nmax - n)
        fps = {1: [], 2: []}
        for rep in range(args.reps):
            for build in (1, 2):
                enc = Encoder(W, H, 28, 16, 1, 30)
                enc.set_pipeline_build(build)
                outs = [r.annexb() for r in enc.encode_batch_device(ptrs[:warm])]
                torch.cuda.synchronize()
                t = time.perf_counter()
                enc.encode_batch_device(ptrs[warm:warm + n], collect=False)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t
                outs += [r.annexb() for r in enc.last_batch_results()]
                st = enc.last_batch_stats()
                exact = all(hashlib.md5(o).hexdigest() == m for o, m in zip(outs, g["frame_md5"]))
                clean = enc.last_pipeline_build() == build and st["fallbacks"] == 0 and st["waits_gave_up"] == 0
                enc.close()
                ok = ok and exact and clean
                fps[build].append(n / dt)
                print(f"run of {n} (after {warm}) build {build} rep {rep}: {n / dt:.2f} fps ({dt * 1e3:.1f} ms) bitexact {exact} clean {clean}", flush=True)
        m1, m2 = sum(fps[1]) / args.reps, sum(fps[2]) / args.reps
        print(f"== run of {n}: 512-lane {m1:.2f} fps (min {min(fps[1]):.2f} max {max(fps[1]):.2f}), 256-lane {m2:.2f} fps "
              f"(min {min(fps[2]):.2f} max {max(fps[2]):.2f}), {100 * (m2 / m1 - 1):+.1f} %", flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
