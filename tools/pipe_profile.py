"""Where the workgroups of a pipelined run spend their time (profiling build,
`make profile`).

  python tools/pipe_profile.py [frames] [workgroups,R,window]

Development tool: 1920x1088 QP28 ME16 deblock; I and P warm-up pictures one
call at a time, then `frames` P pictures in one hl_amd_encode_batch.  Prints
the per-workgroup split of k_pipeline's lifetime (task-start waits,
decisions, deblocking + planes, the rest = taking tasks / draining) and the
per-MB phases of the decisions.
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from hartallo_amd import _lib  # noqa: E402

_lib.load_library(os.environ.get("HL_LIB") or os.path.join(ROOT, "build", "prof", "hartallo_amd", "libhartallo_amd.so"))
from hartallo_amd import Encoder, synth  # noqa: E402

PHASES = ["eval:block", "eval:nC", "eval:reduce", "search_partition", "mvp", "guess_intra(P)", "mb_begin", "mb_end", "whole MB",
          "reach_wait", "intra:i16", "intra:i4", "early-term modes", "inter finalize", "", "", "step:candidates", "step:selection", "", "helper join"]
PHASES[14], PHASES[15], PHASES[18] = "reconstruct_chroma", "intra tail (chroma, CBP)", "inter_pred_mb"  # default profiling build
if os.environ.get("HL_BAR_NAMES"):  # a build with -DHL_BAR_PROF: barrier cycles per MB (all waves / most / least waiting wave)
    PHASES[14] = "barriers:all waves"
    PHASES[15] = "barriers:max wave"
    PHASES[18] = "barriers:min wave"
if os.environ.get("HL_I4_NAMES"):  # a build with -DHL_I4_PROF: slots 12..15 time guess_i4's wavefront steps
    PHASES[12:16] = ["i4:neighbours+nC", "i4:modes", "i4:step barrier", "i4:resolution"]
if os.environ.get("HL_STEP_NAMES"):  # a build with -DHL_STEP_PROF: slots 12..15, 18, 19 time the steps' sub-phases
    PHASES[12:16] = ["step:loads", "step:quad work", "step:eval barrier", "step:results+minima"]
    PHASES[18] = "step:chain resolved"
    PHASES[19] = "step:cands generated"


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 24
    geo = tuple(map(int, sys.argv[2].split(","))) if len(sys.argv) > 2 else (0, 2, 64)
    W, H = 1920, 1088
    nmb = (W // 16) * (H // 16)
    clip = synth.clip(W, H, n + 2, 11)
    dev = torch.from_numpy(clip).cuda()
    torch.cuda.synchronize()
    ny, nc = W * H, W * H // 4
    ptrs = [(dev[i].data_ptr(), dev[i].data_ptr() + ny, dev[i].data_ptr() + ny + nc) for i in range(n + 2)]
    enc = Encoder(W, H, 28, 16, 1, 30)
    enc.set_pipeline(*geo)
    if os.environ.get("HL_PROF_HELPERS") == "0":
        enc.set_intra_helpers(False)
    enc.set_timing(True)
    for i in range(2):
        enc.encode_device(*ptrs[i], collect=False)
    enc.profile_counters(64)  # reset
    t = time.perf_counter()
    enc.encode_batch_device(ptrs[2:], collect=False)
    dt = time.perf_counter() - t
    ms = enc.timing_ms()
    nmb_ = nmb
    nsites = int(os.environ.get("HL_BAR_SITES", "0"))  # an HL_BAR_PROF=2 build: 2560 barrier sites after the timeline
    base = 64 + 4 * nmb_ + 2 * nsites  # the pop's eight words follow the timeline (and the barrier sites)
    import ctypes
    raw = (ctypes.c_ulonglong * (base + 8))()
    if enc.lib.hl_amd_profile_counters(enc._h, raw, base + 8) == 0:
        cnt = list(raw)
        pop = cnt[base:base + 8]
    else:  # a library from before the pop's words: it refuses the longer read
        cnt = enc.profile_counters(base) if nsites else enc.profile_counters(64)
        pop = None
    print(f"wg,R,window={geo}: {n} P pictures in {dt * 1e3:.1f} ms (kernel {ms[1]:.1f} ms, reruns {enc.last_reruns()}) helpers {enc.last_helper_stats()}")
    life, wait, mb, filt, tasks = cnt[44], cnt[40], cnt[41], cnt[42], cnt[43]
    if life:
        wgs = geo[0] or (512 if enc.last_pipeline_build() == 2 else 256)  # (HL_AMD_T256=2: two workgroups per CU)
        print(f"   workgroups {wgs}, tasks {tasks} ({tasks / max(1, n * nmb):.2f} per MB), mean lifetime {life / wgs / 1e6:.1f} Mcycles"
              f" (~{life / wgs / (ms[1] * 1e-3) / 1e9:.2f} GHz shader clock if the kernel spans it)")
        hlp, hn = cnt[45], cnt[46]
        print(f"   pops: {cnt[47]} attempts on a macroblock ({cnt[47] / max(1, tasks):.2f} per task), {cnt[48]} lost to another "
              f"workgroup ({100.0 * cnt[48] / max(1, cnt[47]):.1f} %), {cnt[49]} rounds with nothing ready ({cnt[49] / max(1, tasks):.1f} per task)")
        hwait = 0
        if pop:
            # where a pop's time goes (cycles, back-off included): rounds lost to another workgroup, rounds that
            # found nothing ready, rounds that stood back from entries they saw, the round that took a task
            # (macroblock or helper); then the part of all that which ended in a helper task
            lost, nothing, win, stood_c, stood_n, seen, moved, hwait = pop
            inpop = lost + nothing + win + stood_c
            print(f"   stood back: {stood_n} rounds ({stood_n / max(1, tasks):.1f} per task); slots seen taken {seen / max(1, tasks):.2f}, "
                  f"head advances {moved / max(1, tasks):.2f} per task")
            print(f"   inside pop_task: {100.0 * inpop / life:.1f} % of the workgroups' time ({inpop / max(1, tasks) / 1e3:.1f} kcycles/task): lost rounds "
                  f"{100.0 * lost / life:.1f} %, nothing ready {100.0 * nothing / life:.1f} %, stood back {100.0 * stood_c / life:.1f} %, "
                  f"winning round {100.0 * win / life:.1f} %")
            print(f"   of the task-start waits below: {100.0 * wait / life:.1f} % ended in a macroblock (prof[40], all a library without the "
                  f"pop's words reports), {100.0 * hwait / life:.1f} % in a helper task")
        if hn:
            print(f"   helper tasks {hn} ({hn / max(1, n * nmb):.2f} per MB), {hlp / hn / 1e3:.1f} kcycles each")
        if cnt[59]:
            print(f"   of which 8x8-family partitioning helpers {cnt[59]}, {cnt[58] / cnt[59] / 1e3:.1f} kcycles each; "
                  f"partitionings the MB found unclaimed {cnt[60]}, still running {cnt[61]} (waited {cnt[63] / max(1, n * nmb) / 1e3:.1f} "
                  f"kcycles/MB), done {cnt[62]}")
        print(f"   after the filters: barrier {cnt[50] / max(1, tasks) / 1e3:.1f}, release fence {cnt[51] / max(1, tasks) / 1e3:.1f}, "
              f"successors {cnt[52] / max(1, tasks) / 1e3:.1f} kcycles/task; early release block (in the filters) {cnt[53] / max(1, tasks) / 1e3:.1f} "
              f"(fence {cnt[54] / max(1, tasks) / 1e3:.1f}, release {cnt[55] / max(1, tasks) / 1e3:.1f}, spin {cnt[56] / max(1, tasks) / 1e3:.1f}, "
              f"acquire {cnt[57] / max(1, tasks) / 1e3:.1f})")
        # task-start waits: pop, acquire and barrier of every task start, macroblock or helper
        for name, v in (("task-start waits", wait + hwait), ("decisions", mb), ("deblock + planes", filt), ("intra helpers", hlp),
                        ("rest", life - wait - hwait - mb - filt - hlp)):
            print(f"   {name:18s} {100.0 * v / life:6.1f} %   {v / max(1, tasks) / 1e3:9.1f} kcycles/task")
    default_build = not any(os.environ.get(k) for k in ("HL_I4_NAMES", "HL_STEP_NAMES"))
    if default_build and cnt[25]:  # slot 12 of the default profiling build: wave 0's evaluation passes / those whose quads all hit the memo
        print(f"   eval:memo          wave 0 skipped the quad rounds in {cnt[24]} of {cnt[25]} passes ({100.0 * cnt[24] / cnt[25]:.1f} %; "
              f"{cnt[25] / (n * nmb):.1f} passes/MB)")
    for i, name in enumerate(PHASES):
        cyc, calls = cnt[2 * i], cnt[2 * i + 1]
        if calls and name and not (default_build and i == 12):  # (no early termination here: the slot counts the memo's skips, above)
            print(f"   {name:18s} calls/MB {calls / (n * nmb):8.1f}  cycles/call {cyc / calls:10.0f}  kcycles/MB {cyc / (n * nmb) / 1e3:9.1f}")
    if nsites:  # barrier sites by their wait (source line = 2 * site or 2 * site + 1, any header)
        base = 64 + 4 * nmb
        sites = [(cnt[base + 2 * k], cnt[base + 2 * k + 1], k) for k in range(nsites) if cnt[base + 2 * k + 1]]
        tot = sum(w for w, _, _ in sites)
        print(f"   barrier sites: {len(sites)}, wait summed over the waves {tot / (n * nmb) / 1e3:.1f} kcycles/MB")
        for w, c_, k in sorted(sites, reverse=True)[:30]:
            print(f"     line {2 * k:5d}-{2 * k + 1:<5d} calls/MB {c_ / (n * nmb):7.2f}  wait/call (all waves) {w / c_:8.0f}  "
                  f"kcycles/MB {w / (n * nmb) / 1e3:8.1f}  ({100.0 * w / max(1, tot):4.1f} %)")
    enc.close()


if __name__ == "__main__":
    main()
