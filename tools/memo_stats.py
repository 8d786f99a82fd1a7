"""Development tool (CPU, emulator): the counters of the candidate
evaluation's memo (hl_mbcore.h kMemoSlots) on golden configurations or the
first pictures of the bench stream -- how many (prediction, block) items an
MB had already evaluated, how many passes and 128-item rounds have nothing
new, keys per MB, and what a smaller table loses.

  python tools/memo_stats.py [name ...] [slots=N[,N...]] [probe=P]

  name   a golden configuration (tests/hl_testlib.py) or `bench`
         (1920x1088 seed 11; FRAMES=4 pictures by default)
  slots  table sizes to run (default: the built capacity; 0 = off)
  probe  probe length of the emulator's path (default 4, the device's)
"""
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

from hl_testlib import GOLDEN_CONFIGS, GOLDEN_ET_CONFIGS, EmuEncoder, emu_lib, golden_input  # noqa: E402

STAT = ("items", "hits", "bypassed", "not_inserted", "inserted", "mb_keys_max", "mbs", "passes", "passes_all_hit", "rounds",
        "rounds_miss", "wave_rounds", "wave_rounds_miss")


def stats(reset=True):
    a = (ctypes.c_longlong * len(STAT))()
    emu_lib().emu_memo_stats(a, len(STAT), 1 if reset else 0)
    return dict(zip(STAT, list(a)))


def main():
    names = [a for a in sys.argv[1:] if "=" not in a] or ["w480_h272_qp28_me16"]
    opts = dict(a.split("=", 1) for a in sys.argv[1:] if "=" in a)
    cap = emu_lib().emu_memo_capacity()
    sizes = [int(v) for v in opts["slots"].split(",")] if "slots" in opts else [cap]
    probe = int(opts.get("probe", 4))
    cfgs = list(GOLDEN_CONFIGS + GOLDEN_ET_CONFIGS)
    if "bench" in names:
        cfgs.append(("bench", 1920, 1088, int(os.environ.get("FRAMES", "4")), 28, 16, 1, 30, 11))
    for cfg in cfgs:
        if cfg[0] not in names:
            continue
        name, w, h, n, qp, mer, db, gop, seed = cfg
        if name == "bench":
            from hartallo_amd import synth

            clip = synth.clip(w, h, 150, seed)[:n]
        else:
            clip = golden_input(cfg)
        for slots in sizes:
            enc = EmuEncoder(w, h, qp, mer, db, gop, 1 if name.startswith("et_") else 0)
            if enc.lib.emu_set_memo(slots, probe):  # (process-wide)
                print(f"{name}: {slots} slots / probe {probe} refused (built capacity {cap})")
                continue
            stats()
            for f in range(n):
                enc.encode(clip[f])
            s = stats()
            it, mbs = max(1, s["items"]), max(1, s["mbs"])
            print(f"{name} ({n} pictures, {s['mbs']} MBs with a search) slots {slots} probe {probe}: items {s['items']}, "
                  f"hits {s['hits']} ({100.0 * s['hits'] / it:.1f} %), bypassed {s['bypassed']}, "
                  f"not inserted {s['not_inserted']} ({100.0 * s['not_inserted'] / it:.2f} %), "
                  f"keys/MB {(s['inserted'] + s['not_inserted']) / mbs:.0f} (max {s['mb_keys_max']}), "
                  f"passes {s['passes']} with no new item {s['passes_all_hit']} ({100.0 * s['passes_all_hit'] / max(1, s['passes']):.1f} %), "
                  f"128-item rounds {s['rounds']} -> with a new item {s['rounds_miss']}, "
                  f"wave shares of rounds {s['wave_rounds']} -> with a new item {s['wave_rounds_miss']}", flush=True)


if __name__ == "__main__":
    main()
