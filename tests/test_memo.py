"""The memo of the per-block candidate evaluation (hl_mbcore.h kMemoSlots,
eval_candidates) on the host path: the emulator with the memo at its default
capacity, off, and forced to 8 slots with a probe length of 1 must give the
reference's golden streams byte for byte, and the key must determine what the
block's quad reads.  Tolerance: none."""
import ctypes
import json
import os

import numpy as np
import pytest

from hl_testlib import GOLDEN, GOLDEN_CONFIGS, GOLDEN_ET_CONFIGS, EmuEncoder, emu_lib, first_diff, golden_input, md5

GOLD = json.load(open(os.path.join(GOLDEN, "golden.json")))
NAMES = ["tiny_32x16_qp26", "et_w64_h32_qp36", "qcif_qp12_me2", "qcif_qp40_me16_gop4", "w480_h272_qp28_me16"]
CFGS = [next(c for c in GOLDEN_CONFIGS + GOLDEN_ET_CONFIGS if c[0] == n) for n in NAMES]
STAT = ("items", "hits", "bypassed", "not_inserted", "inserted", "mb_keys_max", "mbs", "passes", "passes_all_hit", "rounds",
        "rounds_miss", "wave_rounds", "wave_rounds_miss")


def memo_stats(reset=True):
    a = (ctypes.c_longlong * len(STAT))()
    n = emu_lib().emu_memo_stats(a, len(STAT), 1 if reset else 0)
    assert n == len(STAT)
    return dict(zip(STAT, list(a)))


def _encode(cfg, slots, probe):
    name, w, h, n, qp, mer, db, gop, seed = cfg
    clip = golden_input(cfg)
    enc = EmuEncoder(w, h, qp, mer, db, gop, GOLD[name].get("early_term", 0))
    assert enc.lib.emu_set_memo(slots, probe) == 0  # (a setting of the whole process)
    try:
        memo_stats()
        out = b""
        for f in range(n):
            out += enc.encode(clip[f])
            assert md5(enc.recon()) == GOLD[name]["recon_md5"][f], f"{name}: recon of frame {f}"
        return out, memo_stats()
    finally:
        assert enc.lib.emu_set_memo(-1, 4) == 0  # the default again, for whatever runs next


@pytest.mark.parametrize("cfg", CFGS, ids=NAMES)
def test_memo_settings_match_reference(cfg):
    ref = open(os.path.join(GOLDEN, cfg[0] + ".264"), "rb").read()
    for what, slots, probe in (("default", -1, 4), ("off", 0, 4), ("8 slots, probe 1", 8, 1)):
        out, st = _encode(cfg, slots, probe)
        print(cfg[0], what, st)
        assert out == ref, f"{cfg[0]} memo {what}: first differing byte {first_diff(out, ref)}"
        assert st["items"] > 0
        # vacuity guards
        if slots < 0:
            assert st["hits"] > 0, st
        elif slots == 0:
            assert st["hits"] == 0 and st["inserted"] == 0 and st["not_inserted"] == 0, st
        else:
            assert st["not_inserted"] > 0, st


def test_memo_setting_refused():
    lib = emu_lib()
    cap = lib.emu_memo_capacity()
    for slots, probe in ((3, 4), (2 * cap, 4), (8, 0), (8, 5)):
        assert lib.emu_set_memo(slots, probe) == 1
    assert lib.emu_set_memo(-1, 4) == 0


# (num_part, num_sub, sub_w, sub_h, part_w, part_h) of kParts (hl_mbcore.h)
PARTS = [(1, 1, 16, 16, 16, 16), (2, 1, 16, 8, 16, 8), (2, 1, 8, 16, 8, 16), (4, 1, 8, 8, 8, 8), (4, 2, 8, 4, 8, 8), (4, 2, 4, 8, 8, 8),
         (4, 4, 4, 4, 8, 8)]


def _blocks(j):
    """(pi, spi, k, bx, by, px, py) of every 4x4 block of every partition of kParts[j]."""
    num_part, num_sub, sw, sh, pw, ph = PARTS[j]
    for pi in range(num_part):
        px, py = (pi % (16 // pw)) * pw, (pi // (16 // pw)) * ph
        for spi in range(num_sub):
            sx = sy = 0
            if num_part == 4:
                sx, sy = (spi % (8 // sw)) * sw, (spi // (8 // sw)) * sh
            for k in range((sw // 4) * (sh // 4)):
                hx, hy = k % (sw // 4), k // (sw // 4)
                yield pi, spi, k, px + sx + 4 * hx, py + sy + 4 * hy, px + sx, py + sy


def _key_cases(W, H, mvs, mbxs=None, js=range(7)):
    lib = emu_lib()
    lib.emu_memo_key.argtypes = [ctypes.c_int] * 10 + [ctypes.POINTER(ctypes.c_longlong)]
    out = (ctypes.c_longlong * 4)()
    for mby in range(H // 16):
        for mbx in mbxs or range(W // 16):
            for j in js:
                for pi, spi, k, bx, by, px, py in _blocks(j):
                    for mvx, mvy in mvs:
                        assert lib.emu_memo_key(W, H, mbx, mby, j, pi, spi, mvx, mvy, k, out) == 0
                        # the partition's clamped integer displacement (put_cand), worked out here
                        dx = min(max(mbx * 16 + px + (mvx >> 2), -17), W + 17) - (mbx * 16 + px)
                        dy = min(max(mby * 16 + py + (mvy >> 2), -17), H + 17) - (mby * 16 + py)
                        yield (mbx, mby, j, bx, by, mvx, mvy, dx, dy), tuple(out)


def test_key_determines_what_the_quad_reads():
    """64x48, every kParts geometry and block, MVs of all 16 phases whose
    integer parts run past both clamps on all four edges: candidates with
    equal keys read the same two prediction rows and the same source row."""
    W, H = 64, 48
    ints_x = [-90, -66, -33, -18, -17, -9, -2, 0, 1, 7, 16, 17, 31, 50, 65, 90]  # MB x up to 48, clamp at -17 / W + 17
    ints_y = [-80, -49, -33, -18, -17, -5, 0, 3, 16, 17, 30, 49, 66, 80]
    rng = np.random.RandomState(5)
    mvs = [(0, 0)]
    for ix in ints_x:  # every x against a few y, every phase somewhere: a few hundred MVs
        for iy in rng.choice(ints_y, 3, replace=False):
            ph = int(rng.randint(16))
            mvs.append((ix * 4 + (ph & 3), int(iy) * 4 + (ph >> 2)))
    for ph in range(16):
        mvs.append((4 * 3 + (ph & 3), -4 * 2 + (ph >> 2)))
        mvs.append((-4 * 70 + (ph & 3), 4 * 70 + (ph >> 2)))
    seen, phases, clamped = {}, set(), set()
    n = 0
    for (mbx, mby, j, bx, by, mvx, mvy, dx, dy), (key, r1, r2, src) in _key_cases(W, H, mvs):
        n += 1
        assert key != 0, "no displacement of a 64x48 picture leaves the key's fields"
        phases.add((mvx & 3, mvy & 3))
        if dx != (mvx >> 2):
            clamped.add("L" if dx > (mvx >> 2) else "R")
        if dy != (mvy >> 2):
            clamped.add("T" if dy > (mvy >> 2) else "B")
        # the key's fields, as documented at kMemoSlots
        assert key == ((dx & 0x7FF) | ((dy & 0x7FF) << 11) | ((((mvy & 3) << 2) | (mvx & 3)) << 22) | (1 << 26)
                       | ((((by >> 2) << 2) | (bx >> 2)) << 27))
        # keys are per MB (the table is empty at every MB start)
        reads = (r1, r2, src)
        assert seen.setdefault((mbx, mby, key), reads) == reads, (mbx, mby, j, bx, by, mvx, mvy)
    assert len(phases) == 16 and clamped == {"L", "R", "T", "B"}, (phases, clamped)
    assert len(seen) < n  # equal keys did occur (the same block reached through several geometries)


def test_bypass_is_exactly_what_does_not_fit():
    """A picture wide and tall enough for displacements outside the key's 11-bit
    fields: those candidates bypass, and no other does."""
    W, H = 2304, 16
    mvs = [(4 * i + 1, 2) for i in (-1100, -1025, -1024, -1000, 0, 1000, 1023, 1024, 1100, 2200)]
    byp = fit = 0
    for (mbx, mby, j, bx, by, mvx, mvy, dx, dy), (key, r1, r2, src) in _key_cases(W, H, mvs, (0, 70, 143), (0, 6)):
        fits = -1024 <= dx <= 1023 and -1024 <= dy <= 1023
        assert (key != 0) == fits, (mbx, j, bx, by, mvx, dx, dy, key)
        byp += not fits
        fit += fits
    assert byp > 0 and fit > 0
