"""The rendition ladder on the CPU (hl_amd_encode_ladder_frame(s), DESIGN.md
6.15): k_scale_fan's block selection and the per-lane functions it shares with
k_scale, looped over a launch behind one ingest per frame and built for the
host (tests/emu/libhl_ladder_emu.so), against sk_testlib's numpy model for
every rung of every ladder, format, colour setting, pitch and content, and
against the single-rung host build (tests/emu/libhl_scale_emu.so); the
launch's geometry; and the decoding of grid z into frame and rung.  Everything
is integer: exact equality.
"""
import ctypes

import numpy as np
import pytest

import in_testlib as it
import ld_testlib as ld
import sk_testlib as sk

FORMATS = ["i420", "nv12", "rgb24", "rgba32", "rgbp"]
KEYS = [(it.BT601, it.LIMITED), (it.BT709, it.FULL)]
KEY_IDS = ["601l", "709f"]
KINDS = ("noise", 0, 255, "edge", "checker")


def pads_of(fmt, extra):
    return tuple(extra for _ in it.pack(fmt, sk.content_planes(fmt, 2, 2, 0)))


def test_the_model_on_the_ladders():
    """the facts the ladders were chosen for, on the model alone"""
    for name, (src, rungs) in ld.LADDERS.items():
        assert 1 <= len(rungs) <= 8
        for disp, coded in rungs:
            assert all(v % 2 == 0 for v in (*src, *disp)) and all(v % 16 == 0 for v in coded)
            assert all(d <= s <= 8 * d and d <= c for s, d, c in zip(src, disp, coded)), (name, disp)
    src, rungs = ld.LADDERS["L1"]
    yuv = sk.content_planes(it.I420, *src, "noise", 5)
    ident, half, odd = (sk.model_planes(it.I420, yuv, KEYS[0], d, c) for d, c in rungs)
    for p, q in zip(ident, yuv):
        assert np.array_equal(p, q)  # s = d: the identity
    for p, q in zip(half, yuv):
        assert np.array_equal(p, sk.down2(q))  # 2:1 is the 2x2 box
    assert (odd[0][:, 34:] == odd[0][:, 33:34]).all() and (odd[0][18:] == odd[0][17:18]).all()  # edges on both sides
    assert max(len(sk.taps(382, 48, j)[1]) for j in range(48)) == 9 and max(len(sk.taps(382, 192, j)[1]) for j in range(192)) == 3  # L3


@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", sorted(ld.LADDERS))
def test_host_build_is_the_model_and_the_single_rung_build(name, fmt, key):
    src, rungs = ld.LADDERS[name]
    F = it.FORMATS[fmt]
    other = sk.content_planes(F, *src, "noise", 12)  # the call's second frame: z = frame * count + r with frame > 0
    for kind in KINDS:
        contents = [sk.content_planes(F, *src, kind, 11), other]
        want = [[sk.model_planes(F, c, key, disp, coded) for c in contents] for disp, coded in rungs]
        for pad, fill in ((0, 0xA5), (10, 0xA5), (10, 0x3C)):
            got = ld.emu_ladder(F, contents, key, pads_of(F, pad), fill, src, rungs)
            for r, (disp, coded) in enumerate(rungs):
                for i, content in enumerate(contents):
                    for pname, g, m in zip("YUV", got[r][i], want[r][i]):
                        assert g.shape == m.shape and np.array_equal(g, m), f"{name} {fmt} {kind} rung {r} frame {i}: {pname}: {np.count_nonzero(g != m)} samples differ"
        # every rung is what k_scale's host build makes of the same frame, alone
        for r, (disp, coded) in enumerate(rungs):
            for i, content in enumerate(contents):
                alone = sk.emu_frame(F, content, key, pads_of(F, 10), 0x3C, src, disp, coded)
                for g, a in zip(got[r][i], alone):
                    assert np.array_equal(g, a), (name, fmt, kind, r, i)


@pytest.mark.parametrize("name", sorted(ld.LADDERS))
def test_the_launch_geometry(name):
    src, rungs = ld.LADDERS[name]
    lib = ld.ladder_emu_lib()
    out = (ctypes.c_int32 * 10)()
    assert lib.ladder_emu_geometry(*src, len(rungs), ld.sizes_array(rungs), out) == 0
    tiles = [-(-w // 64) * -(-h // 16) for _, (w, h) in rungs]
    parm = (ctypes.c_uint32 * 9)()
    lrows = []
    for disp, coded in rungs:
        assert sk.scale_emu_lib().scale_emu_parm(*src, *disp, *coded, parm) == 0
        lrows.append(parm[8])
        assert parm[8] == -(-16 * sk.ratio(src[1], disp[1])[0] // sk.ratio(src[1], disp[1])[1]) + 1
    assert list(out)[2:2 + len(rungs)] == tiles
    assert out[0] == max(tiles) and out[1] == max(lrows) * 64 * 4 and out[1] <= 33024
    # grid z = frame * count + rung; a workgroup beyond its rung's, or its plane's, tiles leaves
    o3 = (ctypes.c_int32 * 3)()
    count = len(rungs)
    for z in range(3 * count):
        for c in range(3):
            w, h = rungs[z % count][1]
            have = -(-(w >> (c > 0)) // 64) * -(-(h >> (c > 0)) // 16)
            for x in range(out[0]):
                assert lib.ladder_emu_block(*src, count, ld.sizes_array(rungs), x, c, z, o3) == 0
                assert list(o3) == [z // count, z % count, int(x < have)], (name, x, c, z)


def test_the_geometry_of_the_ladders_it_was_built_for():
    lib = ld.ladder_emu_lib()
    out = (ctypes.c_int32 * 10)()
    rungs = [((1920, 1080), (1920, 1088)), ((1280, 720), (1280, 720)), ((854, 480), (864, 480))]
    assert lib.ladder_emu_geometry(3840, 2160, 3, ld.sizes_array(rungs), out) == 0
    assert list(out)[:5] == [30 * 68, (72 + 1) * 256, 30 * 68, 20 * 45, 14 * 30]  # 854 -> 480 rows at 4.5: 16 * 9 / 2 + 1 rows of LDS
    # refusals: no rung, nine rungs, an upscaling rung, a ratio above 8
    one = [((48, 32), (48, 32))]
    assert lib.ladder_emu_geometry(96, 64, 0, ld.sizes_array(one), out) == -1
    assert lib.ladder_emu_geometry(96, 64, 9, ld.sizes_array(one * 9), out) == -1
    assert lib.ladder_emu_geometry(96, 64, 8, ld.sizes_array(one * 8), out) == 0
    assert lib.ladder_emu_geometry(32, 32, 1, ld.sizes_array(one), out) == -1
    assert lib.ladder_emu_geometry(400, 64, 1, ld.sizes_array(one), out) == -1
