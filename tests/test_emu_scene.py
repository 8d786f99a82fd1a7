"""Scene-cut analysis on the CPU: the host build of
hl_scene.h (tests/emu/libhl_scene_emu.so: the staging indices and the
per-macroblock code k_scene's workgroups run) against the numpy model of the
definition (sc_testlib), the rule hl_amd_scene_is_cut through the product
library, and the separation the default threshold rests on."""
import functools

import numpy as np
import pytest

import hartallo_amd
from hartallo_amd import synth
from sc_testlib import ab_stats, emu_costs, frame_sums, is_cut, mb_costs

SIZES = [(16, 16), (48, 32), (176, 144), (1920, 32)]
RANGES = [0, 3, 8, 16]


@functools.lru_cache(maxsize=None)
def synth_luma(w, h, margin):
    """A synth frame with `margin` samples around the w x h picture (so that a shifted crop has real content everywhere)."""
    y = next(synth.frames(w + 2 * margin, h + 2 * margin, 1, 11))[0]
    y.setflags(write=False)
    return y


def crop(y, w, h, margin, dx, dy):
    return np.ascontiguousarray(y[margin + dy:margin + dy + h, margin + dx:margin + dx + w])


def check(cur, prev, R):
    """The emulation equals the model exactly; returns the model's values."""
    inter, intra = mb_costs(cur, prev, R)
    P, I = frame_sums(inter, intra)
    e_inter, e_intra, e_P, e_I = emu_costs(cur, prev, R)
    assert np.array_equal(e_intra, intra)
    assert np.array_equal(e_inter, inter), np.argwhere(e_inter != inter)[:4]
    assert (e_P, e_I) == (P, I)
    return inter, intra, P, I


@pytest.mark.parametrize("R", RANGES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_random_pairs(size, R):
    w, h = size
    rng = np.random.default_rng(w * 131 + h * 7 + R)
    check(rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8), R)


@pytest.mark.parametrize("R", RANGES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_identical_flat_and_extreme_frames(size, R):
    w, h = size
    y = crop(synth_luma(w, h, 17), w, h, 17, 0, 0)
    inter, intra, P, I = check(y, y, R)  # identical frames
    assert P == 0 and not inter.any() and I > 0
    flat = np.full((h, w), 93, np.uint8)
    inter, intra, P, I = check(flat, y, R)  # a flat frame: no intra cost, no cut at any threshold
    assert I == 0 and P == 0
    assert not any(is_cut(P, I, t) for t in (1, 192, 256))
    inter, intra, P, I = check(np.full((h, w), 255, np.uint8), np.zeros((h, w), np.uint8), R)
    assert (inter == 255 * 256).all() and I == 0 and P == 0


@pytest.mark.parametrize("R", RANGES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_exact_shifts(size, R):
    """cur(x, y) = prev(x + R, y - R): macroblocks whose block at (R, -R)
    lies inside the picture find it (inter = 0); one sample further, (R + 1,
    0), is out of the search's reach."""
    w, h = size
    base = synth_luma(w, h, 17)
    prev = crop(base, w, h, 17, 0, 0)
    inter, intra, P, I = check(crop(base, w, h, 17, R, -R), prev, R)
    mbx, mby = np.meshgrid(np.arange(w // 16), np.arange(h // 16))
    reach = (16 * mbx + R + 16 <= w) & (16 * mby - R >= 0)
    assert not inter[reach].any()
    if R:
        assert inter[~reach].all()
    inter, intra, P, I = check(crop(base, w, h, 17, R + 1, 0), prev, R)
    assert inter.all()


def test_is_cut_rule():
    cut = hartallo_amd.load_library().hl_amd_scene_is_cut
    assert cut(192, 256, 192) == 1 and cut(191, 256, 192) == 0  # 256 P == thr I counts as a cut
    assert cut(3, 4, 192) == 1 and cut(3, 4, 193) == 0
    assert cut(0, 0, 1) == 0 and cut(5, 0, 1) == 0  # I = 0 is never a cut
    assert cut(0, 7, 1) == 0 and cut(1, 256, 1) == 1
    assert cut(1000, 1000, 256) == 1 and cut(999, 1000, 256) == 0
    for bad in (0, -1, 257, 1 << 20):
        assert cut(1, 1, bad) == -1
    big = 1 << 40
    assert cut(big, big, 256) == 1 and cut(big - 1, big, 256) == 0
    assert cut(3 * big, 4 * big, 192) == 1 and cut(3 * big - 1, 4 * big, 192) == 0
    assert cut((1 << 62) - 1, 1 << 62, 256) == 0 and cut(1 << 62, 1 << 62, 256) == 1
    for P, I, t in ((192, 256, 192), (191, 256, 192), (0, 0, 1), (big, big, 256), (3 * big - 1, 4 * big, 192)):
        assert cut(P, I, t) == int(is_cut(P, I, t))  # the model's rule is the library's


@pytest.mark.parametrize("size", [(176, 144), (64, 48)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_default_threshold_separates_motion_from_cuts(size):
    """A[0:4] + B[0:3] + [A[6]] (synth seeds 5 and 9), R = 8: the cuts at
    frames 4 and 7 have 256 P / I >= 224, every other frame <= 160."""
    w, h = size
    stats = ab_stats(w, h, "aba", 8)
    assert stats[0] is None
    for k in range(1, 8):
        P, I = stats[k][:2]
        ratio = 256 * P / I
        print(f"{w}x{h} frame {k}: 256 P / I = {ratio:.1f}")
        if k in (4, 7):
            assert 256 * P >= 224 * I, (k, ratio)
        else:
            assert 256 * P <= 160 * I, (k, ratio)
