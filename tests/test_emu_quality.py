"""The quality metric on the CPU: the host build of
hl_quality.h (tests/emu/libhl_quality_emu.so: the staging indices and the
per-strip and per-window code k_quality's workgroups run) against the numpy
model of the definition (q_testlib), and the pure functions hl_amd_psnr_db /
hl_amd_ssim_mean through the product library."""
import math

import numpy as np
import pytest

import hartallo_amd
from hartallo_amd import synth
from q_testlib import emu_plane, mb_sse, plane_quality, quality_emu_lib, window_terms

# 16x16: 9 windows; 8x8: one (the chroma of a 16x16 picture); 1920x32: many
# tiles wide, two block rows of windows short of a tile; the kernel's tile is
# 256 x 32 samples: 264x40 is wider and 40x72 taller than it by a non-multiple
# (one strip, one window row into the next tile), 520x72 both.
SIZES = [(16, 16), (8, 8), (48, 32), (176, 144), (1920, 32), (264, 40), (40, 72), (520, 72)]
ids = lambda s: f"{s[0]}x{s[1]}"  # noqa: E731


def check(a, b):
    """The emulation equals the model exactly; returns the model's values."""
    h, w = a.shape
    want = plane_quality(a, b)
    d = a.astype(np.int64) - b.astype(np.int64)
    assert want["sse"] == int((d * d).sum())  # the block sums' identity
    if w % 16 == 0 and h % 16 == 0:
        sse, q, mb = emu_plane(a, b, True)
        assert np.array_equal(mb, mb_sse(a, b)), np.argwhere(mb != mb_sse(a, b))[:4]
        assert int(mb.astype(np.uint64).sum()) == sse
    else:
        sse, q = emu_plane(a, b)
    assert sse == want["sse"]
    assert q == want["ssim_q30"], (q, want["ssim_q30"])
    return want


@pytest.mark.parametrize("size", SIZES, ids=ids)
def test_random_pairs(size):
    w, h = size
    rng = np.random.default_rng(w * 131 + h * 7)
    a, b = rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)
    want = check(a, b)
    if size == (16, 16):
        assert want["ssim_q30"] < 0  # uncorrelated noise: the floor of negative quotients matters already here
    near = np.clip(a.astype(np.int16) + rng.integers(-2, 3, (h, w)), 0, 255).astype(np.uint8)  # what a coded picture looks like
    want = check(a, near)
    assert 0 < want["ssim_q30"] < want["windows"] << 30


@pytest.mark.parametrize("size", SIZES, ids=ids)
def test_identical_and_extreme_pairs(size):
    w, h = size
    rng = np.random.default_rng(w + 3 * h)
    a = rng.integers(0, 256, (h, w), dtype=np.uint8)
    for p in (a, np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8)):
        want = check(p, p)
        assert want["sse"] == 0 and want["ssim_q30"] == want["windows"] << 30
    white, black = np.full((h, w), 255, np.uint8), np.zeros((h, w), np.uint8)
    for p, q in ((white, black), (black, white)):
        want = check(p, q)
        # no variance, no covariance: Q = floor(2^30 C1 / (16320^2 + C1)) = 1677 in every window
        assert want["sse"] == 255 * 255 * w * h and want["ssim_q30"] == 1677 * want["windows"]
    yy, xx = np.mgrid[0:h, 0:w]
    board = (((xx + yy) & 1) * 255).astype(np.uint8)
    want = check(board, 255 - board)  # the largest |num|
    assert want["ssim_q30"] < 0 and want["sse"] == 255 * 255 * w * h
    num, den = window_terms(board, 255 - board)
    assert int(np.abs(num).max()) < 1 << 55 and int(den.max()) < 1 << 55 and (np.abs(num) <= den).all()


@pytest.mark.parametrize("size", [(176, 144), (48, 32)], ids=ids)
def test_synth_frame_pair(size):
    w, h = size
    (y0, u0, v0), (y1, u1, v1) = list(synth.frames(w, h, 2, 7))
    for a, b in ((y0, y1), (u0, u1), (v0, v1)):
        want = check(a, b)
        assert want["sse"] > 0 and want["ssim_q30"] < want["windows"] << 30


def test_division():
    """q_div30 = floor(num 2^30 / den) on both signs, exact quotients and remainders."""
    div = quality_emu_lib().quality_emu_div30
    rng = np.random.default_rng(5)
    cases = [(0, 1), (1, 1), (-1, 1), (7, 7), (-7, 7), (1, 3), (-1, 3), (-1, (1 << 55) - 1), ((1 << 55) - 2, (1 << 55) - 1),
             (-((1 << 55) - 2), (1 << 55) - 1), (3, 1 << 31), (-3, 1 << 31)]
    for _ in range(2000):
        den = int(rng.integers(1, 1 << 55))
        cases.append((int(rng.integers(-den, den + 1)), den))
    for num, den in cases:
        assert div(num, den) == (num << 30) // den, (num, den)


def test_pure_functions():
    lib = hartallo_amd.load_library()
    assert lib.hl_amd_psnr_db(0, 25344) == math.inf and hartallo_amd.psnr_db(0, 1) == math.inf
    for sse, n in ((25344, 25344), (1, 64), (123456789, 1920 * 1088), (255 * 255 * 64, 64)):
        assert abs(hartallo_amd.psnr_db(sse, n) - 10 * math.log10(255 * 255 * n / sse)) < 1e-12
    assert hartallo_amd.psnr_db(255 * 255 * 64, 64) == 0.0
    assert math.isnan(hartallo_amd.psnr_db(5, 0)) and math.isnan(hartallo_amd.psnr_db(0, 0))
    for windows in (1, 9, 1505, 479 * 271):
        assert hartallo_amd.ssim_mean(windows << 30, windows) == 1.0
        assert hartallo_amd.ssim_mean(-(windows << 30), windows) == -1.0
        assert hartallo_amd.ssim_mean(0, windows) == 0.0
    assert hartallo_amd.ssim_mean(3 << 28, 1) == 0.75 and hartallo_amd.ssim_mean(-(1 << 29), 2) == -0.25
    assert math.isnan(hartallo_amd.ssim_mean(1, 0)) and math.isnan(hartallo_amd.ssim_mean((1 << 30) + 1, 1))
