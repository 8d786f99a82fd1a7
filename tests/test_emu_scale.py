"""The area downscaler on the CPU (hl_amd_set_source_size): the
product's tap derivation (hl_amd_scale_taps, a pure function) against the
model's; the facts the definition was chosen for, pinned on the model and on
the host build; k_scale's per-lane functions behind the ingest's tiles, built
for the host (tests/emu/libhl_scale_emu.so), against sk_testlib's numpy model
over every shape, format, pitch and content; and the rounding division at the
edges of every quotient.  Everything is integer: exact equality.
"""
import ctypes

import numpy as np
import pytest

import in_testlib as it
import sk_testlib as sk

FORMATS = ["i420", "nv12", "rgb24", "rgba32", "rgbp"]
KEYS = [(it.BT601, it.LIMITED), (it.BT709, it.FULL)]
KEY_IDS = ["601l", "709f"]
# every axis of the shapes (luma and chroma), and five more
AXES = sorted({a for s, d, _ in sk.SHAPES for a in ((s[0], d[0]), (s[1], d[1]), (s[0] // 2, d[0] // 2), (s[1] // 2, d[1] // 2))}
              | {(3840, 1280), (1080, 480), (1920, 854), (4096, 512), (4095, 4094)})
TAP_COUNTS = {(3840, 1280): ((3, 1), 3), (1080, 480): ((9, 4), 3), (1920, 854): ((960, 427), 4), (50, 34): ((25, 17), 3)}


# ---- taps ------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", AXES, ids=lambda a: f"{a[0]}to{a[1]}")
def test_taps_are_the_models(axis):
    from hartallo_amd import scale_taps

    s, d = axis
    sr, dr = sk.ratio(s, d)
    most = 0
    for j in range(d):
        first, w = scale_taps(s, d, j)
        assert (first, w) == sk.taps(s, d, j), (s, d, j)
        assert first == (j * sr) // dr and first + len(w) - 1 == ((j + 1) * sr - 1) // dr
        assert sum(w) == sr and min(w) > 0 and len(w) <= 9 and len(w) <= -(-sr // dr) + 1, (s, d, j, w)
        most = max(most, len(w))
    if axis in TAP_COUNTS:
        assert ((sr, dr), most) == TAP_COUNTS[axis]
    if axis == (382, 48):
        assert most == 9  # the maximum


def test_taps_refusals():
    from hartallo_amd import load_library, scale_taps

    lib = load_library()
    first, w = ctypes.c_int32(-7), (ctypes.c_uint32 * 9)(*([77] * 9))

    def raw(s, d, j, cap=9):
        return lib.hl_amd_scale_taps(s, d, j, ctypes.byref(first), w, cap)

    assert raw(48, 48, 0) == 1 and first.value == 0 and w[0] == 1 and w[1] == 77  # the identity: one tap of weight sr = 1
    for s, d, j in ((47, 48, 0), (2, 4, 0), (385, 48, 0), (4098, 2049, 0), (48, 0, 0), (48, -48, 0), (0, 0, 0), (96, 48, -1), (96, 48, 48), (96, 48, 1 << 30)):
        before = (first.value, list(w))
        assert raw(s, d, j) == 0, (s, d, j)
        assert (first.value, list(w)) == before  # a refusal writes nothing
        with pytest.raises(ValueError):
            scale_taps(s, d, j)
    assert raw(384, 48, 0) == 8 and raw(4096, 512, 511) == 8 and raw(4096, 4096, 4095) == 1  # the limits themselves
    # cap too small: 382 -> 48 has outputs of 9 taps, 96 -> 48 of 2
    nine = next(j for j in range(48) if len(sk.taps(382, 48, j)[1]) == 9)
    assert raw(382, 48, nine, 8) == 0 and raw(382, 48, nine, 9) == 9
    assert raw(96, 48, 5, 1) == 0 and raw(96, 48, 5, 0) == 0 and raw(96, 48, 5, -3) == 0 and raw(96, 48, 5, 2) == 2
    assert lib.hl_amd_scale_taps(96, 48, 5, None, w, 9) == 0 and lib.hl_amd_scale_taps(96, 48, 5, ctypes.byref(first), None, 9) == 0


# ---- the pinned facts: on the model, and on the host build of the product's arithmetic -------
def both(p, dw, dh):
    p = np.asarray(p, np.uint8)
    m, e = sk.scale_plane(p, dw, dh), sk.emu_plane(p, dw, dh)
    assert e is not None and np.array_equal(m, e), (p.shape, dw, dh)
    return m


def noise_plane():
    return np.random.default_rng(1).integers(0, 256, (64, 96), dtype=np.uint8)


def test_two_to_one_is_down2():
    p = noise_plane()
    assert np.array_equal(both(p, 48, 32), sk.down2(p))


def test_four_to_one_is_not_down2_twice():
    """the staged rounding of two 2x2 boxes against one rounding of the 4x4 area"""
    p = noise_plane()
    one, twice = both(p, 24, 16), sk.down2(sk.down2(p))
    assert one.size == 384 and np.count_nonzero(one != twice) == 77
    assert np.abs(one.astype(int) - twice.astype(int)).max() == 1
    # and the model is the true area mean, rounded once
    exact = (p.astype(np.int64).reshape(16, 4, 24, 4).sum(axis=(1, 3)) + 8) // 16
    assert np.array_equal(one, exact)


def test_equal_sizes_are_the_identity():
    p = noise_plane()
    assert np.array_equal(both(p, 96, 64), p)
    assert np.array_equal(both(p[:3, :5], 5, 3), p[:3, :5])


@pytest.mark.parametrize("value", [0, 1, 127, 254, 255])
def test_a_constant_plane_stays_constant(value):
    for (sw, sh), (dw, dh) in (((96, 64), (48, 32)), ((50, 34), (34, 18)), ((25, 17), (17, 9)), ((382, 254), (48, 32)), ((191, 127), (24, 16))):
        assert (both(np.full((sh, sw), value, np.uint8), dw, dh) == value).all()


def test_worked_examples():
    assert both([[0, 255, 255]], 2, 1).tolist() == [[85, 255]]
    assert both([[0, 255, 255], [255, 0, 0], [1, 2, 3]], 2, 2).tolist() == [[113, 170], [58, 2]]  # D = 9


def test_the_launch_parameters():
    """what the host hands a launch: the reduced ratios, D, the largest tap counts, a tile's LDS rows"""
    lib = sk.scale_emu_lib()
    out = (ctypes.c_uint32 * 9)()
    for src, disp, coded in sk.SHAPES + [((3840, 2160), (1920, 1080), (1920, 1088)), ((1920, 1080), (854, 480), (864, 480))]:
        assert lib.scale_emu_parm(*src, *disp, *coded, out) == 0
        (srw, drw), (srh, drh) = sk.ratio(src[0], disp[0]), sk.ratio(src[1], disp[1])
        ntw = max(len(sk.taps(src[0], disp[0], j)[1]) for j in range(disp[0]))
        nth = max(len(sk.taps(src[1], disp[1], j)[1]) for j in range(disp[1]))
        assert list(out)[:5] == [srw, drw, srh, drh, srw * srh] and list(out)[6:8] == [ntw, nth], (src, disp, list(out))
        # 16 consecutive output rows never touch more source rows than the tile's LDS holds
        span = max(((min(y0 + 16, disp[1])) * srh - 1) // drh - (y0 * srh) // drh + 1 for y0 in range(0, disp[1], 16))
        assert span <= out[8] <= 129 and out[8] == -(-16 * srh // drh) + 1, (src, disp, span, out[8])
    assert lib.scale_emu_parm(384, 256, 48, 32, 48, 32, out) == 0 and out[8] == 129  # ratio 8: 33,024 bytes of LDS
    for bad in ((49, 34, 34, 18), (50, 34, 33, 18), (32, 18, 34, 18), (274, 34, 34, 18), (50, 146, 34, 18), (4098, 34, 1026, 18)):
        assert lib.scale_emu_parm(*bad, 1040 if bad[2] > 48 else 48, 32, out) == -1, bad


# ---- the host build against the model ------------------------------------------------------
def pads_of(fmt, sw, extra):
    return tuple(extra for _ in it.pack(fmt, sk.content_planes(fmt, 2, 2, 0)))


@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("shape", sk.SHAPES, ids=sk.shape_id)
def test_host_build_is_the_model(shape, fmt, key):
    src, disp, coded = shape
    F = it.FORMATS[fmt]
    small = src[0] * src[1] <= 100 * 100
    for kind in ("noise", 0, 255, "edge", "checker"):
        content = sk.content_planes(F, *src, kind, 11)
        want = sk.model_planes(F, content, key, disp, coded)
        outs = [sk.emu_frame(F, content, key, pads_of(F, src[0], pad), fill, src, disp, coded)
                for pad, fill in (((0, 0xA5), (10, 0xA5), (10, 0x3C)) if small or kind == "noise" else ((10, 0xA5),))]
        for got in outs:
            for name, g, m in zip("YUV", got, want):
                assert g.shape == m.shape and np.array_equal(g, m), f"{fmt} {sk.shape_id(shape)} {kind}: {name}: {np.count_nonzero(g != m)} samples differ"


def test_the_checker_is_the_roundings_worst_case():
    """a one-sample checker at 2:1 puts every accumulator exactly on the half: 510 / 4 = 127.5 -> 128"""
    y = sk.content_planes(it.I420, 96, 64, "checker")[0]
    assert (both(y, 48, 32) == 128).all()


# ---- the division ----------------------------------------------------------------------------
@pytest.mark.parametrize("D", [1, 2, 3, 9, 425, 1048573, 16777213, (1 << 24) - 1, 1 << 24])
def test_division_by_reciprocal_is_exact(D):
    """(1048573 and 16777213: the primes below 2^20 and 2^24)"""
    if D in (1048573, 16777213):
        assert all(D % k for k in range(2, 4097))  # (4097^2 > 2^24)
    lib = sk.scale_emu_lib()
    top = 255 * D + (D >> 1)  # the largest admissible n
    assert top < 1 << 32
    ns = {top, top - 1, 0, 1, D >> 1}
    for q in range(256):
        ns.update(n for n in (q * D - 1, q * D, q * D + 1) if 0 <= n <= top)
    for n in sorted(ns):
        assert lib.scale_emu_div(n, D) == n // D, (n, D)


# ---- Python's frame size check (no device: the check comes before the library call) -------------
def test_python_checks_a_frame_against_the_source_size():
    from hartallo_amd import Encoder, Frame, HlAmdError

    class Sized(Encoder):
        def __init__(self, source):
            self._source = source

        source_size = property(lambda self: self._source)

    f = Frame.from_array(np.zeros((34, 50, 3), np.uint8))
    Sized((50, 34))._check_frame(f)
    with pytest.raises(HlAmdError):
        Sized((34, 18))._check_frame(f)
    Sized((34, 18))._check_frame(Frame(it.RGB24, (1,), (0,)))  # a frame of unknown size is left to the library
