"""The display size on the CPU (hl_amd_set_display_size): the
stream headers with cropping fields (hl_amd_stream_headers, a pure function)
through an exp-Golomb parser of the test's own; the frame ingest's full and
edge tiles (in_tile, in_tile_edge) built for the host
(tests/emu/libhl_display_emu.so) against np.pad(mode="edge") of in_testlib's
planes; the same code under AddressSanitizer + UndefinedBehaviorSanitizer over
exactly-sized heap planes (tests/sanitize/ingest_edge_asan, a stand-alone
program); the quality metric over a window against a crop-then-sum model; and
the Python frame size check.  Everything is integer: exact equality.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dp_testlib as dp
import in_testlib as it
import q_testlib as qt
from hl_testlib import ROOT

ASAN_BIN = os.path.join(ROOT, "tests", "sanitize", "ingest_edge_asan")
FORMATS = ["i420", "nv12", "rgb24", "rgba32", "rgbp"]
KEYS = [(it.BT601, it.LIMITED), (it.BT709, it.FULL)]
KEY_IDS = ["601l", "709f"]
# coded size, display size: every even width over one macroblock column at three
# heights; odd chroma (17 x 9); QCIF; the edge column in the second 64-lane
# workgroup column of k_ingest's grid (tile 64 of a row pair)
SHAPES = [(32, 32, dw, dh) for dw in range(18, 33, 2) for dh in (18, 30, 32)] + [(48, 32, 34, 18), (176, 144, 162, 130), (1040, 32, 1026, 18)]

TABLE = [  # the issue's worked examples: coded size, display size, the SPS
    ((176, 144), (176, 144), "27 42 e0 0b 95 a0 b1 31"),
    ((176, 144), (170, 134), "27 42 e0 0b 95 a0 b1 36 49 90"),
    ((1920, 1088), (1920, 1080), "27 42 e0 32 95 a0 1e 00 89 79 50"),
    ((48, 32), (34, 18), "27 42 e0 0a 95 a3 56 22 21"),
]


# ---- headers -----------------------------------------------------------------------
def headers(w, h, dw=None, dh=None, max_ref=1, qp=28):
    from hartallo_amd import stream_headers

    sps, pps = dp.nals(stream_headers(w, h, qp, max_ref, dw, dh))
    return sps, pps


@pytest.mark.parametrize("coded,display,want", TABLE, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_worked_examples(coded, display, want):
    sps, _ = headers(*coded, *display)
    assert sps.hex(" ") == want


def check_headers(w, h, right, bottom, max_ref, plain):
    dw, dh = w - 2 * right, h - 2 * bottom
    sps, pps = headers(w, h, dw, dh, max_ref)
    psps, ppps = plain
    assert pps == ppps, (w, h, dw, dh, max_ref)
    assert dp.needs_no_escape(sps) and dp.needs_no_escape(pps), (w, h, dw, dh, max_ref, sps.hex())
    got, base = dp.parse_sps(sps), dp.parse_sps(psps)
    if right == 0 and bottom == 0:
        assert sps == psps and got["cropping"] == 0
        return
    assert got["cropping"] == 1 and got["crop"] == (0, right, 0, bottom), (w, h, dw, dh, got)
    for k in base:  # level_idc and max_num_ref_frames among them: computed from the coded size
        if k not in ("cropping", "crop"):
            assert got[k] == base[k], (k, w, h, dw, dh, max_ref)
    assert (got["width_mbs_minus1"], got["height_mbs_minus1"]) == (w // 16 - 1, h // 16 - 1)


def test_every_size_one_crop_each():
    """coded sizes 16..2048 in both dimensions, step 16: each with one crop pair and max_ref_frame out of the sweep below"""
    for w in range(16, 2049, 16):
        for h in range(16, 2049, 16):
            k = (w // 16) * 131 + (h // 16) * 17
            max_ref = (1, 4, 16)[k % 3]
            check_headers(w, h, k % 8, (k // 8) % 8, max_ref, headers(w, h, max_ref=max_ref))


@pytest.mark.parametrize("max_ref", [1, 4, 16])
def test_every_crop_at_chosen_sizes(max_ref):
    """all 64 crop pairs (0..7 units right and bottom) at the small sizes, the level boundaries and the largest"""
    sizes = [16, 32, 48, 64, 128, 176, 352, 720, 1280, 1920, 2048]
    for w in sizes:
        for h in sizes:
            plain = headers(w, h, max_ref=max_ref)
            for right in range(8):
                for bottom in range(8):
                    check_headers(w, h, right, bottom, max_ref, plain)


def test_escaping_is_there_for_sizes_nobody_enumerated():
    """a coded width of 2^20 macroblocks puts two aligned zero bytes and six more
    zero bits into the SPS: the escape goes in, the parser takes it out again
    and reads the same fields"""
    w, h = 16 << 20, 64
    sps, pps = headers(w, h, w - 6, h - 10)
    assert b"\x00\x00\x03" in sps and dp.needs_no_escape(sps)
    got = dp.parse_sps(sps)
    assert got["width_mbs_minus1"] == (1 << 20) - 1 and got["crop"] == (0, 3, 0, 5)


def test_refused_settings():
    from hartallo_amd import stream_headers

    ok = stream_headers(176, 144, 28, 1, 170, 134)
    assert ok == stream_headers(176, 144, 28, 1, 170, 134) and len(dp.nals(ok)) == 2
    for dw, dh in ((169, 134), (170, 133), (160, 144), (176, 128), (178, 144), (176, 146), (0, 0), (-2, 144)):
        with pytest.raises(ValueError):
            stream_headers(176, 144, 28, 1, dw, dh)
    for w, h in ((1920, 1080), (0, 16), (170, 144)):  # the coded size stays a multiple of 16
        with pytest.raises(ValueError):
            stream_headers(w, h, 28, 1, w, h)
    with pytest.raises(ValueError):
        stream_headers(176, 144, 52)
    with pytest.raises(ValueError):
        stream_headers(16, 16, 28, 17)  # max_num_ref_frames above 16
    with pytest.raises(ValueError):
        stream_headers(176, 144, 28, -1)
    # the bytes must fit
    from hartallo_amd import _lib as L

    lib = L.load_library()
    p = L._Params(176, 144, 28, 16, 1, 30, 0, 0)
    buf = ctypes.create_string_buffer(64)
    assert lib.hl_amd_stream_headers(ctypes.byref(p), 1, 170, 134, buf, len(ok)) == len(ok) and buf.raw[:len(ok)] == ok
    assert lib.hl_amd_stream_headers(ctypes.byref(p), 1, 170, 134, buf, len(ok) - 1) == 0
    assert lib.hl_amd_stream_headers(None, 1, 170, 134, buf, 64) == 0


# ---- edge ingest -------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    return dp.display_emu_lib()


def emu(lib, fmt, planes, w, h, dw, dh, key=(0, 0)):
    y = np.full((h, w), 0xEE, np.uint8)
    u = np.full((h // 2, w // 2), 0xEE, np.uint8)
    v = np.full((h // 2, w // 2), 0xEE, np.uint8)
    ptrs = (ctypes.c_void_p * 3)(*[p.ctypes.data for p in planes])
    pitches = (ctypes.c_int64 * 3)(*[p.strides[0] for p in planes])
    assert all(p.strides[1] == 1 for p in planes)
    assert lib.display_emu_frame(fmt, key[0], key[1], w, h, dw, dh, ptrs, pitches, y.ctypes.data, u.ctypes.data, v.ctypes.data) == 0
    return y, u, v


def same(got, want, what):
    for name, g, m in zip("YUV", got, want):
        assert g.shape == m.shape
        assert np.array_equal(g, m), f"{what} {name}: {np.count_nonzero(g != m)} samples differ, first at {np.argwhere(g != m)[0].tolist()}"


@pytest.mark.parametrize("kind", ["noise", "edges"])
@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_edge_tiles_replicate_the_converted_planes(lib, fmt, key, kind):
    F = it.FORMATS[fmt]
    for w, h, dw, dh in SHAPES:
        content = dp.content_planes(F, dw, dh, kind, dw * 7 + dh + F)
        want = dp.model_planes(F, content, key, w, h)
        what = f"{fmt} {dw}x{dh} in {w}x{h} {kind}"
        outs = [emu(lib, F, [np.ascontiguousarray(p) for p in it.pack(F, content)], w, h, dw, dh, key)]  # dense
        same(outs[0], want, what + " dense")
        for fill in (0xA5, 0x3C):  # padded pitches (no multiples of 4 among them): what lies between the rows reaches no output
            outs.append(emu(lib, F, [it.padded(p, 6, fill) for p in it.pack(F, content)], w, h, dw, dh, key))
            same(outs[-1], want, what + " padded")
        same(outs[1], outs[2], what + " two fills")


def test_edge_lanes_cover_every_other_tile_once(lib):
    for w, h, dw, dh in SHAPES + [(16, 16, 2, 2), (1920, 1088, 1920, 1080), (48, 32, 48, 32)]:
        full, edge = ctypes.c_int32(), ctypes.c_int32()
        lib.display_emu_tiles(w, h, dw, dh, ctypes.byref(full), ctypes.byref(edge))
        seen = set()
        for i in range(edge.value):
            tx, ty = ctypes.c_int32(), ctypes.c_int32()
            assert lib.display_emu_edge_at(i, w, h, dw, dh, ctypes.byref(tx), ctypes.byref(ty)) == 0
            assert 0 <= tx.value < w // 16 and 0 <= ty.value < h // 2
            assert not (tx.value < dw // 16 and ty.value < dh // 2)  # not a full tile
            seen.add((tx.value, ty.value))
        assert len(seen) == edge.value and full.value + edge.value == (w // 16) * (h // 2)
    assert (full.value, edge.value) == (48 * 16 // 16, 0)  # (the display size is the coded size: nothing for the edge kernel)
    lib.display_emu_tiles(1920, 1088, 1920, 1080, ctypes.byref(full), ctypes.byref(edge))
    assert edge.value == 480 and full.value + edge.value == 65280


def test_refused_descriptions(lib):
    p = np.zeros((32, 4 * 48), np.uint8)
    out = np.zeros(48 * 32, np.uint8)
    o = out.ctypes.data
    ptrs = (ctypes.c_void_p * 3)(p.ctypes.data, p.ctypes.data, p.ctypes.data)

    def call(fmt, w, h, dw, dh, pitch=0):
        return lib.display_emu_frame(fmt, 0, 0, w, h, dw, dh, ptrs, (ctypes.c_int64 * 3)(pitch, pitch, pitch), o, o, o)

    assert call(it.RGB24, 48, 32, 34, 18) == 0
    assert call(it.RGB24, 48, 32, 33, 18) == -1 and call(it.RGB24, 48, 32, 34, 17) == -1  # odd
    assert call(it.RGB24, 48, 32, 32, 18) == -1 and call(it.RGB24, 48, 32, 34, 16) == -1  # a whole macroblock column or row short
    assert call(it.RGB24, 48, 32, 50, 18) == -1 and call(it.RGB24, 48, 32, 34, 34) == -1  # beyond the coded size
    assert call(it.RGB24, 48, 32, 34, 18, 3 * 34 - 1) == -1                                # pitch below the display size's row bytes


def test_sanitizers_over_exactly_sized_planes():
    if not os.path.exists(ASAN_BIN):  # build() makes it; a bare pytest run builds it here
        subprocess.run(["make", "-C", ROOT, "tests/sanitize/ingest_edge_asan"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1")
    r = subprocess.run([ASAN_BIN], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    assert "ingest edge ok" in r.stdout


# ---- quality over a window -----------------------------------------------------------
def emu_quality(lib, a, b, ww, wh, with_mb=False):
    h, w = a.shape
    sse, q, n = ctypes.c_uint64(), ctypes.c_int64(), ctypes.c_uint64()
    mb = np.full((h // 16, w // 16), 0xDEADBEEF, np.uint32) if with_mb else None
    rc = lib.display_emu_quality(a.ctypes.data, b.ctypes.data, w, h, ww, wh, ctypes.byref(sse), ctypes.byref(q), ctypes.byref(n),
                                 mb.ctypes.data if with_mb else None)
    assert rc == 0
    return {"sse": sse.value, "ssim_q30": q.value, "windows": n.value}, mb


def plane_pair(w, h, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w), dtype=np.uint8)
    b = np.clip(a.astype(np.int64) + rng.integers(-9, 10, (h, w)), 0, 255).astype(np.uint8)
    b[:, w // 2:] = rng.integers(0, 256, (h, w - w // 2), dtype=np.uint8)  # (uncorrelated half: negative Q among the windows)
    return a, b


@pytest.mark.parametrize("shape", [(48, 32, 34, 18), (48, 32, 17, 9), (48, 32, 7, 9), (176, 144, 162, 130), (528, 48, 514, 34)],
                         ids=lambda s: f"{s[2]}x{s[3]}in{s[0]}x{s[1]}")
def test_quality_over_a_window(lib, shape):
    """(the last shape: the window ends in the second tile of 256 x 32 samples, in both directions)"""
    w, h, ww, wh = shape
    a, b = plane_pair(w, h, w + 3 * ww)
    want = dp.window_quality(a, b, ww, wh)
    mbs = (w % 16 == 0 and h % 16 == 0)
    got, mb = emu_quality(lib, a, b, ww, wh, mbs)
    assert got == {k: want[k] for k in got}, (got, want)
    assert want["windows"] == max(0, ww // 4 - 1) * max(0, wh // 4 - 1)
    if (ww, wh) == (7, 9):
        assert want["windows"] == 0 and got["ssim_q30"] == 0
    if mbs:
        assert np.array_equal(mb, dp.window_mb_sse(a, b, ww, wh))
        assert int(mb.astype(np.uint64).sum()) == want["sse"]
    # what lies outside the window reaches no result
    a2, b2 = a.copy(), b.copy()
    a2[wh:, :], a2[:, ww:], b2[wh:, :], b2[:, ww:] = 1, 2, 250, 251
    assert emu_quality(lib, a2, b2, ww, wh)[0] == got


@pytest.mark.parametrize("size", [(48, 32), (176, 144), (264, 40)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_full_plane_window_is_the_plane(lib, size):
    w, h = size
    a, b = plane_pair(w, h, w + h)
    got, _ = emu_quality(lib, a, b, w, h)
    sse, q = qt.emu_plane(a, b)
    assert (got["sse"], got["ssim_q30"]) == (sse, q)
    want = qt.plane_quality(a, b)
    assert got == {k: want[k] for k in got}
    assert dp.window_quality(a, b, w, h) == want  # (the two models agree)


# ---- Frame sizes ----------------------------------------------------------------------
def test_frames_are_checked_against_the_display_size():
    """Encoder._check_frame without a device: an encoder object that was never created"""
    from hartallo_amd import Encoder, Frame, HlAmdError

    enc = Encoder.__new__(Encoder)
    enc.width, enc.height = 48, 32
    assert enc.display_size == (48, 32)
    coded = Frame.from_array(np.zeros((32, 48, 3), np.uint8))
    shown = Frame.from_array(np.zeros((18, 34, 3), np.uint8))
    y, c = np.zeros((18, 34), np.uint8), np.zeros((9, 17), np.uint8)
    shown_yuv = [Frame.i420(y, c, c), Frame.nv12(y, np.zeros((9, 34), np.uint8))]
    enc._check_frame(coded)
    for f in [shown] + shown_yuv:
        with pytest.raises(HlAmdError) as e:
            enc._check_frame(f)
        assert e.value.code == 4
    enc._display = (34, 18)  # (what set_display_size leaves)
    assert enc.display_size == (34, 18)
    for f in [shown] + shown_yuv:
        enc._check_frame(f)
    with pytest.raises(HlAmdError) as e:
        enc._check_frame(coded)
    assert e.value.code == 4
    enc._check_frame(Frame(it.RGB24, (1,), (0,)))  # a frame of unknown size is the library's to check
