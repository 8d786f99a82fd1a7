"""The access unit's display size on the CPU (hl_amd_set_au_display_size,
DESIGN.md 6.13): the SVC headers with cropping fields (hl_amd_svc_stream_headers,
a pure function) through exp-Golomb parsers of the tests' own; the frame
ingest's full and edge tiles with margins wider than a macroblock built for the
host (tests/emu/libhl_svc_display_emu.so) against np.pad(mode="edge") of
in_testlib's planes, the layer pyramid applied to them, and the quality window
of every layer against the crop-then-sum model; the same tiles under
AddressSanitizer + UndefinedBehaviorSanitizer over exactly-sized heap planes
(tests/sanitize/ingest_wide_asan, a stand-alone program); and the fixture of
tests/golden/make_svc_display_golden.py through the host build of the kernel
logic.  Everything is integer: exact equality.
"""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

import dp_testlib as dp
import in_testlib as it
import svcd_testlib as st
from hl_testlib import ROOT

ASAN_BIN = os.path.join(ROOT, "tests", "sanitize", "ingest_wide_asan")
FORMATS = ["i420", "nv12", "rgb24", "rgba32", "rgbp"]
KEYS = [(it.BT601, it.LIMITED), (it.BT709, it.FULL)]
KEY_IDS = ["601l", "709f"]
# coded size, display size, layers (max_margin = 16 << K): every multiple of 8
# in 64 x 64 (up to 4 edge tile columns and 28 edge tile rows; 8 x 8 has no full
# tile), margins of 56 and 40, and a right band of 4 tile columns that starts
# in tile 64 of a row pair -- the second 64-lane workgroup column of k_ingest's
# grid -- over a display height of 8
SHAPES = [(64, 64, dw, dh, 3) for dw in range(8, 65, 8) for dh in range(8, 65, 8)] + [(128, 128, 72, 88, 3), (1088, 64, 1032, 8, 3)]

# the issue's two examples, three layers, qp 28, top to base: display size, base coded size, SPS 0, subset SPS 1, subset SPS 2
WORKED = [
    ((1920, 1080), (480, 272), "27 42 e0 1e 95 a0 78 23 7a 40", "2f 53 80 1f 4b 0a d0 1e 02 2b da 50 80", "2f 53 80 32 6b 0a d0 0f 00 44 bc a9 42"),
    ((1280, 720), (320, 192), "27 42 e0 0c 95 a0 50 65 e7 40", "2f 53 80 1e 4b 0a d0 14 06 2f 1a 94 20", "2f 53 80 28 6b 0a d0 0a 00 c2 f0 ca 50 80"),
]


# ---- headers -----------------------------------------------------------------------
def headers(w0, h0, layers, dw=None, dh=None, max_ref=1, qp=28):
    from hartallo_amd import svc_stream_headers

    return st.split_headers(svc_stream_headers(w0, h0, layers, qp, max_ref, dw, dh), layers)


@pytest.mark.parametrize("display,base,sps0,ssps1,ssps2", WORKED, ids=["1080p", "720p"])
def test_worked_examples(display, base, sps0, ssps1, ssps2):
    sps, ssps, pps = headers(*base, 3, *display)
    assert [sps.hex(" ")] + [x.hex(" ") for x in ssps] == [sps0, ssps1, ssps2]
    W, H = base[0] << 2, base[1] << 2
    assert dp.parse_sps(sps)["crop"] == (0, (W - display[0]) // 8, 0, (H - display[1]) // 8)
    for l, x in enumerate(ssps, 1):
        assert st.parse_subset_sps(x)["crop"] == (0, ((W - display[0]) >> (2 - l)) // 2, 0, ((H - display[1]) >> (2 - l)) // 2)
    assert pps == headers(*base, 3)[2]


def check_headers(w0, h0, layers, dw, dh, max_ref, plain):
    K = layers - 1
    W, H = w0 << K, h0 << K
    sps, ssps, pps = headers(w0, h0, layers, dw, dh, max_ref)
    psps, pssps, ppps = plain
    what = (w0, h0, layers, dw, dh, max_ref)
    assert pps == ppps, what  # the PPSs: byte for byte
    for x in [sps] + ssps:
        assert dp.needs_no_escape(x), (what, x.hex())
    if (dw, dh) == (W, H):
        assert sps == psps and ssps == pssps, what
        return
    for l in range(layers):
        got = dp.parse_sps(sps) if l == 0 else st.parse_subset_sps(ssps[l - 1])
        base = dp.parse_sps(psps) if l == 0 else st.parse_subset_sps(pssps[l - 1])
        right, bottom = ((W - dw) >> (K - l)) // 2, ((H - dh) >> (K - l)) // 2
        assert ((w0 << l) - 2 * right, (h0 << l) - 2 * bottom) == (dw >> (K - l), dh >> (K - l))
        assert got["cropping"] == 1 and got["crop"] == (0, right, 0, bottom), (what, l, got)
        assert base["cropping"] == 0
        for k in base:  # level_idc, max_num_ref_frames and the SVC extension among them: those of the coded size
            if k not in ("cropping", "crop"):
                assert got[k] == base[k], (k, what, l)
        assert (got["width_mbs_minus1"], got["height_mbs_minus1"]) == ((w0 << l) // 16 - 1, (h0 << l) // 16 - 1)
        if l:
            assert got["svc_ext"] == (1, 0, 1, 1, 0, 0) and got["sps_id"] == l  # extended_spatial_scalability_idc stays 0


@pytest.mark.parametrize("layers", [2, 3, 4])
def test_every_base_size_one_crop_each(layers):
    """base sizes 16 x 16 .. 480 x 272 (config 4's base), step 16: each with one crop pair and max_ref_frame out of the sweep below"""
    K = layers - 1
    for w0 in range(16, 481, 16):
        for h0 in range(16, 273, 16):
            k = (w0 // 16) * 131 + (h0 // 16) * 17 + layers
            max_ref = (1, 4, 16)[k % 3]
            dws, dhs = st.legal_values(layers, w0 << K), st.legal_values(layers, h0 << K)
            check_headers(w0, h0, layers, dws[k % len(dws)], dhs[(k // 8) % len(dhs)], max_ref, headers(w0, h0, layers, max_ref=max_ref))


@pytest.mark.parametrize("layers", [2, 3, 4])
def test_every_crop_at_chosen_sizes(layers):
    """every legal display size (8 widths x 8 heights, the coded size among them) at four base sizes"""
    K = layers - 1
    for w0, h0 in ((16, 16), (64, 48), (320, 192), (480, 272)):
        for max_ref in (1, 4):
            plain = headers(w0, h0, layers, max_ref=max_ref)
            dws, dhs = st.legal_values(layers, w0 << K), st.legal_values(layers, h0 << K)
            assert len(dws) == 8 and len(dhs) == 8 and dws[-1] == w0 << K and dhs[-1] == h0 << K
            for dw in dws:
                for dh in dhs:
                    assert st.legal(layers, w0 << K, h0 << K, dw, dh)
                    check_headers(w0, h0, layers, dw, dh, max_ref, plain)


def test_no_display_size_gives_the_committed_streams_headers():
    """the header NAL units at the front of svc3_64x48_qp30_gop3.264 (the
    reference's): after the base layer's, the set for two layers and the set for
    three, which are the pure function's for no display size"""
    from hartallo_amd import svc_stream_headers

    g = st.SVC_GOLD["svc3_64x48_qp30_gop3"]
    stream = open(os.path.join(st.GOLDEN_DIR, g["stream"]), "rb").read()
    n = dp.nals(stream)
    assert [st.nal_type(x) for x in n[:12]] == [7, 8, 7, 15, 8, 8, 7, 15, 15, 8, 8, 8]
    W, H = g["w0"] << 2, g["h0"] << 2
    for L, part in ((2, n[2:6]), (3, n[6:12])):
        for disp in ((None, None), (g["w0"] << (L - 1), g["h0"] << (L - 1))):
            assert dp.nals(svc_stream_headers(g["w0"], g["h0"], L, g["qp"], 1, *disp)) == part
    assert (W, H) == (256, 192)


def test_refused_settings():
    from hartallo_amd import _lib as L
    from hartallo_amd import svc_stream_headers

    ok = svc_stream_headers(64, 48, 3, 28, 1, 200, 136)
    assert len(dp.nals(ok)) == 6
    # no multiple of 2 << K; a margin of 16 << K or more; beyond the coded size; nothing
    for dw, dh in ((204, 136), (200, 132), (198, 136), (192, 136), (200, 128), (264, 136), (200, 200), (0, 0), (-8, 136)):
        assert not st.legal(3, 256, 192, dw, dh)
        with pytest.raises(ValueError):
            svc_stream_headers(64, 48, 3, 28, 1, dw, dh)
    svc_stream_headers(64, 48, 2, 28, 1, 100, 68)  # (K = 1: multiples of 4, margins below 32)
    with pytest.raises(ValueError):
        svc_stream_headers(64, 48, 2, 28, 1, 96, 68)
    with pytest.raises(ValueError):
        svc_stream_headers(64, 48, 2, 28, 1, 102, 68)
    for layers in (0, 1, 5):
        with pytest.raises(ValueError):
            svc_stream_headers(64, 48, layers, 28, 1, 64 << max(0, layers - 1), 48 << max(0, layers - 1))
    for w0, h0 in ((60, 48), (0, 16), (64, 40)):  # the coded sizes stay multiples of 16
        with pytest.raises(ValueError):
            svc_stream_headers(w0, h0, 2)
    with pytest.raises(ValueError):
        svc_stream_headers(64, 48, 3, 52)
    with pytest.raises(ValueError):
        svc_stream_headers(16, 16, 2, 28, 17)  # max_num_ref_frames above 16
    with pytest.raises(ValueError):
        svc_stream_headers(64, 48, 3, 28, -1)
    lib = L.load_library()
    p = L._Params(64, 48, 28, 16, 1, 30, 0, 0)
    buf = ctypes.create_string_buffer(256)
    assert lib.hl_amd_svc_stream_headers(ctypes.byref(p), 1, 3, 200, 136, buf, len(ok)) == len(ok) and buf.raw[:len(ok)] == ok
    assert lib.hl_amd_svc_stream_headers(ctypes.byref(p), 1, 3, 200, 136, buf, len(ok) - 1) == 0  # the bytes must fit
    assert lib.hl_amd_svc_stream_headers(None, 1, 3, 200, 136, buf, 256) == 0


# ---- ingest with wide margins, the pyramid, the quality windows ---------------------------------
@pytest.fixture(scope="module")
def lib():
    return st.emu_lib()


def same(got, want, what):
    for name, g, m in zip("YUV", got, want):
        assert g.shape == m.shape, what
        assert np.array_equal(g, m), f"{what} {name}: {np.count_nonzero(g != m)} samples differ, first at {np.argwhere(g != m)[0].tolist()}"


@pytest.mark.parametrize("key", KEYS, ids=KEY_IDS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_wide_margins_replicate_the_converted_planes(lib, fmt, key):
    F = it.FORMATS[fmt]
    for n, (w, h, dw, dh, layers) in enumerate(SHAPES):
        mm = 16 << (layers - 1)
        content = dp.content_planes(F, dw, dh, "edges" if n & 1 else "noise", dw * 7 + dh + F)
        want = dp.model_planes(F, content, key, w, h)
        what = f"{fmt} {dw}x{dh} in {w}x{h}"
        got = st.emu_frame(lib, F, [np.ascontiguousarray(p) for p in it.pack(F, content)], w, h, dw, dh, mm, key)  # dense
        same(got, want, what + " dense")
        outs = []
        for fill in (0xA5, 0x3C):  # padded pitches: what lies between the rows reaches no output
            outs.append(st.emu_frame(lib, F, [it.padded(p, 6, fill) for p in it.pack(F, content)], w, h, dw, dh, mm, key))
            same(outs[-1], want, what + " padded")
        same(outs[0], outs[1], what + " two fills")
        # the pyramid of the padded picture: every layer's display rectangle is _down2 of the cropped source
        src = [tuple(p[:dh >> (c > 0), :dw >> (c > 0)] for c, p in enumerate(want))]
        for _ in range(layers - 1):
            src.insert(0, st.down(src[0]))
        pyr = st.emu_pyramid(got, layers)
        same(pyr[layers - 1], want, what + " top")
        for l in range(layers):
            k = layers - 1 - l
            shown = tuple(p[:(dh >> k) >> (c > 0), :(dw >> k) >> (c > 0)] for c, p in enumerate(pyr[l]))
            same(shown, src[l], f"{what} layer {l} display rectangle")
            same(pyr[l], st.pyramid(want, layers)[l], f"{what} layer {l}")


def test_edge_lanes_cover_every_other_tile_once(lib):
    shapes = [s[:4] + (16 << (s[4] - 1),) for s in SHAPES]
    shapes += [(1920, 1088, 1920, 1080, 64), (1280, 768, 1280, 720, 64), (128, 128, 2, 2, 128), (64, 64, 64, 64, 32), (48, 32, 34, 18, 16)]
    counts = {}
    for w, h, dw, dh, mm in shapes:
        full, edge = ctypes.c_int32(), ctypes.c_int32()
        assert lib.svcd_emu_tiles(w, h, dw, dh, mm, ctypes.byref(full), ctypes.byref(edge)) == 0
        tx, ty = np.full(edge.value + 1, -7, np.int32), np.full(edge.value + 1, -7, np.int32)
        assert lib.svcd_emu_edge_all(w, h, dw, dh, mm, tx.ctypes.data, ty.ctypes.data) == edge.value
        assert tx[-1] == -7 and ty[-1] == -7
        tx, ty = tx[:-1], ty[:-1]
        assert ((tx >= 0) & (tx < w // 16) & (ty >= 0) & (ty < h // 2)).all()
        assert not ((tx < dw // 16) & (ty < dh // 2)).any()  # no full tile among them
        assert len(set(zip(tx.tolist(), ty.tolist()))) == edge.value and full.value + edge.value == (w // 16) * (h // 2), (w, h, dw, dh)
        counts[(w, h, dw, dh)] = edge.value
    assert counts[(1920, 1088, 1920, 1080)] == 480 and counts[(1280, 768, 1280, 720)] == 1920 and counts[(64, 64, 64, 64)] == 0
    assert counts[(128, 128, 2, 2)] == 8 * 64
    # the margins are checked against max_margin
    full, edge = ctypes.c_int32(), ctypes.c_int32()
    assert lib.svcd_emu_tiles(1280, 768, 1280, 720, 32, ctypes.byref(full), ctypes.byref(edge)) == -1
    assert lib.svcd_emu_tiles(1280, 768, 1280, 704, 64, ctypes.byref(full), ctypes.byref(edge)) == -1
    assert lib.svcd_emu_tiles(64, 64, 36, 44, 32, ctypes.byref(full), ctypes.byref(edge)) == 0
    assert lib.svcd_emu_tiles(64, 64, 32, 44, 32, ctypes.byref(full), ctypes.byref(edge)) == -1


@pytest.mark.parametrize("name", sorted(st.GOLD))
def test_quality_windows_of_every_layer(name):
    """the metric's host build over layer l's display rectangle against the
    crop-then-sum model, on the fixture's padded pyramid and a noisy copy"""
    g = st.GOLD[name]
    L, K = g["layers"], g["layers"] - 1
    q = dp.display_emu_lib()
    _, layers = st.workload(name)
    rng = np.random.default_rng(11)
    for l in range(L):
        dw, dh = g["display_width"] >> (K - l), g["display_height"] >> (K - l)
        for c, a in enumerate(layers[1][l]):
            a = np.ascontiguousarray(a)
            b = np.clip(a.astype(np.int64) + rng.integers(-9, 10, a.shape), 0, 255).astype(np.uint8)
            ww, wh = dw >> (c > 0), dh >> (c > 0)
            h, w = a.shape
            sse, s, n = ctypes.c_uint64(), ctypes.c_int64(), ctypes.c_uint64()
            mb = np.zeros((h // 16, w // 16), np.uint32) if c == 0 else None
            assert q.display_emu_quality(a.ctypes.data, b.ctypes.data, w, h, ww, wh, ctypes.byref(sse), ctypes.byref(s), ctypes.byref(n),
                                         mb.ctypes.data if c == 0 else None) == 0
            want = dp.window_quality(a, b, ww, wh)
            assert (sse.value, s.value, n.value) == (want["sse"], want["ssim_q30"], want["windows"]), (name, l, c)
            if c == 0:
                assert np.array_equal(mb, dp.window_mb_sse(a, b, ww, wh))


def test_sanitizers_over_exactly_sized_planes():
    if not os.path.exists(ASAN_BIN):  # build() makes it; a bare pytest run builds it here
        subprocess.run(["make", "-C", ROOT, "tests/sanitize/ingest_wide_asan"], check=True, capture_output=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:halt_on_error=1")
    r = subprocess.run([ASAN_BIN], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout + r.stderr)[-3000:]
    assert "ingest wide margins ok" in r.stdout


# ---- which layers take the reproduced Intra_Base array quirk ------------------------------------
def test_only_the_64x64_layer_takes_the_array_quirk():
    """svc_geom marks exactly the geometry that was compared with the reference
    (a layer of 4 x 4 macroblocks over a 32 x 32 base; svcd2_32x32 below); every
    other layer size, the smaller ones and the other 16-macroblock shapes
    included, runs the plain G.8.6.2 interpolation: the same samples with the
    quirk switched off.  At 64 x 64 the two differ, in the lower rows of the
    macroblocks of even macroblock rows only (sample rows 5..15)."""
    lib = ctypes.CDLL(os.path.join(ROOT, "tests", "emu", "libhl_svc_geom_emu.so"))
    lib.svc_geom_emu_rsa_bytes.argtypes = [ctypes.c_int32] * 2
    lib.svc_geom_emu_intra_base.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p]
    for w in range(32, 545, 32):
        for h in range(32, 545, 32):
            assert lib.svc_geom_emu_rsa_bytes(w, h) == (4096 if (w, h) == (64, 64) else 0), (w, h)
    for w, h in ((960, 544), (1920, 1088), (1280, 768), (3840, 2176)):
        assert lib.svc_geom_emu_rsa_bytes(w, h) == 0

    def intra_base(w, h, plain):
        ref = np.random.default_rng(w * 3 + h).integers(0, 256, (h // 2, w // 2), dtype=np.uint8)
        out = np.empty((h, w), np.uint8)
        assert lib.svc_geom_emu_intra_base(w, h, ref.ctypes.data, plain, out.ctypes.data) == 0
        return out

    for w, h in ((32, 32), (32, 64), (64, 32), (96, 32), (64, 96), (96, 64), (128, 32), (32, 128), (96, 96), (128, 64), (256, 192)):
        assert np.array_equal(intra_base(w, h, 0), intra_base(w, h, 1)), (w, h)
    a, b = intra_base(64, 64, 0), intra_base(64, 64, 1)
    differs = (a != b).reshape(4, 16, 4, 16).any(axis=(1, 3))
    assert differs[0].all() and differs[2].all() and not differs[1].any() and not differs[3].any()
    rows = np.flatnonzero((a != b).any(axis=1))
    # (sample row 5 of such a macroblock is the first whose four taps, array rows 25..28, reach the overlapped rows 28..33)
    assert set(rows // 16) == {0, 2} and set(rows % 16) == set(range(5, 16))


# ---- the fixture ----------------------------------------------------------------------------
def test_fixture_input_is_what_the_maker_states():
    for name, g in st.GOLD.items():
        L, K = g["layers"], g["layers"] - 1
        assert st.legal(L, g["w0"] << K, g["h0"] << K, g["display_width"], g["display_height"]) and g["intra_in_p"] == 0
        shown, layers = st.workload(name)
        assert len(shown) == g["frames"] == len(g["au_md5"])
        top = layers[0][K]
        assert top[0].shape == (g["h0"] << K, g["w0"] << K)
        assert np.array_equal(top[0][:g["display_height"], :g["display_width"]], shown[0][0])
        assert (top[0][:, g["display_width"]:] == top[0][:, g["display_width"] - 1:g["display_width"]]).all()
        assert (top[0][g["display_height"]:, :] == top[0][g["display_height"] - 1:g["display_height"], :]).all()
        assert hashlib.md5(st.stream(name)).hexdigest() == g["stream_md5"]


@pytest.mark.parametrize("name", sorted(st.GOLD))
def test_kernel_logic_reproduces_the_fixture(name):
    """the host build of the kernel logic on the padded layers: the reference's
    stream and reconstructions, nothing outside the pinned scope.  (svcd2_32x32:
    a 64 x 64 layer of 4 x 4 macroblocks, where the reference's Intra_Base array overlaps
    its availability array -- hl_svc.h svc_ref_array_sample.)"""
    from hl_testlib import EmuSvcEncoder

    g = st.GOLD[name]
    L = g["layers"]
    _, layers = st.workload(name)
    enc = EmuSvcEncoder(g["w0"], g["h0"], L, g["qp"], g["me_range"], g["deblock"], g["gop"], g["early_term"])
    out = b""
    for i in range(g["frames"]):
        au = b"".join(enc.encode(l, st.flat(layers[i][l])) for l in range(L))
        assert hashlib.md5(au).hexdigest() == g["au_md5"][i], f"AU {i}: bytes differ ({len(au)} vs {g['au_bytes'][i]})"
        for l in range(L):
            assert hashlib.md5(enc.recon(l).tobytes()).hexdigest() == g["recon_md5"][l][i], f"AU {i} layer {l}: reconstruction differs"
        out += au
    assert out == st.stream(name) and enc.unpinned() == 0
