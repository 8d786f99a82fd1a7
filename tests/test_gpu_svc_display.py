"""The access unit's display size on the GPU (hl_amd_set_au_display_size,
hl_amd_encode_au_frame(s)).  With a display size every slice
NAL unit of every layer stays the reference's for the padded pictures
(tests/golden/svc_display_golden.json, made by the reference encoder) and only
the SPS and the subset SPSs change; frames of the top display size in any format
are converted and padded on the GPU (k_ingest, k_ingest_edge with margins up to
(16 << K) - 2) exactly as np.pad(mode="edge") pads the model's planes, the lower
layers are k_pyramid's of that padded picture, and the access units are those of
encode_au on the padded planes; quality covers each layer's display rectangle;
refusals leave the stream as it was.
"""
import ctypes
import functools
import hashlib

import numpy as np
import pytest

import dp_testlib as dp
import in_testlib as it
import svcd_testlib as st

pytestmark = pytest.mark.gpu

NAMES = sorted(st.GOLD)
KEY = (it.BT709, it.LIMITED)
# NV12 with a pitch of dw + 8, pitched I420, RGB24 and planar RGB
FRAME_FORMATS = ["nv12", "i420", "rgb24", "rgbp"]


def md5(b) -> str:
    return hashlib.md5(b).hexdigest()


def encoder(name, display=True, quality=False):
    from hartallo_amd import SvcEncoder

    g = st.GOLD[name]
    enc = SvcEncoder(g["w0"], g["h0"], g["layers"], g["qp"], g["me_range"], g["deblock"], g["gop"], g["early_term"])
    enc.set_colour(*KEY)
    if quality:
        enc.set_quality(True)
    if display:
        enc.set_au_display_size(g["display_width"], g["display_height"])
        assert enc.au_display_size == (g["display_width"], g["display_height"])
    return enc


def want_headers(name):
    from hartallo_amd import svc_stream_headers

    g = st.GOLD[name]
    return st.split_headers(svc_stream_headers(g["w0"], g["h0"], g["layers"], g["qp"], 1, g["display_width"], g["display_height"]), g["layers"])


def check_against_reference(name, aus):
    """Every NAL unit other than types 7 and 15 is the reference stream's, in
    order and byte for byte; the type 7 and 15 units are svc_stream_headers'."""
    g = st.GOLD[name]
    got, ref = dp.nals(b"".join(aus)), dp.nals(st.stream(name))
    assert [st.nal_type(x) for x in got] == [st.nal_type(x) for x in ref]
    sps, ssps, _ = want_headers(name)
    seen = 0
    for k, (a, b) in enumerate(zip(got, ref)):
        t = st.nal_type(a)
        if t == 7:
            assert a == sps and a != b, f"NAL {k}: SPS"
        elif t == 15:
            l = st.parse_subset_sps(a)["sps_id"]
            assert a == ssps[l - 1] and a != b, f"NAL {k}: subset SPS {l}"
        else:
            assert a == b, f"NAL {k} (type {t}): {len(a)} bytes vs the reference's {len(b)}"
            seen += 1
    assert seen >= g["frames"] * (g["layers"] + 1)


def padded_top(name, i):
    _, layers = st.workload(name)
    return layers[i][-1]


def device_planes(planes):
    """(tensor, (y, u, v) pointers) of dense coded-size planes in HBM"""
    import torch

    flat = st.flat(planes)
    t = torch.from_numpy(flat).cuda()
    torch.cuda.synchronize()
    ny = planes[0].size
    return t, (t.data_ptr(), t.data_ptr() + ny, t.data_ptr() + ny + ny // 4)


# ---- parity with the reference -------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_padded_planes_per_call_match_reference(name):
    g = st.GOLD[name]
    enc = encoder(name)
    aus = []
    for i in range(g["frames"]):
        r = enc.encode_au(*padded_top(name, i))
        assert r.type & 1 and bool(r.type & 2) == (i == 0)
        aus.append(r.annexb())
        for l in range(g["layers"]):
            assert md5(enc.layer_recon(l).tobytes()) == g["recon_md5"][l][i], f"AU {i} layer {l}: reconstruction differs"
    assert enc.unpinned() == 0
    enc.close()
    check_against_reference(name, aus)


@pytest.mark.parametrize("name", NAMES)
def test_padded_planes_batched_match_reference(name):
    g = st.GOLD[name]
    enc = encoder(name)
    dev = [device_planes(padded_top(name, i)) for i in range(g["frames"])]
    res = enc.encode_aus_batch_device([p for _, p in dev])
    for l in range(g["layers"]):
        assert md5(enc.layer_recon(l).tobytes()) == g["recon_md5"][l][-1], f"layer {l}: reconstruction differs"
    assert enc.unpinned() == 0
    enc.close()
    check_against_reference(name, [r.annexb() for r in res])


# ---- frames ------------------------------------------------------------------------------------
def pads_for(F, fmt, dw):
    if fmt == "nv12":
        return (8, 8)
    return tuple(((-rb) % 4) + 8 for rb in ({it.I420: (dw, dw // 2, dw // 2), it.RGB24: (3 * dw,), it.RGBP: (dw,) * 3}[F]))


def host_frame(F, content, pads, dw, dh):
    from hartallo_amd import Frame

    bufs = [it.padded_buffer(p, pad) for p, pad in zip(it.pack(F, content), pads)]
    return Frame(F, [b.ctypes.data for b, _ in bufs], [pitch for _, pitch in bufs], False, bufs, dw, dh)


def device_frame(F, content, pads, dw, dh):
    import torch

    from hartallo_amd import Frame

    bufs = [it.padded_buffer(p, pad) for p, pad in zip(it.pack(F, content), pads)]
    dev = [torch.from_numpy(b).cuda() for b, _ in bufs]
    torch.cuda.synchronize()
    return Frame(F, [d.data_ptr() for d in dev], [pitch for _, pitch in bufs], True, dev, dw, dh)


@functools.lru_cache(maxsize=None)
def model_layers(name, fmt):
    """per access unit the model's [layer 0, ..., top] planes for frames of format fmt"""
    g = st.GOLD[name]
    F = it.FORMATS[fmt]
    shown, _ = st.workload(name)
    W, H = g["w0"] << (g["layers"] - 1), g["h0"] << (g["layers"] - 1)
    return [st.pyramid(dp.model_planes(F, st.frame_content(F, s), KEY, W, H), g["layers"]) for s in shown]


@functools.lru_cache(maxsize=None)
def model_stream(name, fmt):
    """a fresh encoder with the same display size fed the model's padded top through encode_au"""
    enc = encoder(name)
    out = [enc.encode_au(*m[-1]).annexb() for m in model_layers(name, fmt)]
    enc.close()
    return out


def check_layer_inputs(enc, model, what):
    for l, m in enumerate(model):
        got = enc.layer_input(l)
        assert np.array_equal(got, st.flat(m)), f"{what}: layer {l} input: {np.count_nonzero(got != st.flat(m))} samples differ"


@pytest.mark.parametrize("fmt", FRAME_FORMATS)
@pytest.mark.parametrize("name", NAMES)
def test_frames_are_padded_and_coded_as_the_model(name, fmt):
    g = st.GOLD[name]
    F = it.FORMATS[fmt]
    dw, dh = g["display_width"], g["display_height"]
    shown, layers = st.workload(name)
    model, want = model_layers(name, fmt), model_stream(name, fmt)
    pads = pads_for(F, fmt, dw)
    if F in (it.I420, it.NV12):  # the model of a YUV frame is the fixture's input
        for i in range(g["frames"]):
            for l in range(g["layers"]):
                assert all(np.array_equal(a, b) for a, b in zip(model[i][l], layers[i][l]))
    streams = {}
    for side, make in (("host", host_frame), ("device", device_frame)):
        enc = encoder(name)
        out = []
        for i in range(g["frames"]):
            out.append(enc.encode_au_frame(make(F, st.frame_content(F, shown[i]), pads, dw, dh)).annexb())
            check_layer_inputs(enc, model[i], f"{name} {fmt} {side} AU {i}")
        assert enc.unpinned() == 0 or F not in (it.I420, it.NV12)  # (the fixture's condition is about its own content, not the RGB frames')
        if side == "device":
            assert enc.bench_ingest(2) > 0 and enc.bench_pyramid(2) > 0
        enc.close()
        streams[side] = out
    enc = encoder(name)
    frames = [device_frame(F, st.frame_content(F, s), pads, dw, dh) for s in shown]
    streams["batch"] = [r.annexb() for r in enc.encode_au_frames_device(frames)]
    check_layer_inputs(enc, model[-1], f"{name} {fmt} batch")
    assert enc.unpinned() == 0 or F not in (it.I420, it.NV12)
    enc.close()
    for how, out in streams.items():
        assert out == want, f"{name} {fmt} {how}: the stream of encode_au on the model's padded planes"
    assert streams["batch"] == streams["device"]
    if F in (it.I420, it.NV12):
        check_against_reference(name, streams["batch"])


def test_mixed_formats_in_one_batch():
    name = "svcd3_64x48"
    g = st.GOLD[name]
    dw, dh = g["display_width"], g["display_height"]
    shown, _ = st.workload(name)
    fmts = ["nv12", "i420", "nv12", "i420", "nv12"]
    frames = [device_frame(it.FORMATS[f], shown[i], pads_for(it.FORMATS[f], f, dw), dw, dh) for i, f in enumerate(fmts)]
    enc = encoder(name)
    out = [r.annexb() for r in enc.encode_au_frames_device(frames)]
    enc.close()
    assert out == model_stream(name, "nv12")


# ---- no display size ---------------------------------------------------------------------------
def test_without_a_display_size_frames_give_the_committed_stream():
    import torch

    from hartallo_amd import Frame, SvcEncoder, synth

    name = "svc3_64x48_qp30_gop3"
    g = st.SVC_GOLD[name]
    L = g["layers"]
    W, H = g["w0"] << (L - 1), g["h0"] << (L - 1)
    clip = synth.clip(W, H, g["frames"], g["seed"])
    enc = SvcEncoder(g["w0"], g["h0"], L, g["qp"], g["me_range"], g["deblock"], g["gop"], g["early_term"])
    assert enc.au_display_size == (W, H)
    for i in range(g["frames"]):
        r = enc.encode_au_frame(host_frame(it.NV12, st.planes_of(clip[i], W, H), (8, 8), W, H))
        assert md5(r.annexb()) == g["au_md5"][i], f"NV12 AU {i}"
    enc.close()
    # a dense I420 device frame at an odd address: forwarded (hl_amd_encode_au copies what its 8-byte loads cannot take)
    enc = SvcEncoder(g["w0"], g["h0"], L, g["qp"], g["me_range"], g["deblock"], g["gop"], g["early_term"])
    enc.set_au_display_size(W, H)  # (the coded size: none)
    for i in range(g["frames"]):
        t = torch.zeros(clip[i].size + 1, dtype=torch.uint8, device="cuda")
        t[1:] = torch.from_numpy(clip[i]).cuda()
        torch.cuda.synchronize()
        p = t.data_ptr() + 1
        assert p & 1
        f = Frame(it.I420, (p, p + W * H, p + W * H * 5 // 4), (0, W // 2, W // 2), True, t, W, H)
        assert md5(enc.encode_au_frame(f).annexb()) == g["au_md5"][i], f"I420 device AU {i}"
    enc.close()
    enc = SvcEncoder(g["w0"], g["h0"], L, g["qp"], g["me_range"], g["deblock"], g["gop"], g["early_term"])
    dev = [device_frame(it.NV12, st.planes_of(clip[i], W, H), (8, 8), W, H) for i in range(g["frames"])]
    assert [md5(r.annexb()) for r in enc.encode_au_frames_device(dev)] == g["au_md5"]
    enc.close()


# ---- quality -----------------------------------------------------------------------------------
def layer_quality(enc, name, i, k, sources, what, display=True):
    g = st.GOLD[name]
    L, K = g["layers"], g["layers"] - 1
    out = []
    for l in range(L):
        w, h = g["w0"] << l, g["h0"] << l
        dw, dh = (g["display_width"] >> (K - l), g["display_height"] >> (K - l)) if display else (w, h)
        rec = st.planes_of(enc.layer_recon(l), w, h)
        want = dp.picture_window_quality(sources[l], rec, dw, dh)
        got, mb = enc.last_quality(k, layer=l), enc.debug_quality_mb(k, layer=l)
        for key in ("sse", "samples", "ssim_q30", "windows"):
            assert list(got[key]) == want[key], (what, l, key, got[key], want[key])
        assert np.array_equal(mb, want["mb"]), (what, l)
        assert want["samples"] == [dw * dh, dw * dh // 4, dw * dh // 4]
        out.append({key: list(got[key]) for key in ("sse", "samples", "ssim_q30", "windows")})
    return out


@pytest.mark.parametrize("name", NAMES)
def test_quality_covers_every_layers_display_rectangle(name):
    g = st.GOLD[name]
    shown, layers = st.workload(name)
    dw, dh = g["display_width"], g["display_height"]
    enc = encoder(name, quality=True)
    per_call = []
    for i in range(g["frames"]):
        if i & 1:
            enc.encode_au(*layers[i][-1])
        else:
            enc.encode_au_frame(host_frame(it.NV12, shown[i], (8, 8), dw, dh))
        per_call.append(layer_quality(enc, name, i, 0, layers[i], f"{name} AU {i}"))
    enc.close()
    top = per_call[-1][-1]
    assert top["sse"][0] > 0 and 0 < top["ssim_q30"][0] < top["windows"][0] << 30
    enc = encoder(name, quality=True)
    enc.encode_au_frames_device([device_frame(it.NV12, s, (8, 8), dw, dh) for s in shown])
    n = g["frames"]
    layer_quality(enc, name, n - 1, n - 1, layers[n - 1], f"{name} batch, last AU")
    for i in range(n):
        for l in range(g["layers"]):
            got = enc.last_quality(i, layer=l)
            assert {key: list(got[key]) for key in per_call[i][l]} == per_call[i][l], (name, "batch", i, l)
    enc.close()
    # the coded size as the display size means none: the whole pictures
    enc = encoder(name, display=False, quality=True)
    enc.set_au_display_size(g["w0"] << (g["layers"] - 1), g["h0"] << (g["layers"] - 1))
    enc.encode_au(*layers[0][-1])
    whole = layer_quality(enc, name, 0, 0, layers[0], f"{name} no display size", display=False)
    assert whole[-1]["samples"][0] > per_call[0][-1]["samples"][0]
    enc.close()


# ---- what hl_amd_bench_ingest repeats -----------------------------------------------------------
def test_bench_ingest_follows_the_last_frame_call():
    """a refused frame call leaves the last frame call's launches in place; a
    plain access-unit call that follows is not a frame call, and hl_amd_get_input
    has nothing to show on an encoder with layers"""
    from hartallo_amd import Encoder, Frame, HlAmdError

    name = "svcd3_64x48"
    g = st.GOLD[name]
    dw, dh = g["display_width"], g["display_height"]
    shown, layers = st.workload(name)
    want = model_stream(name, "nv12")

    def refused(code, call):
        with pytest.raises(HlAmdError) as e:
            call()
        assert e.value.code == code, (e.value.code, code)

    enc = encoder(name)
    good = device_frame(it.NV12, shown[0], (8, 8), dw, dh)
    refused(3, lambda: enc.bench_ingest(2))  # nothing yet
    assert enc.encode_au_frame(good).annexb() == want[0]
    assert enc.bench_ingest(2) > 0
    bad = Frame(good.format, good.planes, (dw + 6, dw + 8), True, good.source)
    refused(1, lambda: enc.encode_au_frame(bad))
    refused(1, lambda: enc.encode_au_frames_device([good, bad]))
    assert enc.bench_ingest(2) > 0  # the refused calls changed nothing
    refused(3, lambda: Encoder.last_input(enc, 0))
    assert enc.encode_au(*layers[1][-1]).annexb() == want[1]
    refused(3, lambda: enc.bench_ingest(2))  # the last call was not a frame call
    assert enc.encode_au_frames_device([device_frame(it.NV12, shown[2], (8, 8), dw, dh)])[0].annexb() == want[2]
    assert enc.bench_ingest(2) > 0
    enc.encode_layer(0, *layers[3][0])
    refused(3, lambda: enc.bench_ingest(2))
    enc.close()


# ---- refusals ----------------------------------------------------------------------------------
def test_refusals_leave_the_stream_as_it_was():
    from hartallo_amd import Encoder, Frame, HlAmdError
    from hartallo_amd._lib import _Result

    name = "svcd3_64x48"
    g = st.GOLD[name]
    L, K = g["layers"], g["layers"] - 1
    W, H, dw, dh = g["w0"] << K, g["h0"] << K, g["display_width"], g["display_height"]
    shown, layers = st.workload(name)
    want = model_stream(name, "nv12")
    k = 0

    def refused(code, call):
        with pytest.raises(HlAmdError) as e:
            call()
        assert e.value.code == code, (e.value.code, code)

    def next_au_continues(enc):
        nonlocal k
        assert enc.encode_au_frame(host_frame(it.NV12, shown[k], (8, 8), dw, dh)).annexb() == want[k], f"access unit {k} after a refusal"
        k += 1

    enc = encoder(name, display=False)
    # no multiple of 2 << K; a margin of 16 << K or more; beyond the coded size
    for bad in ((dw + 4, dh), (dw, dh + 2), (W - 64, dh), (dw, H - 64), (W + 8, dh), (0, 0)):
        refused(1, lambda: enc.set_au_display_size(*bad))
        assert enc.au_display_size == (W, H)
    # together with a layer range, in either order
    assert enc.lib.hl_amd_set_layer_range(enc._h, 1, K) == 0
    refused(7, lambda: enc.set_au_display_size(dw, dh))
    assert enc.lib.hl_amd_set_layer_range(enc._h, 0, K) == 0
    enc.set_au_display_size(dw, dh)
    assert enc.lib.hl_amd_set_layer_range(enc._h, 1, K) == 7
    enc.set_max_ref_frame(1)  # (the two setters work in either order)
    # what encoders with layers refuse stays refused
    refused(7, lambda: enc.set_display_size(g["w0"] - 2, g["h0"] - 2))
    assert enc.lib.hl_amd_add_layer(enc._h, 2 * W, 2 * H) == 7
    refused(7, lambda: Encoder.encode_frame(enc, host_frame(it.NV12, shown[0], (8, 8), 0, 0)))
    next_au_continues(enc)
    # after the first picture
    refused(3, lambda: enc.set_au_display_size(W, H))
    refused(3, lambda: enc.set_au_display_size(dw + 8, dh))
    assert enc.au_display_size == (dw, dh)
    next_au_continues(enc)
    # a frame of the wrong size (Python's check, then the library's through the pitch), a misaligned device pitch
    good = device_frame(it.NV12, shown[k], (8, 8), dw, dh)
    coded = host_frame(it.NV12, (layers[k][-1][0], layers[k][-1][1], layers[k][-1][2]), (8, 8), W, H)
    refused(4, lambda: enc.encode_au_frame(coded))
    refused(4, lambda: enc.encode_au_frames_device([coded]))
    next_au_continues(enc)

    def mutated(frame, **kw):
        f = Frame(frame.format, frame.planes, frame.pitches, frame.on_device, frame.source)
        for key, val in kw.items():
            setattr(f, key, val)
        return f

    for call in (lambda: enc.encode_au_frame(mutated(good, pitches=(dw - 8, dw - 8))),          # a pitch below the display size's row bytes
                 lambda: enc.encode_au_frame(mutated(good, pitches=(dw + 6, dw + 8)))):         # a device pitch that is no multiple of 4
        refused(1, call)
    next_au_continues(enc)
    for call in (lambda: enc.encode_au_frames_device([good, mutated(good, pitches=(dw + 8, dw + 2))]),
                 lambda: enc.encode_au_frames_device([good, host_frame(it.NV12, shown[0], (8, 8), dw, dh)])):  # a host frame in the batch
        refused(1, call)
    next_au_continues(enc)
    assert k == g["frames"]
    enc.close()

    # rate control (set before the first picture): refused like the layer calls; off again, the stream starts as ever
    k = 0
    enc = encoder(name)
    enc.set_rate_control(256000)
    refused(7, lambda: enc.encode_au_frame(good))
    refused(7, lambda: enc.encode_au_frames_device([good]))
    enc.set_rate_control(0)
    next_au_continues(enc)
    enc.close()

    # the setter and the frame calls inside an access unit of layer calls
    k = 0
    enc = encoder(name)
    next_au_continues(enc)
    r = enc.encode_layer(0, *layers[1][0])
    refused(3, lambda: enc.set_au_display_size(dw, dh))
    refused(3, lambda: enc.encode_au_frame(host_frame(it.NV12, shown[1], (8, 8), dw, dh)))
    refused(3, lambda: enc.encode_au_frames_device([good]))
    for l in range(1, L):  # the access unit goes on where it was
        r = enc.encode_layer(l, *layers[1][l])
    assert b"\x00\x00\x01" + r.data == want[1]
    k = 2
    next_au_continues(enc)
    enc.close()

    # an encoder without layers, and one whose layers are not all there yet
    ref = Encoder(g["w0"], g["h0"], g["qp"], g["me_range"], g["deblock"], g["gop"])
    base = [ref.encode(*layers[i][0]).annexb() for i in range(2)]
    ref.close()
    avc = Encoder(g["w0"], g["h0"], g["qp"], g["me_range"], g["deblock"], g["gop"])
    assert avc.lib.hl_amd_set_au_display_size(avc._h, dw, dh) == 3
    assert avc.encode(*layers[0][0]).annexb() == base[0]
    assert avc.lib.hl_amd_set_au_display_size(avc._h, dw, dh) == 3
    assert avc.encode(*layers[1][0]).annexb() == base[1]
    assert avc.display_size == (g["w0"], g["h0"])
    avc.close()
    part = Encoder(g["w0"], g["h0"], g["qp"], g["me_range"], g["deblock"], g["gop"])
    part.set_colour(*KEY)
    assert part.lib.hl_amd_add_layer(part._h, g["w0"], g["h0"]) == 0
    assert part.lib.hl_amd_set_au_display_size(part._h, dw, dh) == 3  # only the base layer is there
    for l in range(1, L):
        assert part.lib.hl_amd_add_layer(part._h, g["w0"] << l, g["h0"] << l) == 0
    assert part.lib.hl_amd_set_au_display_size(part._h, dw, dh) == 0
    r = _Result()
    c = host_frame(it.NV12, shown[0], (8, 8), dw, dh)
    fc = c._c()
    assert part.lib.hl_amd_encode_au_frame(part._h, ctypes.byref(fc), ctypes.byref(r)) == 0
    assert part._result(r).annexb() == want[0]
    part.close()
