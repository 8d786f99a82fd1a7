"""SVC access units from the top layer's frame alone (SvcEncoder.encode_au /
encode_au_device / encode_aus_batch_device -> hl_amd_encode_au /
hl_amd_encode_aus_batch, the k_pyramid kernel of hartallo_amd/csrc/
hl_pyramid.h).  The derived layers are checked against
hartallo_amd.synth._down2 applied level by level, and the streams against the
goldens the reference encoder produced from synth.svc_clips' layers
(tests/golden/svc_golden.json): the top clip alone must reproduce every
access unit and reconstruction, bit-exact."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

from hartallo_amd import synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "svc_golden.json")))
NAMES = ["svc3_64x48_qp30_gop3", "svc2_qcif_qp28_db", "svc2_qcif_qp36_nodb_gop2"]

pytestmark = pytest.mark.gpu


def md5(b) -> str:
    return hashlib.md5(b).hexdigest()


def _planes(frame, w, h):
    n = w * h
    return frame[:n], frame[n:n + n // 4], frame[n + n // 4:]


@functools.lru_cache(maxsize=None)
def _clips(name):
    g = GOLD[name]
    L = g["layers"]
    return synth.svc_clips(g["w0"] << (L - 1), g["h0"] << (L - 1), L, g["frames"], g["seed"])


def _encoder(name, layers=None, **kw):
    from hartallo_amd import SvcEncoder

    g = GOLD[name]
    return SvcEncoder(g["w0"], g["h0"], g["layers"] if layers is None else layers, g["qp"], g["me_range"], g["deblock"], g["gop"],
                      g["early_term"], **kw)


def _top(name, i):
    g = GOLD[name]
    L = g["layers"]
    return _planes(_clips(name)[L - 1][i], g["w0"] << (L - 1), g["h0"] << (L - 1))


def _device_ptrs(t, w, h):
    n = w * h
    return t.data_ptr(), t.data_ptr() + n, t.data_ptr() + n + n // 4


def _staged(frame, w, h, K):
    """[level 0 (the frame), level 1, ... level K] as concatenated Y|U|V."""
    y, u, v = _planes(frame, w, h)
    p = [y.reshape(h, w), u.reshape(h // 2, w // 2), v.reshape(h // 2, w // 2)]
    out = [frame]
    for _ in range(K):
        p = [synth._down2(a) for a in p]
        out.append(np.concatenate([a.ravel() for a in p]))
    return out


# base 16x16, 2 layers: the top chroma planes (16x16) are one mostly masked
# wave; base 16x16, 4 layers: K = 3; base 80x48, 3 layers: the spans per row
# (40 luma, 20 chroma) are no multiple of a wave on any plane
@pytest.mark.parametrize("device_input", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("w0,h0,L", [(16, 16, 2), (16, 16, 4), (80, 48, 3)])
def test_pyramid_matches_down2_staged(w0, h0, L, device_input):
    import torch

    from hartallo_amd import SvcEncoder

    w, h = w0 << (L - 1), h0 << (L - 1)
    frame = np.random.default_rng(w0 * 100 + L).integers(0, 256, w * h * 3 // 2, dtype=np.uint8)
    want = _staged(frame, w, h, L - 1)
    enc = SvcEncoder(w0, h0, L)
    if device_input:
        t = torch.from_numpy(frame).cuda()
        r = enc.encode_au_device(*_device_ptrs(t, w, h))
    else:
        r = enc.encode_au(*_planes(frame, w, h))
    assert r.type & 1 and r.type & 2 and r.data
    assert np.array_equal(enc.layer_input(L - 1), frame), "the top layer's input is the frame"
    for l in range(L - 1):
        got = enc.layer_input(l)
        assert np.array_equal(got, want[L - 1 - l]), f"layer {l}: {np.count_nonzero(got != want[L - 1 - l])} samples differ"
    enc.close()


@pytest.mark.parametrize("name", NAMES)
def test_encode_au_matches_reference(name):
    g = GOLD[name]
    L = g["layers"]
    enc = _encoder(name)
    for i in range(g["frames"]):
        r = enc.encode_au(*_top(name, i))
        assert r.type & 1 and bool(r.type & 2) == (i == 0)
        assert md5(r.annexb()) == g["au_md5"][i], f"AU {i}: {len(r.annexb())} bytes vs {g['au_bytes'][i]}"
        for l in range(L):
            assert md5(enc.layer_recon(l).tobytes()) == g["recon_md5"][l][i], f"AU {i} layer {l}: reconstruction differs"
    assert enc.unpinned() == 0
    enc.close()


@pytest.mark.parametrize("name,splits", [(NAMES[0], (5,)), (NAMES[0], (2, 5)), (NAMES[1], (4,)), (NAMES[2], (4,))])
def test_encode_aus_batch_matches_reference(name, splits):
    """The whole clip in one hl_amd_encode_aus_batch call, and split 2 + 3 so
    that the state carries across calls."""
    import torch

    g = GOLD[name]
    L = g["layers"]
    w, h = g["w0"] << (L - 1), g["h0"] << (L - 1)
    dev = torch.from_numpy(_clips(name)[L - 1]).cuda()
    enc = _encoder(name)
    md5s, lo = [], 0
    for hi in splits:
        for r in enc.encode_aus_batch_device([_device_ptrs(dev[i], w, h) for i in range(lo, hi)]):
            md5s.append(md5(r.annexb()))
        st = enc.last_batch_stats()
        assert st["fallbacks"] == 0 and st["waits_gave_up"] == 0, st
        lo = hi
    assert md5s == g["au_md5"][:splits[-1]]
    for l in range(L):
        assert md5(enc.layer_recon(l).tobytes()) == g["recon_md5"][l][splits[-1] - 1]
        assert np.array_equal(enc.layer_input(l), _clips(name)[l][splits[-1] - 1]), f"layer {l}: input of the last frame"
    assert enc.unpinned() == 0
    enc.close()


def test_encode_au_mixes_with_encode_layer():
    """Access unit 0 by encode_au, 1 by the layer calls (fed the layers numpy
    derives, which are what layer_input returns), 2 by encode_au: the bytes of
    the all-encode_layer stream."""
    name = NAMES[0]
    g = GOLD[name]
    L, w0, h0 = g["layers"], g["w0"], g["h0"]
    enc = _encoder(name)
    out = [md5(enc.encode_au(*_top(name, 0)).annexb())]
    for l in range(L):
        assert np.array_equal(enc.layer_input(l), _clips(name)[l][0])
    layers = _staged(_clips(name)[L - 1][1], w0 << (L - 1), h0 << (L - 1), L - 1)[::-1]
    au = b""
    for l in range(L):
        r = enc.encode_layer(l, *_planes(layers[l], w0 << l, h0 << l))
        if r.type & 2:
            au += r.hdr
        if l == L - 1:
            au += b"\x00\x00\x01" + r.data
    out.append(md5(au))
    out.append(md5(enc.encode_au(*_top(name, 2)).annexb()))
    assert out == g["au_md5"][:3]
    assert enc.unpinned() == 0
    enc.close()


def _refused(code, fn, *a):
    from hartallo_amd import HlAmdError

    with pytest.raises(HlAmdError) as ei:
        fn(*a)
    assert ei.value.code == code, ei.value


def test_refused_without_layers():
    import torch

    from hartallo_amd._lib import HL_AMD_ERROR_INVALID_STATE

    name = NAMES[0]
    g = GOLD[name]
    L, w0, h0 = g["layers"], g["w0"], g["h0"]
    enc = _encoder(name, layers=1)
    enc.layers = L  # (the sizes of the frame the calls below take)
    _refused(HL_AMD_ERROR_INVALID_STATE, enc.encode_au, *_top(name, 0))
    t = torch.from_numpy(_clips(name)[L - 1][0]).cuda()
    _refused(HL_AMD_ERROR_INVALID_STATE, enc.encode_aus_batch_device, [_device_ptrs(t, w0 << (L - 1), h0 << (L - 1))])
    for l in range(1, L):  # the encoder is as it was: the layers can still be added
        assert enc.lib.hl_amd_add_layer(enc._h, w0 << l, h0 << l) == 0
    assert md5(enc.encode_au(*_top(name, 0)).annexb()) == g["au_md5"][0]
    enc.close()


def test_refused_with_a_layer_range():
    import torch

    from hartallo_amd._lib import HL_AMD_ERROR_INVALID_STATE

    name = NAMES[0]
    g = GOLD[name]
    L, w0, h0 = g["layers"], g["w0"], g["h0"]
    enc = _encoder(name, first=1, last=L - 1)
    _refused(HL_AMD_ERROR_INVALID_STATE, enc.encode_au, *_top(name, 0))
    assert enc.lib.hl_amd_set_layer_range(enc._h, 0, L - 1) == 0  # refused before the stream started
    assert md5(enc.encode_au(*_top(name, 0)).annexb()) == g["au_md5"][0]
    enc.close()
    enc = _encoder(name, first=1, last=L - 1)
    t = torch.from_numpy(_clips(name)[L - 1][0]).cuda()
    _refused(HL_AMD_ERROR_INVALID_STATE, enc.encode_aus_batch_device, [_device_ptrs(t, w0 << (L - 1), h0 << (L - 1))])
    enc.close()


def test_refused_under_rate_control():
    import torch

    from hartallo_amd._lib import HL_AMD_ERROR_NOT_IMPLEMENTED

    name = NAMES[0]
    g = GOLD[name]
    L, w0, h0 = g["layers"], g["w0"], g["h0"]
    enc = _encoder(name)
    enc.set_rate_control(256000)
    _refused(HL_AMD_ERROR_NOT_IMPLEMENTED, enc.encode_au, *_top(name, 0))
    t = torch.from_numpy(_clips(name)[L - 1][0]).cuda()
    _refused(HL_AMD_ERROR_NOT_IMPLEMENTED, enc.encode_aus_batch_device, [_device_ptrs(t, w0 << (L - 1), h0 << (L - 1))])
    enc.set_rate_control(0)  # off again: nothing was coded
    assert md5(enc.encode_au(*_top(name, 0)).annexb()) == g["au_md5"][0]
    enc.close()


def test_refused_inside_an_access_unit():
    from hartallo_amd._lib import HL_AMD_ERROR_INVALID_STATE

    name = NAMES[0]
    g = GOLD[name]
    L, w0, h0 = g["layers"], g["w0"], g["h0"]
    enc = _encoder(name)
    r = enc.encode_layer(0, *_planes(_clips(name)[0][0], w0, h0))
    au = r.hdr if r.type & 2 else b""
    _refused(HL_AMD_ERROR_INVALID_STATE, enc.encode_au, *_top(name, 0))
    for l in range(1, L):  # the access unit goes on where it was
        r = enc.encode_layer(l, *_planes(_clips(name)[l][0], w0 << l, h0 << l))
        if r.type & 2:
            au += r.hdr
    assert md5(au + b"\x00\x00\x01" + r.data) == g["au_md5"][0]
    assert md5(enc.encode_au(*_top(name, 1)).annexb()) == g["au_md5"][1]
    enc.close()
