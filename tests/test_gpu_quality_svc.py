"""Per-picture quality of SVC layers on the GPU (hl_amd_set_quality on an
encoder with layers): with the feature on, the access units
are still the reference's (tests/golden/svc_golden.json), and every layer's
sums equal the numpy model (q_testlib) on the layer's input planes and its
reconstruction -- per layer call, per access unit from the top frame, and for
the layers batch, whose enhancement layers run on a stream of their own."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

from hartallo_amd import synth
from q_testlib import assert_quality, picture_quality

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "svc_golden.json")))
# without deblocking (k_quality follows k_svc_mb), deblocked, three layers
NAMES = ["svc2_qcif_qp36_nodb_gop2", "svc2_qcif_qp28_db", "svc3_64x48_qp30_gop3"]
INVALID_PARAMETER, INVALID_STATE = 1, 3

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


def _encoder(name, quality=True, **kw):
    from hartallo_amd import SvcEncoder

    g = GOLD[name]
    enc = SvcEncoder(g["w0"], g["h0"], g["layers"], g["qp"], g["me_range"], g["deblock"], g["gop"], g["early_term"], **kw)
    if quality:
        enc.set_quality(True)
    return enc


def _expect(code, fn, *a, **kw):
    from hartallo_amd import HlAmdError

    with pytest.raises(HlAmdError) as e:
        fn(*a, **kw)
    assert e.value.code == code, e.value


def _check_layers(enc, name, i, k, inputs, what):
    """Every layer of access unit i (slot k of the last call) against the model
    on (inputs[l], layer_recon(l)); returns the model's values per layer."""
    g = GOLD[name]
    out = []
    for l in range(g["layers"]):
        w, h = g["w0"] << l, g["h0"] << l
        rec = enc.layer_recon(l)
        assert md5(rec.tobytes()) == g["recon_md5"][l][i], f"{what} layer {l}: reconstruction differs from the reference's"
        want = picture_quality(inputs[l], rec, w, h)
        assert_quality(enc.last_quality(k, layer=l), enc.debug_quality_mb(k, layer=l), want, f"{what} layer {l}")
        out.append(want)
    return out


@functools.lru_cache(maxsize=None)
def _per_layer_calls(name):
    """The clip through encode_layer with the feature on, every layer of every
    access unit checked; returns the model's values [access unit][layer]."""
    g = GOLD[name]
    L = g["layers"]
    enc = _encoder(name)
    vals = []
    for i in range(g["frames"]):
        au = b""
        for l in range(L):
            r = enc.encode_layer(l, *_planes(_clips(name)[l][i], g["w0"] << l, g["h0"] << l))
            if r.type & 2:
                au += r.hdr
            if l == L - 1:
                au += b"\x00\x00\x01" + r.data
            elif l + 1 < L:
                _expect(INVALID_STATE, enc.last_quality, 0, layer=L - 1)  # not coded yet in this access unit
        assert md5(au) == g["au_md5"][i], f"{name} AU {i}"
        vals.append(_check_layers(enc, name, i, 0, [_clips(name)[l][i] for l in range(L)], f"{name} AU {i}"))
        _expect(INVALID_STATE, enc.last_quality, 1, layer=1)
        _expect(INVALID_PARAMETER, enc.last_quality, 0, layer=4)
    assert enc.unpinned() == 0
    enc.close()
    return vals


@pytest.mark.parametrize("name", NAMES)
def test_encode_layer(name):
    vals = _per_layer_calls(name)
    top = vals[-1][-1]
    assert top["sse"][0] > 0 and 0 < top["ssim_q30"][0] < top["windows"][0] << 30


@pytest.mark.parametrize("name", NAMES)
def test_encode_au(name):
    """The lower layers' input is derived on the GPU: the model's source is layer_input."""
    g = GOLD[name]
    L = g["layers"]
    enc = _encoder(name)
    for i in range(g["frames"]):
        r = enc.encode_au(*_planes(_clips(name)[L - 1][i], g["w0"] << (L - 1), g["h0"] << (L - 1)))
        assert md5(r.annexb()) == g["au_md5"][i], f"{name} AU {i}"
        inputs = [enc.layer_input(l) for l in range(L)]
        for l in range(L):
            assert np.array_equal(inputs[l], _clips(name)[l][i])
        got = _check_layers(enc, name, i, 0, inputs, f"{name} AU {i} (encode_au)")
        for l in range(L):  # ... and the layer calls' values: the same pictures
            assert all(got[l][f] == _per_layer_calls(name)[i][l][f] for f in ("sse", "ssim_q30")), (i, l)
    enc.close()


@pytest.mark.parametrize("fallback", [False, True], ids=["run", "fallback"])
@pytest.mark.parametrize("name", NAMES)
def test_encode_layers_batch(name, fallback, monkeypatch):
    """k = the access unit.  The base pictures against the model on
    debug_recon(k); the last access unit's enhancement layers against the model
    on layer_recon; every layer of every access unit against the values of the
    layer calls (the same pictures).  `fallback`: the base run is re-encoded
    picture by picture and the enhancement layers are coded a second time."""
    import torch

    g = GOLD[name]
    L, n = g["layers"], g["frames"]
    if fallback:
        monkeypatch.setenv("HL_AMD_FORCE_FALLBACK", "1")
    devs = [torch.from_numpy(_clips(name)[l]).cuda() for l in range(L)]

    def ptrs(l, i):
        s = (g["w0"] << l) * (g["h0"] << l)
        p = devs[l][i].data_ptr()
        return p, p + s, p + s + s // 4

    enc = _encoder(name)
    res = enc.encode_layers_batch_device([[ptrs(l, i) for i in range(n)] for l in range(L)])
    assert [md5(r.annexb()) for r in res] == g["au_md5"]
    assert (enc.last_batch_stats()["fallbacks"] > 0) == fallback
    want = _per_layer_calls(name)
    for i in range(n):
        base = picture_quality(_clips(name)[0][i], enc.debug_recon(i), g["w0"], g["h0"])
        assert_quality(enc.last_quality(i), enc.debug_quality_mb(i), base, f"{name} AU {i} base layer")
        for l in range(L):
            assert_quality(enc.last_quality(i, layer=l), enc.debug_quality_mb(i, layer=l), want[i][l], f"{name} AU {i} layer {l} (batch)")
    _check_layers(enc, name, n - 1, n - 1, [_clips(name)[l][n - 1] for l in range(L)], f"{name} last AU of the batch")
    _expect(INVALID_STATE, enc.last_quality, n, layer=1)
    # the feature off: the same access units, nothing measured
    off = _encoder(name, quality=False)
    res = off.encode_layers_batch_device([[ptrs(l, i) for i in range(n)] for l in range(L)])
    assert [md5(r.annexb()) for r in res] == g["au_md5"]
    for l in range(L):
        _expect(INVALID_STATE, off.last_quality, 0, layer=l)
    enc.close()
    off.close()


def test_layers_coded_elsewhere_and_unaligned_planes():
    import torch

    name = NAMES[0]
    g = GOLD[name]
    w, h = g["w0"] << 1, g["h0"] << 1
    # an encoder that codes layer 0 only: layer 1 reports INVALID_STATE
    enc = _encoder(name, first=0, last=0)
    enc.encode_layer(0, *_planes(_clips(name)[0][0], g["w0"], g["h0"]))
    assert enc.last_quality(0)["sse"][0] > 0
    _expect(INVALID_STATE, enc.last_quality, 0, layer=1)
    enc.close()
    # an enhancement-layer plane that is not 8-byte aligned is refused; the aligned one continues the access unit
    enc = _encoder(name)
    r = enc.encode_layer(0, *_planes(_clips(name)[0][0], g["w0"], g["h0"]))
    au = r.hdr
    buf = torch.zeros(w * h * 3 // 2 + 64, dtype=torch.uint8, device="cuda")
    buf[4:4 + w * h * 3 // 2] = torch.from_numpy(_clips(name)[1][0]).cuda()
    p = buf.data_ptr() + 4
    _expect(INVALID_PARAMETER, enc.encode_layer_device, 1, p, p + w * h, p + w * h * 5 // 4)
    r = enc.encode_layer(1, *_planes(_clips(name)[1][0], w, h))
    au += r.hdr + b"\x00\x00\x01" + r.data
    assert md5(au) == g["au_md5"][0]
    enc.close()
