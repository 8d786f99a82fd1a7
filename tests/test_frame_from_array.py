"""hartallo_amd.Frame: the description (format, plane addresses, pitches) that
Frame.from_array and the I420 / NV12 constructors derive from numpy arrays and
CPU torch tensors -- contiguous, cropped views, channel-strided views -- and
what they refuse.  No GPU and no library call: the descriptor alone.
"""
import numpy as np
import pytest

import hartallo_amd
from hartallo_amd import Frame
from hartallo_amd import _lib as L


def sources():
    out = [("numpy", lambda a: a, lambda a: a.ctypes.data)]
    try:
        import torch

        out.append(("torch", lambda a: torch.from_numpy(a), lambda t: t.data_ptr()))
    except ImportError:
        pass
    return out


SOURCES = sources()


@pytest.mark.parametrize("kind", SOURCES, ids=[s[0] for s in SOURCES])
def test_contiguous(kind):
    _, wrap, addr = kind
    base = np.zeros((32, 48, 3), np.uint8)
    a = wrap(base)
    f = Frame.from_array(a)
    assert (f.format, f.planes, f.pitches[0], f.on_device, f.width, f.height) == (L.HL_AMD_FORMAT_RGB24, (addr(a),), 144, False, 48, 32)
    assert f.source is a
    f = Frame.from_array(wrap(np.zeros((32, 48, 4), np.uint8)))
    assert (f.format, f.pitches[0]) == (L.HL_AMD_FORMAT_RGBA32, 192)
    p = wrap(np.zeros((3, 32, 48), np.uint8))
    f = Frame.from_array(p)
    assert f.format == L.HL_AMD_FORMAT_RGBP
    assert f.planes == (addr(p), addr(p) + 32 * 48, addr(p) + 2 * 32 * 48) and f.pitches == (48, 48, 48)
    c = f._c()
    assert (c.format, c.on_device, c.plane[2], c.pitch[1]) == (L.HL_AMD_FORMAT_RGBP, 0, addr(p) + 2 * 32 * 48, 48)


@pytest.mark.parametrize("kind", SOURCES, ids=[s[0] for s in SOURCES])
def test_cropped_view(kind):
    _, wrap, addr = kind
    big = wrap(np.zeros((64, 80, 3), np.uint8))
    v = big[8:40, 16:64]
    f = Frame.from_array(v)
    assert (f.format, f.width, f.height) == (L.HL_AMD_FORMAT_RGB24, 48, 32)
    assert f.planes == (addr(big) + 8 * 240 + 16 * 3,) and f.pitches[0] == 240
    bigp = wrap(np.zeros((3, 64, 80), np.uint8))
    f = Frame.from_array(bigp[:, 8:40, 16:64])
    assert f.format == L.HL_AMD_FORMAT_RGBP and f.pitches == (80, 80, 80)
    assert f.planes == tuple(addr(bigp) + c * 64 * 80 + 8 * 80 + 16 for c in range(3))


@pytest.mark.parametrize("kind", SOURCES, ids=[s[0] for s in SOURCES])
def test_channel_strided_view(kind):
    """the planes of a (4, H, W) tensor taken with a step, and RGB out of a 5-plane stack"""
    _, wrap, addr = kind
    stack = wrap(np.zeros((5, 32, 48), np.uint8))
    f = Frame.from_array(stack[0:5:2])
    assert f.format == L.HL_AMD_FORMAT_RGBP
    assert f.planes == tuple(addr(stack) + 2 * c * 32 * 48 for c in range(3)) and f.pitches == (48, 48, 48)
    # a (H, W, 3) view of planar data is channel-strided too, but packed RGB cannot express it
    with pytest.raises(ValueError):
        Frame.from_array(wrap(np.zeros((3, 32, 48), np.uint8)).transpose(1, 2, 0) if kind[0] == "numpy"
                         else wrap(np.zeros((3, 32, 48), np.uint8)).permute(1, 2, 0))


@pytest.mark.parametrize("kind", SOURCES, ids=[s[0] for s in SOURCES])
def test_i420_and_nv12_constructors(kind):
    _, wrap, addr = kind
    yb, ub, vb = wrap(np.zeros((32, 72), np.uint8)), wrap(np.zeros((16, 36), np.uint8)), wrap(np.zeros((16, 36), np.uint8))
    y, u, v = yb[:, :48], ub[:, :24], vb[:, :24]
    f = Frame.i420(y, u, v)
    assert (f.format, f.planes, f.pitches) == (L.HL_AMD_FORMAT_I420, (addr(yb), addr(ub), addr(vb)), (72, 36, 36))
    cb = wrap(np.zeros((16, 56), np.uint8))
    f = Frame.nv12(y, cb[:, :48])
    assert (f.format, f.planes, f.pitches[:2], f.width, f.height) == (L.HL_AMD_FORMAT_NV12, (addr(yb), addr(cb)), (72, 56), 48, 32)
    with pytest.raises(ValueError):
        Frame.i420(y, u, v[:, :12])
    with pytest.raises(ValueError):
        Frame.nv12(y, cb[:, :24])


def test_refused_shapes():
    z = np.zeros
    for bad in (z((32, 48), np.uint8),                 # a single plane says nothing about its format
                z((32, 48, 2), np.uint8),              # two channels
                z((32, 48, 3), np.float32),            # not uint8
                z((32, 48, 3), np.uint8)[:, ::2],      # samples not dense
                z((32, 48, 3), np.uint8)[:, :, ::-1],  # BGR as a reversed view
                z((32, 48, 3), np.uint8)[::-1],        # negative pitch
                z((3, 32, 48), np.uint8)[:, :, ::2],   # planar, samples not dense
                z((3, 32, 48), np.uint8)[::-1],        # planes in falling order
                [[1, 2, 3]]):
        with pytest.raises(ValueError):
            Frame.from_array(bad)
    with pytest.raises(ValueError):
        Frame.from_array(z((32, 48, 3), np.uint8), format=L.HL_AMD_FORMAT_RGBA32)
    with pytest.raises(ValueError):
        Frame.from_array(z((32, 48, 3), np.uint8), format=L.HL_AMD_FORMAT_NV12)
    with pytest.raises(ValueError):
        Frame(7, (1,), (0,))
    with pytest.raises(ValueError):
        Frame(L.HL_AMD_FORMAT_NV12, (1,), (0,))
    assert "Frame" in hartallo_amd.__all__
