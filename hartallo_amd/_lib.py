"""ctypes binding of libhartallo_amd.so (include/hartallo_amd.h).

The library is the HIP build for gfx950; there is no CPU fallback.  Loading
fails loudly when the library is missing, and encoding fails loudly when no
GPU is present.
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libhartallo_amd.so")

# include/hartallo_amd.h
HL_AMD_SUCCESS = 0
HL_AMD_ERROR_INVALID_PARAMETER = 1
HL_AMD_ERROR_INVALID_STATE = 3
HL_AMD_ERROR_INVALID_FORMAT = 4
HL_AMD_ERROR_NOT_FOUND = 6
HL_AMD_ERROR_NOT_IMPLEMENTED = 7
HL_AMD_ERROR_OUTOFMEMMORY = 8
HL_AMD_ERROR_OUTOFCAPACITY = 10
HL_AMD_ERROR_SYSTEM = 13
HL_AMD_ERROR_TOOSHORT = 15
HL_AMD_RESULT_TYPE_DATA = 1
HL_AMD_RESULT_TYPE_HDR = 2
# HL_AMD_ENCODING_* (= HL_VIDEO_ENCODING_TYPE_T, hl_types.h:262-274)
HL_AMD_ENCODING_AUTO = 0
HL_AMD_ENCODING_INTRA = 1
HL_AMD_ENCODING_INTER = 2
HL_AMD_ENCODING_LOSSLESS = 3
HL_AMD_ENCODING_RAW = 4
# HL_AMD_FORMAT_*, HL_AMD_MATRIX_*, HL_AMD_RANGE_* (hl_amd_frame_t, hl_amd_set_colour)
HL_AMD_FORMAT_I420 = 0
HL_AMD_FORMAT_NV12 = 1
HL_AMD_FORMAT_RGB24 = 2
HL_AMD_FORMAT_RGBA32 = 3
HL_AMD_FORMAT_RGBP = 4
HL_AMD_MATRIX_BT601 = 0
HL_AMD_MATRIX_BT709 = 1
HL_AMD_RANGE_LIMITED = 0
HL_AMD_RANGE_FULL = 1

# every symbol include/hartallo_amd.h declares
EXPORTED_SYMBOLS = (
    "hl_amd_encoder_create",
    "hl_amd_encoder_destroy",
    "hl_amd_encode",
    "hl_amd_set_lookahead",
    "hl_amd_flush",
    "hl_amd_encode_device",
    "hl_amd_encode_batch",
    "hl_amd_encode_streams",
    "hl_amd_encode_ex",
    "hl_amd_encode_device_ex",
    "hl_amd_encode_batch_ex",
    "hl_amd_encode_streams_ex",
    "hl_amd_set_pipeline",
    "hl_amd_set_rate_control",
    "hl_amd_set_max_ref_frame",
    "hl_amd_set_display_size",
    "hl_amd_get_display_size",
    "hl_amd_stream_headers",
    "hl_amd_last_qp",
    "hl_amd_pipeline_occupancy",
    "hl_amd_set_pipeline_build",
    "hl_amd_last_pipeline_build",
    "hl_amd_pipeline_build_choice",
    "hl_amd_pipeline_build_threshold",
    "hl_amd_bench_planes",
    "hl_amd_get_recon",
    "hl_amd_set_timing",
    "hl_amd_get_timing",
    "hl_amd_last_reruns",
    "hl_amd_last_chain_walks",
    "hl_amd_last_mb_launches",
    "hl_amd_last_batch_stats",
    "hl_amd_set_intra_helpers",
    "hl_amd_last_helper_stats",
    "hl_amd_last_fam3_stats",
    "hl_amd_profile_counters",
    "hl_amd_debug_records",
    "hl_amd_record_size",
    "hl_amd_debug_chain",
    "hl_amd_debug_recon",
    "hl_amd_add_layer",
    "hl_amd_encode_layer",
    "hl_amd_get_layer_recon",
    "hl_amd_svc_unpinned",
    "hl_amd_set_layer_range",
    "hl_amd_layer_state_bytes",
    "hl_amd_export_layer",
    "hl_amd_import_layer",
    "hl_amd_svc_layer_ms",
    "hl_amd_encode_layers_batch",
    "hl_amd_encode_au",
    "hl_amd_encode_aus_batch",
    "hl_amd_get_layer_input",
    "hl_amd_bench_pyramid",
    "hl_amd_set_scenecut",
    "hl_amd_scene_is_cut",
    "hl_amd_last_scene_stats",
    "hl_amd_debug_scene_mb",
    "hl_amd_bench_scene",
    "hl_amd_set_quality",
    "hl_amd_last_quality",
    "hl_amd_debug_quality_mb",
    "hl_amd_bench_quality",
    "hl_amd_psnr_db",
    "hl_amd_ssim_mean",
    "hl_amd_set_colour",
    "hl_amd_encode_frame",
    "hl_amd_encode_frames",
    "hl_amd_get_input",
    "hl_amd_bench_ingest",
    "hl_amd_set_source_size",
    "hl_amd_get_source_size",
    "hl_amd_scale_taps",
    "hl_amd_bench_scale",
    "hl_amd_encode_ladder_frame",
    "hl_amd_encode_ladder_frames",
    "hl_amd_bench_ladder",
    "hl_amd_set_au_display_size",
    "hl_amd_get_au_display_size",
    "hl_amd_svc_stream_headers",
    "hl_amd_encode_au_frame",
    "hl_amd_encode_au_frames",
    "hl_amd_version",
)


class HlAmdError(RuntimeError):
    def __init__(self, code: int, what: str):
        super().__init__(f"{what} failed with HL_ERROR {code}")
        self.code = code


class _Params(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("width", "height", "qp", "me_range", "deblock", "gop_size", "me_early_term", "device")]


class _Result(ctypes.Structure):
    _fields_ = [
        ("type", ctypes.c_int32),
        ("hdr", ctypes.c_void_p),
        ("hdr_size", ctypes.c_size_t),
        ("data", ctypes.c_void_p),
        ("data_size", ctypes.c_size_t),
    ]


class _FrameCtl(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("encoding", "me_range", "deblock", "me_early_term", "gop_size")]


@dataclass
class FrameCtl:
    """hl_amd_frame_ctl_t: what the reference reads on every encode call
    beside the planes -- hl_frame_t.encoding (HL_AMD_ENCODING_*) and the
    hl_codec_t settings at the time of the call, which stay until the next
    change (include/hartallo_amd.h)."""

    encoding: int = HL_AMD_ENCODING_AUTO
    me_range: int = 16
    deblock: int = 1
    me_early_term: int = 0
    gop_size: int = 30

    def _c(self) -> _FrameCtl:
        return _FrameCtl(self.encoding, self.me_range, self.deblock, self.me_early_term, self.gop_size)


def _ctl_array(ctls, n):
    """n FrameCtl objects as a C array (None: no ctl for the call)."""
    if ctls is None:
        return None
    if len(ctls) != n:
        raise HlAmdError(HL_AMD_ERROR_INVALID_PARAMETER, "ctl (one per frame)")
    return (_FrameCtl * n)(*[c._c() for c in ctls])


class _Frame(ctypes.Structure):
    _fields_ = [("format", ctypes.c_int32), ("on_device", ctypes.c_int32), ("plane", ctypes.c_void_p * 3), ("pitch", ctypes.c_int64 * 3)]


_FRAME_PLANES = {HL_AMD_FORMAT_I420: 3, HL_AMD_FORMAT_NV12: 2, HL_AMD_FORMAT_RGB24: 1, HL_AMD_FORMAT_RGBA32: 1, HL_AMD_FORMAT_RGBP: 3}


def _array_view(a):
    """(address, shape, strides in bytes, on_device) of a numpy uint8 array or
    of an object with data_ptr(), stride(), shape and is_cuda (a torch
    tensor); ValueError for anything else and for another element type."""
    if hasattr(a, "data_ptr") and hasattr(a, "stride") and hasattr(a, "is_cuda"):
        if getattr(a, "element_size", lambda: 1)() != 1 or "uint8" not in str(getattr(a, "dtype", "uint8")):
            raise ValueError("frames are uint8")
        return int(a.data_ptr()), tuple(int(d) for d in a.shape), tuple(int(x) for x in a.stride()), bool(a.is_cuda)
    import numpy as np

    if not isinstance(a, np.ndarray):
        raise ValueError("a numpy array or a tensor with data_ptr(), stride(), shape and is_cuda")
    if a.dtype != np.uint8:
        raise ValueError("frames are uint8")
    return int(a.ctypes.data), tuple(a.shape), tuple(int(x) for x in a.strides), False


def _plane_2d(a, width_bytes=None):
    """A plane of rows: (address, rows, row bytes, pitch, on_device); the
    samples of a row must be dense and the pitch positive."""
    ptr, shape, st, dev = _array_view(a)
    if len(shape) != 2 or st[1] != 1 or st[0] < shape[1]:
        raise ValueError("a plane is (rows, bytes) with dense rows and a pitch of at least the row")
    if width_bytes is not None and shape[1] != width_bytes:
        raise ValueError("plane width")
    return ptr, shape[0], shape[1], st[0], dev


@dataclass
class Frame:
    """hl_amd_frame_t: a frame by its format (HL_AMD_FORMAT_*), the addresses
    of its planes, the bytes between their rows (0 = dense) and whether the
    planes are in device memory.  `source` keeps what the addresses point into
    alive; width and height (when known) are checked against the encoder's."""

    format: int
    planes: tuple
    pitches: tuple = (0, 0, 0)
    on_device: bool = False
    source: object = None
    width: int = 0
    height: int = 0

    def __post_init__(self):
        if self.format not in _FRAME_PLANES:
            raise ValueError("format: one of HL_AMD_FORMAT_*")
        self.planes = tuple(int(p) for p in self.planes)
        self.pitches = tuple(int(p) for p in self.pitches)
        n = _FRAME_PLANES[self.format]
        if len(self.planes) < n or len(self.pitches) < n:
            raise ValueError(f"format {self.format} has {n} planes")

    def _c(self) -> _Frame:
        f = _Frame()
        f.format, f.on_device = self.format, 1 if self.on_device else 0
        for c in range(min(3, len(self.planes), len(self.pitches))):
            f.plane[c] = self.planes[c] or None
            f.pitch[c] = self.pitches[c]
        return f

    @classmethod
    def from_array(cls, a, format=None) -> "Frame":
        """An RGB frame from a numpy uint8 array or a uint8 tensor (anything
        with data_ptr(), stride(), shape and is_cuda), which may be a strided
        view: (H, W, 3) is RGB24 and (H, W, 4) RGBA32 -- dimensions 1 and 2
        dense, the pitch is stride 0 -- and (3, H, W) is RGBP with a pitch per
        channel from stride 1.  ValueError for what the descriptor cannot
        express."""
        ptr, shape, st, dev = _array_view(a)
        if len(shape) != 3:
            raise ValueError("(H, W, 3), (H, W, 4) or (3, H, W); I420 and NV12 have their own constructors")
        if format is None:
            if shape[2] in (3, 4) and shape[0] != 3:
                format = HL_AMD_FORMAT_RGB24 if shape[2] == 3 else HL_AMD_FORMAT_RGBA32
            elif shape[0] == 3:
                format = HL_AMD_FORMAT_RGBP
            else:
                raise ValueError("neither (H, W, 3 or 4) nor (3, H, W)")
        if format in (HL_AMD_FORMAT_RGB24, HL_AMD_FORMAT_RGBA32):
            ch = 3 if format == HL_AMD_FORMAT_RGB24 else 4
            h, w = shape[0], shape[1]
            if shape[2] != ch or st[2] != 1 or st[1] != ch or (h > 1 and st[0] < w * ch):
                raise ValueError("packed RGB needs dense samples and rows (strides (pitch, channels, 1))")
            return cls(format, (ptr,), (st[0] if h > 1 else 0,), dev, a, w, h)
        if format == HL_AMD_FORMAT_RGBP:
            h, w = shape[1], shape[2]
            if shape[0] != 3 or st[2] != 1 or (h > 1 and st[1] < w) or st[0] < 0:
                raise ValueError("planar RGB needs dense rows (strides (plane, pitch, 1))")
            return cls(format, tuple(ptr + c * st[0] for c in range(3)), (st[1] if h > 1 else 0,) * 3, dev, a, w, h)
        raise ValueError("from_array makes RGB frames; I420 and NV12 have their own constructors")

    @classmethod
    def i420(cls, y, u, v) -> "Frame":
        """Planar 4:2:0 from three (rows, samples) planes, each with its own pitch."""
        py, h, w, sy, dy = _plane_2d(y)
        pu, hu, wu, su, du = _plane_2d(u, w // 2)
        pv, hv, wv, sv, dv = _plane_2d(v, w // 2)
        if hu != h // 2 or hv != h // 2 or not dy == du == dv:
            raise ValueError("I420: chroma planes of half the size, all on the same side")
        return cls(HL_AMD_FORMAT_I420, (py, pu, pv), (sy, su, sv), dy, (y, u, v), w, h)

    @classmethod
    def nv12(cls, y, uv) -> "Frame":
        """NV12 from a (H, W) luma plane and a (H / 2, W) plane of U, V pairs."""
        py, h, w, sy, dy = _plane_2d(y)
        pc, hc, wc, sc, dc = _plane_2d(uv, w)
        if hc != h // 2 or dy != dc:
            raise ValueError("NV12: an interleaved chroma plane of half the rows, on the same side")
        return cls(HL_AMD_FORMAT_NV12, (py, pc), (sy, sc), dy, (y, uv), w, h)


def _mb_record_dtype():
    """numpy mirror of MbRecord (hartallo_amd/csrc/hl_types.h)."""
    import numpy as np

    return np.dtype([
        ("e_type", "<i4"), ("mb_type", "<i4"), ("flags", "<i4"), ("pm0", "<i4"),
        ("cbp", "<i4"), ("cbp_l", "<i4"), ("cbp_c", "<i4"), ("cbp_l4x4", "<i4"),
        ("cbp_cdc", "<i4", 2), ("cbp_cac", "<i4", 2), ("num_part", "<i4"), ("num_sub", "<i4", 4), ("sub_mb_type", "<i4", 4),
        ("chroma_mode", "<i4"), ("i16mode", "<i4"), ("mvd", "<i2", (4, 4, 2)), ("mv", "<i2", (4, 4, 2)),
        ("prev_flag", "i1", 16), ("rem_mode", "i1", 16), ("i4mode", "i1", 16), ("nc_luma", "i1", 16), ("nc_cac", "i1", (2, 4)),
        ("nc_dc", "i1"), ("pad0", "i1", 3), ("luma", "<i2", (16, 16)), ("i16dc", "<i2", 16), ("cdc", "<i2", (2, 4)),
        ("cac", "<i2", (2, 4, 16)), ("mad", "<i4"), ("pad1", "<i4"),
    ])


try:
    MB_RECORD = _mb_record_dtype()
except ImportError:  # numpy is optional for the plain ctypes binding
    MB_RECORD = None

_lib = None
LOADED_PATH = None  # the library file load_library loaded (bench.py stamps counters with its hash)


def code_sha256(path: str) -> str:
    """SHA-256 of a built library's code and constants: its .hip_fatbin (the
    gfx950 code objects), .text (the host code), .rodata and .data sections,
    in that order (a missing one counts as empty).  Two links of
    the same sources can lay out the ELF string tables differently (the whole
    file's hash then differs while every instruction is the same); counters
    recorded on one are valid for the other."""
    import hashlib
    import struct

    data = open(path, "rb").read()
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", data, 0x3A)
    secs = [struct.unpack_from("<IIQQQQ", data, shoff + i * shentsize) for i in range(shnum)]
    stroff = secs[shstrndx][4]

    def name(off):
        return data[stroff + off:data.index(b"\0", stroff + off)].decode()

    by = {name(sn): (o, sz) for sn, _, _, _, o, sz in secs}
    h = hashlib.sha256()
    for sec in (".hip_fatbin", ".text", ".rodata", ".data"):
        o, sz = by.get(sec, (0, 0))
        h.update(data[o:o + sz])
    return h.hexdigest()


class Quality(ctypes.Structure):
    """hl_amd_quality_t"""
    _fields_ = [("sse", ctypes.c_uint64 * 3), ("samples", ctypes.c_uint64 * 3), ("ssim_q30", ctypes.c_int64 * 3),
                ("windows", ctypes.c_uint64 * 3)]


def psnr_db(sse: int, samples: int) -> float:
    """10 log10(255^2 samples / sse); inf for sse = 0 (hl_amd_psnr_db)."""
    return load_library().hl_amd_psnr_db(sse, samples)


def ssim_mean(q30: int, windows: int) -> float:
    """q30 / 2^30 / windows (hl_amd_ssim_mean)."""
    return load_library().hl_amd_ssim_mean(q30, windows)


def stream_headers(width: int, height: int, qp: int = 28, max_ref_frame: int = 1, display_width: "int | None" = None,
                   display_height: "int | None" = None) -> bytes:
    """The SPS and PPS (with start codes) of an encoder of the coded size width
    x height after set_max_ref_frame(max_ref_frame) and set_display_size(
    display_width, display_height) -- None: the coded size, no cropping
    (hl_amd_stream_headers; no device).  ValueError for settings an encoder
    refuses."""
    p = _Params(width, height, qp, 16, 1, 30, 0, 0)
    buf = ctypes.create_string_buffer(256)
    n = load_library().hl_amd_stream_headers(ctypes.byref(p), max_ref_frame, width if display_width is None else display_width,
                                             height if display_height is None else display_height, buf, len(buf))
    if not n:
        raise ValueError("stream_headers: a size or setting the encoder refuses")
    return buf.raw[:n]


def scale_taps(s: int, d: int, j: int):
    """(first, weights) of output sample j of the area downscaler's axis s -> d
    (hl_amd_scale_taps; no device): the first source sample and the integer
    weights of it and its successors, which sum to s / gcd(s, d).  ValueError
    for what the scaler refuses: s < d, s > 8 d, s > 4096, j outside [0, d)."""
    first, w = ctypes.c_int32(), (ctypes.c_uint32 * 9)()
    n = load_library().hl_amd_scale_taps(s, d, j, ctypes.byref(first), w, 9)
    if n <= 0:
        raise ValueError("scale_taps: an axis or a sample the scaler refuses")
    return first.value, [int(x) for x in w[:n]]


def svc_stream_headers(width: int, height: int, layers: int, qp: int = 28, max_ref_frame: int = 1, display_width: "int | None" = None,
                       display_height: "int | None" = None) -> bytes:
    """Every header NAL unit (SPS 0, the subset SPSs, the PPSs, with start
    codes) of an SvcEncoder(width, height, layers) -- width x height is the
    base layer -- after set_max_ref_frame(max_ref_frame) and
    set_au_display_size(display_width, display_height) -- None: the top coded
    size, no cropping (hl_amd_svc_stream_headers; no device).  ValueError for
    settings an encoder refuses."""
    p = _Params(width, height, qp, 16, 1, 30, 0, 0)
    buf = ctypes.create_string_buffer(1024)
    k = layers - 1
    n = load_library().hl_amd_svc_stream_headers(ctypes.byref(p), max_ref_frame, layers, (width << k) if display_width is None else display_width,
                                                 (height << k) if display_height is None else display_height, buf, len(buf))
    if not n:
        raise ValueError("svc_stream_headers: a size or setting the encoder refuses")
    return buf.raw[:n]


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    """Loads the HIP library.  torch (if installed) is imported first so the
    process ends up with one HIP runtime (torch ships its own
    libamdhip64.so.7, which then also satisfies this library)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} is missing: build it with `make product` (hipcc --offload-arch=gfx950)")
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(path)
    global LOADED_PATH
    LOADED_PATH = os.path.abspath(path)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.hl_amd_encoder_create.argtypes = [ctypes.POINTER(_Params), ctypes.POINTER(vp)]
    lib.hl_amd_encoder_create.restype = i32
    lib.hl_amd_encoder_destroy.argtypes = [vp]
    lib.hl_amd_encoder_destroy.restype = None
    for f in (lib.hl_amd_encode, lib.hl_amd_encode_device):
        f.argtypes = [vp, vp, vp, vp, ctypes.POINTER(_Result)]
        f.restype = i32
    pp = ctypes.POINTER(ctypes.c_void_p)
    lib.hl_amd_encode_batch.argtypes = [vp, i32, pp, pp, pp, ctypes.POINTER(_Result)]
    lib.hl_amd_encode_batch.restype = i32
    if hasattr(lib, "hl_amd_encode_streams"):  # (absent from builds before round 4 loaded through HL_LIB)
        lib.hl_amd_encode_streams.argtypes = [ctypes.POINTER(vp), i32, i32, pp, pp, pp, ctypes.POINTER(_Result)]
        lib.hl_amd_encode_streams.restype = i32
    pc = ctypes.POINTER(_FrameCtl)
    for f in (lib.hl_amd_encode_ex, lib.hl_amd_encode_device_ex):
        f.argtypes = [vp, vp, vp, vp, pc, ctypes.POINTER(_Result)]
        f.restype = i32
    lib.hl_amd_encode_batch_ex.argtypes = [vp, i32, pp, pp, pp, pc, ctypes.POINTER(_Result)]
    lib.hl_amd_encode_batch_ex.restype = i32
    lib.hl_amd_encode_streams_ex.argtypes = [ctypes.POINTER(vp), i32, i32, pp, pp, pp, pc, ctypes.POINTER(_Result)]
    lib.hl_amd_encode_streams_ex.restype = i32
    lib.hl_amd_set_pipeline.argtypes = [vp, i32, i32, i32]
    lib.hl_amd_set_pipeline.restype = i32
    lib.hl_amd_set_rate_control.argtypes = [vp, ctypes.c_int64, i32, i32, i32, i32, i32]
    lib.hl_amd_set_rate_control.restype = i32
    if hasattr(lib, "hl_amd_set_max_ref_frame"):  # (absent from builds before round 5 loaded through HL_LIB)
        lib.hl_amd_set_max_ref_frame.argtypes = [vp, i32]
        lib.hl_amd_set_max_ref_frame.restype = i32
    if hasattr(lib, "hl_amd_set_display_size"):  # (absent from builds before the display size loaded through HL_LIB)
        lib.hl_amd_set_display_size.argtypes = [vp, i32, i32]
        lib.hl_amd_set_display_size.restype = i32
        lib.hl_amd_get_display_size.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]
        lib.hl_amd_get_display_size.restype = i32
        lib.hl_amd_stream_headers.argtypes = [ctypes.POINTER(_Params), i32, i32, i32, vp, ctypes.c_size_t]
        lib.hl_amd_stream_headers.restype = ctypes.c_size_t
    lib.hl_amd_last_qp.argtypes = [vp]
    lib.hl_amd_last_qp.restype = i32
    lib.hl_amd_pipeline_occupancy.argtypes = []
    lib.hl_amd_pipeline_occupancy.restype = i32
    for name, args in (("hl_amd_set_pipeline_build", [vp, i32]), ("hl_amd_last_pipeline_build", [vp]),
                       ("hl_amd_pipeline_build_choice", [i32, i32, i32]), ("hl_amd_pipeline_build_threshold", [])):
        if hasattr(lib, name):  # (absent from builds before round 10 loaded through HL_LIB)
            getattr(lib, name).argtypes = args
            getattr(lib, name).restype = i32
    lib.hl_amd_bench_planes.argtypes = [vp, i32, ctypes.POINTER(ctypes.c_float)]
    lib.hl_amd_bench_planes.restype = i32
    lib.hl_amd_get_recon.argtypes = [vp, vp, vp, vp]
    lib.hl_amd_get_recon.restype = i32
    lib.hl_amd_set_timing.argtypes = [vp, i32]
    lib.hl_amd_set_timing.restype = i32
    lib.hl_amd_get_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    lib.hl_amd_get_timing.restype = i32
    lib.hl_amd_last_reruns.argtypes = [vp]
    lib.hl_amd_last_reruns.restype = i32
    lib.hl_amd_last_chain_walks.argtypes = [vp]
    lib.hl_amd_last_chain_walks.restype = i32
    lib.hl_amd_last_mb_launches.argtypes = [vp]
    lib.hl_amd_last_mb_launches.restype = i32
    lib.hl_amd_last_batch_stats.argtypes = [vp, ctypes.POINTER(i32)]
    lib.hl_amd_last_batch_stats.restype = i32
    for name, args in (("hl_amd_set_intra_helpers", [vp, i32]), ("hl_amd_last_helper_stats", [vp, ctypes.POINTER(i32)]),
                       ("hl_amd_last_fam3_stats", [vp, ctypes.POINTER(i32)]), ("hl_amd_set_lookahead", [vp, i32]),
                       ("hl_amd_flush", [vp, ctypes.POINTER(_Result)])):
        if hasattr(lib, name):  # (absent from builds before round 4 loaded through HL_LIB)
            getattr(lib, name).argtypes = args
            getattr(lib, name).restype = i32
    lib.hl_amd_profile_counters.argtypes = [vp, ctypes.POINTER(ctypes.c_ulonglong), i32]
    lib.hl_amd_profile_counters.restype = i32
    # diagnostics entry points (absent from older builds loaded through HL_LIB)
    for name, args in (("hl_amd_debug_records", [vp, i32, vp, ctypes.c_size_t]), ("hl_amd_debug_chain", [vp, i32, vp, ctypes.c_size_t]),
                       ("hl_amd_debug_recon", [vp, i32, vp, vp, vp]), ("hl_amd_record_size", [])):
        if hasattr(lib, name):
            getattr(lib, name).argtypes = args
            getattr(lib, name).restype = i32
    lib.hl_amd_add_layer.argtypes = [vp, i32, i32]
    lib.hl_amd_add_layer.restype = i32
    lib.hl_amd_encode_layer.argtypes = [vp, i32, i32, vp, vp, vp, i32, ctypes.POINTER(_Result)]
    lib.hl_amd_encode_layer.restype = i32
    lib.hl_amd_get_layer_recon.argtypes = [vp, i32, vp, vp, vp]
    lib.hl_amd_get_layer_recon.restype = i32
    lib.hl_amd_svc_unpinned.argtypes = [vp]
    lib.hl_amd_svc_unpinned.restype = i32
    lib.hl_amd_set_layer_range.argtypes = [vp, i32, i32]
    lib.hl_amd_set_layer_range.restype = i32
    lib.hl_amd_layer_state_bytes.argtypes = [vp, i32]
    lib.hl_amd_layer_state_bytes.restype = ctypes.c_size_t
    lib.hl_amd_export_layer.argtypes = [vp, i32, vp]
    lib.hl_amd_export_layer.restype = i32
    lib.hl_amd_import_layer.argtypes = [vp, i32, vp]
    lib.hl_amd_import_layer.restype = i32
    lib.hl_amd_encode_layers_batch.argtypes = [vp, i32, i32, pp, ctypes.POINTER(_Result)]
    lib.hl_amd_encode_layers_batch.restype = i32
    for name, args in (("hl_amd_encode_au", [vp, vp, vp, vp, i32, ctypes.POINTER(_Result)]),
                       ("hl_amd_encode_aus_batch", [vp, i32, pp, ctypes.POINTER(_Result)]),
                       ("hl_amd_get_layer_input", [vp, i32, vp, vp, vp]),
                       ("hl_amd_bench_pyramid", [vp, i32, ctypes.POINTER(ctypes.c_float)])):
        if hasattr(lib, name):  # (absent from builds before the layer pyramid loaded through HL_LIB)
            getattr(lib, name).argtypes = args
            getattr(lib, name).restype = i32
    u64 = ctypes.c_uint64
    for name, args in (("hl_amd_set_scenecut", [vp, i32, i32, i32]), ("hl_amd_scene_is_cut", [u64, u64, i32]),
                       ("hl_amd_last_scene_stats", [vp, i32, ctypes.POINTER(u64)]),
                       ("hl_amd_debug_scene_mb", [vp, i32, vp, vp, ctypes.c_size_t]),
                       ("hl_amd_bench_scene", [vp, i32, ctypes.POINTER(ctypes.c_float)])):
        if hasattr(lib, name):  # (absent from builds before scene-cut detection loaded through HL_LIB)
            getattr(lib, name).argtypes = args
            getattr(lib, name).restype = i32
    for name, args in (("hl_amd_set_quality", [vp, i32]), ("hl_amd_last_quality", [vp, i32, i32, ctypes.POINTER(Quality)]),
                       ("hl_amd_debug_quality_mb", [vp, i32, i32, vp, ctypes.c_size_t]),
                       ("hl_amd_bench_quality", [vp, i32, ctypes.POINTER(ctypes.c_float)])):
        if hasattr(lib, name):  # (absent from builds before the quality metric loaded through HL_LIB)
            getattr(lib, name).argtypes = args
            getattr(lib, name).restype = i32
    for name, args in (("hl_amd_psnr_db", [u64, u64]), ("hl_amd_ssim_mean", [ctypes.c_int64, u64])):
        if hasattr(lib, name):
            getattr(lib, name).argtypes = args
            getattr(lib, name).restype = ctypes.c_double
    pf = ctypes.POINTER(_Frame)
    for name, args in (("hl_amd_set_colour", [vp, i32, i32]), ("hl_amd_encode_frame", [vp, pf, pc, ctypes.POINTER(_Result)]),
                       ("hl_amd_encode_frames", [vp, i32, pf, pc, ctypes.POINTER(_Result)]),
                       ("hl_amd_get_input", [vp, i32, vp, vp, vp]), ("hl_amd_bench_ingest", [vp, i32, ctypes.POINTER(ctypes.c_float)])):
        if hasattr(lib, name):  # (absent from builds before the frame ingest loaded through HL_LIB)
            getattr(lib, name).argtypes = args
            getattr(lib, name).restype = i32
    for name, args in (("hl_amd_set_au_display_size", [vp, i32, i32]),
                       ("hl_amd_get_au_display_size", [vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]),
                       ("hl_amd_encode_au_frame", [vp, pf, ctypes.POINTER(_Result)]),
                       ("hl_amd_encode_au_frames", [vp, i32, pf, ctypes.POINTER(_Result)])):
        if hasattr(lib, name):  # (absent from builds before the access unit's display size loaded through HL_LIB)
            getattr(lib, name).argtypes = args
            getattr(lib, name).restype = i32
    for name, args in (("hl_amd_set_source_size", [vp, i32, i32]),
                       ("hl_amd_get_source_size", [vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]),
                       ("hl_amd_scale_taps", [i32, i32, i32, ctypes.POINTER(i32), ctypes.POINTER(ctypes.c_uint32), i32]),
                       ("hl_amd_bench_scale", [vp, i32, ctypes.POINTER(ctypes.c_float)])):
        if hasattr(lib, name):  # (absent from builds before the source size loaded through HL_LIB)
            getattr(lib, name).argtypes = args
            getattr(lib, name).restype = i32
    pvp = ctypes.POINTER(ctypes.c_void_p)
    for name, args in (("hl_amd_encode_ladder_frame", [pvp, i32, pf, pc, ctypes.POINTER(_Result)]),
                       ("hl_amd_encode_ladder_frames", [pvp, i32, i32, pf, pc, ctypes.POINTER(_Result)]),
                       ("hl_amd_bench_ladder", [vp, i32, ctypes.POINTER(ctypes.c_float)])):
        if hasattr(lib, name):  # (absent from builds before the rendition ladder loaded through HL_LIB)
            getattr(lib, name).argtypes = args
            getattr(lib, name).restype = i32
    if hasattr(lib, "hl_amd_svc_stream_headers"):
        lib.hl_amd_svc_stream_headers.argtypes = [ctypes.POINTER(_Params), i32, i32, i32, i32, vp, ctypes.c_size_t]
        lib.hl_amd_svc_stream_headers.restype = ctypes.c_size_t
    lib.hl_amd_svc_layer_ms.argtypes = [vp]
    lib.hl_amd_svc_layer_ms.restype = ctypes.c_float
    lib.hl_amd_version.argtypes = []
    lib.hl_amd_version.restype = ctypes.c_char_p
    _lib = lib
    return lib


@dataclass
class EncodeResult:
    """hl_codec_result_t of one encode() call (hl_codec.h:152-168)."""

    type: int
    data: bytes
    hdr: bytes

    def annexb(self) -> bytes:
        """Bytes the reference's test harness writes for this frame
        (test_encoder.c:220-236): headers when signalled, then a start code
        and the slice NAL."""
        out = self.hdr if self.type & HL_AMD_RESULT_TYPE_HDR else b""
        return out + b"\x00\x00\x01" + self.data


class Encoder:
    """One H.264 encode stream on one GPU (one hl_codec_t, not reentrant)."""

    def __init__(self, width: int, height: int, qp: int = 28, me_range: int = 16, deblock: int = 1, gop_size: int = 30,
                 me_early_term: int = 0, device: int = 0):
        self.lib = load_library()
        self.width, self.height = width, height
        p = _Params(width, height, qp, me_range, deblock, gop_size, me_early_term, device)
        h = ctypes.c_void_p()
        rc = self.lib.hl_amd_encoder_create(ctypes.byref(p), ctypes.byref(h))
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_encoder_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self.lib.hl_amd_encoder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _result(self, r: _Result) -> EncodeResult:
        data = ctypes.string_at(r.data, r.data_size) if r.type & HL_AMD_RESULT_TYPE_DATA else b""
        hdr = ctypes.string_at(r.hdr, r.hdr_size) if r.type & HL_AMD_RESULT_TYPE_HDR else b""
        return EncodeResult(r.type, data, hdr)

    def encode(self, y, u, v, ctl: "FrameCtl | None" = None) -> EncodeResult:
        """Encodes planar YUV420 from host memory (numpy uint8 arrays); ctl:
        the frame's encoding type and the settings from this frame on
        (hl_amd_encode_ex)."""
        import numpy as np

        ys = [np.ascontiguousarray(p, dtype=np.uint8) for p in (y, u, v)]
        if ys[0].size != self.width * self.height or ys[1].size != self.width * self.height // 4 or ys[2].size != ys[1].size:
            raise HlAmdError(HL_AMD_ERROR_INVALID_FORMAT, "encode (plane sizes)")
        r = _Result()
        if ctl is None:
            rc = self.lib.hl_amd_encode(self._h, ys[0].ctypes.data, ys[1].ctypes.data, ys[2].ctypes.data, ctypes.byref(r))
        else:
            rc = self.lib.hl_amd_encode_ex(self._h, ys[0].ctypes.data, ys[1].ctypes.data, ys[2].ctypes.data, ctypes.byref(ctl._c()),
                                           ctypes.byref(r))
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_encode" if ctl is None else "hl_amd_encode_ex")
        return self._result(r)

    def set_lookahead(self, frames: int) -> None:
        """Look-ahead for per-frame callers (hl_amd_set_lookahead): encode()
        queues frames and codes them `frames` at a time; each call returns the
        next coded result in order (type 0 while the queue fills), flush()
        the rest."""
        rc = self.lib.hl_amd_set_lookahead(self._h, frames)
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_set_lookahead")

    def flush(self) -> EncodeResult:
        """Codes what the look-ahead still queues and returns the next
        result (type 0 once none is left)."""
        r = _Result()
        rc = self.lib.hl_amd_flush(self._h, ctypes.byref(r))
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_flush")
        return self._result(r)

    def encode_device(self, y_ptr: int, u_ptr: int, v_ptr: int, collect: bool = True, ctl: "FrameCtl | None" = None):
        """Encodes planes already resident in device memory (raw pointers);
        ctl as in encode (hl_amd_encode_device_ex)."""
        r = _Result()
        planes = (ctypes.c_void_p(y_ptr), ctypes.c_void_p(u_ptr), ctypes.c_void_p(v_ptr))
        if ctl is None:
            rc = self.lib.hl_amd_encode_device(self._h, *planes, ctypes.byref(r))
        else:
            rc = self.lib.hl_amd_encode_device_ex(self._h, *planes, ctypes.byref(ctl._c()), ctypes.byref(r))
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_encode_device" if ctl is None else "hl_amd_encode_device_ex")
        return self._result(r) if collect else r.data_size

    def encode_batch_device(self, ptrs, collect: bool = True, ctl=None):
        """Encodes consecutive frames already resident in device memory;
        ptrs = [(y_ptr, u_ptr, v_ptr), ...].  Runs of P pictures are
        frame-pipelined (hl_amd_encode_batch); returns one result per frame
        (or, with collect=False, the total bitstream bytes).  ctl: one
        FrameCtl per frame (hl_amd_encode_batch_ex); a forced IDR or a
        changed setting stays inside the pipelined run."""
        n = len(ptrs)
        arr = [(ctypes.c_void_p * n)(*[p[i] for p in ptrs]) for i in range(3)]
        res = (_Result * n)()
        if ctl is None:
            rc = self.lib.hl_amd_encode_batch(self._h, n, arr[0], arr[1], arr[2], res)
        else:
            rc = self.lib.hl_amd_encode_batch_ex(self._h, n, arr[0], arr[1], arr[2], _ctl_array(ctl, n), res)
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_encode_batch" if ctl is None else "hl_amd_encode_batch_ex")
        self._last_batch = res  # the results stay valid until the next encode call
        return [self._result(r) for r in res] if collect else sum(r.data_size for r in res)

    @staticmethod
    def encode_streams_device(encoders, ptrs, collect: bool = True, ctl=None):
        """hl_amd_encode_streams: frames of several streams in shared
        pipelined runs; encoders[s] codes ptrs[s] (each a list of (y, u, v)
        device pointers, the same length).  Returns per stream its results (or,
        with collect=False, its total bitstream bytes).  ctl: per stream a
        list of one FrameCtl per frame (hl_amd_encode_streams_ex)."""
        S, n = len(encoders), len(ptrs[0])
        assert len(ptrs) == S and all(len(p) == n for p in ptrs)
        lib = encoders[0].lib
        hs = (ctypes.c_void_p * S)(*[e._h for e in encoders])
        flat = [f for p in ptrs for f in p]
        arr = [(ctypes.c_void_p * (S * n))(*[f[i] for f in flat]) for i in range(3)]
        res = (_Result * (S * n))()
        if ctl is None:
            rc = lib.hl_amd_encode_streams(hs, S, n, arr[0], arr[1], arr[2], res)
        else:
            if len(ctl) != S:
                raise HlAmdError(HL_AMD_ERROR_INVALID_PARAMETER, "ctl (one list per stream)")
            for c in ctl:
                _ctl_array(c, n)  # (one per frame)
            rc = lib.hl_amd_encode_streams_ex(hs, S, n, arr[0], arr[1], arr[2], _ctl_array([c for cs in ctl for c in cs], S * n), res)
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_encode_streams" if ctl is None else "hl_amd_encode_streams_ex")
        out = []
        for s, e in enumerate(encoders):
            rs = res[s * n:(s + 1) * n]
            e._last_batch = rs
            out.append([e._result(r) for r in rs] if collect else sum(r.data_size for r in rs))
        return out

    def last_batch_results(self):
        """The results of the last encode_batch_device call (also after
        collect=False), valid until the next encode call."""
        return [self._result(r) for r in self._last_batch]

    def set_rate_control(self, bitrate: int, fps_num: int = 1, fps_den: int = 15, basicunit: int = -1, qp_min: int = -1,
                         qp_max: int = -1):
        """Rate control (hl_codec_t.rc_bitrate > 0 and its companions; call
        before the first frame; bitrate <= 0 turns it off)."""
        rc = self.lib.hl_amd_set_rate_control(self._h, bitrate, fps_num, fps_den, basicunit, qp_min, qp_max)
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_set_rate_control")

    def set_max_ref_frame(self, max_ref_frame: int):
        """hl_codec_t.max_ref_frame: SPS/PPS fields only (hl_codec_264_sps.c:620-636); before the first frame."""
        rc = self.lib.hl_amd_set_max_ref_frame(self._h, max_ref_frame)
        if rc:
            raise HlAmdError(rc, "hl_amd_set_max_ref_frame")

    def set_display_size(self, width: int, height: int) -> None:
        """The size a decoder shows (hl_amd_set_display_size): even, within the
        last macroblock column and row of the coded size the encoder was
        created with.  The SPS then carries the cropping offsets, encode_frame
        and encode_frames_device take frames of this size and pad them on the
        GPU by edge replication, and quality covers the display rectangle;
        encode, encode_device and encode_batch_device keep taking planes of the
        coded size.  Before the first frame."""
        rc = self.lib.hl_amd_set_display_size(self._h, width, height)
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_set_display_size")
        w, h = ctypes.c_int32(), ctypes.c_int32()
        rc = self.lib.hl_amd_get_display_size(self._h, ctypes.byref(w), ctypes.byref(h))
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_get_display_size")
        self._display = (w.value, h.value)

    @property
    def display_size(self):
        """(width, height) a decoder shows: the coded size unless set_display_size set another."""
        return getattr(self, "_display", None) or (self.width, self.height)

    def last_qp(self) -> int:
        """SliceQPY of the last encoded picture."""
        return self.lib.hl_amd_last_qp(self._h)

    def set_scenecut(self, threshold: int, min_gap: int = 1, range: int = 8) -> None:
        """Scene-cut detection (hl_amd_set_scenecut): every input frame is
        compared with the one before it on the GPU, and a cut -- 256 P >=
        threshold I, at least min_gap pictures after the last IDR, encoding
        AUTO -- is coded as if the caller had forced an IDR.  threshold 0: off
        (the default); range: the search range in samples, 0..16."""
        rc = self.lib.hl_amd_set_scenecut(self._h, threshold, min_gap, range)
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_set_scenecut")

    def last_scene_stats(self, k: int) -> dict:
        """Picture k of the last encode call (hl_amd_last_scene_stats): P, I,
        whether it was analysed and whether the detector turned it into an
        IDR."""
        a = (ctypes.c_uint64 * 4)()
        rc = self.lib.hl_amd_last_scene_stats(self._h, k, a)
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_last_scene_stats")
        return {"P": int(a[0]), "I": int(a[1]), "analysed": bool(a[2]), "turned": bool(a[3])}

    def debug_scene_mb(self, k: int):
        """(inter, intra) of every macroblock of picture k of the last encode
        call, uint32 arrays of shape (mbh, mbw) (hl_amd_debug_scene_mb)."""
        import numpy as np

        mbh, mbw = self.height // 16, self.width // 16
        inter, intra = np.zeros((mbh, mbw), np.uint32), np.zeros((mbh, mbw), np.uint32)
        rc = self.lib.hl_amd_debug_scene_mb(self._h, k, inter.ctypes.data, intra.ctypes.data, mbh * mbw)
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_debug_scene_mb")
        return inter, intra

    def bench_scene(self, iters: int = 50) -> float:
        """average ms of the scene analysis launch of the last encode call,
        whose frames must still be there (diagnostics)"""
        ms = ctypes.c_float()
        rc = self.lib.hl_amd_bench_scene(self._h, iters, ctypes.byref(ms))
        if rc:
            raise HlAmdError(rc, "hl_amd_bench_scene")
        return ms.value

    def set_quality(self, on: bool = True) -> None:
        """Per-picture quality (hl_amd_set_quality): every coded picture is
        compared on the GPU with the planes it was coded from.  Off by
        default; it changes no byte of the stream."""
        rc = self.lib.hl_amd_set_quality(self._h, 1 if on else 0)
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_set_quality")

    def last_quality(self, k: int, layer: int = 0) -> dict:
        """Picture k (of layer `layer`) of the last encode call
        (hl_amd_last_quality): the integers sse, samples, ssim_q30, windows as
        lists over Y, U, V, plus psnr_y/u/v (dB) and ssim_y/u/v."""
        q = Quality()
        rc = self.lib.hl_amd_last_quality(self._h, layer, k, ctypes.byref(q))
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_last_quality")
        out = {f: [int(x) for x in getattr(q, f)] for f in ("sse", "samples", "ssim_q30", "windows")}
        for c, name in enumerate("yuv"):
            out["psnr_" + name] = self.lib.hl_amd_psnr_db(out["sse"][c], out["samples"][c])
            out["ssim_" + name] = self.lib.hl_amd_ssim_mean(out["ssim_q30"][c], out["windows"][c])
        return out

    def debug_quality_mb(self, k: int, layer: int = 0):
        """sum (source - reconstruction)^2 of every luma macroblock of that
        picture, a uint32 array of shape (mbh, mbw) (hl_amd_debug_quality_mb)."""
        import numpy as np

        mbh, mbw = (self.height << layer) // 16, (self.width << layer) // 16
        out = np.zeros((mbh, mbw), np.uint32)
        rc = self.lib.hl_amd_debug_quality_mb(self._h, layer, k, out.ctypes.data, mbh * mbw)
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_debug_quality_mb")
        return out

    def bench_quality(self, iters: int = 50) -> float:
        """average ms of the last measurement launch of the AVC path, whose
        planes must still be there; drops the last call's results (diagnostics)"""
        ms = ctypes.c_float()
        rc = self.lib.hl_amd_bench_quality(self._h, iters, ctypes.byref(ms))
        if rc:
            raise HlAmdError(rc, "hl_amd_bench_quality")
        return ms.value

    def set_colour(self, matrix: int = HL_AMD_MATRIX_BT601, range: int = HL_AMD_RANGE_LIMITED) -> None:
        """The matrix and range RGB frames are converted with from now on
        (hl_amd_set_colour); the default is BT.601 limited."""
        rc = self.lib.hl_amd_set_colour(self._h, matrix, range)
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_set_colour")

    def set_source_size(self, width: int, height: int) -> None:
        """The size of the frames encode_frame and encode_frames_device take
        from now on (hl_amd_set_source_size): even, between the display size
        and min(8 x it, 4096) on each axis.  The frames are scaled to the
        display size on the GPU by an exact integer area filter (2:1 is the SVC
        layers' 2x2 box) and then coded as frames of that size; the display
        size itself turns scaling off.  Between any two calls: a source may
        change its resolution mid-stream.  Set the display size first."""
        rc = self.lib.hl_amd_set_source_size(self._h, width, height)
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_set_source_size")
        w, h = ctypes.c_int32(), ctypes.c_int32()
        rc = self.lib.hl_amd_get_source_size(self._h, ctypes.byref(w), ctypes.byref(h))
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_get_source_size")
        self._source = (w.value, h.value) if (w.value, h.value) != self.display_size else None

    @property
    def source_size(self):
        """(width, height) of the frames the frame calls take: the display size unless set_source_size set another."""
        return getattr(self, "_source", None) or self.display_size

    def bench_scale(self, iters: int = 50) -> float:
        """average ms of the k_scale launch(es) of the last frame call, whose
        intermediate planes are the encoder's (diagnostics)"""
        ms = ctypes.c_float()
        rc = self.lib.hl_amd_bench_scale(self._h, iters, ctypes.byref(ms))
        if rc:
            raise HlAmdError(rc, "hl_amd_bench_scale")
        return ms.value

    @staticmethod
    def _ladder_ctl(ctl, count, n):
        """per rung a list of n FrameCtl objects -> the call's C array, ctl[r * n + i]"""
        if ctl is None:
            return None
        if len(ctl) != count:
            raise HlAmdError(HL_AMD_ERROR_INVALID_PARAMETER, "ctl (one list per rung)")
        for c in ctl:
            _ctl_array(c, n)  # (one per frame)
        return _ctl_array([c for cs in ctl for c in cs], count * n)

    @staticmethod
    def encode_ladder_frame(encoders, frame: "Frame", ctl=None):
        """One frame of the encoders' common source size, converted once and
        scaled for every encoder (a "rung") by one GPU launch, then coded by
        each as encode_frame codes it (hl_amd_encode_ladder_frame).  ctl: one
        FrameCtl per rung.  Returns one EncodeResult per rung."""
        count = len(encoders)
        if count and frame.width and any((frame.width, frame.height) != e.source_size for e in encoders):
            raise HlAmdError(HL_AMD_ERROR_INVALID_FORMAT, "frame (picture size)")
        lib = encoders[0].lib if count else load_library()
        hs = (ctypes.c_void_p * max(count, 1))(*[e._h for e in encoders])
        res = (_Result * max(count, 1))()
        c = frame._c()
        rc = lib.hl_amd_encode_ladder_frame(hs, count, ctypes.byref(c), Encoder._ladder_ctl([[x] for x in ctl] if ctl is not None else None, count, 1), res)
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_encode_ladder_frame")
        return [e._result(res[r]) for r, e in enumerate(encoders)]

    @staticmethod
    def encode_ladder_frames_device(encoders, frames, ctl=None, collect: bool = True):
        """Consecutive device frames of the encoders' common source size,
        converted once and scaled for every rung by one GPU launch, then coded
        rung after rung as encode_frames_device codes them
        (hl_amd_encode_ladder_frames).  ctl: per rung a list of one FrameCtl
        per frame.  Returns per rung its results (or, with collect=False, its
        total bitstream bytes)."""
        count, n = len(encoders), len(frames)
        for f in frames:
            if count and f.width and any((f.width, f.height) != e.source_size for e in encoders):
                raise HlAmdError(HL_AMD_ERROR_INVALID_FORMAT, "frame (picture size)")
        lib = encoders[0].lib if count else load_library()
        hs = (ctypes.c_void_p * max(count, 1))(*[e._h for e in encoders])
        arr = (_Frame * max(n, 1))(*[f._c() for f in frames])
        res = (_Result * max(count * n, 1))()
        rc = lib.hl_amd_encode_ladder_frames(hs, count, n, arr, Encoder._ladder_ctl(ctl, count, n), res)
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_encode_ladder_frames")
        out = []
        for r, e in enumerate(encoders):
            rs = res[r * n:(r + 1) * n]
            e._last_batch = rs
            out.append([e._result(x) for x in rs] if collect else sum(x.data_size for x in rs))
        return out

    def bench_ladder(self, iters: int = 50) -> float:
        """average ms of the k_scale_fan launch(es) of the last ladder call,
        whose first encoder this is (diagnostics)"""
        ms = ctypes.c_float()
        rc = self.lib.hl_amd_bench_ladder(self._h, iters, ctypes.byref(ms))
        if rc:
            raise HlAmdError(rc, "hl_amd_bench_ladder")
        return ms.value

    def _check_frame(self, f: "Frame"):
        """a frame of a known size has the source size (the display size unless
        one was set; the coded size unless that was set)"""
        if f.width and (f.width, f.height) != self.source_size:
            raise HlAmdError(HL_AMD_ERROR_INVALID_FORMAT, "frame (picture size)")

    def encode_frame(self, frame: "Frame", ctl: "FrameCtl | None" = None) -> EncodeResult:
        """One frame by its description -- pitched I420, NV12, RGB24, RGBA32
        or planar RGB, on the host or in device memory -- converted on the GPU
        and coded as encode / encode_device code a frame (hl_amd_encode_frame)."""
        self._check_frame(frame)
        r = _Result()
        c = frame._c()
        rc = self.lib.hl_amd_encode_frame(self._h, ctypes.byref(c), ctypes.byref(ctl._c()) if ctl is not None else None, ctypes.byref(r))
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_encode_frame")
        return self._result(r)

    def encode_frames_device(self, frames, ctl=None, collect: bool = True):
        """Consecutive frames in device memory by their descriptions, converted
        on the GPU and coded as encode_batch_device codes frames
        (hl_amd_encode_frames); one result per frame."""
        n = len(frames)
        for f in frames:
            self._check_frame(f)
        arr = (_Frame * n)(*[f._c() for f in frames])
        res = (_Result * n)()
        rc = self.lib.hl_amd_encode_frames(self._h, n, arr, _ctl_array(ctl, n), res)
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_encode_frames")
        self._last_batch = res
        return [self._result(r) for r in res] if collect else sum(r.data_size for r in res)

    def last_input(self, k: int = 0):
        """The dense planes (y, u, v) picture k of the last encode_frame /
        encode_frames_device call was coded from (hl_amd_get_input)."""
        import numpy as np

        y = np.empty((self.height, self.width), np.uint8)
        u = np.empty((self.height // 2, self.width // 2), np.uint8)
        v = np.empty_like(u)
        rc = self.lib.hl_amd_get_input(self._h, k, y.ctypes.data, u.ctypes.data, v.ctypes.data)
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_get_input")
        return y, u, v

    def bench_ingest(self, iters: int = 50) -> float:
        """average ms of the k_ingest launch(es) of the last frame call, whose
        frames must still be there (diagnostics)"""
        ms = ctypes.c_float()
        rc = self.lib.hl_amd_bench_ingest(self._h, iters, ctypes.byref(ms))
        if rc:
            raise HlAmdError(rc, "hl_amd_bench_ingest")
        return ms.value

    def bench_planes(self, iters: int = 50) -> float:
        """average ms per launch of the quarter-pel plane kernel (diagnostics)"""
        ms = ctypes.c_float()
        rc = self.lib.hl_amd_bench_planes(self._h, iters, ctypes.byref(ms))
        if rc:
            raise HlAmdError(rc, "hl_amd_bench_planes")
        return ms.value

    def set_pipeline(self, workgroups: int, reach: int, window: int):
        rc = self.lib.hl_amd_set_pipeline(self._h, workgroups, reach, window)
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_set_pipeline")

    def set_pipeline_build(self, mode: int):
        """hl_amd_set_pipeline_build: 0 chosen per run, 1 the 512-lane build,
        2 the 256-lane build for every run of more than one picture."""
        rc = self.lib.hl_amd_set_pipeline_build(self._h, mode)
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_set_pipeline_build")

    def last_pipeline_build(self) -> int:
        """The build the last pipelined run launched (0 with the 8x8-family
        helper tasks, 1 512-lane, 2 256-lane; -1 before any run)."""
        return self.lib.hl_amd_last_pipeline_build(self._h)

    def recon(self):
        import numpy as np

        y = np.empty(self.width * self.height, np.uint8)
        u = np.empty(self.width * self.height // 4, np.uint8)
        v = np.empty_like(u)
        rc = self.lib.hl_amd_get_recon(self._h, y.ctypes.data, u.ctypes.data, v.ctypes.data)
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_get_recon")
        return y, u, v

    def set_timing(self, on: bool):
        self.lib.hl_amd_set_timing(self._h, 1 if on else 0)

    def timing_ms(self):
        a = (ctypes.c_float * 4)()
        self.lib.hl_amd_get_timing(self._h, a)
        return list(a)

    def last_reruns(self) -> int:
        return self.lib.hl_amd_last_reruns(self._h)

    def last_chain_walks(self) -> int:
        """resolve_chain walks of the last pipelined run (diagnostics)"""
        return self.lib.hl_amd_last_chain_walks(self._h)

    def profile_counters(self, n: int = 32):
        a = (ctypes.c_ulonglong * n)()
        self.lib.hl_amd_profile_counters(self._h, a, n)
        return list(a)

    def debug_records(self, k: int):
        """MbRecord structs of picture k of the last encode call (numpy
        structured array, one element per macroblock), or None when the
        call did not keep them."""
        import numpy as np

        if not hasattr(self.lib, "hl_amd_debug_records"):
            return None
        nmb = (self.width // 16) * (self.height // 16)
        dt = MB_RECORD
        if self.lib.hl_amd_record_size() == MB_RECORD.itemsize + 32:  # diagnostic build (HL_DIAG_INPUTS)
            dt = np.dtype(MB_RECORD.descr + [("dbg", "<u4", 8)])
        assert self.lib.hl_amd_record_size() == dt.itemsize
        out = np.zeros(nmb, dt)
        rc = self.lib.hl_amd_debug_records(self._h, k, out.ctypes.data, out.nbytes)
        if rc == HL_AMD_ERROR_INVALID_STATE:
            return None
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_debug_records")
        return out

    def debug_chain(self, k: int):
        """MbChain records (s_in, s_out, dep, fresh, spec per macroblock) of
        picture k of the last encode call, as an (nmb, 5) int32 array."""
        import numpy as np

        if not hasattr(self.lib, "hl_amd_debug_chain"):
            return None
        nmb = (self.width // 16) * (self.height // 16)
        out = np.zeros((nmb, 5), np.int32)
        rc = self.lib.hl_amd_debug_chain(self._h, k, out.ctypes.data, out.nbytes)
        if rc == HL_AMD_ERROR_INVALID_STATE:
            return None
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_debug_chain")
        return out

    def debug_recon(self, k: int):
        """Reconstructed planes of picture k of the last encode call,
        concatenated Y|U|V (None when not kept)."""
        import numpy as np

        if not hasattr(self.lib, "hl_amd_debug_recon"):
            return None
        n = self.width * self.height
        out = np.zeros(n * 3 // 2, np.uint8)
        rc = self.lib.hl_amd_debug_recon(self._h, k, out.ctypes.data, out.ctypes.data + n, out.ctypes.data + n + n // 4)
        if rc == HL_AMD_ERROR_INVALID_STATE:
            return None
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_debug_recon")
        return out

    def last_mb_launches(self) -> int:
        return self.lib.hl_amd_last_mb_launches(self._h)

    def last_batch_stats(self) -> dict:
        """How the last encode call ran (hl_amd_last_batch_stats): pipelined
        runs, pictures on the per-picture path, runs that fell back to it,
        bounded waits that gave up, in-kernel rdo.Single_ctr walks."""
        a = (ctypes.c_int32 * 5)()
        rc = self.lib.hl_amd_last_batch_stats(self._h, a)
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_last_batch_stats")
        return dict(zip(("runs", "per_picture", "fallbacks", "waits_gave_up", "chain_walks"), list(a)))

    def set_intra_helpers(self, enable: bool) -> None:
        rc = self.lib.hl_amd_set_intra_helpers(self._h, 1 if enable else 0)
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_set_intra_helpers")

    def last_helper_stats(self) -> dict:
        """How the last encode call's intra fallbacks ran
        (hl_amd_last_helper_stats): helper Intra4x4 decisions kept, rejected,
        helpers no workgroup had claimed in time."""
        a = (ctypes.c_int32 * 3)()
        rc = self.lib.hl_amd_last_helper_stats(self._h, a)
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_last_helper_stats")
        r = dict(zip(("i4_kept", "i4_rejected", "taken_over"), list(a)))
        if hasattr(self.lib, "hl_amd_last_fam3_stats"):
            b = (ctypes.c_int32 * 2)()
            if self.lib.hl_amd_last_fam3_stats(self._h, b) == HL_AMD_SUCCESS:
                r["fam3_kept"], r["fam3_rejected"] = b[0], b[1]
        return r


class SvcEncoder(Encoder):
    """Spatial SVC stream (hl_codec_add_layer + one encode per layer and
    access unit, base first): layer l is (width << l) x (height << l)."""

    def __init__(self, width: int, height: int, layers: int, qp: int = 28, me_range: int = 16, deblock: int = 1, gop_size: int = 30,
                 me_early_term: int = 0, device: int = 0, first: int = 0, last: int = -1):
        super().__init__(width, height, qp, me_range, deblock, gop_size, me_early_term, device)
        self.layers = layers
        for l in range(layers):
            rc = self.lib.hl_amd_add_layer(self._h, width << l, height << l)
            if rc != HL_AMD_SUCCESS:
                raise HlAmdError(rc, "hl_amd_add_layer")
        self.first, self.last = first, (layers - 1 if last < 0 else last)
        if (self.first, self.last) != (0, layers - 1):
            rc = self.lib.hl_amd_set_layer_range(self._h, self.first, self.last)
            if rc != HL_AMD_SUCCESS:
                raise HlAmdError(rc, "hl_amd_set_layer_range")

    def size(self, layer: int):
        return self.width << layer, self.height << layer

    def encode_layer(self, layer: int, y, u, v) -> EncodeResult:
        """One layer's frame from host memory (numpy uint8 planes)."""
        import numpy as np

        w, h = self.size(layer)
        ys = [np.ascontiguousarray(p, dtype=np.uint8) for p in (y, u, v)]
        if ys[0].size != w * h or ys[1].size != w * h // 4 or ys[2].size != ys[1].size:
            raise HlAmdError(HL_AMD_ERROR_INVALID_FORMAT, "encode_layer (plane sizes)")
        r = _Result()
        rc = self.lib.hl_amd_encode_layer(self._h, w, h, ys[0].ctypes.data, ys[1].ctypes.data, ys[2].ctypes.data, 0, ctypes.byref(r))
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_encode_layer")
        return self._result(r)

    def encode_layer_device(self, layer: int, y_ptr: int, u_ptr: int, v_ptr: int, collect: bool = True):
        w, h = self.size(layer)
        r = _Result()
        rc = self.lib.hl_amd_encode_layer(self._h, w, h, ctypes.c_void_p(y_ptr), ctypes.c_void_p(u_ptr), ctypes.c_void_p(v_ptr), 1,
                                          ctypes.byref(r))
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_encode_layer")
        return self._result(r) if collect else r.data_size

    def layer_recon(self, layer: int):
        import numpy as np

        w, h = self.size(layer)
        out = np.empty(w * h * 3 // 2, np.uint8)
        n = w * h
        rc = self.lib.hl_amd_get_layer_recon(self._h, layer, out.ctypes.data, out.ctypes.data + n, out.ctypes.data + n + n // 4)
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_get_layer_recon")
        return out

    def unpinned(self) -> int:
        return self.lib.hl_amd_svc_unpinned(self._h)

    def layer_state_bytes(self, layer: int) -> int:
        return self.lib.hl_amd_layer_state_bytes(self._h, layer)

    def export_layer(self, layer: int, dst_ptr: int):
        rc = self.lib.hl_amd_export_layer(self._h, layer, ctypes.c_void_p(dst_ptr))
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_export_layer")

    def import_layer(self, layer: int, src_ptr: int):
        rc = self.lib.hl_amd_import_layer(self._h, layer, ctypes.c_void_p(src_ptr))
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_import_layer")

    def layer_ms(self) -> float:
        return self.lib.hl_amd_svc_layer_ms(self._h)

    def encode_layers_batch_device(self, ptrs):
        """n access units of every layer resident in HBM: ptrs[l][i] =
        (y_ptr, u_ptr, v_ptr) of layer l's frame of access unit i.  Returns
        one EncodeResult per access unit (hl_amd_encode_layers_batch)."""
        L, n = len(ptrs), len(ptrs[0])
        flat = (ctypes.c_void_p * (3 * L * n))(*[ptrs[l][i][c] for l in range(L) for i in range(n) for c in range(3)])
        res = (_Result * n)()
        rc = self.lib.hl_amd_encode_layers_batch(self._h, n, L, flat, res)
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_encode_layers_batch")
        return [self._result(r) for r in res]

    def encode_au(self, y, u, v) -> EncodeResult:
        """One access unit from the top layer's frame alone (host numpy uint8
        planes): the lower layers' input is derived on the GPU
        (hl_amd_encode_au).  hdr holds every header set the layers' calls
        signalled, in order; annexb() is the access unit as a caller of
        encode_layer assembles it."""
        import numpy as np

        w, h = self.size(self.layers - 1)
        ys = [np.ascontiguousarray(p, dtype=np.uint8) for p in (y, u, v)]
        if ys[0].size != w * h or ys[1].size != w * h // 4 or ys[2].size != ys[1].size:
            raise HlAmdError(HL_AMD_ERROR_INVALID_FORMAT, "encode_au (plane sizes)")
        r = _Result()
        rc = self.lib.hl_amd_encode_au(self._h, ys[0].ctypes.data, ys[1].ctypes.data, ys[2].ctypes.data, 0, ctypes.byref(r))
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_encode_au")
        return self._result(r)

    def encode_au_device(self, y_ptr: int, u_ptr: int, v_ptr: int, collect: bool = True):
        """encode_au with the top layer's planes already in device memory."""
        r = _Result()
        rc = self.lib.hl_amd_encode_au(self._h, ctypes.c_void_p(y_ptr), ctypes.c_void_p(u_ptr), ctypes.c_void_p(v_ptr), 1, ctypes.byref(r))
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_encode_au")
        return self._result(r) if collect else r.data_size

    def encode_aus_batch_device(self, ptrs):
        """n access units from n top-layer frames resident in HBM: ptrs[i] =
        (y_ptr, u_ptr, v_ptr) of access unit i's frame.  Returns one
        EncodeResult per access unit (hl_amd_encode_aus_batch)."""
        n = len(ptrs)
        flat = (ctypes.c_void_p * (3 * n))(*[ptrs[i][c] for i in range(n) for c in range(3)])
        res = (_Result * n)()
        rc = self.lib.hl_amd_encode_aus_batch(self._h, n, flat, res)
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_encode_aus_batch")
        return [self._result(r) for r in res]

    def layer_input(self, layer: int):
        """The input planes (concatenated Y|U|V) the last encode_au /
        encode_aus_batch_device derived for `layer`; the top layer's is the
        frame itself (hl_amd_get_layer_input)."""
        import numpy as np

        w, h = self.size(layer)
        n = w * h
        out = np.empty(n * 3 // 2, np.uint8)
        rc = self.lib.hl_amd_get_layer_input(self._h, layer, out.ctypes.data, out.ctypes.data + n, out.ctypes.data + n + n // 4)
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_get_layer_input")
        return out

    def set_au_display_size(self, width: int, height: int) -> None:
        """The size a decoder shows of the top layer (hl_amd_set_au_display_size):
        multiples of 2 << K within 16 << K of the top coded size (K = layers -
        1); layer l shows it shifted right by K - l.  SPS 0 and every subset
        SPS then carry the cropping offsets, encode_au_frame and
        encode_au_frames_device take frames of this size and pad them on the
        GPU, and quality covers each layer's display rectangle; every other
        encode call keeps taking planes of the coded sizes.  Before the first
        picture."""
        rc = self.lib.hl_amd_set_au_display_size(self._h, width, height)
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_set_au_display_size")

    @property
    def au_display_size(self):
        """(width, height) a decoder shows of the top layer: its coded size unless set_au_display_size set another."""
        w, h = ctypes.c_int32(), ctypes.c_int32()
        rc = self.lib.hl_amd_get_au_display_size(self._h, ctypes.byref(w), ctypes.byref(h))
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_get_au_display_size")
        return w.value, h.value

    def _check_frame(self, f: "Frame"):
        """a frame of a known size has the top layer's display size (its coded size unless one was set)"""
        if f.width and (f.width, f.height) != self.au_display_size:
            raise HlAmdError(HL_AMD_ERROR_INVALID_FORMAT, "frame (picture size)")

    def encode_au_frame(self, frame: "Frame") -> EncodeResult:
        """One access unit from one frame by its description -- any format, on
        the host or in device memory, of the top display size -- converted and
        padded on the GPU and coded as encode_au codes the padded top planes
        (hl_amd_encode_au_frame)."""
        self._check_frame(frame)
        r = _Result()
        c = frame._c()
        rc = self.lib.hl_amd_encode_au_frame(self._h, ctypes.byref(c), ctypes.byref(r))
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_encode_au_frame")
        return self._result(r)

    def encode_au_frames_device(self, frames):
        """n access units from n frames in device memory by their descriptions,
        converted on the GPU (one launch per format) and coded as
        encode_aus_batch_device codes frames (hl_amd_encode_au_frames)."""
        n = len(frames)
        for f in frames:
            self._check_frame(f)
        arr = (_Frame * n)(*[f._c() for f in frames])
        res = (_Result * n)()
        rc = self.lib.hl_amd_encode_au_frames(self._h, n, arr, res)
        if rc != HL_AMD_SUCCESS:
            raise HlAmdError(rc, "hl_amd_encode_au_frames")
        return [self._result(r) for r in res]

    def bench_pyramid(self, iters: int = 50) -> float:
        """average ms per launch of k_pyramid on the last encode_au's frame (diagnostics)"""
        ms = ctypes.c_float()
        rc = self.lib.hl_amd_bench_pyramid(self._h, iters, ctypes.byref(ms))
        if rc:
            raise HlAmdError(rc, "hl_amd_bench_pyramid")
        return ms.value
