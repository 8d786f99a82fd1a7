"""hartallo_amd -- MI355X (gfx950) native H.264 Baseline encode path of
allweax/hartallo: the per-macroblock RDO loop (diamond ME, quarter-pel
interpolation, 4x4 transform/quant, CAVLC rate, intra RDO, deblocking) as
hand-written HIP kernels, and its spatial-SVC enhancement layers, bit-exact
with the reference encoder, behind a
C ABI (include/hartallo_amd.h) that a hartallo plugin forwards to.
"""
from ._lib import (EXPORTED_SYMBOLS, HL_AMD_FORMAT_I420, HL_AMD_FORMAT_NV12, HL_AMD_FORMAT_RGB24, HL_AMD_FORMAT_RGBA32,
                   HL_AMD_FORMAT_RGBP, HL_AMD_MATRIX_BT601, HL_AMD_MATRIX_BT709, HL_AMD_RANGE_FULL, HL_AMD_RANGE_LIMITED,
                   HL_AMD_RESULT_TYPE_DATA, HL_AMD_RESULT_TYPE_HDR, LIB_PATH, EncodeResult, Encoder, Frame, FrameCtl, HlAmdError,
                   Quality, SvcEncoder, load_library, psnr_db, scale_taps, ssim_mean, stream_headers, svc_stream_headers)

__all__ = [
    "Encoder",
    "SvcEncoder",
    "EncodeResult",
    "FrameCtl",
    "Frame",
    "HlAmdError",
    "load_library",
    "Quality",
    "psnr_db",
    "ssim_mean",
    "stream_headers",
    "svc_stream_headers",
    "scale_taps",
    "LIB_PATH",
    "EXPORTED_SYMBOLS",
    "HL_AMD_RESULT_TYPE_DATA",
    "HL_AMD_RESULT_TYPE_HDR",
    "HL_AMD_FORMAT_I420",
    "HL_AMD_FORMAT_NV12",
    "HL_AMD_FORMAT_RGB24",
    "HL_AMD_FORMAT_RGBA32",
    "HL_AMD_FORMAT_RGBP",
    "HL_AMD_MATRIX_BT601",
    "HL_AMD_MATRIX_BT709",
    "HL_AMD_RANGE_LIMITED",
    "HL_AMD_RANGE_FULL",
]
