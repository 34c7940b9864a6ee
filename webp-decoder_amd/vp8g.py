"""vp8g -- Python mirror of the C ABI in include/vp8g.h (ctypes; no torch types cross it).

Loads the in-tree libraries built by the top-level Makefile:
  lib/libvp8host.so  C11 front end (reference m01-m05 equivalents) + synthetic frame generator
  lib/libvp8g.so     HIP gfx950 kernels behind the reference's m06/m07 entry points + batch API

The structures below are layout-identical to the reference's (reference src/m02_vp8_header/
vp8_header.h:7-18, src/m05_tokens/vp8_tokens.h:7-99, src/m06_recon/vp8_recon.h:10-18), so a
Vp8DecodedFrame produced by either front end can be handed to either reconstruction library.

Nothing here falls back to the CPU: if libvp8g.so (or a GPU) is missing, the GPU entry points
raise.
"""
from __future__ import annotations

import ctypes as C
import os
import pathlib
from types import SimpleNamespace

import numpy as np

import vp8g_stage as S
from vp8g_stage import ByteSpan, device_copy, image_bytes as _image_bytes  # noqa: F401  (names callers know from here)

PKG_DIR = pathlib.Path(__file__).resolve().parent
REPO_DIR = PKG_DIR.parent
LIB_DIR = PKG_DIR / "lib"


class Vp8KeyFrameHeader(C.Structure):
    _fields_ = [
        ("is_key_frame", C.c_int),
        ("profile", C.c_uint8),
        ("show_frame", C.c_int),
        ("first_partition_len", C.c_uint32),
        ("start_code_ok", C.c_int),
        ("width", C.c_uint16),
        ("height", C.c_uint16),
        ("x_scale", C.c_uint8),
        ("y_scale", C.c_uint8),
    ]


class Vp8CoeffStats(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in (
        "mb_cols", "mb_rows", "mb_total", "part0_size_bytes", "part0_bytes_used")] + [
        ("part0_overread", C.c_uint8), ("part0_overread_bytes", C.c_uint32),
        ("token_part_size_bytes", C.c_uint32), ("token_part_bytes_used", C.c_uint32),
        ("token_overread", C.c_uint8)] + [(n, C.c_uint32) for n in (
            "token_overread_bytes", "token_overread_mb_index", "token_overread_plane",
            "token_overread_block_index", "token_overread_coeff_i", "token_overread_stage",
            "mb_skip_coeff", "mb_b_pred")] + [
        ("ymode_counts", C.c_uint32 * 5), ("uv_mode_counts", C.c_uint32 * 4),
        ("bmode_counts", C.c_uint32 * 10)] + [(n, C.c_uint32) for n in (
            "blocks_total_y2", "blocks_total_y", "blocks_total_u", "blocks_total_v",
            "blocks_nonzero_y2", "blocks_nonzero_y", "blocks_nonzero_u", "blocks_nonzero_v",
            "coeff_nonzero_total", "coeff_eob_tokens", "coeff_abs_max")] + [
        ("coeff_hash_fnv1a64", C.c_uint64)]


class Vp8DecodedFrame(C.Structure):
    _fields_ = [
        ("mb_cols", C.c_uint32), ("mb_rows", C.c_uint32), ("mb_total", C.c_uint32),
        ("q_index", C.c_uint8), ("y1_dc_delta_q", C.c_int8), ("y2_dc_delta_q", C.c_int8),
        ("y2_ac_delta_q", C.c_int8), ("uv_dc_delta_q", C.c_int8), ("uv_ac_delta_q", C.c_int8),
        ("segmentation_enabled", C.c_uint8), ("segmentation_abs", C.c_uint8),
        ("seg_quant_idx", C.c_int8 * 4), ("seg_lf_level", C.c_int8 * 4),
        ("lf_use_simple", C.c_uint8), ("lf_level", C.c_uint8), ("lf_sharpness", C.c_uint8),
        ("lf_delta_enabled", C.c_uint8), ("lf_ref_delta", C.c_int8 * 4), ("lf_mode_delta", C.c_int8 * 4),
        ("segment_id", C.POINTER(C.c_uint8)), ("skip_coeff", C.POINTER(C.c_uint8)),
        ("has_coeff", C.POINTER(C.c_uint8)), ("ymode", C.POINTER(C.c_uint8)),
        ("uv_mode", C.POINTER(C.c_uint8)), ("bmode", C.POINTER(C.c_uint8)),
        ("coeff_y2", C.POINTER(C.c_int16)), ("coeff_y", C.POINTER(C.c_int16)),
        ("coeff_u", C.POINTER(C.c_int16)), ("coeff_v", C.POINTER(C.c_int16)),
        ("stats", Vp8CoeffStats),
    ]


class Yuv420Image(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("stride_y", C.c_uint32),
                ("stride_uv", C.c_uint32), ("y", C.POINTER(C.c_uint8)), ("u", C.POINTER(C.c_uint8)),
                ("v", C.POINTER(C.c_uint8))]


class Vp8gFrameDesc(C.Structure):
    _fields_ = [
        ("mb_cols", C.c_uint32), ("mb_rows", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32),
        ("stride_y", C.c_uint32), ("stride_uv", C.c_uint32), ("mb_offset", C.c_uint64),
        ("out_y", C.c_uint64), ("out_u", C.c_uint64), ("out_v", C.c_uint64),
        ("src_y", C.c_uint64), ("src_u", C.c_uint64), ("src_v", C.c_uint64),
        ("flags", C.c_uint32), ("src_stride_y", C.c_uint32), ("src_stride_uv", C.c_uint32),
        ("reserved", C.c_uint32), ("dq", (C.c_int16 * 6) * 4), ("lf", ((C.c_uint8 * 4) * 2) * 4),
    ]


class Vp8gLaunchPlan(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in (
        "quad", "waves", "global_ctx", "parts", "workgroups", "ordered", "mirror_split", "interleave", "whole",
        "ord_first", "lds_bytes", "mode")] + [(n, C.c_uint64) for n in (
            "gctx_bytes", "mbox_bytes", "snap_bytes", "flags_bytes")]


class Vp8gBatchArrays(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "coeff_y", "coeff_u", "coeff_v", "coeff_y2", "ymode", "uv_mode", "segment_id", "has_coeff",
        "bmode", "src", "status")]


class Vp8gEncDesc(C.Structure):
    _fields_ = [
        ("width", C.c_uint32), ("height", C.c_uint32), ("stride_y", C.c_uint32), ("stride_uv", C.c_uint32),
        ("src_y", C.c_uint64), ("src_u", C.c_uint64), ("src_v", C.c_uint64), ("out", C.c_uint64),
        ("file_len", C.c_uint64), ("format", C.c_uint32), ("prefix_len", C.c_uint32), ("row_bytes", C.c_uint32),
        ("raw_len", C.c_uint32), ("span0", C.c_uint32), ("nspans", C.c_uint32), ("zend", C.c_uint32),
        ("crc_init", C.c_uint32), ("prefix", C.c_uint8 * 48), ("reserved", C.c_uint32 * 4),
        ("crc_ops", (C.c_uint32 * 32) * 10),
    ]


class Vp8gPackedFrame(C.Structure):
    """include/vp8g.h: packed m05 output (per block a non-zero mask, then the non-zero values)."""
    _fields_ = [("kf", Vp8KeyFrameHeader), ("f", Vp8DecodedFrame), ("masks", C.POINTER(C.c_uint16)),
                ("mb_off", C.POINTER(C.c_uint32)), ("values", C.POINTER(C.c_int16)), ("n_values", C.c_uint64)]


class Vp8gTokFrame(C.Structure):
    """include/vp8g.h: device m05 job of one frame (partition-0 bool state + token probabilities)."""
    _fields_ = [("data", C.c_uint64), ("mb_offset", C.c_uint64), ("b_value", C.c_uint64), ("b_bits", C.c_int32),
                ("b_range", C.c_uint32), ("b_next", C.c_uint32), ("p0_end", C.c_uint32), ("tok_off", C.c_uint32),
                ("tok_end", C.c_uint32), ("mb_cols", C.c_uint32), ("mb_rows", C.c_uint32),
                ("seg_enabled", C.c_uint8), ("seg_map_update", C.c_uint8), ("use_skip", C.c_uint8),
                ("skip_prob", C.c_uint8), ("seg_probs", C.c_uint8 * 3), ("reserved", C.c_uint8),
                ("coeff_probs", C.c_uint8 * (4 * 8 * 3 * 12)), ("nparts", C.c_uint32),
                ("part_off", C.c_uint32 * 8), ("part_end", C.c_uint32 * 8), ("reserved2", C.c_uint32 * 3)]


class Vp8gScaleOpt(C.Structure):
    """include/vp8g.h: crop window + target size (libwebp's use_cropping / use_scaling); all-zero = identity."""
    _fields_ = [(n, C.c_uint32) for n in ("crop_left", "crop_top", "crop_w", "crop_h", "scaled_w", "scaled_h", "flags")]


class Vp8gScalePlane(C.Structure):
    _fields_ = [("src", C.c_uint64), ("dst", C.c_uint64)] + [(n, C.c_uint32) for n in (
        "src_stride", "dst_stride", "src_w", "src_h", "dst_w", "dst_h", "fx", "fy", "fxy", "group", "tile_w", "run_h",
        "tiles_x", "ntasks", "pitch", "block_rows")]


class Vp8gScaleDesc(C.Structure):
    """include/vp8g.h: per-image descriptor of the scale kernel (vp8g_make_scale_desc)."""
    _fields_ = [(n, C.c_uint32) for n in ("width", "height", "task0", "ntasks", "src_width", "src_height", "crop_left",
                                          "crop_top")] + [("p", Vp8gScalePlane * 3)]


class Vp8fScaleGeom(C.Structure):
    """host/vp8_front.h: a Vp8gScaleOpt resolved against a picture size."""
    _fields_ = [(n, C.c_uint32) for n in ("left", "top", "win_w", "win_h", "out_w", "out_h", "scaling")]


class Vp8gTensorOpt(C.Structure):
    """include/vp8g.h: picture size, element type, layout and normalisation of a device RGB tensor."""
    _fields_ = [(n, C.c_uint32) for n in ("width", "height", "dtype", "layout", "flags")] + [
        ("scale", C.c_float * 3), ("bias", C.c_float * 3)]


class Vp8gTensorDesc(C.Structure):
    """include/vp8g.h: per-image descriptor of the tensor kernel (vp8g_make_tensor_desc)."""
    _fields_ = [(n, C.c_uint64) for n in ("src_y", "src_u", "src_v", "dst")] + [(n, C.c_uint32) for n in (
        "stride_y", "stride_uv", "task0", "ntasks")]


class WebPStill(C.Structure):
    """host/vp8_front.h: a still picture located in its file by webp_locate_still (an offset of 0 = no such chunk)."""
    _fields_ = [("data", C.c_void_p), ("size", C.c_size_t), ("vp8_offset", C.c_size_t), ("alph_offset", C.c_size_t),
                ("vp8l_offset", C.c_size_t)] + [(n, C.c_uint32) for n in (
        "vp8_size", "alph_size", "vp8l_size", "width", "height", "riff_size", "extended", "vp8x_flags")]


WEBP_ACCEPT_EXTENDED, WEBP_ACCEPT_LOSSLESS = 1, 2


class WebPContainerX(C.Structure):
    """host/vp8_front.h: what webp_parse_extended found (alph_chunk_offset 0 = no alpha)."""
    _fields_ = [("riff_size", C.c_uint32), ("actual_size", C.c_size_t), ("vp8_chunk_offset", C.c_size_t),
                ("vp8_chunk_size", C.c_uint32), ("alph_chunk_offset", C.c_size_t), ("alph_chunk_size", C.c_uint32),
                ("extended", C.c_uint32), ("vp8x_flags", C.c_uint32), ("canvas_width", C.c_uint32),
                ("canvas_height", C.c_uint32)]


ALPHA_STATS = ("raw", "lossless", "predictor", "cross_color", "subtract_green", "color_index", "pack_bits_1",
               "pack_bits_2", "pack_bits_4", "pack_bits_8", "multi_group", "backrefs", "short_dist", "cache_hits",
               "simple_codes", "normal_codes", "repeat_16", "repeat_17", "repeat_18")


class Vp8fAlphaStats(C.Structure):
    """host/vp8_front.h: which features of the format an ALPH stream used (counters, in ALPHA_STATS order)."""
    _fields_ = [(n, C.c_uint32) for n in ALPHA_STATS]


class Vp8gAlphaDesc(C.Structure):
    """include/vp8g.h: per-plane descriptor of the alpha un-prediction kernel."""
    _fields_ = [("src", C.c_uint64), ("dst", C.c_uint64)] + [(n, C.c_uint32) for n in (
        "width", "height", "src_stride", "dst_stride", "filter", "task0", "ntasks", "reserved")]


class Vp8gTensorAlpha(C.Structure):
    """include/vp8g.h: the alpha plane of one image of the 4-channel tensor kernel (src_a = 2^64 - 1: opaque)."""
    _fields_ = [("src_a", C.c_uint64), ("stride_a", C.c_uint32), ("reserved", C.c_uint32)]


class WebPContainerL(C.Structure):
    """host/vp8_front.h: what webp_parse_any found (vp8l_chunk_offset 0 = a lossy file)."""
    _fields_ = WebPContainerX._fields_ + [("vp8l_chunk_offset", C.c_size_t), ("vp8l_chunk_size", C.c_uint32)]


class Vp8fLosslessTransform(C.Structure):
    """host/vp8_front.h: one transform of a lossless stream, as vp8f_lossless_decode leaves it."""
    _fields_ = [(n, C.c_uint32) for n in ("type", "bits", "xsize", "ncolors")] + [("data", C.POINTER(C.c_uint32))]


class Vp8fLosslessImage(C.Structure):
    """host/vp8_front.h: the entropy-decoded residual image and the transforms of a lossless stream."""
    _fields_ = [(n, C.c_uint32) for n in ("width", "height", "alpha_hint", "xsize", "ntransforms", "reserved")] + [
        ("argb", C.POINTER(C.c_uint32)), ("tr", Vp8fLosslessTransform * 4)]


class Vp8gLosslessTransform(C.Structure):
    """include/vp8g.h: one transform of an image of the lossless kernel (data = byte offset in the source buffer)."""
    _fields_ = [("data", C.c_uint64)] + [(n, C.c_uint32) for n in ("type", "bits", "xsize", "ncolors")]


class Vp8gLosslessDesc(C.Structure):
    """include/vp8g.h: per-image descriptor of the lossless kernel (vp8g_make_lossless_desc)."""
    _fields_ = [("src", C.c_uint64), ("dst", C.c_uint64)] + [(n, C.c_uint32) for n in (
        "width", "height", "ntransforms", "task0")] + [("tr", Vp8gLosslessTransform * 4)]


class Vp8gTensorArgbDesc(C.Structure):
    """include/vp8g.h: per-image descriptor of the ARGB tensor kernel (vp8g_make_tensor_argb_desc)."""
    _fields_ = [("src", C.c_uint64), ("dst", C.c_uint64), ("task0", C.c_uint32), ("ntasks", C.c_uint32)]


class Vp8gScaleArgbDesc(C.Structure):
    """include/vp8g.h: per-picture descriptor of the ARGB crop / rescale (vp8g_make_scale_argb_desc)."""
    _fields_ = [(n, C.c_uint64) for n in ("src", "work", "dst", "work_bytes")] + [(n, C.c_uint32) for n in (
        "width", "height", "src_width", "src_height", "crop_left", "crop_top", "win_w", "win_h", "plane_stride", "out_stride",
        "nplanes", "plane0", "split_task0", "split_ntasks", "scale_task0", "scale_ntasks", "merge_task0", "merge_ntasks")] + [
        ("reserved", C.c_uint32 * 2), ("plane", Vp8gScaleDesc * 4)]


class Vp8gScaleArgbTensorDesc(C.Structure):
    """include/vp8g.h: per-picture descriptor of the fused ARGB crop / shrink into a tensor (vp8g_make_scale_argb_tensor_desc)."""
    _fields_ = [("src", C.c_uint64), ("dst", C.c_uint64)] + [(n, C.c_uint32) for n in (
        "width", "height", "src_width", "src_height", "crop_left", "crop_top", "win_w", "win_h", "fx", "fy", "fxy", "group", "tile_w",
        "run_h", "tiles_x", "pitch", "block_rows", "task0", "ntasks", "reserved")]


class WebPAnimInfo(C.Structure):
    """host/vp8_front.h: what webp_parse_anim found in an animated file as a whole."""
    _fields_ = [(n, C.c_uint32) for n in ("canvas_width", "canvas_height", "bgcolor", "loop_count", "nframes", "vp8x_flags")]


class WebPAnimFrame(C.Structure):
    """host/vp8_front.h: one ANMF chunk (payload offsets and sizes of its sub-chunks; a size of 0 = absent)."""
    _fields_ = [(n, C.c_size_t) for n in ("offset", "alph_offset", "vp8_offset", "vp8l_offset")] + [(n, C.c_uint32) for n in (
        "size", "alph_size", "vp8_size", "vp8l_size", "x", "y", "width", "height", "duration", "blend", "dispose", "has_alpha")]


class Vp8fAnimFrame(C.Structure):
    """host/vp8_front.h: one frame as vp8f_anim_compose sees it."""
    _fields_ = [("argb", C.c_void_p)] + [(n, C.c_uint32) for n in ("x", "y", "width", "height", "blend", "dispose", "has_alpha", "key")]


class Vp8gAnimFrame(C.Structure):
    """include/vp8g.h: one frame record of the compositor kernel (vp8g_make_anim_desc completes it)."""
    _fields_ = [("src", C.c_uint64)] + [(n, C.c_uint32) for n in ("x", "y", "width", "height", "flags", "seg_first", "seg_end", "reserved")]


class Vp8gAnimDesc(C.Structure):
    """include/vp8g.h: per-animation descriptor of the compositor kernel (vp8g_make_anim_desc)."""
    _fields_ = [("frames", C.c_uint64), ("h_frames", C.c_void_p), ("dst", C.c_uint64)] + [(n, C.c_uint32) for n in (
        "width", "height", "nframes", "nsegs", "task0", "ntasks")]


ANIM_BLEND, ANIM_DISPOSE, ANIM_HAS_ALPHA, ANIM_KEY = 1, 2, 4, 8  # VP8G_ANIM_*

# transform types (RFC 9649 4)
L_PREDICTOR, L_CROSS_COLOR, L_SUBTRACT_GREEN, L_COLOR_INDEX = 0, 1, 2, 3


def lossless_geometry():
    """vp8g_lossless_geometry: (tile step, band rows, round bands) of the lossless kernel as the library was built --
    columns per barrier group, rows per wave, bands per workgroup round.  The boundary sizes of the tests come from it."""
    g = (C.c_uint32 * 3)()
    gpu_lib().vp8g_lossless_geometry(g)
    return int(g[0]), int(g[1]), int(g[2])


def band_handover(kernel: str):
    """vp8g_lossless_handover / vp8g_alpha_handover: the hand-over geometry of a banded wavefront kernel as the library
    was built.  "lossless": (row skew, band delay in groups, ring in pixels, full-width row at most, in pixels);
    "alpha": (tile step, band delay in tile steps, ring in bytes, full-width row in bytes).  tests/bands.py states
    the same numbers for its model of the schedule."""
    g = (C.c_uint32 * 4)()
    getattr(gpu_lib(), f"vp8g_{kernel}_handover")(g)
    return tuple(int(v) for v in g)


T_OPAQUE = 0xFFFFFFFFFFFFFFFF
VP8G_X_ALPHA = 1
VP8G_X_LOSSLESS = 2
VP8G_X_LOSSLESS_SCALE = 16
VP8G_SCALE_DWEBP_FILTER = 1
VP8G_SCALE_EXPAND = 4

T_DTYPES = {"uint8": 0, "float16": 1, "bfloat16": 2, "float32": 3}  # VP8G_T_U8 / F16 / BF16 / F32
T_ELEM = {0: 1, 1: 2, 2: 2, 3: 4}
T_LAYOUTS = {"NHWC": 0, "NCHW": 1}
VP8G_T_BGR = 1

PK_BLOCKS = 25  # per MB: Y 0..15, U 0..3, V 0..3, Y2
VP8G_BATCH_DEVICE_M05, VP8G_BATCH_MULTI_PARTITION = S.BATCH_DEVICE_M05, S.BATCH_MULTI_PARTITION
VP8F_PACK_HASH = 1
VP8F_MULTI_PARTITION = 2

ENC_FORMATS = {"rgb": 0, "ppm": 1, "png": 2}
ENC_SPAN = 32768

assert C.sizeof(Vp8gEncDesc) == 1432
assert C.sizeof(Vp8KeyFrameHeader) == 28
assert C.sizeof(Vp8CoeffStats) == 200
assert C.sizeof(Vp8DecodedFrame) == 320
assert C.sizeof(Yuv420Image) == 40
assert C.sizeof(Vp8gFrameDesc) == 176
assert C.sizeof(Vp8gTokFrame) == 1296
assert C.sizeof(Vp8gScaleOpt) == 28
assert C.sizeof(Vp8gScalePlane) == 80
assert C.sizeof(Vp8gScaleDesc) == 272
assert C.sizeof(Vp8gTensorOpt) == 44
assert C.sizeof(Vp8gTensorDesc) == 48
assert C.sizeof(Vp8gScaleArgbDesc) == 1200 and C.sizeof(Vp8gScaleArgbTensorDesc) == 96
assert C.sizeof(WebPAnimFrame) == 80 and C.sizeof(Vp8gAnimFrame) == 40 and C.sizeof(Vp8gAnimDesc) == 48

VP8G_F_LOOPFILTER = 1
VP8G_F_SIMPLE = 2
VP8G_F_LF_ONLY = 4

# Arrays of a decoded frame: (field, dtype, elements per MB)
FRAME_ARRAYS = [
    ("coeff_y", np.int16, 256), ("coeff_u", np.int16, 64), ("coeff_v", np.int16, 64),
    ("coeff_y2", np.int16, 16), ("ymode", np.uint8, 1), ("uv_mode", np.uint8, 1),
    ("segment_id", np.uint8, 1), ("has_coeff", np.uint8, 1), ("bmode", np.uint8, 16),
    ("skip_coeff", np.uint8, 1),
]
# Algorithmic bytes the hot path reads per macroblock: 800 B of dense int16
# coefficients + 20 B side info (ymode, uv_mode, segment_id, has_coeff, 16 x bmode).
BYTES_READ_PER_MB = 820


def i420_size(w: int, h: int) -> int:
    return w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)


_DIG_K = np.uint64(0x9E3779B97F4A7C15)


def digest64(buf) -> int:
    """Digest of a byte string as vp8g_frame_digests computes it on the device (include/vp8g.h):
    L*K + sum_i mix(w_i + (i+1)*K) mod 2^64 over little-endian u64 words (last zero-padded),
    mix = splitmix64's finaliser.  Returned as an unsigned Python int."""
    b = np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else buf.view(np.uint8).reshape(-1)
    n = b.size
    pad = (-n) % 8
    if pad:
        b = np.concatenate([b, np.zeros(pad, np.uint8)])
    w = b.view("<u8")
    z = w + (np.arange(1, w.size + 1, dtype=np.uint64) * _DIG_K)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z ^= z >> np.uint64(31)
    return (n * 0x9E3779B97F4A7C15 + int(z.sum(dtype=np.uint64))) & 0xFFFFFFFFFFFFFFFF


_libs: dict = {}


def _load(name: str, path: pathlib.Path):
    if name not in _libs:
        if not path.exists():
            raise OSError(f"{path} not built (run `make` at the repo root)")
        _libs[name] = C.CDLL(str(path), use_errno=True)
    return _libs[name]


def host_lib():
    lib = _load("host", LIB_DIR / "libvp8host.so")
    if not getattr(lib, "_typed", False):
        lib.vp8f_decode_file.argtypes = [C.c_char_p, C.POINTER(Vp8KeyFrameHeader), C.POINTER(Vp8DecodedFrame),
                                         C.POINTER(C.c_int)]
        lib.vp8f_decode_memory.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(Vp8KeyFrameHeader),
                                           C.POINTER(Vp8DecodedFrame), C.POINTER(C.c_int)]
        lib.vp8f_synth_frame.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_int, C.POINTER(Vp8KeyFrameHeader),
                                         C.POINTER(Vp8DecodedFrame)]
        lib.vp8_decoded_frame_free.argtypes = [C.POINTER(Vp8DecodedFrame)]
        lib.vp8_decoded_frame_free.restype = None
        lib.vp8f_fnv1a64.argtypes = [C.c_void_p, C.c_size_t, C.c_uint64]
        lib.vp8f_fnv1a64.restype = C.c_uint64
        lib.vp8f_decode_packed_memory.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(Vp8gPackedFrame),
                                                  C.POINTER(C.c_int), C.c_uint]
        lib.vp8f_packed_free.argtypes = [C.POINTER(Vp8gPackedFrame)]
        lib.vp8f_token_header_memory.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(Vp8KeyFrameHeader),
                                                 C.POINTER(Vp8DecodedFrame), C.POINTER(Vp8gTokFrame),
                                                 C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_int),
                                                 C.c_uint]
        lib.vp8f_packed_free.restype = None
        lib.vp8f_scale_resolve.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(Vp8gScaleOpt), C.POINTER(Vp8fScaleGeom)]
        lib.vp8f_scale_filtered.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(Vp8gScaleOpt), C.c_int]
        lib.vp8f_scale_i420.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                        C.POINTER(Vp8gScaleOpt), C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]
        if hasattr(lib, "vp8f_scale_yuv444"):  # (libraries built before libwebp's scaled RGB)
            lib.vp8f_scale_yuv444.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                              C.POINTER(Vp8gScaleOpt), C.c_void_p, C.c_void_p, C.c_void_p]
        lib.webp_parse_simple_lossy.argtypes = [ByteSpan, C.c_void_p]
        lib.vp8_parse_keyframe_header.argtypes = [ByteSpan, C.POINTER(Vp8KeyFrameHeader)]
        lib.webp_locate_still.argtypes = [ByteSpan, C.c_uint, C.POINTER(WebPStill)]
        lib.webp_parse_extended.argtypes = [ByteSpan, C.POINTER(WebPContainerX)]
        lib.vp8f_alpha_decode.argtypes = [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_void_p,
                                          C.POINTER(C.c_uint32), C.POINTER(Vp8fAlphaStats)]
        lib.vp8f_alpha_unfilter.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
        lib.webp_parse_any.argtypes = [ByteSpan, C.POINTER(WebPContainerL)]
        lib.vp8f_lossless_header.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                             C.POINTER(C.c_uint32)]
        lib.vp8f_lossless_decode.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(Vp8fLosslessImage),
                                             C.POINTER(Vp8fAlphaStats)]
        lib.vp8f_lossless_free.argtypes = [C.POINTER(Vp8fLosslessImage)]
        lib.vp8f_lossless_free.restype = None
        lib.vp8f_lossless_apply.argtypes = [C.POINTER(Vp8fLosslessImage), C.c_void_p]
        if hasattr(lib, "vp8f_argb_scale"):  # (libraries built before the scaled lossless path: A/B of old builds)
            lib.vp8f_scale_resolve_argb.argtypes = lib.vp8f_scale_resolve.argtypes
            lib.vp8f_argb_mult_row.argtypes = [C.c_void_p, C.c_uint32, C.c_int]
            lib.vp8f_argb_mult_row.restype = None
            lib.vp8f_argb_scale.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(Vp8gScaleOpt), C.c_void_p]
        lib.webp_parse_anim.argtypes = [ByteSpan, C.POINTER(WebPAnimInfo), C.POINTER(WebPAnimFrame), C.c_uint32]
        lib.vp8f_anim_keyframes.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(Vp8fAnimFrame), C.c_uint32]
        lib.vp8f_anim_compose.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(Vp8fAnimFrame), C.c_uint32, C.c_void_p]
        lib._typed = True
    return lib


# vp8g_last_launch_mode bits (include/vp8g.h)
MODE_CHAIN, MODE_MIRROR_SPLIT, MODE_INTERLEAVE, MODE_QUAD, MODE_SPLIT_PARTS = 1, 2, 4, 8, 16
# vp8g_plan_launch callers
PLAN_REFERENCE, PLAN_PIPELINE, PLAN_NO_SPLIT = 0, 1, 2


def plan_launch(descs, cus: int, *, hint: int = 0, split: int = 0, waves: int = 0, chain: int = -1, splitchain: int = -1,
                chain_il: int = -1, order: int = 1, policy: int = PLAN_REFERENCE, may_cross: bool = True) -> Vp8gLaunchPlan:
    """vp8g_plan_launch: the recon launch the library makes for `descs` (a ctypes array of Vp8gFrameDesc)
    on a device of `cus` CUs.  Host code only: no device call, the environment is not read."""
    out = Vp8gLaunchPlan()
    if gpu_lib().vp8g_plan_launch(descs, len(descs), cus, hint, split, waves, chain, splitchain, chain_il, order, policy,
                                  int(may_cross), C.byref(out)) != 0:
        raise ValueError(f"vp8g_plan_launch: errno={C.get_errno()}")
    return out


def gpu_lib():
    """libvp8g.so: the product path.  Raises if it is not built."""
    lib = _load("gpu", pathlib.Path(os.environ.get("VP8G_LIB", LIB_DIR / "libvp8g.so")))
    if not getattr(lib, "_typed", False):
        P = C.POINTER
        lib.vp8_reconstruct_keyframe_yuv.argtypes = [P(Vp8KeyFrameHeader), P(Vp8DecodedFrame), P(Yuv420Image)]
        lib.vp8_reconstruct_keyframe_yuv_filtered.argtypes = [P(Vp8KeyFrameHeader), P(Vp8DecodedFrame),
                                                              P(Yuv420Image)]
        lib.vp8_loopfilter_apply_keyframe.argtypes = [P(Yuv420Image), P(Vp8DecodedFrame)]
        lib.yuv420_alloc.argtypes = [P(Yuv420Image), C.c_uint32, C.c_uint32]
        lib.yuv420_free.argtypes = [P(Yuv420Image)]
        lib.yuv420_free.restype = None
        lib.vp8g_make_frame_desc.argtypes = [P(Vp8KeyFrameHeader), P(Vp8DecodedFrame), C.c_int, C.c_uint64,
                                             C.c_uint64, P(Vp8gFrameDesc)]
        lib.vp8g_i420_size.argtypes = [C.c_uint32, C.c_uint32]
        lib.vp8g_i420_size.restype = C.c_uint64
        lib.vp8g_decode_batch_device.argtypes = [P(Vp8gFrameDesc), C.c_void_p, C.c_uint32, P(Vp8gBatchArrays),
                                                 C.c_void_p, C.c_void_p, C.c_uint32]
        lib.vp8g_frame_digests.argtypes = [P(Vp8gFrameDesc), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                           C.c_void_p]
        lib.vp8g_reconstruct_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, P(Yuv420Image)]
        lib.vp8g_last_error.restype = C.c_char_p
        lib.vp8g_abi_version.restype = C.c_uint32
        if hasattr(lib, "vp8g_last_launch_mode"):  # (libraries built before round 5 lack it: A/B of old builds)
            lib.vp8g_last_launch_mode.restype = C.c_uint32
        if hasattr(lib, "vp8g_plan_launch"):  # (A/B of libraries built before it existed)
            lib.vp8g_plan_launch.argtypes = [P(Vp8gFrameDesc), C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                             C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_int,
                                             P(Vp8gLaunchPlan)]
        lib.yuv420_write_ppm_fd.argtypes = [C.c_int, P(Yuv420Image)]
        lib.yuv420_write_png_fd.argtypes = [C.c_int, P(Yuv420Image)]
        lib.vp8g_encoded_size.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
        lib.vp8g_encoded_size.restype = C.c_uint64
        lib.vp8g_encode_workspace_size.argtypes = [C.c_uint32]
        lib.vp8g_encode_workspace_size.restype = C.c_uint64
        lib.vp8g_make_enc_desc.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64,
                                           C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, P(Vp8gEncDesc)]
        lib.vp8g_make_enc_desc.restype = C.c_uint32
        lib.vp8g_encode_batch_device.argtypes = [P(Vp8gEncDesc), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p]
        lib.vp8g_decode_webp_batch.argtypes = [P(ByteSpan), C.c_uint32, C.c_int, C.c_uint32, P(Yuv420Image),
                                               P(C.c_int)]
        lib.vp8g_decode_webp_batch_ex.argtypes = [P(ByteSpan), C.c_uint32, C.c_int, C.c_uint32, C.c_uint32,
                                                  P(Yuv420Image), P(C.c_int)]
        lib.vp8g_m05_batch_device.argtypes = [P(Vp8gTokFrame), C.c_void_p, C.c_uint32, C.c_void_p,
                                              P(Vp8gBatchArrays), C.c_void_p]
        lib.vp8g_scaled_size.argtypes = [C.c_uint32, C.c_uint32, P(Vp8gScaleOpt), P(C.c_uint32), P(C.c_uint32)]
        lib.vp8g_make_scale_desc.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32,
                                             C.c_uint32, P(Vp8gScaleOpt), C.c_uint64, C.c_uint32, P(Vp8gScaleDesc)]
        lib.vp8g_scale_batch_device.argtypes = [P(Vp8gScaleDesc), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                                C.c_void_p]
        lib.yuv420_rescale.argtypes = [P(Yuv420Image), P(Vp8gScaleOpt), P(Yuv420Image)]
        lib.vp8g_decode_webp_batch_scaled.argtypes = [P(ByteSpan), C.c_uint32, C.c_int, C.c_uint32, C.c_uint32,
                                                      P(Vp8gScaleOpt), C.c_uint32, P(Yuv420Image), P(C.c_int)]
        if not hasattr(lib, "vp8g_tensor_batch_device"):  # (libraries built before the tensor path: A/B of old builds)
            lib._typed = True
            return lib
        lib.vp8g_tensor_slot_size.argtypes = [P(Vp8gTensorOpt)]
        lib.vp8g_tensor_slot_size.restype = C.c_uint64
        lib.vp8g_make_tensor_desc.argtypes = [P(Vp8gTensorOpt), C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32,
                                              C.c_uint64, C.c_uint32, P(Vp8gTensorDesc)]
        lib.vp8g_tensor_batch_device.argtypes = [P(Vp8gTensorDesc), C.c_void_p, C.c_uint32, P(Vp8gTensorOpt), C.c_void_p,
                                                 C.c_void_p, C.c_void_p]
        lib.vp8g_decode_webp_batch_tensor.argtypes = [P(ByteSpan), C.c_uint32, C.c_int, C.c_uint32, C.c_uint32,
                                                      P(Vp8gScaleOpt), C.c_uint32, P(Vp8gTensorOpt), C.c_void_p, P(C.c_int)]
        if hasattr(lib, "vp8g_alpha_unfilter_batch_device"):  # (libraries built before the alpha path: A/B of old builds)
            lib.vp8g_make_scale_desc_plane.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, P(Vp8gScaleOpt), C.c_uint64,
                                                       C.c_uint32, P(Vp8gScaleDesc)]
            lib.vp8g_make_alpha_desc.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint64,
                                                 C.c_uint32, C.c_uint32, P(Vp8gAlphaDesc)]
            lib.vp8g_alpha_unfilter_batch_device.argtypes = [P(Vp8gAlphaDesc), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                                             C.c_void_p]
            lib.vp8g_decode_webp_batch_x.argtypes = [P(ByteSpan), C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, P(Vp8gScaleOpt),
                                                     C.c_uint32, P(Yuv420Image), P(C.c_int)]
            lib.vp8g_decode_webp_batch_tensor_x.argtypes = [P(ByteSpan), C.c_uint32, C.c_int, C.c_uint32, C.c_uint32,
                                                            P(Vp8gScaleOpt), C.c_uint32, P(Vp8gTensorOpt), C.c_uint32, C.c_void_p,
                                                            P(C.c_int)]
            lib.vp8g_tensor_slot_size_a.argtypes = [P(Vp8gTensorOpt)]
            lib.vp8g_tensor_slot_size_a.restype = C.c_uint64
            lib.vp8g_tensor_batch_device_a.argtypes = [P(Vp8gTensorDesc), C.c_void_p, P(Vp8gTensorAlpha), C.c_void_p, C.c_uint32,
                                                       P(Vp8gTensorOpt), C.c_void_p, C.c_void_p, C.c_void_p]
        if hasattr(lib, "vp8g_lossless_batch_device"):  # (libraries built before the lossless path: A/B of old builds)
            lib.vp8g_lossless_geometry.argtypes = [P(C.c_uint32)]
            lib.vp8g_lossless_geometry.restype = None
            for name in ("vp8g_lossless_handover", "vp8g_alpha_handover"):  # (libraries built before the tests' model of the bands)
                if hasattr(lib, name):
                    getattr(lib, name).argtypes = [P(C.c_uint32)]
                    getattr(lib, name).restype = None
            lib.vp8g_make_lossless_desc.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32,
                                                    P(Vp8gLosslessTransform), C.c_uint32, P(Vp8gLosslessDesc)]
            lib.vp8g_lossless_batch_device.argtypes = [P(Vp8gLosslessDesc), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                                       C.c_void_p]
            lib.vp8g_make_tensor_argb_desc.argtypes = [P(Vp8gTensorOpt), C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32,
                                                       P(Vp8gTensorArgbDesc)]
            lib.vp8g_tensor_batch_device_argb.argtypes = [P(Vp8gTensorArgbDesc), C.c_void_p, C.c_uint32, P(Vp8gTensorOpt),
                                                          C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
            lib.vp8g_decode_webp_batch_tensor_any.argtypes = [P(ByteSpan), C.c_uint32, C.c_int, C.c_uint32, C.c_uint32,
                                                              P(Vp8gScaleOpt), C.c_uint32, P(Vp8gTensorOpt), C.c_uint32,
                                                              C.c_void_p, P(C.c_int)]
        if hasattr(lib, "vp8g_scale_argb_batch_device"):  # (libraries built before the scaled lossless path)
            lib.vp8g_scale_argb_work_size.argtypes = [C.c_uint32, C.c_uint32, P(Vp8gScaleOpt)]
            lib.vp8g_scale_argb_work_size.restype = C.c_uint64
            lib.vp8g_scale_argb_head_size.argtypes = [C.c_uint32]
            lib.vp8g_scale_argb_head_size.restype = C.c_uint64
            lib.vp8g_make_scale_argb_desc.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, P(Vp8gScaleOpt), C.c_uint64, C.c_uint64,
                                                      C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, P(Vp8gScaleArgbDesc)]
            lib.vp8g_scale_argb_batch_device.argtypes = [P(Vp8gScaleArgbDesc), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                                         C.c_void_p, C.c_void_p]
        if hasattr(lib, "vp8g_anim_compose_batch_device"):  # (libraries built before the animation path)
            lib.vp8g_anim_geometry.argtypes = [P(C.c_uint32)]
            lib.vp8g_anim_geometry.restype = None
            lib.vp8g_make_anim_desc.argtypes = [C.c_uint32, C.c_uint32, P(Vp8gAnimFrame), C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32,
                                                P(Vp8gAnimDesc)]
            lib.vp8g_anim_compose_batch_device.argtypes = [P(Vp8gAnimDesc), C.c_void_p, C.c_uint32, P(Vp8gTensorOpt), C.c_uint32,
                                                           C.c_void_p, C.c_void_p, C.c_void_p]
            lib.vp8g_anim_info.argtypes = [P(ByteSpan), C.c_uint32, P(C.c_uint32), P(C.c_uint32), P(C.c_uint32), P(C.c_uint32), P(C.c_int)]
            lib.vp8g_decode_webp_anim_tensor.argtypes = [P(ByteSpan), C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, P(Vp8gTensorOpt),
                                                         C.c_uint32, C.c_void_p, P(C.c_uint32), P(C.c_int)]
        if hasattr(lib, "vp8g_scale_argb_tensor_batch_device"):  # (libraries built before the scaled animation path)
            lib.vp8g_scale_argb_fused_geometry.argtypes = [P(C.c_uint32)]
            lib.vp8g_scale_argb_fused_geometry.restype = None
            lib.vp8g_make_scale_argb_tensor_desc.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, P(Vp8gScaleOpt), C.c_uint64, C.c_uint32,
                                                             P(Vp8gScaleArgbTensorDesc)]
            lib.vp8g_scale_argb_tensor_batch_device.argtypes = [P(Vp8gScaleArgbTensorDesc), C.c_void_p, C.c_uint32, P(Vp8gTensorOpt), C.c_uint32,
                                                                C.c_void_p, C.c_void_p, C.c_void_p]
            lib.vp8g_decode_webp_anim_tensor_scaled.argtypes = [P(ByteSpan), C.c_uint32, C.c_int, C.c_uint32, C.c_uint32, P(Vp8gScaleOpt),
                                                                C.c_uint32, C.c_uint64, P(Vp8gTensorOpt), C.c_uint32, C.c_void_p,
                                                                P(C.c_uint32), P(C.c_int)]
        if hasattr(lib, "vp8g_tensor_batch_device_444"):  # (libraries built before libwebp's scaled RGB)
            lib.vp8g_make_scale_desc_444.argtypes = lib.vp8g_make_scale_desc.argtypes
            lib.vp8g_make_tensor_desc_444.argtypes = lib.vp8g_make_tensor_desc.argtypes
            lib.vp8g_tensor_batch_device_444.argtypes = [P(Vp8gTensorDesc), C.c_void_p, P(Vp8gTensorAlpha), C.c_void_p, C.c_uint32,
                                                         P(Vp8gTensorOpt), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
            lib.vp8g_decode_webp_batch_tensor_rgb.argtypes = lib.vp8g_decode_webp_batch_tensor_any.argtypes
        lib._typed = True
    return lib


# Skew build only (lib/diag/libvp8g_skew.so under VP8G_LIB; csrc/vp8g_skew.h): wait sites in census order.
# The first SKEW_MUTANTS of them are the `early_site` values.
SKEW_SITES = ("quad_need", "quad_ring0", "frame_wg", "frame_part", "quad_flag", "quad_start", "quad_slot", "m05_ring",
              "m05_prod", "m05_up")
SKEW_MUTANTS = 5


def skew_set(seed: int, length: int, early_site: int = -1):
    """Seed and length (count of s_sleep(127)) of the delays after a publish, and the one wait site whose
    threshold is a step too low (-1: none), in both translation units that have hand-offs."""
    lib = gpu_lib()
    for tag in ("recon", "m05"):
        if getattr(lib, f"vp8g_skew_set_{tag}")(C.c_uint32(seed), C.c_uint32(length), C.c_int(early_site)) != 0:
            raise RuntimeError(f"vp8g_skew_set_{tag}({seed}, {length}, {early_site}) failed")


BAND_MUTANTS = ("none", "delay", "round", "ring", "nolong")  # csrc/vp8g_skew.h: kBandMut*


def band_mutant(kernel: str, mutant: str = "none"):
    """Skew build only: the one term of the banded schedule of `kernel` ("lossless" / "alpha") that is altered from
    the next launch on -- the band delay one step less, the round one step shorter, the ring's mask halved, the
    long-round branch dropped ("none": the shipped schedule)."""
    if getattr(gpu_lib(), f"vp8g_band_mutant_{kernel}")(C.c_uint32(BAND_MUTANTS.index(mutant))) != 0:
        raise RuntimeError(f"vp8g_band_mutant_{kernel}({mutant}) failed")


def skew_census(reset: bool = True) -> dict:
    """{site: (entered satisfied, had to spin)} since the last reset, over both translation units."""
    lib = gpu_lib()
    tot = np.zeros(2 * len(SKEW_SITES), np.int64)
    for tag in ("recon", "m05"):
        out = (C.c_uint * (2 * len(SKEW_SITES)))()
        if getattr(lib, f"vp8g_skew_census_{tag}")(out, int(reset)) != 0:
            raise RuntimeError(f"vp8g_skew_census_{tag} failed")
        tot += np.frombuffer(out, np.uint32)
    return {s: (int(tot[2 * i]), int(tot[2 * i + 1])) for i, s in enumerate(SKEW_SITES)}


class Frame:
    """Owns one Vp8DecodedFrame (+ its key-frame header) allocated by libvp8host."""

    def __init__(self, kf: Vp8KeyFrameHeader, frame: Vp8DecodedFrame):
        self.kf = kf
        self.frame = frame
        self._alive = True

    @property
    def width(self) -> int:
        return int(self.kf.width)

    @property
    def height(self) -> int:
        return int(self.kf.height)

    @property
    def mb_total(self) -> int:
        return int(self.frame.mb_total)

    def array(self, name: str) -> np.ndarray:
        for n, dt, per in FRAME_ARRAYS:
            if n == name:
                ptr = getattr(self.frame, name)
                if not ptr:
                    return np.zeros(self.mb_total * per, dtype=dt)
                return np.ctypeslib.as_array(ptr, shape=(self.mb_total * per,)).view(dt)
        raise KeyError(name)

    def free(self):
        if self._alive:
            host_lib().vp8_decoded_frame_free(C.byref(self.frame))
            self._alive = False

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def decode_file(path) -> Frame:
    lib = host_lib()
    kf, fr, st = Vp8KeyFrameHeader(), Vp8DecodedFrame(), C.c_int(0)
    if lib.vp8f_decode_file(str(path).encode(), C.byref(kf), C.byref(fr), C.byref(st)) != 0:
        raise ValueError(f"decode failed at stage {st.value}: {path}")
    return Frame(kf, fr)


def synth_frame(width: int, height: int, seed: int, profile: int = 0) -> Frame:
    lib = host_lib()
    kf, fr = Vp8KeyFrameHeader(), Vp8DecodedFrame()
    if lib.vp8f_synth_frame(width, height, seed & 0xFFFFFFFFFFFFFFFF, profile, C.byref(kf), C.byref(fr)) != 0:
        raise ValueError("synth failed")
    return Frame(kf, fr)


class PackedFrame:
    """Owns one Vp8gPackedFrame decoded by libvp8host (vp8f_decode_packed_memory)."""

    def __init__(self, data: bytes, hash_coeffs: bool = False, multi_partition: bool = False):
        self.p = Vp8gPackedFrame()
        st = C.c_int(0)
        buf = (C.c_uint8 * len(data)).from_buffer_copy(data)
        flags = (VP8F_PACK_HASH if hash_coeffs else 0) | (VP8F_MULTI_PARTITION if multi_partition else 0)
        if host_lib().vp8f_decode_packed_memory(buf, len(data), C.byref(self.p), C.byref(st), flags) != 0:
            raise ValueError(f"packed decode failed at stage {st.value}")
        self._alive = True

    def side(self, name: str) -> np.ndarray:
        per = 16 if name == "bmode" else 1
        return np.ctypeslib.as_array(getattr(self.p.f, name), shape=(int(self.p.f.mb_total) * per,)).copy()

    def masks(self) -> np.ndarray:
        return np.ctypeslib.as_array(self.p.masks, shape=(int(self.p.f.mb_total), PK_BLOCKS)).copy()

    def mb_off(self) -> np.ndarray:
        return np.ctypeslib.as_array(self.p.mb_off, shape=(int(self.p.f.mb_total),)).copy()

    def values(self) -> np.ndarray:
        n = int(self.p.n_values)
        return np.ctypeslib.as_array(self.p.values, shape=(n,)).copy() if n else np.zeros(0, np.int16)

    def free(self):
        if self._alive:
            host_lib().vp8f_packed_free(C.byref(self.p))
            self._alive = False

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def unpack_coeffs(pf: PackedFrame) -> dict:
    """Host restatement of the device expansion (expand_kernel): packed -> the four dense arrays
    (test infrastructure)."""
    masks, off, vals = pf.masks().astype(np.uint32), pf.mb_off().astype(np.int64), pf.values()
    nmb = masks.shape[0]
    dense = np.zeros((nmb, PK_BLOCKS, 16), np.int16)
    bits = ((masks[:, :, None] >> np.arange(16, dtype=np.uint32)) & 1).astype(bool)  # [mb, block, pos]
    flat = bits.reshape(nmb, -1)
    rank = np.cumsum(flat, axis=1) - 1  # index of each non-zero among the MB's values
    src = off[:, None] + rank
    dense.reshape(nmb, -1)[flat] = vals[src[flat]]
    return {"coeff_y": dense[:, :16].reshape(-1), "coeff_u": dense[:, 16:20].reshape(-1),
            "coeff_v": dense[:, 20:24].reshape(-1), "coeff_y2": dense[:, 24].reshape(-1)}


def token_header(data: bytes, multi_partition: bool = False):
    """vp8f_token_header_memory: (kf, hdr, Vp8gTokFrame, payload offset, payload size) or raises."""
    lib = host_lib()
    kf, hdr, tf = Vp8KeyFrameHeader(), Vp8DecodedFrame(), Vp8gTokFrame()
    off, size, st = C.c_uint64(0), C.c_uint32(0), C.c_int(0)
    buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(data or b"\0")
    if lib.vp8f_token_header_memory(buf, len(data), C.byref(kf), C.byref(hdr), C.byref(tf), C.byref(off),
                                    C.byref(size), C.byref(st), VP8F_MULTI_PARTITION if multi_partition else 0) != 0:
        raise ValueError(f"vp8f_token_header_memory: stage {st.value}")
    return kf, hdr, tf, off.value, size.value


def gpu_m05(files: list[bytes], multi_partition: bool = False) -> list[dict]:
    """vp8g_m05_batch_device over .webp images (one launch): per frame the m05 arrays as numpy,
    named as FRAME_ARRAYS (skip_coeff excepted: the device does not keep it)."""
    import torch
    lib = gpu_lib()
    hdrs = [token_header(b, multi_partition) for b in files]
    n = len(files)
    jobs = (Vp8gTokFrame * n)()
    slots, mbs = [], []
    bo = mo = 0
    for i, (kf, hdr, tf, off, size) in enumerate(hdrs):
        jobs[i] = tf
        jobs[i].data, jobs[i].mb_offset = bo, mo
        slots.append((bo, off, size))
        mbs.append(hdr.mb_total)
        bo += (size + 512 + 15) & ~15  # >= 512 readable bytes after each payload
        mo += hdr.mb_total
    bits = np.zeros(max(bo, 16), np.uint8)
    for (b0, off, size), data in zip(slots, files):
        bits[b0:b0 + size] = np.frombuffer(data, np.uint8, size, off)
    dev = torch.device("cuda:0")
    d_bits = torch.from_numpy(bits).to(dev)
    d_jobs = device_copy(jobs)
    per = {n_: (dt, k) for n_, dt, k in FRAME_ARRAYS}
    names = ["coeff_y", "coeff_u", "coeff_v", "coeff_y2", "ymode", "uv_mode", "segment_id", "has_coeff", "bmode"]
    tdt = {np.dtype(np.int16): torch.int16, np.dtype(np.uint8): torch.uint8}
    d = {k: torch.zeros(mo * per[k][1], dtype=tdt[np.dtype(per[k][0])], device=dev) for k in names}
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    arr = Vp8gBatchArrays(**{k: d[k].data_ptr() for k in names}, src=None, status=status.data_ptr())
    torch.cuda.synchronize()
    if lib.vp8g_m05_batch_device(jobs, d_jobs.data_ptr(), n, d_bits.data_ptr(), C.byref(arr), None) != 0:
        raise RuntimeError(f"vp8g_m05_batch_device failed: {lib.vp8g_last_error()!r}")
    torch.cuda.synchronize()
    if int(status.item()) != 0:
        raise RuntimeError(f"vp8g_m05_batch_device: device status {int(status.item())}")
    host = {k: v.cpu().numpy() for k, v in d.items()}
    out, m0 = [], 0
    for m in mbs:
        out.append({k: host[k][m0 * per[k][1]:(m0 + m) * per[k][1]] for k in names})
        m0 += m
    return out


def gpu_decode_webp_batch(files: list[bytes], filtered: bool = True, threads: int = 0, device_m05: bool = False,
                          multi_partition: bool = False):
    """vp8g_decode_webp_batch(_ex): .webp images -> (list of I420 bytes or None, list of errno).
    device_m05: m05 on the device (VP8G_BATCH_DEVICE_M05) instead of the host threads."""
    lib = gpu_lib()
    n = len(files)
    bufs, spans = S.file_spans(files)
    flags = S.batch_flags(device_m05, multi_partition)
    imgs = (Yuv420Image * n)()
    st = (C.c_int * n)()
    import time
    t0 = time.perf_counter()
    rc = lib.vp8g_decode_webp_batch_ex(spans, n, int(filtered), threads, flags, imgs, st)
    gpu_decode_webp_batch.seconds = time.perf_counter() - t0  # the C call alone (no Python copies)
    if rc != 0 and all(s == 5 for s in st):  # EIO: device failure, nothing returned
        raise RuntimeError(f"vp8g_decode_webp_batch failed: {lib.vp8g_last_error()!r}")
    return S.take_images(lib, imgs, st, with_size=False), list(st)


def scale_opt(crop=None, scale=None, dwebp_filter: bool = False, expand: bool = False) -> Vp8gScaleOpt:
    """Vp8gScaleOpt from crop = (left, top, w, h) or None and scale = (w, h) or None (0 = derived).
    expand: VP8G_SCALE_EXPAND, a target may exceed the (cropped) source in either dimension."""
    c = crop or (0, 0, 0, 0)
    s = scale or (0, 0)
    flags = (VP8G_SCALE_DWEBP_FILTER if dwebp_filter else 0) | (VP8G_SCALE_EXPAND if expand else 0)
    return Vp8gScaleOpt(c[0], c[1], c[2], c[3], s[0], s[1], flags)


def scaled_size(w: int, h: int, opt: Vp8gScaleOpt):
    """vp8f_scale_resolve: the output (w, h) of `opt` on a w x h picture; ValueError if invalid."""
    g = Vp8fScaleGeom()
    if host_lib().vp8f_scale_resolve(w, h, C.byref(opt), C.byref(g)) != 0:
        raise ValueError(f"invalid scale options for {w}x{h}")
    return int(g.out_w), int(g.out_h)


def host_scale(i420: bytes, w: int, h: int, opt: Vp8gScaleOpt):
    """vp8f_scale_i420 (the sequential CPU restatement of libwebp's rescaler) on cropped I420 bytes:
    (scaled I420 bytes, out_w, out_h)."""
    ow, oh = scaled_size(w, h, opt)
    a = np.frombuffer(i420, dtype=np.uint8)
    assert a.size == i420_size(w, h)
    cw, ch, ocw, och = (w + 1) // 2, (h + 1) // 2, (ow + 1) // 2, (oh + 1) // 2
    out = np.empty(i420_size(ow, oh), dtype=np.uint8)
    sb, ob = a.ctypes.data, out.ctypes.data
    if host_lib().vp8f_scale_i420(sb, sb + w * h, sb + w * h + cw * ch, w, cw, w, h, C.byref(opt), ob, ob + ow * oh,
                                  ob + ow * oh + ocw * och, ow, ocw) != 0:
        raise RuntimeError(f"vp8f_scale_i420 failed: errno={C.get_errno()}")
    return out.tobytes(), ow, oh


def gpu_scale(i420: bytes, w: int, h: int, opt: Vp8gScaleOpt):
    """yuv420_rescale through libvp8g.so (upload, the HIP scale kernel, download):
    (scaled I420 bytes, out_w, out_h)."""
    lib = gpu_lib()
    img, keep = image_from_i420(i420, w, h)
    out = Yuv420Image()
    if lib.yuv420_rescale(C.byref(img), C.byref(opt), C.byref(out)) != 0:
        raise RuntimeError(f"yuv420_rescale failed: errno={C.get_errno()} {lib.vp8g_last_error()!r}")
    del keep
    try:
        return _image_bytes(out), int(out.width), int(out.height)
    finally:
        lib.yuv420_free(C.byref(out))


def gpu_decode_webp_batch_scaled(files: list[bytes], scale, filtered: bool = True, threads: int = 0,
                                 device_m05: bool = False, multi_partition: bool = False):
    """vp8g_decode_webp_batch_scaled: .webp images decoded, cropped / downscaled on the device and only
    the small I420 downloaded.  scale: one Vp8gScaleOpt for every frame, or a list of one per frame.
    Returns (list of (I420 bytes, w, h) or None, list of errno)."""
    lib = gpu_lib()
    n = len(files)
    bufs, spans = S.file_spans(files)
    c_opts, nopts = S.scale_opts(scale)
    flags = S.batch_flags(device_m05, multi_partition)
    imgs = (Yuv420Image * n)()
    st = (C.c_int * n)()
    import time
    t0 = time.perf_counter()
    rc = lib.vp8g_decode_webp_batch_scaled(spans, n, int(filtered), threads, flags, c_opts, nopts, imgs, st)
    gpu_decode_webp_batch_scaled.seconds = time.perf_counter() - t0  # the C call alone
    en = C.get_errno()
    if rc != 0 and (all(s == 5 for s in st) or not any(st)):  # EIO: device failure; or the call itself refused
        raise RuntimeError(f"vp8g_decode_webp_batch_scaled failed: errno={en} {lib.vp8g_last_error()!r}")
    return S.take_images(lib, imgs, st, with_size=True), list(st)


def _c_bytes(data: bytes):
    bufs, spans = S.file_spans([data])
    return bufs[0], spans[0]


def parse_simple(data: bytes):
    """webp_parse_simple_lossy: (payload offset, payload size); OSError with its errno if refused."""
    out = (C.c_uint8 * 64)()
    buf, span = _c_bytes(data)
    if host_lib().webp_parse_simple_lossy(span, out) != 0:
        raise OSError(C.get_errno(), "webp_parse_simple_lossy")
    return int.from_bytes(bytes(out[16:24]), "little"), int.from_bytes(bytes(out[24:28]), "little")


def locate_still(data: bytes, accept: int = 0) -> dict:
    """webp_locate_still (accept: WEBP_ACCEPT_*): the fields of WebPStill but the base pointer, as a dict; OSError with
    its errno (EINVAL, ENOTSUP) if refused.  The three parsers below are views of this record."""
    s = WebPStill()
    buf, span = _c_bytes(data)
    if host_lib().webp_locate_still(span, accept, C.byref(s)) != 0:
        raise OSError(C.get_errno(), "webp_locate_still")
    return {n: int(getattr(s, n)) for n, _ in WebPStill._fields_ if n != "data"}


def parse_extended(data: bytes) -> dict:
    """webp_parse_extended: the fields of WebPContainerX as a dict, plus "alpha" (an ALPH chunk was found);
    OSError with its errno (EINVAL, ENOTSUP) if refused."""
    c = WebPContainerX()
    buf, span = _c_bytes(data)
    if host_lib().webp_parse_extended(span, C.byref(c)) != 0:
        raise OSError(C.get_errno(), "webp_parse_extended")
    d = {n: int(getattr(c, n)) for n, _ in WebPContainerX._fields_}
    d["alpha"] = d["alph_chunk_offset"] != 0
    return d


def alpha_decode_host(alph: bytes, w: int, h: int):
    """vp8f_alpha_decode of an ALPH chunk payload: (residual plane uint8 [h, w], filter, stats dict);
    OSError with its errno if the stream does not decode."""
    res = np.zeros((max(h, 0), max(w, 0)), np.uint8)
    flt, st = C.c_uint32(), Vp8fAlphaStats()
    buf, _ = _c_bytes(alph)
    if host_lib().vp8f_alpha_decode(buf, len(alph), w, h, res.ctypes.data, C.byref(flt), C.byref(st)) != 0:
        raise OSError(C.get_errno(), "vp8f_alpha_decode")
    return res, int(flt.value), {n: int(getattr(st, n)) for n in ALPHA_STATS}


def host_alpha_unfilter(residual, filter: int) -> np.ndarray:
    """vp8f_alpha_unfilter (the sequential CPU restatement of the un-prediction) of a uint8 [h, w] plane."""
    r = np.ascontiguousarray(residual, dtype=np.uint8)
    out = np.empty_like(r)
    if r.ndim != 2 or host_lib().vp8f_alpha_unfilter(r.ctypes.data, r.shape[1], r.shape[0], filter, out.ctypes.data) != 0:
        raise OSError(C.get_errno() or 22, "vp8f_alpha_unfilter")
    return out


def host_alpha_plane(data: bytes):
    """The alpha plane of an extended .webp on the host (container, ALPH decode, un-prediction): uint8 [h, w],
    or None for a picture without alpha.  OSError as the stages raise it."""
    c = parse_extended(data)
    if not c["alpha"]:
        return None
    kf = Vp8KeyFrameHeader()
    buf, _ = _c_bytes(data[c["vp8_chunk_offset"]:c["vp8_chunk_offset"] + c["vp8_chunk_size"]])
    host_lib().vp8_parse_keyframe_header(ByteSpan(C.cast(buf, C.POINTER(C.c_uint8)), c["vp8_chunk_size"]), C.byref(kf))
    res, flt, _ = alpha_decode_host(data[c["alph_chunk_offset"]:c["alph_chunk_offset"] + c["alph_chunk_size"]],
                                    kf.width, kf.height)
    return host_alpha_unfilter(res, flt)


def stage_alpha_unfilter(planes, filters, src_pad: int = 0, guard: int = 0, fill: int = 0xEE):
    """The host half of gpu_alpha_unfilter: descriptors, source bytes (rows padded by src_pad) and the guarded destination."""
    lib = gpu_lib()
    descs = (Vp8gAlphaDesc * len(planes))()
    source, dst, task0 = S.Source(), S.Guarded(guard, fill), 0
    for i, (p, f) in enumerate(zip(planes, filters)):
        h, w = np.asarray(p).shape
        padded = np.pad(np.asarray(p, dtype=np.uint8), ((0, 0), (0, src_pad)), constant_values=S.PAD)
        if lib.vp8g_make_alpha_desc(w, h, f, source.put(padded), w + src_pad, dst.add(w * h), w, task0, C.byref(descs[i])) != 0:
            raise ValueError(f"vp8g_make_alpha_desc failed: errno={C.get_errno()}")
        task0 += descs[i].ntasks
    return SimpleNamespace(descs=descs, source=source, src=source.finish(tail=0), dst=dst)


def _run(name: str, st, what: str, *opt_args, mutate=None, desc_tail: int = 0, ptr_shift=(), einval=None):
    """The device half of a staged call: upload, lib.<name>(descs, device descs, n, *opt_args, src, [work,] dst, stream),
    and the destination back on the host (a torch CPU uint8 tensor) once the guards are seen to hold their fill --
    AssertionError("<what> were written") otherwise.  ptr_shift: bytes added to the source, output and descriptor pointers."""
    work = getattr(st, "work", None)
    d_src, d_dst, d_descs = S.upload(st.src), st.dst.on_device(), device_copy(st.descs, desc_tail)
    d_work = [work.on_device()] if work else []
    if mutate:  # (after the device copies are made: the kernel never sees what a test breaks in the host copies)
        mutate()
    stream, shift = S.stream(), (*ptr_shift, 0, 0, 0)
    S.call(gpu_lib(), name, st.descs, (d_descs, shift[2]), len(st.descs), *opt_args, (d_src, shift[0]), *d_work, (d_dst, shift[1]),
           stream.cuda_stream, einval=einval, untouched=(d_dst, st.dst.fill))
    stream.synchronize()
    host = st.dst.fetch(d_dst, what)
    if work:
        work.fetch(d_work[0], what.split(":")[0] + ": bytes outside the work regions")
    return host


def gpu_alpha_unfilter(planes, filters, src_pad: int = 0, guard: int = 0, fill: int = 0xEE):
    """vp8g_alpha_unfilter_batch_device over residual planes (uint8 [h, w] each) of mixed sizes and filters in
    one launch: the list of un-predicted planes.  src_pad: extra bytes per source row (a padded stride);
    guard: bytes kept around every destination plane, which the call checks still hold `fill`."""
    st = stage_alpha_unfilter(planes, filters, src_pad, guard, fill)
    host = _run("vp8g_alpha_unfilter_batch_device", st, "gpu_alpha_unfilter: bytes outside the planes").numpy()
    return [host[o:o + n].reshape(np.asarray(p).shape).copy() for (o, n), p in zip(st.dst.regions, planes)]


def host_scale_plane(plane, opt: Vp8gScaleOpt) -> np.ndarray:
    """One uint8 [h, w] plane through vp8f_scale_i420 as its luma plane (the A plane: libwebp rescales it with the
    luma arithmetic and window)."""
    p = np.ascontiguousarray(plane, dtype=np.uint8)
    h, w = p.shape
    i420 = p.tobytes() + bytes(2 * ((w + 1) // 2) * ((h + 1) // 2))
    out, ow, oh = host_scale(i420, w, h, opt)
    return np.frombuffer(out, np.uint8, ow * oh).reshape(oh, ow).copy()


def stage_scale_planes(planes, opts):
    """The host half of gpu_scale_planes: descriptors, the planes back to back, the destination with a 16-byte tail."""
    lib = gpu_lib()
    descs = (Vp8gScaleDesc * len(planes))()
    source, dst, task0 = S.Source(), S.Guarded(0, 0xEE), 0
    for i, (p, opt) in enumerate(zip(planes, opts)):
        h, w = p.shape
        if lib.vp8g_make_scale_desc_plane(w, h, source.put(np.asarray(p, dtype=np.uint8)), w, C.byref(opt), dst.size, task0,
                                          C.byref(descs[i])) != 0:
            raise ValueError(f"vp8g_make_scale_desc_plane failed: errno={C.get_errno()}")
        task0 += descs[i].ntasks
        dst.add(descs[i].width * descs[i].height)
    dst.size += 16  # (no guards between the planes: a tail only)
    return SimpleNamespace(descs=descs, source=source, src=source.finish(tail=0), dst=dst)


def gpu_scale_planes(planes, opts):
    """vp8g_make_scale_desc_plane + vp8g_scale_batch_device over uint8 [h, w] planes (opts: one Vp8gScaleOpt per
    plane) in one launch: the list of scaled planes."""
    st = stage_scale_planes(planes, opts)
    host = _run("vp8g_scale_batch_device", st, "gpu_scale_planes: bytes after the planes").numpy()
    return [host[o:o + n].reshape(d.height, d.width).copy() for (o, n), d in zip(st.dst.regions, st.descs)]


def _dtype_name(dtype) -> str:
    name = dtype if isinstance(dtype, str) else (str(dtype) if str(dtype).startswith("torch.") else np.dtype(dtype).name)
    name = name.replace("torch.", "")
    if name not in T_DTYPES:
        raise ValueError(f"tensor dtype {dtype!r}: one of {sorted(T_DTYPES)}")
    return name


def tensor_opt(size, dtype, layout: str = "NCHW", mean=None, std=None, scale=None, bias=None,
               bgr: bool = False) -> Vp8gTensorOpt:
    """Vp8gTensorOpt for pictures of size = (w, h).  out = u8 * scale[c] + bias[c] per OUTPUT channel, either
    given directly or as mean / std on the 0..1 range (scale = 1 / (255 std), bias = -mean / std, computed in
    Python floats and stored as float32: what the structure holds is the contract).  Scalars apply to
    every channel.  Default: scale 1, bias 0."""
    if (mean is not None or std is not None) and (scale is not None or bias is not None):
        raise ValueError("give mean / std or scale / bias, not both")

    def three(v, default):
        v = default if v is None else v
        v = [v] * 3 if isinstance(v, (int, float)) else list(v)
        if len(v) != 3:
            raise ValueError("per-channel values come in threes")
        return [float(x) for x in v]

    if mean is not None or std is not None:
        m, s = three(mean, 0.0), three(std, 1.0)
        sc, bi = [1.0 / (255.0 * x) for x in s], [-a / x for a, x in zip(m, s)]
    else:
        sc, bi = three(scale, 1.0), three(bias, 0.0)
    if layout not in T_LAYOUTS:
        raise ValueError(f"tensor layout {layout!r}: NHWC or NCHW")
    return Vp8gTensorOpt(int(size[0]), int(size[1]), T_DTYPES[_dtype_name(dtype)], T_LAYOUTS[layout], VP8G_T_BGR if bgr else 0,
                         (C.c_float * 3)(*sc), (C.c_float * 3)(*bi))


def _tensor_shape(n: int, opt: Vp8gTensorOpt, channels: int = 3):
    return (n, channels, opt.height, opt.width) if opt.layout == T_LAYOUTS["NCHW"] else (n, opt.height, opt.width, channels)


def _torch_dtype(opt: Vp8gTensorOpt):
    import torch
    return (torch.uint8, torch.float16, torch.bfloat16, torch.float32)[opt.dtype]


def host_alpha_channel(alpha, opt: Vp8gTensorOpt):
    """The fourth channel of the tensor for a uint8 [h, w] alpha plane: the byte, or
    np.float32(a) / np.float32(255) (255 -> 1.0 exactly) rounded once to the 16-bit element types.  A torch CPU
    tensor [H, W]."""
    import torch
    a = np.ascontiguousarray(alpha, dtype=np.uint8)
    if opt.dtype == T_DTYPES["uint8"]:
        return torch.from_numpy(a.copy())
    f = a.astype(np.float32) / np.float32(255)
    assert f.dtype == np.float32
    if opt.dtype == T_DTYPES["float16"]:
        return torch.from_numpy(f.astype(np.float16))
    if opt.dtype == T_DTYPES["bfloat16"]:
        return torch.from_numpy(f).to(torch.bfloat16)
    return torch.from_numpy(f)


def host_tensor(i420: bytes, w: int, h: int, opt: Vp8gTensorOpt, alpha=None):
    """The numpy / torch-CPU restatement of the tensor semantics (include/vp8g.h) for one cropped
    I420 picture: the m08 restatement's RGB (oracle_encode), the channel order, a float32 multiply and
    then a float32 add, one rounding to the element type, the layout.  A torch CPU tensor [3, H, W] or
    [H, W, 3].  Tests and tools use it as the expected value.
    alpha: a uint8 [h, w] plane, or "opaque": the 4-channel tensor ([4, H, W] / [H, W, 4]) whose first three
    channels are the above and whose fourth is host_alpha_channel (§16)."""
    import torch
    assert (w, h) == (opt.width, opt.height)
    if alpha is not None:
        rgb3 = host_tensor(i420, w, h, opt)
        a = host_alpha_channel(np.full((h, w), 255, np.uint8) if isinstance(alpha, str) else alpha, opt)
        planar = opt.layout == T_LAYOUTS["NCHW"]
        return torch.cat([rgb3, a.unsqueeze(0 if planar else 2)], dim=0 if planar else 2).contiguous()
    ppm = oracle_encode(i420, w, h, "ppm")
    return _rgb_elements(np.frombuffer(ppm, np.uint8, w * h * 3, len(ppm) - w * h * 3).reshape(h, w, 3), opt)


def _rgb_elements(rgb, opt: Vp8gTensorOpt):
    """host_tensor from the RGB bytes on ([h, w, 3] uint8): channel order, elements, layout."""
    import torch
    if opt.flags & VP8G_T_BGR:
        rgb = rgb[:, :, ::-1]
    if opt.dtype == T_DTYPES["uint8"]:
        out = torch.from_numpy(np.array(rgb))  # (a writable, contiguous copy)
    else:
        scale, bias = np.array(list(opt.scale), np.float32), np.array(list(opt.bias), np.float32)
        f = rgb.astype(np.float32) * scale + bias  # (two float32 operations, each rounded to nearest)
        assert f.dtype == np.float32
        if opt.dtype == T_DTYPES["float16"]:
            with np.errstate(over="ignore"):
                out = torch.from_numpy(f.astype(np.float16))
        elif opt.dtype == T_DTYPES["bfloat16"]:
            out = torch.from_numpy(f).to(torch.bfloat16)
        else:
            out = torch.from_numpy(f)
    return out.permute(2, 0, 1).contiguous() if opt.layout == T_LAYOUTS["NCHW"] else out.contiguous()


def gpu_tensor(i420_list, w: int, h: int, opt: Vp8gTensorOpt, alpha=None):
    """vp8g_tensor_batch_device over cropped I420 pictures of one size: upload them, one launch, and the
    torch.Tensor [N, 3, H, W] or [N, H, W, 3] it leaves on the device.
    alpha: a list with one uint8 [h, w] plane or None (opaque) per picture: vp8g_tensor_batch_device_a, the
    4-channel tensor."""
    import torch
    lib = gpu_lib()
    dev = torch.device("cuda", 0)
    n, fsz, cw, ch = len(i420_list), i420_size(w, h), (w + 1) // 2, (h + 1) // 2
    slot = lib.vp8g_tensor_slot_size(C.byref(opt)) if alpha is None else lib.vp8g_tensor_slot_size_a(C.byref(opt))
    if not slot or (w, h) != (opt.width, opt.height) or any(len(b) != fsz for b in i420_list):
        raise ValueError("gpu_tensor: invalid options or picture sizes")
    descs = (Vp8gTensorDesc * n)()
    task0 = 0
    for i in range(n):
        o = i * fsz
        if lib.vp8g_make_tensor_desc(C.byref(opt), o, o + w * h, o + w * h + cw * ch, w, cw, i * slot, task0,
                                     C.byref(descs[i])) != 0:
            raise ValueError("vp8g_make_tensor_desc failed")
        task0 += descs[i].ntasks
    d_descs = device_copy(descs)
    stream = torch.cuda.current_stream(dev)
    if alpha is not None:
        if len(alpha) != n:
            raise ValueError("gpu_tensor: one alpha entry per picture")
        al, parts, ao = (Vp8gTensorAlpha * n)(), [], n * fsz
        for i, a in enumerate(alpha):
            if a is None:
                al[i] = Vp8gTensorAlpha(T_OPAQUE, 0, 0)
                continue
            a = np.ascontiguousarray(a, dtype=np.uint8)
            if a.shape != (h, w):
                raise ValueError("gpu_tensor: alpha plane of another size")
            al[i] = Vp8gTensorAlpha(ao, w, 0)
            parts.append(a.reshape(-1))
            ao += w * h
        src = S.upload(np.concatenate([np.frombuffer(b"".join(i420_list), dtype=np.uint8)] + parts))
        d_al = device_copy(al)
        out = torch.empty(_tensor_shape(n, opt, 4), dtype=_torch_dtype(opt), device=dev)
        S.call(lib, "vp8g_tensor_batch_device_a", descs, d_descs, al, d_al, n, C.byref(opt), src, out, stream.cuda_stream)
    else:
        src = S.upload(np.frombuffer(b"".join(i420_list), dtype=np.uint8).copy())
        out = torch.empty(_tensor_shape(n, opt), dtype=_torch_dtype(opt), device=dev)
        S.call(lib, "vp8g_tensor_batch_device", descs, d_descs, n, C.byref(opt), src, out, stream.cuda_stream)
    stream.synchronize()
    return out


# ---- scaled RGB exact to libwebp's: 4:4:4 planes ----------------------------


def yuv_to_rgb(y, u, v) -> np.ndarray:
    """libwebp's VP8YuvToRgb on uint8 arrays of one shape: [..., 3] uint8 (14-bit fixed point, clip of v >> 6)."""
    y, u, v = (np.asarray(a).astype(np.int32) for a in (y, u, v))
    yy = (y * 19077) >> 8
    r = yy + ((v * 26149) >> 8) - 14234
    g = yy - ((u * 6419) >> 8) - ((v * 13320) >> 8) + 8708
    b = yy + ((u * 33050) >> 8) - 17685
    return (np.clip(np.stack([r, g, b], axis=-1), 0, 16383) >> 6).astype(np.uint8)


def host_scale_yuv444(i420: bytes, w: int, h: int, opt: Vp8gScaleOpt) -> np.ndarray:
    """vp8f_scale_yuv444 on I420 bytes: the three planes libwebp converts to a scaled RGB picture, uint8 [3, oh, ow]
    (Y, U, V each rescaled straight to the target size).  ValueError for an option that does not fit or has no target size."""
    a = np.frombuffer(i420, dtype=np.uint8)
    assert a.size == i420_size(w, h)
    if not (opt.scaled_w or opt.scaled_h):
        raise ValueError("host_scale_yuv444: an option without a target size")
    ow, oh = scaled_size(w, h, opt)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    out = np.empty((3, oh, ow), np.uint8)
    sb, ob = a.ctypes.data, out.ctypes.data
    if host_lib().vp8f_scale_yuv444(sb, sb + w * h, sb + w * h + cw * ch, w, cw, w, h, C.byref(opt), ob, ob + ow * oh, ob + 2 * ow * oh) != 0:
        raise RuntimeError(f"vp8f_scale_yuv444 failed: errno={C.get_errno()}")
    return out


def host_scale_rgb(i420: bytes, w: int, h: int, opt: Vp8gScaleOpt, alpha=None) -> np.ndarray:
    """libwebp's scaled RGB of a decoded lossy picture on the host (WebPDecode with use_scaling into MODE_RGB, or, with
    alpha = the picture's uint8 [h, w] plane, MODE_RGBA): uint8 [oh, ow, 3 | 4].  The I420 must be decoded as libwebp
    decodes for that option (vp8f_scale_filtered with VP8G_SCALE_DWEBP_FILTER)."""
    p = host_scale_yuv444(i420, w, h, opt)
    rgb = yuv_to_rgb(p[0], p[1], p[2])
    if alpha is None:
        return rgb
    return np.concatenate([rgb, host_scale_plane(alpha, opt)[:, :, None]], axis=2)


def host_tensor_444(planes, opt: Vp8gTensorOpt, alpha=None):
    """host_tensor for three uint8 [h, w] planes (Y, U, V of the picture's own size): pixel = VP8YuvToRgb of its own
    samples, then the elements and layout of host_tensor.  alpha as there."""
    import torch
    y, u, v = (np.asarray(p, dtype=np.uint8) for p in planes)
    assert y.shape == u.shape == v.shape == (opt.height, opt.width)
    rgb3 = _rgb_elements(yuv_to_rgb(y, u, v), opt)
    if alpha is None:
        return rgb3
    a = host_alpha_channel(np.full(y.shape, 255, np.uint8) if isinstance(alpha, str) else alpha, opt)
    planar = opt.layout == T_LAYOUTS["NCHW"]
    return torch.cat([rgb3, a.unsqueeze(0 if planar else 2)], dim=0 if planar else 2).contiguous()


def stage_scale_batch(jobs, guard: int = 64, fill: int = 0xEE, src_shift: int = 1):
    """The host half of gpu_scale_batch.  jobs: (kind, data, w, h, opt) with kind "444" (I420 bytes through
    vp8g_make_scale_desc_444), "420" (I420 bytes through vp8g_make_scale_desc) or "plane" (a uint8 [h, w] plane through
    vp8g_make_scale_desc_plane).  Every source starts src_shift bytes off a 16-byte boundary; every output has guard bytes
    around it."""
    lib = gpu_lib()
    descs = (Vp8gScaleDesc * len(jobs))()
    source, dst, task0, shapes = S.Source(), S.Guarded(guard, fill), 0, []
    for i, (kind, data, w, h, opt) in enumerate(jobs):
        ow, oh = scaled_size(w, h, opt)
        cw, ch = (w + 1) // 2, (h + 1) // 2
        if kind == "plane":
            o = source.put(np.asarray(data, dtype=np.uint8).reshape(h, w), 16, src_shift)
            rc = lib.vp8g_make_scale_desc_plane(w, h, o, w, C.byref(opt), dst.add(ow * oh), task0, C.byref(descs[i]))
            shapes.append((oh, ow))
        else:
            a = np.frombuffer(data, np.uint8)
            assert a.size == i420_size(w, h)
            o = source.put(a, 16, src_shift)
            if kind == "444":
                rc = lib.vp8g_make_scale_desc_444(w, h, o, o + w * h, o + w * h + cw * ch, w, cw, C.byref(opt), dst.add(3 * ow * oh), task0,
                                                  C.byref(descs[i]))
                shapes.append((3, oh, ow))
            else:
                rc = lib.vp8g_make_scale_desc(w, h, o, o + w * h, o + w * h + cw * ch, w, cw, C.byref(opt), dst.add(i420_size(ow, oh)), task0,
                                              C.byref(descs[i]))
                shapes.append((i420_size(ow, oh),))
        if rc != 0:
            raise ValueError(f"scale descriptor {i} ({kind}) refused: errno={C.get_errno()}")
        task0 += descs[i].ntasks
    return SimpleNamespace(descs=descs, source=source, src=source.finish(), dst=dst, shapes=shapes)


def gpu_scale_batch(jobs, guard: int = 64, fill: int = 0xEE, src_shift: int = 1):
    """vp8g_scale_batch_device over mixed descriptors (stage_scale_batch) in one call: per job the three planes uint8
    [3, oh, ow] ("444"), the scaled I420 bytes as a flat uint8 array ("420") or the plane uint8 [oh, ow] ("plane")."""
    st = stage_scale_batch(jobs, guard, fill, src_shift)
    host = _run("vp8g_scale_batch_device", st, "gpu_scale_batch: bytes outside the outputs").numpy()
    return [host[o:o + n].reshape(shape).copy() for (o, n), shape in zip(st.dst.regions, st.shapes)]


def gpu_scale_yuv444(i420_list, sizes, opts):
    """vp8g_make_scale_desc_444 + vp8g_scale_batch_device over I420 pictures (sizes: (w, h) each; opts: one Vp8gScaleOpt
    each) in one launch: the list of uint8 [3, oh, ow] planes, as host_scale_yuv444 gives them."""
    return gpu_scale_batch([("444", b, w, h, o) for b, (w, h), o in zip(i420_list, sizes, opts)])


def stage_tensor_444(planes_list, w: int, h: int, opt: Vp8gTensorOpt, alpha=None, guard: int = 64, fill: int = 0xEE, src_shift: int = 1,
                     src_pad: int = 0):
    """The host half of gpu_tensor_444: descriptors (and alpha entries), the planes -- every one src_shift bytes off a
    16-byte boundary, rows padded by src_pad -- and the destination with guard bytes around every slot."""
    lib = gpu_lib()
    n, channels = len(planes_list), 3 if alpha is None else 4
    if alpha is not None and len(alpha) != n:
        raise ValueError("gpu_tensor_444: one alpha entry per picture")
    slot = lib.vp8g_tensor_slot_size(C.byref(opt)) if alpha is None else lib.vp8g_tensor_slot_size_a(C.byref(opt))
    if not slot or (w, h) != (opt.width, opt.height):
        raise ValueError("gpu_tensor_444: invalid options or picture size")
    descs, al = (Vp8gTensorDesc * n)(), (Vp8gTensorAlpha * n)() if alpha is not None else None
    source, dst, task0 = S.Source(), S.Guarded(guard, fill), 0

    def put(plane):
        p = np.asarray(plane, dtype=np.uint8)
        if p.shape != (h, w):
            raise ValueError("gpu_tensor_444: a plane of another size")
        return source.put(np.pad(p, ((0, 0), (0, src_pad)), constant_values=S.PAD), 16, src_shift)

    for i, planes in enumerate(planes_list):
        oy, ou, ov = (put(p) for p in planes)
        if lib.vp8g_make_tensor_desc_444(C.byref(opt), oy, ou, ov, w + src_pad, w + src_pad, dst.add(slot), task0, C.byref(descs[i])) != 0:
            raise ValueError("vp8g_make_tensor_desc_444 failed")
        task0 += descs[i].ntasks
        if alpha is not None:
            al[i] = Vp8gTensorAlpha(T_OPAQUE, 0, 0) if alpha[i] is None else Vp8gTensorAlpha(put(alpha[i]), w + src_pad, 0)
    return SimpleNamespace(descs=descs, alpha=al, channels=channels, source=source, src=source.finish(), dst=dst, opt=opt)


def run_tensor_444(st, mutate=None, null=(), channels=None, ptr_shift=(0, 0), einval=None):
    """The device half: upload, vp8g_tensor_batch_device_444, and the slots back as torch CPU tensors ([C, H, W] or
    [H, W, C] each) once the guard bytes are seen to hold their fill.  For the refusals: mutate() breaks the host copies
    after the device copies are made, null names arguments passed as NULL ("descs", "d_descs", "alpha", "d_alpha", "src",
    "dst"), channels overrides the count, ptr_shift = bytes added to the (source, output) pointers; einval as S.call."""
    import torch
    opt = st.opt
    d_src, d_dst, d_descs = S.upload(st.src), st.dst.on_device(), device_copy(st.descs)
    d_al = device_copy(st.alpha) if st.alpha is not None else None
    if mutate:
        mutate()
    args = {"descs": st.descs, "d_descs": d_descs, "alpha": st.alpha, "d_alpha": d_al, "src": (d_src, ptr_shift[0]), "dst": (d_dst, ptr_shift[1])}
    a = {k: (None if k in null else v) for k, v in args.items()}
    stream = S.stream()
    S.call(gpu_lib(), "vp8g_tensor_batch_device_444", a["descs"], a["d_descs"], a["alpha"], a["d_alpha"], len(st.descs), C.byref(opt),
           st.channels if channels is None else channels, a["src"], a["dst"], stream.cuda_stream, einval=einval,
           untouched=(d_dst, st.dst.fill))
    stream.synchronize()
    host = st.dst.fetch(d_dst, "gpu_tensor_444: bytes outside the slots")
    shape = _tensor_shape(1, opt, st.channels)[1:]
    return [host[o:o + nb].clone().view(_torch_dtype(opt)).reshape(shape) for o, nb in st.dst.regions]


def gpu_tensor_444(planes_list, w: int, h: int, opt: Vp8gTensorOpt, alpha=None, **stage):
    """vp8g_tensor_batch_device_444 over pictures given as (Y, U, V) uint8 [h, w] planes of one size, in one launch: the
    list of torch CPU tensors [3, H, W] / [H, W, 3] (4 channels with alpha: a list with one uint8 [h, w] plane or None
    = opaque per picture).  The planes start off their alignment and the slots sit between guard bytes (stage_tensor_444)."""
    return run_tensor_444(stage_tensor_444(planes_list, w, h, opt, alpha, **stage))


# ---- lossless (VP8L) images -------------------------------------------------


def parse_any(data: bytes) -> dict:
    """webp_parse_any: the fields of WebPContainerL as a dict, plus "alpha" and "lossless" (the image chunk is
    VP8L); OSError with its errno (EINVAL, ENOTSUP) if refused."""
    c = WebPContainerL()
    buf, span = _c_bytes(data)
    if host_lib().webp_parse_any(span, C.byref(c)) != 0:
        raise OSError(C.get_errno(), "webp_parse_any")
    d = {n: int(getattr(c, n)) for n, _ in WebPContainerL._fields_}
    d["alpha"] = d["alph_chunk_offset"] != 0
    d["lossless"] = d["vp8l_chunk_offset"] != 0
    return d


def _sub_shape(t: dict, h: int):
    r = (1 << t["bits"]) - 1
    return ((h + r) >> t["bits"], (t["xsize"] + r) >> t["bits"])


def lossless_decode_host(data: bytes) -> dict:
    """vp8f_lossless_decode of a VP8L chunk payload: {"width", "height", "alpha_hint", "residual": uint32
    [h, xsize], "transforms": [{"type", "bits", "xsize", "ncolors", "data": uint32 array (the sub-image [bh, bw]
    or the colour table)}, ...] in stream order, "stats": dict}; OSError with its errno if the stream does not decode."""
    im, st = Vp8fLosslessImage(), Vp8fAlphaStats()
    buf, _ = _c_bytes(data)
    lib = host_lib()
    if lib.vp8f_lossless_decode(buf, len(data), C.byref(im), C.byref(st)) != 0:
        raise OSError(C.get_errno(), "vp8f_lossless_decode")
    try:
        h, xs = int(im.height), int(im.xsize)
        out = {"width": int(im.width), "height": h, "alpha_hint": int(im.alpha_hint),
               "residual": np.ctypeslib.as_array(im.argb, (h, xs)).copy(), "transforms": [],
               "stats": {n: int(getattr(st, n)) for n in ALPHA_STATS}}
        for k in range(im.ntransforms):
            t = {n: int(getattr(im.tr[k], n)) for n in ("type", "bits", "xsize", "ncolors")}
            if t["type"] == L_COLOR_INDEX:
                t["data"] = np.ctypeslib.as_array(im.tr[k].data, (t["ncolors"],)).copy()
            elif t["type"] == L_SUBTRACT_GREEN:
                t["data"] = np.zeros(0, np.uint32)
            else:
                t["data"] = np.ctypeslib.as_array(im.tr[k].data, _sub_shape(t, h)).copy()
            out["transforms"].append(t)
    finally:
        lib.vp8f_lossless_free(C.byref(im))
    return out


def lossless_image(residual, transforms, width: int | None = None) -> dict:
    """An image in lossless_decode_host's form from a uint32 [h, xsize] residual and a list of transforms (dicts
    with "type", "bits" and, by type, "data" / "ncolors"): xsize is filled in as the stream would have it."""
    res = np.ascontiguousarray(residual, dtype=np.uint32)
    h = res.shape[0]
    packs = [t["bits"] for t in transforms if t["type"] == L_COLOR_INDEX]
    if width is None:
        if packs and packs[0]:
            raise ValueError("lossless_image: give the width of an image with packed pixels")
        width = res.shape[1]
    xs, trs = width, []
    for t in transforms:
        t = dict(t, xsize=xs, ncolors=int(t.get("ncolors", 0)))
        t["data"] = np.ascontiguousarray(t.get("data", np.zeros(0, np.uint32)), dtype=np.uint32)
        if t["type"] == L_COLOR_INDEX:
            t["ncolors"] = t["data"].size
            xs = (xs + (1 << t["bits"]) - 1) >> t["bits"]
        trs.append(t)
    if xs != res.shape[1]:
        raise ValueError("lossless_image: residual width does not match the transforms")
    return {"width": width, "height": h, "alpha_hint": 1, "residual": res, "transforms": trs}


def lossless_struct(img: dict):
    """The Vp8fLosslessImage of an image in lossless_decode_host's form, and the arrays it points into (keep them)."""
    im = Vp8fLosslessImage()
    res = np.ascontiguousarray(img["residual"], dtype=np.uint32)
    keep = [res]
    if res.shape[0] != img["height"]:
        raise ValueError("lossless_struct: residual of another height")
    im.width, im.height, im.xsize, im.ntransforms = img["width"], img["height"], res.shape[1], len(img["transforms"])
    im.argb = res.ctypes.data_as(C.POINTER(C.c_uint32))
    for k, t in enumerate(img["transforms"]):
        d = np.ascontiguousarray(t["data"], dtype=np.uint32)
        keep.append(d)
        im.tr[k].type, im.tr[k].bits, im.tr[k].xsize, im.tr[k].ncolors = t["type"], t["bits"], t["xsize"], t["ncolors"]
        if t["type"] in (L_PREDICTOR, L_CROSS_COLOR) and d.shape != _sub_shape(t, img["height"]):
            raise ValueError("lossless_struct: sub-image of another size")
        im.tr[k].data = d.ctypes.data_as(C.POINTER(C.c_uint32)) if d.size else None
    return im, keep


def host_lossless_apply(img: dict) -> np.ndarray:
    """vp8f_lossless_apply (the sequential CPU restatement of the inverse transforms) of an image in
    lossless_decode_host's form: uint32 [h, w] 0xAARRGGBB."""
    im, keep = lossless_struct(img)
    out = np.empty((img["height"], img["width"]), np.uint32)
    if host_lib().vp8f_lossless_apply(C.byref(im), out.ctypes.data) != 0:
        raise OSError(C.get_errno() or 22, "vp8f_lossless_apply")
    return out


def argb_to_rgba(argb) -> np.ndarray:
    """uint32 [h, w] 0xAARRGGBB -> uint8 [h, w, 4] R, G, B, A (WebPDecodeRGBA's bytes)."""
    a = np.asarray(argb, dtype=np.uint32)
    return np.stack([(a >> 16) & 255, (a >> 8) & 255, a & 255, a >> 24], axis=-1).astype(np.uint8)


def host_lossless_argb(data: bytes) -> np.ndarray:
    """A lossless .webp on the host: container, entropy decode, inverse transforms.  uint32 [h, w]."""
    c = parse_any(data)
    if not c["lossless"]:
        raise OSError(22, "not a lossless file")
    return host_lossless_apply(lossless_decode_host(data[c["vp8l_chunk_offset"]:c["vp8l_chunk_offset"] + c["vp8l_chunk_size"]]))


def stage_lossless_argb(images, src_shift: int = 1, guard: int = 64, fill: int = 0xEE):
    """The host half of gpu_lossless_argb: descriptors, the residual images, sub-images and colour tables src_shift bytes
    off a dword boundary, the guarded destination."""
    lib = gpu_lib()
    descs = (Vp8gLosslessDesc * len(images))()
    source, dst = S.Source(), S.Guarded(guard, fill)
    for i, img in enumerate(images):
        tr = (Vp8gLosslessTransform * 4)()
        src = source.put(np.asarray(img["residual"], dtype=np.uint32), 4, src_shift)
        for k, t in enumerate(img["transforms"]):
            data = np.asarray(t["data"], dtype=np.uint32)
            tr[k] = Vp8gLosslessTransform(source.put(data, 4, src_shift) if data.size else 0, t["type"], t["bits"], t["xsize"], t["ncolors"])
        if lib.vp8g_make_lossless_desc(img["width"], img["height"], src, dst.add(4 * img["width"] * img["height"]), len(img["transforms"]),
                                       tr, i, C.byref(descs[i])) != 0:
            raise ValueError(f"vp8g_make_lossless_desc failed: errno={C.get_errno()}")
    return SimpleNamespace(descs=descs, source=source, src=source.finish(), dst=dst)


def gpu_lossless_argb(images, src_shift: int = 1, guard: int = 64, fill: int = 0xEE):
    """vp8g_lossless_batch_device over images in lossless_decode_host's form, of mixed sizes and transform lists, in
    one launch: the list of uint32 [h, w] pictures.  src_shift: every residual image, sub-image and colour table
    starts at an offset that is this much off a dword boundary; guard: bytes kept around every output, which the
    call checks still hold `fill`."""
    st = stage_lossless_argb(images, src_shift, guard, fill)
    host = _run("vp8g_lossless_batch_device", st, "gpu_lossless_argb: bytes outside the images").numpy()
    return [host[o:o + n].view(np.uint32).reshape(img["height"], img["width"]).copy() for (o, n), img in zip(st.dst.regions, images)]


def scaled_size_argb(w: int, h: int, opt: Vp8gScaleOpt):
    """vp8f_scale_resolve_argb: ((left, top, win_w, win_h), (out_w, out_h)) of `opt` on a w x h ARGB picture -- the
    window's origin as given, not rounded to even; ValueError if invalid."""
    g = Vp8fScaleGeom()
    if host_lib().vp8f_scale_resolve_argb(w, h, C.byref(opt), C.byref(g)) != 0:
        raise ValueError(f"invalid scale options for {w}x{h}")
    return (int(g.left), int(g.top), int(g.win_w), int(g.win_h)), (int(g.out_w), int(g.out_h))


def host_argb_mult(argb, inverse: bool = False) -> np.ndarray:
    """vp8f_argb_mult_row: libwebp's alpha premultiply (or its inverse) of uint32 0xAARRGGBB pixels; a copy."""
    a = np.array(argb, dtype=np.uint32)
    flat = np.ascontiguousarray(a.reshape(-1))
    host_lib().vp8f_argb_mult_row(flat.ctypes.data, flat.size, int(inverse))
    return flat.reshape(a.shape)


def host_scale_argb(argb, opt: Vp8gScaleOpt) -> np.ndarray:
    """vp8f_argb_scale (the sequential CPU restatement of libwebp's crop / rescale of a lossless picture) of a uint32
    [h, w] 0xAARRGGBB picture: uint32 [h', w'].  OSError with its errno (EINVAL) if the option does not fit."""
    a = np.ascontiguousarray(argb, dtype=np.uint32)
    h, w = a.shape
    g = Vp8fScaleGeom()
    lib = host_lib()
    if lib.vp8f_scale_resolve_argb(w, h, C.byref(opt), C.byref(g)) != 0:
        raise OSError(C.get_errno() or 22, "vp8f_scale_resolve_argb")
    out = np.empty((g.out_h, g.out_w), np.uint32)
    if lib.vp8f_argb_scale(a.ctypes.data, w, h, C.byref(opt), out.ctypes.data) != 0:
        raise OSError(C.get_errno() or 22, "vp8f_argb_scale")
    return out


def stage_scale_argb(argb_list, opts, src_shift: int = 1, guard: int = 64, fill: int = 0xEE):
    """The host half of gpu_scale_argb: descriptors, the pictures src_shift dwords off a 16-byte boundary, the guarded work
    area (its head exempt) and the guarded destination of 16-byte outputs."""
    lib = gpu_lib()
    n = len(argb_list)
    descs = (Vp8gScaleArgbDesc * n)()
    source, dst = S.Source(), S.Guarded(guard, fill, round_to=16)
    work = S.Guarded(guard, fill, head=int(lib.vp8g_scale_argb_head_size(n)))
    planes = t_split = t_scale = t_merge = 0
    for i, (a, opt) in enumerate(zip(argb_list, opts)):
        a = np.asarray(a, dtype=np.uint32)
        h, w = a.shape
        if lib.vp8g_make_scale_argb_desc(w, h, source.put(a, 16, 4 * src_shift), C.byref(opt), work.size, dst.size, planes, t_split, t_scale,
                                         t_merge, C.byref(descs[i])) != 0:
            raise ValueError(f"vp8g_make_scale_argb_desc failed: errno={C.get_errno()}")
        d = descs[i]
        assert d.work_bytes == lib.vp8g_scale_argb_work_size(w, h, C.byref(opt))
        planes, t_split, t_scale, t_merge = planes + d.nplanes, t_split + d.split_ntasks, t_scale + d.scale_ntasks, t_merge + d.merge_ntasks
        work.add(d.work_bytes)
        dst.add(4 * d.width * d.height)
    return SimpleNamespace(descs=descs, source=source, src=source.finish(), dst=dst, work=work)


def gpu_scale_argb(argb_list, opts, src_shift: int = 1, guard: int = 64, fill: int = 0xEE):
    """vp8g_make_scale_argb_desc + vp8g_scale_argb_batch_device over uint32 [h, w] 0xAARRGGBB pictures of mixed sizes
    (opts: one Vp8gScaleOpt per picture) in one launch: the list of scaled uint32 [h', w'] pictures.  src_shift: every
    source picture starts this many DWORDS off a 16-byte boundary; guard (a multiple of 16): bytes kept around every
    picture's work region and every output, which the call checks still hold `fill`."""
    st = stage_scale_argb(argb_list, opts, src_shift, guard, fill)
    host = _run("vp8g_scale_argb_batch_device", st, "gpu_scale_argb: bytes outside the outputs").numpy()
    return [host[o:o + n].view(np.uint32).reshape(d.height, d.width).copy() for (o, n), d in zip(st.dst.regions, st.descs)]


def host_tensor_argb(argb, opt: Vp8gTensorOpt, channels: int = 4):
    """The numpy / torch-CPU restatement of vp8g_tensor_batch_device_argb for one uint32 [h, w] 0xAARRGGBB picture:
    R, G, B as host_tensor treats them (the channel order, a float32 multiply and then a float32 add, one rounding),
    A as host_alpha_channel, the layout.  A torch CPU tensor [C, H, W] or [H, W, C]."""
    import torch
    rgba = argb_to_rgba(argb)
    assert rgba.shape[:2] == (opt.height, opt.width) and channels in (3, 4)
    rgb = rgba[:, :, :3]
    if opt.flags & VP8G_T_BGR:
        rgb = rgb[:, :, ::-1]
    if opt.dtype == T_DTYPES["uint8"]:
        out = torch.from_numpy(np.array(rgb))
    else:
        scale, bias = np.array(list(opt.scale), np.float32), np.array(list(opt.bias), np.float32)
        f = rgb.astype(np.float32) * scale + bias  # (two float32 operations, each rounded to nearest)
        assert f.dtype == np.float32
        if opt.dtype == T_DTYPES["float16"]:
            with np.errstate(over="ignore"):
                out = torch.from_numpy(f.astype(np.float16))
        elif opt.dtype == T_DTYPES["bfloat16"]:
            out = torch.from_numpy(f).to(torch.bfloat16)
        else:
            out = torch.from_numpy(f)
    if channels == 4:
        out = torch.cat([out, host_alpha_channel(rgba[:, :, 3], opt).unsqueeze(2)], dim=2)
    return out.permute(2, 0, 1).contiguous() if opt.layout == T_LAYOUTS["NCHW"] else out.contiguous()


def gpu_tensor_argb(argb_list, opt: Vp8gTensorOpt, channels: int = 4, slot_shift: int = 0):
    """vp8g_tensor_batch_device_argb over uint32 [h, w] pictures of the tensor's size: upload them, one launch, and the
    torch.Tensor [N, C, H, W] or [N, H, W, C] it leaves on the device.  slot_shift: the tensor starts this many
    ELEMENTS into its allocation (a slot that is not 16-byte aligned)."""
    import torch
    lib = gpu_lib()
    dev = torch.device("cuda", 0)
    n, w, h = len(argb_list), opt.width, opt.height
    slot = lib.vp8g_tensor_slot_size(C.byref(opt)) if channels == 3 else lib.vp8g_tensor_slot_size_a(C.byref(opt))
    if not slot or any(np.asarray(a).shape != (h, w) for a in argb_list):
        raise ValueError("gpu_tensor_argb: invalid options or picture sizes")
    descs = (Vp8gTensorArgbDesc * n)()
    task0 = 0
    for i in range(n):
        if lib.vp8g_make_tensor_argb_desc(C.byref(opt), channels, i * 4 * w * h, i * slot, task0, C.byref(descs[i])) != 0:
            raise ValueError("vp8g_make_tensor_argb_desc failed")
        task0 += descs[i].ntasks
    src = S.upload(np.concatenate([np.ascontiguousarray(a, dtype=np.uint32).reshape(-1) for a in argb_list]).view(np.uint8))
    d_descs = device_copy(descs)
    shape = _tensor_shape(n, opt, channels)
    flat = torch.zeros(int(np.prod(shape)) + slot_shift, dtype=_torch_dtype(opt), device=dev)
    out = flat[slot_shift:].view(shape)
    stream = torch.cuda.current_stream(dev)
    S.call(lib, "vp8g_tensor_batch_device_argb", descs, d_descs, n, C.byref(opt), channels, src, out, stream.cuda_stream)
    stream.synchronize()
    return out


def scale_argb_fused_geometry():
    """vp8g_scale_argb_fused_geometry: (pixels per 16-byte load, pixels of the longest row segment a task stages, source
    rows per run) of the fused kernel as the library was built.  The boundary sizes of the tests come from it."""
    g = (C.c_uint32 * 3)()
    gpu_lib().vp8g_scale_argb_fused_geometry(g)
    return int(g[0]), int(g[1]), int(g[2])


def make_scale_argb_tensor_desc(w: int, h: int, opt: Vp8gScaleOpt, src: int = 0, dst: int = 0, task0: int = 0) -> Vp8gScaleArgbTensorDesc:
    """vp8g_make_scale_argb_tensor_desc for a w x h picture; OSError with its errno (EINVAL, or ENOTSUP for valid options
    that are not the fused kernel's) if refused."""
    d = Vp8gScaleArgbTensorDesc()
    if gpu_lib().vp8g_make_scale_argb_tensor_desc(w, h, src, C.byref(opt), dst, task0, C.byref(d)) != 0:
        raise OSError(C.get_errno(), "vp8g_make_scale_argb_tensor_desc")
    return d


def stage_scale_argb_tensor(argb_list, opts, topt: Vp8gTensorOpt, channels: int = 4, src_shift: int = 1, guard: int = 64, fill: int = 0xEE):
    """The host half of gpu_scale_argb_tensor: descriptors, the pictures src_shift dwords off a 16-byte boundary, the guarded
    destination of 8-byte slots.  OSError with the maker's errno if it refuses a picture."""
    lib = gpu_lib()
    descs = (Vp8gScaleArgbTensorDesc * len(argb_list))()
    source, dst, task0 = S.Source(), S.Guarded(guard, fill, round_to=8), 0
    for i, (a, opt) in enumerate(zip(argb_list, opts)):
        a = np.asarray(a, dtype=np.uint32)
        h, w = a.shape
        if lib.vp8g_make_scale_argb_tensor_desc(w, h, source.put(a, 16, 4 * src_shift), C.byref(opt), dst.size, task0, C.byref(descs[i])) != 0:
            raise OSError(C.get_errno(), "vp8g_make_scale_argb_tensor_desc")
        task0 += descs[i].ntasks
        dst.add(channels * descs[i].width * descs[i].height * T_ELEM[topt.dtype])
    return SimpleNamespace(descs=descs, source=source, src=source.finish(), dst=dst)


def gpu_scale_argb_tensor(argb_list, opts, topt: Vp8gTensorOpt, channels: int = 4, src_shift: int = 1, guard: int = 64, fill: int = 0xEE,
                          mutate=None, ptr_shift=(0, 0, 0)):
    """vp8g_make_scale_argb_tensor_desc + vp8g_scale_argb_tensor_batch_device over uint32 [h, w] 0xAARRGGBB pictures of mixed
    sizes (opts: one Vp8gScaleOpt per picture) in one launch: the list of torch CPU tensors [C, h', w'] or [h', w', C] of
    topt's dtype (topt's width and height are not read).  src_shift: every source picture starts this many DWORDS off a
    16-byte boundary; guard (a multiple of 8): bytes kept in front of, between and behind the slots, which the call checks
    still hold `fill`.  mutate(descs): called on the host descriptors after the device copies are made; ptr_shift: bytes
    added to the source, output and descriptor pointers handed to the call (both for tests of the entry point's checks: a
    refusal raises ValueError, once the output is seen untouched)."""
    st = stage_scale_argb_tensor(argb_list, opts, topt, channels, src_shift, guard, fill)
    host = _run("vp8g_scale_argb_tensor_batch_device", st, "gpu_scale_argb_tensor: bytes outside the slots", C.byref(topt), channels,
                mutate=mutate and (lambda: mutate(st.descs)), desc_tail=8, ptr_shift=ptr_shift, einval=ValueError)
    planar = topt.layout == T_LAYOUTS["NCHW"]
    return [host[o:o + n].clone().view(_torch_dtype(topt)).view((channels, d.height, d.width) if planar else (d.height, d.width, channels))
            for (o, n), d in zip(st.dst.regions, st.descs)]


# ---- animated files ---------------------------------------------------------


def parse_anim(data: bytes) -> dict:
    """webp_parse_anim: {"canvas": [w, h], "loop_count", "bgcolor", "vp8x_flags", "frames": [{the fields of
    WebPAnimFrame}, ...]}; OSError with EINVAL if refused (a still picture included)."""
    info = WebPAnimInfo()
    buf, span = _c_bytes(data)
    lib = host_lib()
    if lib.webp_parse_anim(span, C.byref(info), None, 0) != 0:
        raise OSError(C.get_errno(), "webp_parse_anim")
    fr = (WebPAnimFrame * info.nframes)()
    if lib.webp_parse_anim(span, C.byref(info), fr, info.nframes) != 0:
        raise OSError(C.get_errno(), "webp_parse_anim")
    return {"canvas": [int(info.canvas_width), int(info.canvas_height)], "loop_count": int(info.loop_count),
            "bgcolor": int(info.bgcolor), "vp8x_flags": int(info.vp8x_flags),
            "frames": [{n: int(getattr(f, n)) for n, _ in WebPAnimFrame._fields_} for f in fr]}


def wrap_anim_frame(data: bytes, f: dict) -> bytes:
    """One frame of parse_anim(data) as a file of its own: 'VP8 ' alone, VP8X + ALPH + 'VP8 ', or 'VP8L' (what the
    end-to-end entry hands to the still-picture decoder)."""
    def chunk(tag, off, n):
        return tag + n.to_bytes(4, "little") + data[off:off + n] + (b"\0" if n & 1 else b"")
    if f["vp8l_size"]:
        body = chunk(b"VP8L", f["vp8l_offset"], f["vp8l_size"])
    else:
        body = chunk(b"VP8 ", f["vp8_offset"], f["vp8_size"])
        if f["alph_size"] or f["alph_offset"]:
            x = bytes([0x10, 0, 0, 0]) + (f["width"] - 1).to_bytes(3, "little") + (f["height"] - 1).to_bytes(3, "little")
            body = b"VP8X" + (10).to_bytes(4, "little") + x + chunk(b"ALPH", f["alph_offset"], f["alph_size"]) + body
    return b"RIFF" + (len(body) + 4).to_bytes(4, "little") + b"WEBP" + body


def decode_lossy_still(data: bytes, c: dict | None = None) -> Frame:
    """The VP8 frame of a lossy still (simple or extended container; c = its parse_any record) through the host front end."""
    c = c or parse_any(data)
    kf, fr, st = Vp8KeyFrameHeader(), Vp8DecodedFrame(), C.c_int(0)
    p = data[c["vp8_chunk_offset"]:c["vp8_chunk_offset"] + c["vp8_chunk_size"]]
    simple = b"RIFF" + (len(p) + (len(p) & 1) + 12).to_bytes(4, "little") + b"WEBPVP8 " + len(p).to_bytes(4, "little") + p + (
        b"\0" if len(p) & 1 else b"")
    buf, _ = _c_bytes(simple)
    if host_lib().vp8f_decode_memory(buf, len(simple), C.byref(kf), C.byref(fr), C.byref(st)) != 0:
        raise OSError(C.get_errno() or 22, f"vp8f_decode_memory (stage {st.value})")
    return Frame(kf, fr)


def host_still_scaled_rgb(data: bytes, opt: Vp8gScaleOpt, channels: int = 4) -> np.ndarray:
    """A lossy still .webp on the host as libwebp decodes it into MODE_RGB / MODE_RGBA with the cropping / scaling of
    `opt` (which has a target size): front end, the oracle's reconstruction with the loop filter as
    vp8f_scale_filtered decides it, host_scale_rgb with the alpha plane of host_alpha_plane (opaque without one).
    uint8 [oh, ow, channels]."""
    c = parse_any(data)
    f = decode_lossy_still(data, c)
    w, h = f.width, f.height
    i420 = oracle_reconstruct(f, bool(host_lib().vp8f_scale_filtered(w, h, C.byref(opt), 1)))
    f.free()
    a = host_alpha_plane(data) if channels == 4 and c["extended"] else None
    rgb = host_scale_rgb(i420, w, h, opt, a)
    if channels == 3 or a is not None:
        return rgb
    # (a picture without alpha is opaque: libwebp rescales no plane for it -- a rescaled plane of 255 is not 255 everywhere)
    return np.concatenate([rgb, np.full(rgb.shape[:2] + (1,), 255, np.uint8)], axis=2)


def host_still_argb(data: bytes) -> np.ndarray:
    """A still .webp (lossy, lossy with alpha, or lossless) on the host as uint32 [h, w] 0xAARRGGBB, the bytes
    WebPDecodeRGBA gives: the lossless restatement, or the oracle's reconstruction (loop filter on) and RGB conversion
    with the alpha plane of host_alpha_plane (255 without one)."""
    c = parse_any(data)
    if c["lossless"]:
        return host_lossless_argb(data)
    f = decode_lossy_still(data, c)
    w, h = f.width, f.height
    ppm = oracle_encode(oracle_reconstruct(f, True), w, h, "ppm")
    f.free()
    rgb = np.frombuffer(ppm, np.uint8)[len(ppm) - 3 * w * h:].reshape(h, w, 3).astype(np.uint32)
    a = host_alpha_plane(data) if c["extended"] else None
    a = np.full((h, w), 255, np.uint32) if a is None else a.astype(np.uint32)
    return a << 24 | rgb[:, :, 0] << 16 | rgb[:, :, 1] << 8 | rgb[:, :, 2]


def host_anim_frames(data: bytes):
    """An animated file's frames decoded on the host: ([w, h] of the canvas, list of frames in host_anim_compose's
    form, list of cumulative end times in ms)."""
    a = parse_anim(data)
    frames, ts, t = [], [], 0
    for f in a["frames"]:
        frames.append({"argb": host_still_argb(wrap_anim_frame(data, f)), "x": f["x"], "y": f["y"], "blend": f["blend"],
                       "dispose": f["dispose"], "has_alpha": f["has_alpha"]})
        t += f["duration"]
        ts.append(t)
    return a["canvas"], frames, ts


def _anim_host_structs(frames):
    fr = (Vp8fAnimFrame * len(frames))()
    keep = []
    for k, f in enumerate(frames):
        a = np.ascontiguousarray(f["argb"], dtype=np.uint32)
        keep.append(a)
        fr[k] = Vp8fAnimFrame(a.ctypes.data, f["x"], f["y"], a.shape[1], a.shape[0], int(f["blend"]), int(f["dispose"]),
                              int(f["has_alpha"]), 0)
    return fr, keep


def host_anim_compose(canvas_w: int, canvas_h: int, frames):
    """vp8f_anim_compose (the sequential CPU restatement of libwebp's WebPAnimDecoder) over frames given as dicts
    {"argb": uint32 [h, w], "x", "y", "blend", "dispose", "has_alpha"}: (uint32 [F, canvas_h, canvas_w] canvases,
    list of key-frame flags).  OSError with its errno (EINVAL) for a frame outside the canvas."""
    fr, keep = _anim_host_structs(frames)
    out = np.empty((len(frames), canvas_h, canvas_w), np.uint32)
    lib = host_lib()
    if lib.vp8f_anim_compose(canvas_w, canvas_h, fr, len(frames), out.ctypes.data) != 0:
        raise OSError(C.get_errno() or 22, "vp8f_anim_compose")
    if lib.vp8f_anim_keyframes(canvas_w, canvas_h, fr, len(frames)) != 0:
        raise OSError(C.get_errno() or 22, "vp8f_anim_keyframes")
    return out, [int(f.key) for f in fr]


def host_anim_scaled(data: bytes, opt: Vp8gScaleOpt):
    """Every scaled canvas of an animated file on the host: host_anim_compose, then host_scale_argb of
    each canvas with `opt` resolved against the canvas.  (uint32 [F, h', w'], timestamps); OSError with EINVAL if the
    option does not fit the canvas."""
    (cw, ch), frames, ts = host_anim_frames(data)
    canvases, _ = host_anim_compose(cw, ch, frames)
    return np.stack([host_scale_argb(c, opt) for c in canvases]), ts


def anim_geometry():
    """vp8g_anim_geometry: (pixels per thread, pixels per task, frames per task or 0 for no limit) of the compositor
    kernel as the library was built.  The boundary sizes of the tests come from it."""
    g = (C.c_uint32 * 3)()
    gpu_lib().vp8g_anim_geometry(g)
    return int(g[0]), int(g[1]), int(g[2])


def anim_records(frames, srcs):
    """The Vp8gAnimFrame array of frames in host_anim_compose's form whose pictures sit at byte offsets srcs."""
    rec = (Vp8gAnimFrame * len(frames))()
    for k, f in enumerate(frames):
        h, w = np.asarray(f["argb"]).shape
        rec[k] = Vp8gAnimFrame(srcs[k], f["x"], f["y"], w, h, (ANIM_BLEND if f["blend"] else 0) | (ANIM_DISPOSE if f["dispose"] else 0)
                               | (ANIM_HAS_ALPHA if f["has_alpha"] else 0), 0, 0, 0)
    return rec


def stage_anim_compose(anims, opt: Vp8gTensorOpt, channels: int = 4, src_shift: int = 1, guard: int = 64, fill: int = 0xEE):
    """The host half of gpu_anim_compose: descriptors, every frame picture src_shift dwords off a 16-byte boundary with each
    animation's record array (`recs`, as vp8g_make_anim_desc completed them) behind its pictures, the guarded destination."""
    lib = gpu_lib()
    descs = (Vp8gAnimDesc * len(anims))()
    source, dst, task0, recs = S.Source(), S.Guarded(guard, fill), 0, []
    for i, (cw, ch, frames) in enumerate(anims):
        rec = anim_records(frames, [source.put(np.asarray(f["argb"], dtype=np.uint32), 16, 4 * src_shift) for f in frames])
        at = source.reserve(C.sizeof(rec), 8)  # (its offset goes into the descriptor, whose maker completes the records)
        if lib.vp8g_make_anim_desc(cw, ch, rec, len(frames), at, dst.add(len(frames) * channels * cw * ch * T_ELEM[opt.dtype]), task0,
                                   C.byref(descs[i])) != 0:
            raise ValueError(f"vp8g_make_anim_desc failed: errno={C.get_errno()}")
        source.fill(at, bytes(rec))
        task0 += descs[i].ntasks
        recs.append(rec)
    return SimpleNamespace(descs=descs, source=source, src=source.finish(), dst=dst, recs=recs)


def gpu_anim_compose(anims, opt: Vp8gTensorOpt, channels: int = 4, src_shift: int = 1, guard: int = 64, fill: int = 0xEE,
                     mutate=None, ptr_shift=(0, 0)):
    """vp8g_make_anim_desc + vp8g_anim_compose_batch_device over animations [(canvas_w, canvas_h, frames in
    host_anim_compose's form), ...] of mixed canvases and frame counts in one launch: the list of torch CPU tensors
    [F, C, H, W] or [F, H, W, C] of opt's dtype (opt's width and height are not read).  src_shift: every frame picture
    starts this many DWORDS off a 16-byte boundary; guard (a multiple of 8): bytes kept in front of, between and behind
    the animations' canvases, which the call checks still hold `fill` (an animation's canvases are contiguous: a write
    into a neighbouring canvas shows in the comparison).  mutate(descs, records): called on the host descriptors and the
    list of record arrays after the device copies are made; ptr_shift: bytes added to the source and output pointers handed
    to the call (both for tests of the entry point's checks: a refusal raises ValueError, once the output is seen
    untouched)."""
    st = stage_anim_compose(anims, opt, channels, src_shift, guard, fill)
    host = _run("vp8g_anim_compose_batch_device", st, "gpu_anim_compose: bytes outside the canvases", C.byref(opt), channels,
                mutate=mutate and (lambda: mutate(st.descs, st.recs)), ptr_shift=ptr_shift, einval=ValueError)
    planar = opt.layout == T_LAYOUTS["NCHW"]
    return [host[o:o + n].clone().view(_torch_dtype(opt)).view((len(fr), channels, ch, cw) if planar else (len(fr), ch, cw, channels))
            for (o, n), (cw, ch, fr) in zip(st.dst.regions, anims)]


def anim_info(files: list[bytes]):
    """vp8g_anim_info: (list of {"canvas": [w, h], "nframes", "loop_count"}, list of errno) -- a refused file has no frames."""
    lib = gpu_lib()
    n = len(files)
    bufs, spans = S.file_spans(files)
    cw, ch, nf, lc = ((C.c_uint32 * n)() for _ in range(4))
    st = (C.c_int * n)()
    lib.vp8g_anim_info(spans, n, cw, ch, nf, lc, st)
    return [{"canvas": [int(cw[i]), int(ch[i])], "nframes": int(nf[i]), "loop_count": int(lc[i])} for i in range(n)], list(st)


def gpu_decode_webp_anim_tensor(files: list[bytes], opt: Vp8gTensorOpt, alpha: bool = True, filtered: bool = True, threads: int = 0,
                                device_m05: bool = False, multi_partition: bool = False, prefill=None, scale=None, stage_bytes: int = 0):
    """vp8g_decode_webp_anim_tensor: animated .webp files decoded and composited on the device into one dense tensor
    of canvases, [sum of frames, C, H, W] or [.., H, W, C] with C = 4 (alpha) or 3.  Returns (the torch.Tensor on the
    device, each file's first slot, the timestamps (cumulative end time in ms of every slot), list of errno); the
    slots of a failed file are zero, and a file that is no animation has none.  torch only allocates the tensor
    (prefill: a value it is filled with before the call, for tests of the zero slots).
    scale: None (vp8g_decode_webp_anim_tensor: every canvas must have the tensor's size), or one Vp8gScaleOpt, or a list of
    one per file -- vp8g_decode_webp_anim_tensor_scaled: each file's canvases cropped and rescaled to the tensor's size as
    host_anim_scaled does; stage_bytes caps the canvas bytes of one staging group (0: the library's default)."""
    import time
    import torch
    lib = gpu_lib()
    n = len(files)
    info, _ = anim_info(files)
    first = [sum(a["nframes"] for a in info[:i]) for i in range(n)]
    total = sum(a["nframes"] for a in info)
    bufs, spans = S.file_spans(files)
    channels = 4 if alpha else 3
    dev = torch.device("cuda", 0)
    out = torch.empty(_tensor_shape(max(total, 1), opt, channels), dtype=_torch_dtype(opt), device=dev)
    if prefill is not None:
        out.fill_(prefill)
    torch.cuda.synchronize(dev)
    ts = (C.c_uint32 * max(total, 1))()
    st = (C.c_int * n)()
    c_opts, nopts = S.scale_opts(scale)
    bflags = S.batch_flags(device_m05, multi_partition)
    t0 = time.perf_counter()
    if scale is None:
        rc = lib.vp8g_decode_webp_anim_tensor(spans, n, int(filtered), threads, bflags, C.byref(opt), channels, C.c_void_p(out.data_ptr()),
                                              ts, st)
    else:
        rc = lib.vp8g_decode_webp_anim_tensor_scaled(spans, n, int(filtered), threads, bflags, c_opts, nopts, stage_bytes, C.byref(opt),
                                                     channels, C.c_void_p(out.data_ptr()), ts, st)
    gpu_decode_webp_anim_tensor.seconds = time.perf_counter() - t0  # the C call alone
    en = C.get_errno()
    if rc != 0 and (all(s == st[0] for s in st) and st[0] in (5, 12) or not any(st)):  # EIO / ENOMEM: every file; or the call itself refused
        raise RuntimeError(f"vp8g_decode_webp_anim_tensor failed: errno={en} {lib.vp8g_last_error()!r}")
    return out[:total], first, list(ts)[:total], list(st)


def gpu_decode_webp_batch_x(files: list[bytes], scale=None, filtered: bool = True, threads: int = 0, device_m05: bool = False,
                            multi_partition: bool = False):
    """vp8g_decode_webp_batch_x: gpu_decode_webp_batch_scaled (scale: None, one Vp8gScaleOpt, or a list of one per
    frame) with the extended container in front; alpha is ignored.  Returns (list of (I420 bytes, w, h) or
    None, list of errno)."""
    lib = gpu_lib()
    n = len(files)
    bufs, spans = S.file_spans(files)
    c_opts, nopts = S.scale_opts(scale)
    bflags = S.batch_flags(device_m05, multi_partition)
    imgs = (Yuv420Image * n)()
    st = (C.c_int * n)()
    rc = lib.vp8g_decode_webp_batch_x(spans, n, int(filtered), threads, bflags, c_opts, nopts, imgs, st)
    en = C.get_errno()
    if rc != 0 and (all(s == 5 for s in st) or not any(st)):  # EIO: device failure; or the call itself refused
        raise RuntimeError(f"vp8g_decode_webp_batch_x failed: errno={en} {lib.vp8g_last_error()!r}")
    return S.take_images(lib, imgs, st, with_size=True), list(st)


def gpu_decode_webp_batch_tensor(files: list[bytes], opt: Vp8gTensorOpt, scale=None, filtered: bool = True, threads: int = 0,
                                 device_m05: bool = False, multi_partition: bool = False, extended: bool = False,
                                 alpha: bool = False, lossless: bool = False, lossless_scale: bool = False, libwebp_rgb: bool = False):
    """vp8g_decode_webp_batch_tensor: .webp images decoded, optionally cropped / downscaled (scale: None,
    one Vp8gScaleOpt for every frame, or a list of one per frame), converted and left on the device.
    Returns (torch.Tensor on the device, [N, 3, H, W] or [N, H, W, 3] of the requested dtype, list of
    errno); the slot of a failed frame is zero.  extended: vp8g_decode_webp_batch_tensor_x (VP8X files decode);
    alpha: with VP8G_X_ALPHA, the tensor has four channels (R, G, B, A; opaque A for a picture without alpha).
    lossless: vp8g_decode_webp_batch_tensor_any with VP8G_X_LOSSLESS (implies the extended container): lossless
    (VP8L) files decode beside the lossy ones; one whose scale option is not the identity gets ENOTSUP, unless
    lossless_scale (VP8G_X_LOSSLESS_SCALE; needs lossless): then a lossless file's option is applied as libwebp applies
    it to such a file -- the crop window's origin as given, not rounded to even, and RGBA bit-exact to libwebp's
    (host_scale_argb) -- and only an option that does not fit the file, or whose result is not the tensor's size, fails
    (EINVAL).  libwebp_rgb: vp8g_decode_webp_batch_tensor_rgb with the flags the other keywords give (implies the extended
    container): a lossy file whose option has a target size gets libwebp's own scaled RGB -- Y, U and V each rescaled to
    the target, VP8YuvToRgb per pixel, no upsampler (host_scale_rgb; dwebp -ppm -scale with dwebp_filter) -- and every other
    frame goes as without it.  torch only allocates the tensor: its data_ptr() is handed to the C call."""
    import time
    import torch
    extended = extended or alpha  # (alpha arrives through the _x call only)
    lib = gpu_lib()
    n = len(files)
    bufs, spans = S.file_spans(files)
    c_opts, nopts = S.scale_opts(scale)
    bflags = S.batch_flags(device_m05, multi_partition)
    if not lib.vp8g_tensor_slot_size(C.byref(opt)):
        raise ValueError("gpu_decode_webp_batch_tensor: invalid tensor options")
    dev = torch.device("cuda", 0)
    out = torch.empty(_tensor_shape(n, opt, 4 if alpha else 3), dtype=_torch_dtype(opt), device=dev)
    torch.cuda.synchronize(dev)
    st = (C.c_int * n)()
    t0 = time.perf_counter()
    if lossless or lossless_scale or libwebp_rgb:
        entry = lib.vp8g_decode_webp_batch_tensor_rgb if libwebp_rgb else lib.vp8g_decode_webp_batch_tensor_any
        rc = entry(spans, n, int(filtered), threads, bflags, c_opts, nopts, C.byref(opt),
                   (VP8G_X_LOSSLESS if lossless else 0) | (VP8G_X_ALPHA if alpha else 0) | (VP8G_X_LOSSLESS_SCALE if lossless_scale else 0),
                   C.c_void_p(out.data_ptr()), st)
    elif extended:  # (routed to the _x call only when asked)
        rc = lib.vp8g_decode_webp_batch_tensor_x(spans, n, int(filtered), threads, bflags, c_opts, nopts, C.byref(opt),
                                                 VP8G_X_ALPHA if alpha else 0, C.c_void_p(out.data_ptr()), st)
    else:
        rc = lib.vp8g_decode_webp_batch_tensor(spans, n, int(filtered), threads, bflags, c_opts, nopts, C.byref(opt),
                                               C.c_void_p(out.data_ptr()), st)
    gpu_decode_webp_batch_tensor.seconds = time.perf_counter() - t0  # the C call alone
    en = C.get_errno()
    if rc != 0 and (all(s == 5 for s in st) or not any(st)):  # EIO: device failure; or the call itself refused
        raise RuntimeError(f"vp8g_decode_webp_batch_tensor failed: errno={en} {lib.vp8g_last_error()!r}")
    return out, list(st)


def fnv1a64(buf: bytes | np.ndarray, h: int = 1469598103934665603) -> int:
    b = np.ascontiguousarray(np.frombuffer(buf, dtype=np.uint8) if isinstance(buf, (bytes, bytearray)) else buf)
    return int(host_lib().vp8f_fnv1a64(b.ctypes.data, b.nbytes, h))


def gpu_reconstruct(f: Frame, filtered: bool) -> bytes:
    """Reference entry point vp8_reconstruct_keyframe_yuv[_filtered] through libvp8g.so."""
    lib = gpu_lib()
    img = Yuv420Image()
    fn = lib.vp8_reconstruct_keyframe_yuv_filtered if filtered else lib.vp8_reconstruct_keyframe_yuv
    if fn(C.byref(f.kf), C.byref(f.frame), C.byref(img)) != 0:
        raise RuntimeError(f"vp8g reconstruction failed: errno={C.get_errno()} {lib.vp8g_last_error()!r}")
    try:
        return _image_bytes(img)
    finally:
        lib.yuv420_free(C.byref(img))


def gpu_reconstruct_batch(frames: list[Frame], filtered: bool) -> list[bytes]:
    lib = gpu_lib()
    n = len(frames)
    kfs = (C.POINTER(Vp8KeyFrameHeader) * n)(*[C.pointer(f.kf) for f in frames])
    frs = (C.POINTER(Vp8DecodedFrame) * n)(*[C.pointer(f.frame) for f in frames])
    imgs = (Yuv420Image * n)()
    if lib.vp8g_reconstruct_batch(C.cast(kfs, C.c_void_p), C.cast(frs, C.c_void_p), n, int(filtered), imgs) != 0:
        raise RuntimeError(f"vp8g batch failed: {lib.vp8g_last_error()!r}")
    out = []
    for i in range(n):
        out.append(_image_bytes(imgs[i]))
        lib.yuv420_free(C.byref(imgs[i]))
    return out


def gpu_encode(i420: bytes, w: int, h: int, fmt: str) -> bytes:
    """The reference's m08/m09 writers (yuv420_write_ppm_fd / yuv420_write_png_fd) through
    libvp8g.so: the file they write for a cropped I420 image."""
    import tempfile
    lib = gpu_lib()
    img, keep = image_from_i420(i420, w, h)
    fn = lib.yuv420_write_ppm_fd if fmt == "ppm" else lib.yuv420_write_png_fd
    with tempfile.TemporaryFile() as t:
        if fn(t.fileno(), C.byref(img)) != 0:
            raise RuntimeError(f"vp8g {fmt} writer failed: errno={C.get_errno()} {lib.vp8g_last_error()!r}")
        t.seek(0)
        data = t.read()
    del keep
    return data


def make_enc_descs(sizes, fmt: str, src_offsets, out_align: int = 256):
    """Descriptors for images of the given (w, h) sizes whose planes sit at src_offsets[i] =
    (y, u, v) with tight strides, outputs packed at out_align-aligned offsets.  Returns
    (array of Vp8gEncDesc, output offsets, total output bytes, total tasks)."""
    lib = gpu_lib()
    n = len(sizes)
    descs = (Vp8gEncDesc * n)()
    outs, o, span0 = [], 0, 0
    for i, (w, h) in enumerate(sizes):
        y, u, v = src_offsets[i]
        k = lib.vp8g_make_enc_desc(w, h, ENC_FORMATS[fmt], y, u, v, w, (w + 1) // 2, o, span0, C.byref(descs[i]))
        if k == 0:
            raise ValueError(f"vp8g_make_enc_desc failed for {w}x{h} {fmt}")
        outs.append(o)
        o = (o + descs[i].file_len + out_align - 1) // out_align * out_align
        span0 += k
    return descs, outs, o, span0


def make_desc(f: Frame, filtered: bool, mb_offset: int, out_offset: int) -> Vp8gFrameDesc:
    d = Vp8gFrameDesc()
    if gpu_lib().vp8g_make_frame_desc(C.byref(f.kf), C.byref(f.frame), int(filtered), mb_offset, out_offset,
                                      C.byref(d)) != 0:
        raise ValueError("vp8g_make_frame_desc failed")
    return d


# ---- test/bench-only loaders (oracle/ is test infrastructure) ------------------------------

def oracle_lib():
    lib = _load("oracle", REPO_DIR / "oracle" / "liboracle.so")
    if not getattr(lib, "_typed", False):
        P = C.POINTER
        lib.oracle_reconstruct_i420.argtypes = [P(Vp8KeyFrameHeader), P(Vp8DecodedFrame), C.c_void_p, C.c_int]
        lib.oracle_recon_padded.argtypes = [P(Vp8DecodedFrame), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        lib.oracle_loopfilter.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, P(Vp8DecodedFrame)]
        lib.oracle_time_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        lib.oracle_time_batch.restype = C.c_double
        lib.oracle_ppm_size.argtypes = [C.c_uint32, C.c_uint32]
        lib.oracle_ppm_size.restype = C.c_size_t
        lib.oracle_png_size.argtypes = [C.c_uint32, C.c_uint32]
        lib.oracle_png_size.restype = C.c_size_t
        lib.oracle_ppm.argtypes = [P(Yuv420Image), C.c_void_p, C.c_size_t]
        lib.oracle_ppm.restype = C.c_long
        lib.oracle_png.argtypes = [P(Yuv420Image), C.c_void_p, C.c_size_t]
        lib.oracle_png.restype = C.c_long
        lib._typed = True
    return lib


def image_from_i420(buf: bytes, w: int, h: int):
    """A Yuv420Image view of cropped I420 bytes (Y w*h, U, V each ceil(w/2)*ceil(h/2)); the
    returned numpy array keeps the memory alive."""
    a = np.frombuffer(buf, dtype=np.uint8).copy()
    cw, ch = (w + 1) // 2, (h + 1) // 2
    img = Yuv420Image(w, h, w, cw)
    base = a.ctypes.data
    img.y = C.cast(base, C.POINTER(C.c_uint8))
    img.u = C.cast(base + w * h, C.POINTER(C.c_uint8))
    img.v = C.cast(base + w * h + cw * ch, C.POINTER(C.c_uint8))
    return img, a


def oracle_encode(i420: bytes, w: int, h: int, fmt: str) -> bytes:
    """m08/m09 restatement: the PPM ("ppm") or PNG ("png") file of a cropped I420 image."""
    lib = oracle_lib()
    img, keep = image_from_i420(i420, w, h)
    n = (lib.oracle_ppm_size if fmt == "ppm" else lib.oracle_png_size)(w, h)
    out = np.empty(n, dtype=np.uint8)
    got = (lib.oracle_ppm if fmt == "ppm" else lib.oracle_png)(C.byref(img), out.ctypes.data, n)
    del keep
    if got != n:
        raise RuntimeError(f"oracle {fmt} failed ({got} of {n})")
    return out.tobytes()


def oracle_reconstruct(f: Frame, filtered: bool) -> bytes:
    buf = np.empty(i420_size(f.width, f.height), dtype=np.uint8)
    if oracle_lib().oracle_reconstruct_i420(C.byref(f.kf), C.byref(f.frame), buf.ctypes.data, int(filtered)) != 0:
        raise RuntimeError("oracle failed")
    return buf.tobytes()


LF_KINDS = ("simple", "normal MB edge", "normal sub-block edge")
LF_CELLS = ("mask fail", "pass, hev", "pass, no hev")


def oracle_loopfilter_census(planes, frame: Vp8DecodedFrame) -> np.ndarray:
    """oracle_loopfilter_census on padded planes (y, u, v as uint8 arrays; they are not modified):
    uint64[3][3] of edge positions the oracle's loop-filter walk visits, [LF_KINDS][LF_CELLS]."""
    lib = oracle_lib()
    # bound here, not in oracle_lib(): a liboracle.so built before the census existed still serves every other call
    if not hasattr(lib, "oracle_loopfilter_census"):
        raise OSError("oracle/liboracle.so has no oracle_loopfilter_census (rebuild it: `make` at the repo root)")
    lib.oracle_loopfilter_census.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Vp8DecodedFrame), C.c_void_p]
    counts = np.zeros((3, 3), dtype=np.uint64)
    y, u, v = [np.ascontiguousarray(p, dtype=np.uint8) for p in planes]
    if lib.oracle_loopfilter_census(y.ctypes.data, u.ctypes.data, v.ctypes.data, C.byref(frame),
                                             counts.ctypes.data) != 0:
        raise RuntimeError("oracle census failed")
    return counts


def oracle_frame_census(f: Frame) -> np.ndarray:
    """The census of the loop filter on the frame's own unfiltered reconstruction (what the filtered
    decode of `f` makes the filter do)."""
    w, h = int(f.frame.mb_cols) * 16, int(f.frame.mb_rows) * 16
    y, u, v = np.empty(w * h, np.uint8), np.empty(w * h // 4, np.uint8), np.empty(w * h // 4, np.uint8)
    if oracle_lib().oracle_recon_padded(C.byref(f.frame), y.ctypes.data, u.ctypes.data, v.ctypes.data, 0) != 0:
        raise RuntimeError("oracle failed")
    return oracle_loopfilter_census((y, u, v), f.frame)


# oracle_loopfilter_arith_census (oracle/vp8_oracle.h): counts[LF_ARITH_PATHS][cell]; cell 0 of every path is
# the number of filtered positions, None marks a cell the path does not have
LF_ARITH_PATHS = ("simple", "MB edge, hev", "MB edge, no hev (MB adjust)", "sub-block edge, hev", "sub-block edge, no hev")
_OUTER = ("calls", "p1-q1 > 127", "p1-q1 < -128", "a > 127", "a < -128", "a in 124..127", "q0-f1 < 0", "q0-f1 > 255",
          "p0+f2 < 0", "p0+f2 > 255", None, None)
_INNER = _OUTER[:1] + (None, None) + _OUTER[3:10] + ("p1+a2 | q1-a2 < 0", "p1+a2 | q1-a2 > 255")
_MBADJ = ("calls", "w > 127", "w < -128", "p1/q1 tap < 0", "p1/q1 tap > 255", "p2/q2 tap < 0", "p2/q2 tap > 255",
          "p1-q1 > 127", "p1-q1 < -128", "p0/q0 tap < 0", "p0/q0 tap > 255", None)
LF_ARITH_CELLS = (_OUTER, _OUTER, _MBADJ, _OUTER, _INNER)


def oracle_loopfilter_arith_census(planes, frame: Vp8DecodedFrame) -> np.ndarray:
    """oracle_loopfilter_arith_census on padded planes (y, u, v as uint8 arrays; they are not modified):
    uint64[5][12], per path of the filter how many edge positions drive each clamp of its arithmetic,
    [LF_ARITH_PATHS][LF_ARITH_CELLS[path]]."""
    lib = oracle_lib()
    # bound here, as oracle_loopfilter_census is: an older liboracle.so still serves every other call
    if not hasattr(lib, "oracle_loopfilter_arith_census"):
        raise OSError("oracle/liboracle.so has no oracle_loopfilter_arith_census (rebuild it: `make` at the repo root)")
    lib.oracle_loopfilter_arith_census.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Vp8DecodedFrame), C.c_void_p]
    counts = np.zeros((len(LF_ARITH_PATHS), len(_OUTER)), dtype=np.uint64)
    y, u, v = [np.ascontiguousarray(p, dtype=np.uint8) for p in planes]
    if lib.oracle_loopfilter_arith_census(y.ctypes.data, u.ctypes.data, v.ctypes.data, C.byref(frame),
                                          counts.ctypes.data) != 0:
        raise RuntimeError("oracle arithmetic census failed")
    return counts


def oracle_frame_arith_census(f: Frame) -> np.ndarray:
    """The arithmetic census of the loop filter on the frame's own unfiltered reconstruction."""
    w, h = int(f.frame.mb_cols) * 16, int(f.frame.mb_rows) * 16
    y, u, v = np.empty(w * h, np.uint8), np.empty(w * h // 4, np.uint8), np.empty(w * h // 4, np.uint8)
    if oracle_lib().oracle_recon_padded(C.byref(f.frame), y.ctypes.data, u.ctypes.data, v.ctypes.data, 0) != 0:
        raise RuntimeError("oracle failed")
    return oracle_loopfilter_arith_census((y, u, v), f.frame)


def ref_lib():
    """oracle/_ref/libref.so: the reference's own m01-m07 compiled here (may be absent)."""
    lib = _load("ref", REPO_DIR / "oracle" / "_ref" / "libref.so")
    if not getattr(lib, "_typed", False):
        P = C.POINTER
        lib.ref_decode_i420.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.c_int]
        lib.ref_decode_i420.restype = C.c_long
        lib.ref_recon_i420.argtypes = [P(Vp8KeyFrameHeader), P(Vp8DecodedFrame), C.c_void_p, C.c_int]
        lib.ref_decode_frame.argtypes = [C.c_char_p, P(Vp8KeyFrameHeader), P(Vp8DecodedFrame)]
        lib.ref_free_frame.argtypes = [P(Vp8DecodedFrame)]
        lib.ref_free_frame.restype = None
        lib.ref_coeff_hash.argtypes = [C.c_char_p]
        lib.ref_coeff_hash.restype = C.c_uint64
        lib.ref_loopfilter_padded.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                              P(Vp8DecodedFrame)]
        lib.ref_time_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        lib.ref_time_batch.restype = C.c_double
        lib._typed = True
    return lib


def ref_available() -> bool:
    return (REPO_DIR / "oracle" / "_ref" / "libref.so").exists()


def ref_reconstruct(f: Frame, filtered: bool) -> bytes:
    buf = np.empty(i420_size(f.width, f.height), dtype=np.uint8)
    if ref_lib().ref_recon_i420(C.byref(f.kf), C.byref(f.frame), buf.ctypes.data, int(filtered)) != 0:
        raise RuntimeError("reference recon failed")
    return buf.tobytes()


def cpu_time_batch(frames: list[Frame], n: int, threads: int, filtered: bool, kind: str = "port") -> float:
    """Seconds for `n` frame reconstructions on `threads` host threads (oracle port or reference)."""
    lib = oracle_lib() if kind == "port" else ref_lib()
    fn = lib.oracle_time_batch if kind == "port" else lib.ref_time_batch
    k = len(frames)
    kfs = (C.POINTER(Vp8KeyFrameHeader) * k)(*[C.pointer(f.kf) for f in frames])
    frs = (C.POINTER(Vp8DecodedFrame) * k)(*[C.pointer(f.frame) for f in frames])
    return float(fn(C.cast(kfs, C.c_void_p), C.cast(frs, C.c_void_p), k, n, threads, int(filtered)))
