"""ctypes loader for libssw_hip.so (the C ABI declared in include/ssw.h).

There is deliberately no fallback: if the shared library has not been built, or
no GPU is present when a context is created, the caller gets an exception.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SSW_LIB_PATH: a diagnostic build of the same library (e.g. -DSSW_TILE_TRACE), never a different implementation
LIB_PATH = os.environ.get("SSW_LIB_PATH") or os.path.join(_HERE, "lib", "libssw_hip.so")

SSW_OK = 0
STATUS_NAMES = {
    0: "SSW_OK", 1: "SSW_ERR_BAD_ARG", 2: "SSW_ERR_BAD_DIMS", 3: "SSW_ERR_LENGTH_MISMATCH",
    4: "SSW_ERR_K_TOO_LARGE", 5: "SSW_ERR_NOT_BASE", 6: "SSW_ERR_UNSUPPORTED", 7: "SSW_ERR_CONSUMED",
    8: "SSW_ERR_HIP", 9: "SSW_ERR_NO_DEVICE", 10: "SSW_ERR_OUT_OF_MEMORY",
}
(SSW_ERR_BAD_ARG, SSW_ERR_BAD_DIMS, SSW_ERR_LENGTH_MISMATCH, SSW_ERR_K_TOO_LARGE, SSW_ERR_NOT_BASE,
 SSW_ERR_UNSUPPORTED, SSW_ERR_CONSUMED, SSW_ERR_HIP, SSW_ERR_NO_DEVICE, SSW_ERR_OUT_OF_MEMORY) = range(1, 11)

ORDER_ENERGY, ORDER_ENERGY_ORTHOGONAL, ORDER_LEGACY, ORDER_CUSTOM = 0, 1, 2, 3
OPTION1, OPTION2, OPTION3, METHOD_CUSTOM = 1, 2, 3, 4
DCT2, DCT2_ORTHOGONAL, DCT3 = 0, 1, 2
PRECISION_F32, PRECISION_F64 = 0, 1
STAGES = ["rgb_to_yiq", "dct_row", "dct_col", "select", "embed", "extract", "similarity", "yiq_to_rgb",
          "resize", "convert", "dct_prep", "dct_row_main", "dct_col_main", "locate", "locate_coarse"]
DCT_FOLDING_DEFAULT = 5
TRACE_NONE = 0xFFFFFFFF      # ssw_fingerprint_trace: dev_best of a suspect that carries no mark
PLAN_FLAGS = {"pair_f64": 1, "rows_deep": 2, "cols_deep": 4, "rows_level2": 8, "cols_level2": 16, "class_major": 32, "fused_cols": 64}
TRANSFER_STATS = ["h2d_bytes", "d2h_bytes", "h2d_seconds", "d2h_seconds", "staged_bytes", "direct_bytes"]


class Config(C.Structure):
    _fields_ = [("ordering", C.c_int32), ("method", C.c_int32), ("alpha", C.c_float), ("precision", C.c_int32)]


class Placement(C.Structure):
    """ssw_placement (include/ssw.h): the suspect as it is, and the rectangle of the original's frame it covers."""
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("channels", C.c_uint32),
                ("x", C.c_uint32), ("y", C.c_uint32), ("pw", C.c_uint32), ("ph", C.c_uint32)]


class ScaleRange(C.Structure):
    """ssw_scale_range (include/ssw.h): the widths a cut-out may have had in the original."""
    _fields_ = [("wmin", C.c_uint32), ("wmax", C.c_uint32)]


class ImageShape(C.Structure):
    """ssw_image_shape (include/ssw.h): one frame of ssw_signature_rgb8, [h][w][channels] u8."""
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("channels", C.c_uint32)]


# ssw_signature_rgb8 / ssw_signature_match (csrc/catalogue.hip): bytes of a signature, the sentinel of an empty slot, and the
# kernel's constants -- catalogue entries of a tile, of one launch (chunk), queries of a tile
SIGNATURE_BYTES = 1024
MATCH_NONE = 0xFFFFFFFF
MATCH_TILE, MATCH_CHUNK, MATCH_QUERY_TILE, MATCH_TOP_MAX = 128, 32768, 128, 8


class Coalition(C.Structure):
    """ssw_coalition (include/ssw.h): one forgery of ssw_collude_rgb8 -- a method and `count` of the call's frames."""
    _fields_ = [("method", C.c_uint32), ("count", C.c_uint32), ("member", C.c_uint32 * 16)]


# ssw_collude_method, by the names the Python surface and the CLI accept; members of a coalition
COLLUDE_AVERAGE, COLLUDE_MEDIAN, COLLUDE_MIN, COLLUDE_MAX, COLLUDE_MINMAX, COLLUDE_MOSAIC = range(6)
COLLUDE_METHODS = {"average": 0, "median": 1, "min": 2, "max": 3, "minmax": 4, "mosaic": 5}
COLLUDE_MAX_MEMBERS = 16


class JpegJob(C.Structure):
    """ssw_jpeg_job (include/ssw.h): one result of ssw_jpeg_rgb8 -- a frame of the call and a quality 1 .. 100."""
    _fields_ = [("frame", C.c_uint32), ("quality", C.c_uint32)]


JPEG_MIN_SIDE = 8            # ssw_jpeg_rgb8 refuses smaller frames


class FilterJob(C.Structure):
    """ssw_filter_job (include/ssw.h): one result of ssw_filter_rgb8 -- a frame of the call, a kind and its parameters; the
    fields a kind does not use are 0."""
    _fields_ = [("frame", C.c_uint32), ("kind", C.c_uint32), ("radius", C.c_float), ("percent", C.c_uint32), ("threshold", C.c_uint32)]


FILTER_BLUR, FILTER_UNSHARP, FILTER_MEDIAN3 = range(3)


class ScaleJob(C.Structure):
    """ssw_scale_job (include/ssw.h): one result of ssw_scale_attack_rgb8 -- a frame of the call, the thumbnail's size and the
    ssw_resample_filter that makes it."""
    _fields_ = [("frame", C.c_uint32), ("nw", C.c_uint32), ("nh", C.c_uint32), ("filter", C.c_uint32)]


# ssw_resample_filter, by the names the Python surface and the CLI accept (Pillow's)
RESAMPLE_BOX, RESAMPLE_BILINEAR, RESAMPLE_BICUBIC, RESAMPLE_LANCZOS = range(4)
RESAMPLE_FILTERS = {"box": 0, "bilinear": 1, "bicubic": 2, "lanczos": 3}
RESAMPLE_SIDE_MAX = 65535
SCALE_FACTOR_MAX = 4.0       # api.Scale: the largest factor


class RotateJob(C.Structure):
    """ssw_rotate_job (include/ssw.h): one result of ssw_rotate_attack_rgb8 / ssw_unrotate_rgb8 -- a frame of the call, the
    ssw_affine_filter and fill of the attack, the matrix of the angle and the matrix of its negative."""
    _fields_ = [("frame", C.c_uint32), ("filter", C.c_uint32), ("fill", C.c_uint8 * 4), ("forward", C.c_double * 6), ("back", C.c_double * 6)]


class CropJob(C.Structure):
    """ssw_crop_job (include/ssw.h): one result of ssw_crop_attack_rgb8 / ssw_crop_search_attack_rgb8 -- a frame of the call, the
    rectangle cut out of it, and the thumbnail's size and ssw_resample_filter (tw = th = 0: the piece is not scaled)."""
    _fields_ = [("frame", C.c_uint32), ("x", C.c_uint32), ("y", C.c_uint32), ("cw", C.c_uint32), ("ch", C.c_uint32),
                ("tw", C.c_uint32), ("th", C.c_uint32), ("filter", C.c_uint32)]


class CropSearch(C.Structure):
    """ssw_crop_search (include/ssw.h): the widths the piece may have had in the original; 0, 0: its own size."""
    _fields_ = [("wmin", C.c_uint32), ("wmax", C.c_uint32)]


class AngleFound(C.Structure):
    """ssw_angle_found (include/ssw.h): one answer of ssw_find_angle_rgb8 -- the angle is n / 32 degrees, sad and count its D and c."""
    _fields_ = [("n", C.c_int32), ("n_rungs", C.c_uint32), ("sad", C.c_uint64), ("count", C.c_uint64)]


class TurnedShape(C.Structure):
    """ssw_turned_shape (include/ssw.h): a suspect of ssw_locate_turned_rgb8 -- its width, height and channels."""
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("channels", C.c_uint32)]


class TurnedFound(C.Structure):
    """ssw_turned_found (include/ssw.h): one answer of ssw_locate_turned_rgb8 -- the angle is n / 32 degrees, the template tw x th
    lies at (x, y) of the original with the sum of absolute luma differences sad."""
    _fields_ = [("n", C.c_int32), ("x", C.c_uint32), ("y", C.c_uint32), ("tw", C.c_uint32), ("th", C.c_uint32), ("n_rungs", C.c_uint32),
                ("sad", C.c_uint64)]


class TurnedJob(C.Structure):
    """ssw_turned_job (include/ssw.h): one suspect of ssw_restore_turned_rgb8 -- turned by `angle` degrees, its centre at (cx, cy)
    pixels of the original."""
    _fields_ = [("angle", C.c_double), ("cx", C.c_double), ("cy", C.c_double)]


ANGLE_PER_DEGREE = 32        # ssw_find_angle_rgb8: the answer's resolution
ANGLE_MIN_SIDE = 32          # ... refuses smaller frames
LOCATE_SCALED_MIN_SIDE = 32  # ssw_locate_scaled_rgb8 refuses a range whose smallest rung has a side below this
LOCATE_FREE_MAX_SLACK = 4    # ssw_locate_free_rgb8: sizes within 1 .. 4 pixels of the ladder's answer
ANGLE_MAX_PIXELS = 1 << 27   # ... and larger ones

# ssw_affine_filter, by the names the Python surface and the CLI accept (Pillow's)
AFFINE_BILINEAR, AFFINE_BICUBIC = range(2)
AFFINE_FILTERS = {"bilinear": 0, "bicubic": 1}
FILTER_RADIUS_MAX = 8.0      # keeps the box radius of a blur pass at 7 or below
QUALITY_STATS = 6            # ssw_quality_rgb8: u64 per copy -- SSE of R, G, B, SSE of the luma, changed bytes, max |d|
SSIM_MIN_SIDE = 8            # ssw_ssim_rgb8 refuses smaller frames
SSIM_ONE = 1 << 30           # the fixed-point value of two identical windows
SSIM_STATS = 2               # u64 per copy: the sum of the windows' values (signed), (worst value + SSIM_ONE) << 32 | its index
SSIM_TILE_W, SSIM_TILE_H = 252, 60     # pixels of windows a block of ssim_kernel owns

_vp, _f32p, _u32p, _u64p, _sz = C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t
_cfgp = C.POINTER(Config)
_plp = C.POINTER(Placement)

# name -> (restype, argtypes); this table is also what tests check against include/ssw.h
SIGNATURES = {
    "ssw_version": (C.c_char_p, []),
    "ssw_build_all_strategies": (C.c_int, []),
    "ssw_ctx_transform_plan": (C.c_int, [_vp, _sz, _sz, _sz, C.c_int, C.POINTER(C.c_uint32)]),
    "ssw_status_string": (C.c_char_p, [C.c_int]),
    "ssw_last_error": (C.c_char_p, []),
    "ssw_config_default": (None, [_cfgp]),
    "ssw_ctx_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "ssw_ctx_destroy": (C.c_int, [_vp]),
    "ssw_ctx_synchronize": (C.c_int, [_vp]),
    "ssw_ctx_stream": (_vp, [_vp]),
    "ssw_ctx_set_stream": (C.c_int, [_vp, _vp]),
    "ssw_ctx_wait_event": (C.c_int, [_vp, _vp]),
    "ssw_ctx_record_event": (C.c_int, [_vp, _vp]),
    "ssw_ctx_set_chunk_frames": (C.c_int, [_vp, _sz]),
    "ssw_ctx_pass_frames": (_sz, [_vp, _sz, _sz, _sz]),
    "ssw_ctx_set_dct_folding": (C.c_int, [_vp, C.c_int]),
    "ssw_ctx_enable_timing": (C.c_int, [_vp, C.c_int]),
    "ssw_ctx_reset_timing": (C.c_int, [_vp]),
    "ssw_ctx_get_timing": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "ssw_ctx_get_work": (C.c_int, [_vp, C.POINTER(C.c_double)]),
    "ssw_ctx_get_traffic": (C.c_int, [_vp, C.POINTER(C.c_double)]),
    "ssw_ctx_set_overlap": (C.c_int, [_vp, C.c_int]),
    "ssw_ctx_set_prune": (C.c_int, [_vp, C.c_int]),
    "ssw_ctx_set_odd_split": (C.c_int, [_vp, C.c_int]),
    "ssw_tuning_set": (C.c_int, [C.c_char_p, C.c_longlong]),
    "ssw_tuning_get": (C.c_int, [C.c_char_p, C.POINTER(C.c_longlong)]),
    "ssw_tuning_reset": (C.c_int, [C.c_char_p]),
    "ssw_ctx_get_prune_stats": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "ssw_ctx_get_base_prune_stats": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "ssw_ctx_get_base_prune_tail_jobs": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "ssw_debug_base_prune_bound": (C.c_int, [_vp, _vp, _vp, _sz, _sz, _sz, _sz, _vp]),
    "ssw_debug_select_masked": (C.c_int, [_vp, _vp, _sz, _sz, _sz, C.c_int, _sz, _vp, _sz, _vp]),
    "ssw_ctx_get_select_stats": (C.c_int, [_vp, C.POINTER(C.c_uint64)]),
    "ssw_dev_mem_info": (C.c_int, [_vp, C.POINTER(_sz), C.POINTER(_sz)]),
    "ssw_dev_alloc": (C.c_int, [_vp, _sz, C.POINTER(_vp)]),
    "ssw_dev_free": (C.c_int, [_vp, _vp]),
    "ssw_copy_to_dev": (C.c_int, [_vp, _vp, _vp, _sz]),
    "ssw_copy_to_host": (C.c_int, [_vp, _vp, _vp, _sz]),
    "ssw_host_alloc": (C.c_int, [_vp, _sz, C.POINTER(_vp)]),
    "ssw_host_free": (C.c_int, [_vp, _vp]),
    "ssw_ctx_set_copy_threads": (C.c_int, [_vp, C.c_int]),
    "ssw_ctx_get_transfer_stats": (C.c_int, [_vp, C.POINTER(C.c_double), C.c_int]),
    "ssw_rgb_to_yiq": (C.c_int, [_vp, _f32p, _sz, _sz, _sz, _f32p, _f32p, _f32p]),
    "ssw_yiq_to_rgb": (C.c_int, [_vp, _f32p, _f32p, _f32p, _sz, _sz, _sz, _f32p]),
    "ssw_dct2d": (C.c_int, [_vp, C.c_int, C.c_int, _sz, _sz, _sz, _f32p]),
    "ssw_topk_indices": (C.c_int, [_vp, _f32p, _sz, _sz, _sz, C.c_int, _sz, _u32p]),
    "ssw_embed_coefficients": (C.c_int, [_vp, _f32p, _sz, _sz, _u32p, _sz, C.c_int, C.c_float, _f32p, _sz]),
    "ssw_extract_coefficients": (C.c_int, [_vp, _f32p, _f32p, _sz, _sz, _u32p, _sz, C.c_int, C.c_float, _f32p]),
    "ssw_similarity_batch": (C.c_int, [_vp, _f32p, _f32p, _sz, _sz, _f32p]),
    "ssw_similarity_matrix": (C.c_int, [_vp, _f32p, _sz, _f32p, _sz, _sz, _f32p]),
    "ssw_batch_embed": (C.c_int, [_vp, _cfgp, _f32p, _sz, _sz, _sz, _f32p, _sz, _f32p, _f32p, _u32p]),
    "ssw_batch_extract": (C.c_int, [_vp, _cfgp, _f32p, _f32p, _sz, _sz, _sz, _sz, _f32p, _f32p, _f32p]),
    "ssw_convert_rgb8_to_f32": (C.c_int, [_vp, _vp, _sz, _f32p]),
    "ssw_convert_f32_to_rgb8": (C.c_int, [_vp, _f32p, _sz, _vp]),
    "ssw_resize_rgb8": (C.c_int, [_vp, _vp, _sz, _sz, _sz, _sz, _sz, _vp]),
    "ssw_batch_embed_rgb8": (C.c_int, [_vp, _cfgp, _vp, _sz, _sz, _sz, _f32p, _sz, _vp]),
    "ssw_batch_embed_host_rgb8": (C.c_int, [_vp, _cfgp, C.POINTER(_vp), _sz, _sz, _sz, _f32p, _sz, C.POINTER(_vp)]),
    "ssw_batch_extract_host_rgb8": (C.c_int, [_vp, _cfgp, C.POINTER(_vp), C.POINTER(_vp), _sz, _sz, _sz, _sz, _f32p, _f32p, _f32p]),
    "ssw_convert_rgb16_to_f32": (C.c_int, [_vp, _vp, _sz, _f32p]),
    "ssw_convert_f32_to_rgb16": (C.c_int, [_vp, _f32p, _sz, _vp]),
    "ssw_batch_embed_rgb16": (C.c_int, [_vp, _cfgp, _vp, _sz, _sz, _sz, _f32p, _sz, _f32p]),
    "ssw_batch_extract_rgb16": (C.c_int, [_vp, _cfgp, _vp, _vp, _sz, _sz, _sz, _sz, _f32p, _f32p, _f32p]),
    "ssw_batch_extract_rgb8": (C.c_int, [_vp, _cfgp, _vp, _vp, _sz, _sz, _sz, _sz, _f32p, _f32p, _f32p]),
    "ssw_writer_create": (C.c_int, [_vp, _vp, _sz, _sz, _cfgp, C.POINTER(_vp)]),
    "ssw_writer_create_rgb8": (C.c_int, [_vp, _vp, _sz, _sz, _cfgp, C.POINTER(_vp)]),
    "ssw_writer_create_rgb16": (C.c_int, [_vp, _vp, _sz, _sz, _cfgp, C.POINTER(_vp)]),
    "ssw_writer_coefficients": (C.c_int, [_vp, _vp]),
    "ssw_writer_embed": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_sz), _sz]),
    "ssw_writer_result": (C.c_int, [_vp, _vp]),
    "ssw_writer_mark": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_sz), _sz, _vp]),
    "ssw_writer_result_rgb8": (C.c_int, [_vp, _vp]),
    "ssw_writer_mark_rgb8": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_sz), _sz, _vp]),
    "ssw_fingerprint_embed": (C.c_int, [_vp, _cfgp, _f32p, _sz, _sz, _f32p, _sz, _sz, _f32p, _u32p]),
    "ssw_fingerprint_embed_rgb8": (C.c_int, [_vp, _cfgp, _vp, _sz, _sz, _f32p, _sz, _sz, _vp, _u32p]),
    "ssw_fingerprint_trace": (C.c_int, [_vp, _cfgp, _f32p, _f32p, _sz, _sz, _sz, _sz, _f32p, _sz, C.c_float, _f32p, _f32p, _u32p, _f32p, _u32p]),
    "ssw_fingerprint_trace_rgb8": (C.c_int, [_vp, _cfgp, _vp, _vp, _sz, _sz, _sz, _sz, _f32p, _sz, C.c_float, _f32p, _f32p, _u32p, _f32p, _u32p]),
    "ssw_fingerprint_trace_host_rgb8": (C.c_int, [_vp, _cfgp, _vp, C.POINTER(_vp), _sz, _sz, _sz, _sz, _f32p, _sz, C.c_float, _f32p, _f32p, _u32p,
                                                  _f32p, _u32p]),
    "ssw_reader_trace_host_rgb8": (C.c_int, [_vp, C.POINTER(_vp), _sz, _sz, _f32p, _sz, C.c_float, _f32p, _f32p, _u32p, _f32p, _u32p]),
    "ssw_restore_rgb8": (C.c_int, [_vp, _vp, _sz, _sz, C.POINTER(_vp), _plp, _sz, _vp]),
    "ssw_locate_rgb8": (C.c_int, [_vp, _vp, _sz, _sz, C.POINTER(_vp), _plp, _sz, C.POINTER(C.c_uint64)]),
    "ssw_locate_scaled_rgb8": (C.c_int, [_vp, _vp, _sz, _sz, C.POINTER(_vp), _plp, C.POINTER(ScaleRange), _sz, C.POINTER(C.c_uint64)]),
    "ssw_locate_rung_boxes": (C.c_int, [_vp, _vp, _sz, _sz, _sz, _sz, _sz, _vp]),
    "ssw_locate_free_rgb8": (C.c_int, [_vp, _vp, _sz, _sz, C.POINTER(_vp), _plp, C.POINTER(ScaleRange), C.POINTER(C.c_uint32), _sz,
                                       C.POINTER(C.c_uint64)]),
    "ssw_locate_free_sums_rgb8": (C.c_int, [_vp, _vp, _sz, _sz, _vp, _sz, _sz, _sz, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.c_uint32,
                                            C.POINTER(C.c_uint64), _plp, C.POINTER(C.c_uint64)]),
    "ssw_signature_rgb8": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(ImageShape), _sz, _vp]),
    "ssw_signature_host_rgb8": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(ImageShape), _sz, _vp]),
    "ssw_signature_match": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _sz, _u32p, _u32p, _u32p]),
    "ssw_quality_rgb8": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _sz, _sz, _u64p]),
    "ssw_collude_rgb8": (C.c_int, [_vp, _vp, _sz, _sz, _sz, C.POINTER(Coalition), _sz, _vp]),
    "ssw_jpeg_rgb8": (C.c_int, [_vp, _vp, _sz, _sz, _sz, C.POINTER(JpegJob), _sz, _vp]),
    "ssw_filter_rgb8": (C.c_int, [_vp, _vp, _sz, _sz, _sz, C.POINTER(FilterJob), _sz, _vp]),
    "ssw_resample_rgb8": (C.c_int, [_vp, _vp, _sz, _sz, _sz, _sz, _sz, C.c_int, _vp]),
    "ssw_scale_attack_rgb8": (C.c_int, [_vp, _vp, _sz, _sz, _sz, C.POINTER(ScaleJob), _sz, _vp]),
    "ssw_affine_rgb8": (C.c_int, [_vp, _vp, _sz, _sz, _sz, _sz, _sz, C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_uint8), _vp]),
    "ssw_rotate_attack_rgb8": (C.c_int, [_vp, _vp, _vp, _sz, _sz, _sz, C.POINTER(RotateJob), _sz, _vp]),
    "ssw_unrotate_rgb8": (C.c_int, [_vp, _vp, _vp, _sz, _sz, _sz, C.POINTER(RotateJob), _vp]),
    "ssw_unrotate_kept": (C.c_int, [_vp, _sz, _sz, C.POINTER(RotateJob), _sz, _u64p]),
    "ssw_affine_plan": (C.c_int, [_sz, _sz, C.POINTER(C.c_double), C.POINTER(C.c_int), _u32p, _u32p]),
    "ssw_rotation_matrix": (C.c_int, [C.c_double, _sz, _sz, C.POINTER(C.c_double)]),
    "ssw_find_angle_rgb8": (C.c_int, [_vp, _vp, _vp, _sz, _sz, _sz, C.c_double, C.c_double, C.POINTER(AngleFound), _u64p]),
    "ssw_rotate_search_attack_rgb8": (C.c_int, [_vp, _vp, _vp, _sz, _sz, _sz, C.POINTER(RotateJob), _sz, C.c_double, C.c_double, _vp, _vp,
                                                C.POINTER(AngleFound), _u64p, _u64p]),
    "ssw_crop_attack_rgb8": (C.c_int, [_vp, _vp, _vp, _sz, _sz, _sz, C.POINTER(CropJob), _sz, _vp, _vp]),
    "ssw_crop_search_attack_rgb8": (C.c_int, [_vp, _vp, _vp, _sz, _sz, _sz, C.POINTER(CropJob), C.POINTER(CropSearch), _sz, _vp, _vp, _plp,
                                              _u64p]),
    "ssw_locate_turned_rgb8": (C.c_int, [_vp, _vp, _sz, _sz, C.POINTER(C.c_void_p), C.POINTER(TurnedShape), _sz, C.c_double, C.c_double,
                                         C.POINTER(TurnedFound), _u64p]),
    "ssw_restore_turned_rgb8": (C.c_int, [_vp, _vp, _sz, _sz, C.POINTER(C.c_void_p), C.POINTER(TurnedShape), C.POINTER(TurnedJob), _sz, _vp]),
    "ssw_locate_turned_rung_boxes": (C.c_int, [_vp, _vp, _sz, _sz, C.c_int32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _vp]),
    "ssw_angle_table": (C.c_int, [C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "ssw_ssim_rgb8": (C.c_int, [_vp, _vp, _sz, _vp, _sz, _sz, _sz, _u64p, _vp]),
    "ssw_fingerprint_trace_restored_host_rgb8": (C.c_int, [_vp, _cfgp, _vp, _sz, _sz, C.POINTER(_vp), _plp, _sz, _sz, _f32p, _sz, C.c_float,
                                                           _f32p, _f32p, _u32p, _f32p, _u32p]),
    "ssw_reader_trace_restored_host_rgb8": (C.c_int, [_vp, _vp, C.POINTER(_vp), _plp, _sz, _sz, _f32p, _sz, C.c_float, _f32p, _f32p, _u32p,
                                                      _f32p, _u32p]),
    "ssw_writer_mark_copies": (C.c_int, [_vp, _f32p, _sz, _sz, _vp]),
    "ssw_writer_mark_copies_rgb8": (C.c_int, [_vp, _f32p, _sz, _sz, _vp]),
    "ssw_writer_destroy": (C.c_int, [_vp]),
    "ssw_reader_create": (C.c_int, [_vp, _vp, _sz, _sz, C.c_int, _cfgp, C.POINTER(_vp)]),
    "ssw_reader_create_rgb8": (C.c_int, [_vp, _vp, _sz, _sz, C.c_int, _cfgp, C.POINTER(_vp)]),
    "ssw_reader_create_rgb16": (C.c_int, [_vp, _vp, _sz, _sz, C.c_int, _cfgp, C.POINTER(_vp)]),
    "ssw_reader_coefficients": (C.c_int, [_vp, _vp]),
    "ssw_reader_indices": (C.c_int, [_vp, _sz, _vp]),
    "ssw_reader_extract": (C.c_int, [_vp, _vp, _vp, _sz]),
    "ssw_reader_destroy": (C.c_int, [_vp]),
    "ssw_similarity": (C.c_int, [_vp, _vp, _sz, _vp, _sz, C.POINTER(C.c_float)]),
    "ssw_synth_frames": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _sz, _sz, _sz, _f32p]),
}

_lib = None


class SswLibraryMissing(ImportError):
    pass


def load() -> C.CDLL:
    """dlopen the HIP library; raises loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SswLibraryMissing(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(make -C spread_spectrum_watermarking_amd/csrc). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the ABI is incomplete
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def all_strategies() -> bool:
    """Always False: the library has one build (ssw_build_all_strategies, include/ssw.h)."""
    return bool(load().ssw_build_all_strategies())


class SswError(RuntimeError):
    """Raised where the Rust reference would panic (or on a HIP failure)."""

    def __init__(self, status: int, where: str = ""):
        self.status = status
        lib = load()
        msg = lib.ssw_status_string(status).decode()
        detail = lib.ssw_last_error().decode() if status in (SSW_ERR_HIP, SSW_ERR_NO_DEVICE, SSW_ERR_OUT_OF_MEMORY) else ""
        super().__init__(f"{where}: {STATUS_NAMES.get(status, status)}: {msg}" + (f" [{detail}]" if detail else ""))


def check(status: int, where: str = "ssw"):
    if status != SSW_OK:
        raise SswError(status, where)
