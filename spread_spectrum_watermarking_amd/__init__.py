"""MI355X-native spread-spectrum watermarking hot path (gfx950 HIP kernels behind a C ABI).

Public surface mirrors the reference crate's re-exports (lib.rs:81-85).
"""
from ._lib import SswError, SswLibraryMissing, LIB_PATH  # noqa: F401
from .api import (Catalogue, Collusion, Context, Crop, CropResult, DeviceBuffer, Extraction, Filter, FilterResult, FoundAngle, Identified, Insertion, JpegResult, Locate, Located, LocatedTurned, MarkBuf, OrderingMethod, Placement, Precision,  # noqa: F401
                  Quality, ReadConfig, Reader, ReaderDerived, Rotate, RotateResult, Rotated, Scale, ScaleResult, Similarity, Ssim, StrengthRow, Tester, TraceResult, WriteConfig, Writer,
                  affine, collude, crop_attack, crop_search_attack, default_context, extract_many, filter, find_angle, identify, jpeg, locate, locate_turned, mark_many, quality, resample, restore, restore_turned, rotate, rotate_attack, rotate_search_attack, rotation_matrix, scale_attack, signature, ssim, strength_report, trace_many, unrotate,
                  tuning)

__all__ = ["MarkBuf", "Tester", "Extraction", "Insertion", "OrderingMethod", "ReadConfig", "Reader",
           "ReaderDerived", "WriteConfig", "Writer", "Similarity", "Context", "Precision", "SswError"]
