"""Host-side mirror of the crate's public surface (lib.rs:81-85) over the C ABI.

Same names, argument meaning and error behaviour as the Rust reference
(file:line relative to the reference tree):

  Writer / WriteConfig / Insertion        src/algorithm.rs:68-112, :285-433
  Reader / ReaderDerived / ReadConfig      src/algorithm.rs:114-140, :435-594
  OrderingMethod                           src/algorithm.rs:142-191
  MarkBuf (Mark)                           src/algorithm.rs:596-666
  Tester / Similarity                      src/algorithm.rs:668-715

Images are numpy arrays [H, W, 3]: float32 in [0, 1] (what `into_rgb32f()` yields,
algorithm.rs:308) or uint8 (handed to the library as they are: `into_rgb32f()`, v / 255 like the
image crate does, runs on the device and 3 instead of 12 bytes per pixel cross PCIe).
Where the reference panics, an SswError is raised.  All arithmetic runs on the
GPU through libssw_hip.so; there is no CPU path in this package.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from contextlib import contextmanager
from dataclasses import dataclass, field
from typing import Any, Callable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib as L
from ._lib import SswError, check


# ---- context ---------------------------------------------------------------------------------
class Context:
    """One per GPU (include/ssw.h: ssw_ctx).  Not thread-safe, like the reference's !Send types."""

    def __init__(self, device_id: int = 0):
        self._lib = L.load()
        h = C.c_void_p()
        check(self._lib.ssw_ctx_create(device_id, C.byref(h)), "ssw_ctx_create")
        self.handle = h
        self.device_id = device_id

    def close(self):
        if getattr(self, "handle", None):
            self._lib.ssw_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        check(self._lib.ssw_ctx_synchronize(self.handle), "ssw_ctx_synchronize")

    def set_stream(self, hip_stream=None):
        """Enqueue on the caller's hipStream_t (an int / c_void_p, e.g. torch.cuda.current_stream().cuda_stream);
        None returns to the context's private stream.  See the stream contract in include/ssw.h."""
        check(self._lib.ssw_ctx_set_stream(self.handle, C.c_void_p(hip_stream) if hip_stream else None), "ssw_ctx_set_stream")

    def wait_event(self, hip_event):
        check(self._lib.ssw_ctx_wait_event(self.handle, C.c_void_p(hip_event)), "ssw_ctx_wait_event")

    def record_event(self, hip_event):
        check(self._lib.ssw_ctx_record_event(self.handle, C.c_void_p(hip_event)), "ssw_ctx_record_event")

    def set_chunk_frames(self, n: int):
        check(self._lib.ssw_ctx_set_chunk_frames(self.handle, n), "ssw_ctx_set_chunk_frames")

    def pass_frames(self, n_frames: int, w: int, h: int) -> int:
        """Frames per internal pass a batch call over n_frames frames of w x h would use."""
        return int(self._lib.ssw_ctx_pass_frames(self.handle, n_frames, w, h))

    def set_dct_folding(self, level=True):
        """Basis-GEMM strategy (include/ssw.h): False / 0 dense; 1 (= 2) one folding level inside the GEMM
        kernel; 3 / 4 operand-ready GEMMs with one / two
        folding levels; 5 a third level on long forward row passes; 6 the same without the size
        threshold.  True selects the default (5)."""
        lvl = (L.DCT_FOLDING_DEFAULT if level else 0) if isinstance(level, bool) else int(level)
        check(self._lib.ssw_ctx_set_dct_folding(self.handle, lvl), "ssw_ctx_set_dct_folding")

    def enable_timing(self, on: bool = True):
        check(self._lib.ssw_ctx_enable_timing(self.handle, int(on)), "ssw_ctx_enable_timing")

    def reset_timing(self):
        check(self._lib.ssw_ctx_reset_timing(self.handle), "ssw_ctx_reset_timing")

    def timing(self) -> dict:
        """Per stage: milliseconds, timed regions, and the work done in them (flop for the GEMM stages,
        algorithmic bytes for the HBM-bound ones)."""
        ms = (C.c_double * len(L.STAGES))()
        n = (C.c_uint64 * len(L.STAGES))()
        work = (C.c_double * len(L.STAGES))()
        check(self._lib.ssw_ctx_get_timing(self.handle, ms, n), "ssw_ctx_get_timing")
        check(self._lib.ssw_ctx_get_work(self.handle, work), "ssw_ctx_get_work")
        traffic = (C.c_double * len(L.STAGES))()
        check(self._lib.ssw_ctx_get_traffic(self.handle, traffic), "ssw_ctx_get_traffic")
        return {s: {"ms": ms[i], "launches": int(n[i]), "work": work[i], "bytes": traffic[i]} for i, s in enumerate(L.STAGES)}

    def transform_plan(self, n_frames: int, w: int, h: int, dct_type: int = L.DCT2) -> dict:
        """Which strategy of the 2-D transform a batch of this shape takes (include/ssw.h: ssw_ctx_transform_plan)."""
        f = C.c_uint32()
        check(self._lib.ssw_ctx_transform_plan(self.handle, n_frames, w, h, dct_type, C.byref(f)), "ssw_ctx_transform_plan")
        return {name: bool(f.value & bit) for name, bit in L.PLAN_FLAGS.items()}

    def set_overlap(self, on: bool = True):
        """Two chunks in flight on two streams in the batch entry points (default) or one at a time."""
        check(self._lib.ssw_ctx_set_overlap(self.handle, int(on)), "ssw_ctx_set_overlap")

    def set_prune(self, on: bool = True):
        """Batch extract: derived frames transformed only where extract reads them (default) or fully."""
        check(self._lib.ssw_ctx_set_prune(self.handle, int(on)), "ssw_ctx_set_prune")

    def set_odd_split(self, on: bool = True):
        """f64 transforms: odd halves as rotated quarter-length cosine + sine pairs (default) or as exact folded sums."""
        check(self._lib.ssw_ctx_set_odd_split(self.handle, int(on)), "ssw_ctx_set_odd_split")

    def prune_stats(self) -> dict:
        st = (C.c_uint64 * 3)()
        check(self._lib.ssw_ctx_get_prune_stats(self.handle, st), "ssw_ctx_get_prune_stats")
        bp = (C.c_uint64 * 3)()
        check(self._lib.ssw_ctx_get_base_prune_stats(self.handle, bp), "ssw_ctx_get_base_prune_stats")
        jobs = C.c_uint64(0)
        check(self._lib.ssw_ctx_get_base_prune_tail_jobs(self.handle, C.byref(jobs)), "ssw_ctx_get_base_prune_tail_jobs")
        return {"pruned_chunks": int(st[0]), "redone_chunks": int(st[1]), "columns_needed": int(st[2]),
                "base_tiles": int(bp[0]), "base_tiles_computed": int(bp[1]), "base_frames_extended": int(bp[2]),
                "base_tail_jobs": int(jobs.value)}

    def select_stats(self) -> dict:
        st = (C.c_uint64 * 2)()
        check(self._lib.ssw_ctx_get_select_stats(self.handle, st), "ssw_ctx_get_select_stats")
        return {"frames": int(st[0]), "exact_fallback_frames": int(st[1])}

    def set_copy_threads(self, n: int = 0):
        """Host threads that move pageable buffers through the pinned staging ring (0 = automatic)."""
        check(self._lib.ssw_ctx_set_copy_threads(self.handle, int(n)), "ssw_ctx_set_copy_threads")

    def transfer_stats(self, reset: bool = False) -> dict:
        """Bytes / host seconds of the host-buffer entry points' uploads and downloads (include/ssw.h)."""
        st = (C.c_double * len(L.TRANSFER_STATS))()
        check(self._lib.ssw_ctx_get_transfer_stats(self.handle, st, int(reset)), "ssw_ctx_get_transfer_stats")
        return {n: float(st[i]) for i, n in enumerate(L.TRANSFER_STATS)}

    def pinned_empty(self, shape, dtype) -> np.ndarray:
        """numpy array in pinned (page-locked) host memory: the handles DMA straight from / into it.
        The memory belongs to the context and is released when the array (and its views) are gone."""
        dt = np.dtype(dtype)
        n = int(np.prod(shape)) * dt.itemsize
        p = C.c_void_p()
        check(self._lib.ssw_host_alloc(self.handle, n, C.byref(p)), "ssw_host_alloc")
        return np.asarray(_PinnedBlock(self, p, n))[:n].view(dt).reshape(shape)

    def mem_info(self):
        free, total = C.c_size_t(), C.c_size_t()
        check(self._lib.ssw_dev_mem_info(self.handle, C.byref(free), C.byref(total)), "ssw_dev_mem_info")
        return int(free.value), int(total.value)

    # device memory for hosts without their own allocator (tests; the bench uses torch tensors)
    def alloc(self, nbytes: int) -> "DeviceBuffer":
        return DeviceBuffer(self, nbytes)

    def to_device(self, array: np.ndarray) -> "DeviceBuffer":
        a = np.ascontiguousarray(array)
        buf = DeviceBuffer(self, a.nbytes)
        check(self._lib.ssw_copy_to_dev(self.handle, buf.ptr, a.ctypes.data, a.nbytes), "ssw_copy_to_dev")
        return buf


class _PinnedBlock:
    """Owner of one ssw_host_alloc block, exposed to numpy through __array_interface__: arrays made from it
    (and their views) keep it alive, the block is released with the last of them."""

    def __init__(self, ctx: Context, ptr, nbytes: int):
        self.ctx, self.ptr, self.nbytes = ctx, ptr, nbytes
        self.__array_interface__ = {"data": (int(ptr.value), False), "shape": (max(nbytes, 1),), "typestr": "|u1", "version": 3}

    def __del__(self):
        try:
            if self.ptr and self.ctx.handle:
                self.ctx._lib.ssw_host_free(self.ctx.handle, self.ptr)
            self.ptr = None
        except Exception:
            pass


class DeviceBuffer:
    def __init__(self, ctx: Context, nbytes: int):
        self.ctx, self.nbytes = ctx, nbytes
        p = C.c_void_p()
        check(ctx._lib.ssw_dev_alloc(ctx.handle, nbytes, C.byref(p)), "ssw_dev_alloc")
        self.ptr = p

    def to_host(self, dtype, shape) -> np.ndarray:
        out = np.empty(shape, dtype)
        assert out.nbytes <= self.nbytes
        check(self.ctx._lib.ssw_copy_to_host(self.ctx.handle, out.ctypes.data, self.ptr, out.nbytes), "ssw_copy_to_host")
        return out

    def free(self):
        if self.ptr and self.ctx.handle:
            self.ctx._lib.ssw_dev_free(self.ctx.handle, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


_default_ctx: Optional[Context] = None


class tuning:
    """Process-wide strategy thresholds / A-B switches (include/ssw.h: ssw_tuning_set).  `with tuning(efold_min=256): ...`
    sets them for the block and restores the previous state; use a fresh Context inside (workspaces and cached plans of an
    existing context were built under the old values)."""

    def __init__(self, **values):
        self._values = values
        self._lib = L.load()

    @staticmethod
    def get(name: str) -> int:
        v = C.c_longlong()
        check(L.load().ssw_tuning_get(name.encode(), C.byref(v)), "ssw_tuning_get")
        return int(v.value)

    def __enter__(self):
        self._previous = {name: tuning.get(name) for name in self._values}      # raises on an unknown name before anything is set
        for name, v in self._values.items():
            check(self._lib.ssw_tuning_set(name.encode(), int(v)), f"ssw_tuning_set({name})")
        return self

    def __exit__(self, *exc):
        for name, v in self._previous.items():        # nested blocks restore the enclosing block's value, not the default
            self._lib.ssw_tuning_set(name.encode(), v)
        return False


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None or _default_ctx.handle is None:
        _default_ctx = Context(0)
    return _default_ctx


# ---- configuration enums (algorithm.rs:68-77, :115-124, :143-152) ---------------------------
@dataclass(frozen=True)
class _Method:
    tag: int
    alpha: float = 0.0
    function: Optional[Callable] = None


class Insertion:
    """x' = x + a w | x (1 + a w) | x exp(a w) | custom closure (algorithm.rs:68-77)."""
    @staticmethod
    def Option1(alpha: float): return _Method(L.OPTION1, float(alpha))
    @staticmethod
    def Option2(alpha: float): return _Method(L.OPTION2, float(alpha))
    @staticmethod
    def Option3(alpha: float): return _Method(L.OPTION3, float(alpha))
    @staticmethod
    def Custom(function: Callable): return _Method(L.METHOD_CUSTOM, 0.0, function)


Extraction = Insertion      # same variants, inverse functions (algorithm.rs:115-124)


@dataclass(frozen=True)
class _Ordering:
    tag: int
    function: Optional[Callable] = None


class OrderingMethod:
    Energy = _Ordering(L.ORDER_ENERGY)
    EnergyOrthogonal = _Ordering(L.ORDER_ENERGY_ORTHOGONAL)
    Legacy = _Ordering(L.ORDER_LEGACY)
    @staticmethod
    def Custom(function: Callable): return _Ordering(L.ORDER_CUSTOM, function)


class Precision:
    F32 = L.PRECISION_F32      # v_mfma_f32_32x32x2_f32 basis GEMMs: ~1.8x faster, f32-chain accuracy
    F64 = L.PRECISION_F64      # default: v_mfma_f64_16x16x4_f64, correctly rounded ("canonical")


@dataclass
class WriteConfig:
    """algorithm.rs:99-112; default Option2(0.1) + Energy."""
    insertion: _Method = field(default_factory=lambda: Insertion.Option2(0.1))
    ordering: _Ordering = OrderingMethod.Energy
    precision: int = Precision.F64

    @staticmethod
    def default(): return WriteConfig()

    def _c(self) -> L.Config:
        return L.Config(self.ordering.tag, self.insertion.tag, self.insertion.alpha, self.precision)


@dataclass
class ReadConfig:
    """algorithm.rs:127-140; default Option2(0.1) + Energy."""
    extraction: _Method = field(default_factory=lambda: Extraction.Option2(0.1))
    ordering: _Ordering = OrderingMethod.Energy
    precision: int = Precision.F64

    @staticmethod
    def default(): return ReadConfig()

    def _c(self) -> L.Config:
        return L.Config(self.ordering.tag, self.extraction.tag, self.extraction.alpha, self.precision)


def _as_rgb(image) -> np.ndarray:
    """What crosses the C ABI for a `DynamicImage`: 8- and 16-bit images as they are (`into_rgb32f()`, algorithm.rs:308,
    :476, then runs on the device: v / 255, v / 65535), everything else as f32."""
    a = np.asarray(image)
    if a.ndim != 3 or a.shape[2] not in (3, 4):
        raise ValueError("image must be [H, W, 3] (or RGBA [H, W, 4])")
    a = a[:, :, :3]
    if a.dtype in (np.uint8, np.uint16):
        return np.ascontiguousarray(a)
    return np.ascontiguousarray(a, dtype=np.float32)


# ---- marks (algorithm.rs:596-666) --------------------------------------------------------------
class MarkBuf:
    def __init__(self, data: Optional[Sequence[float]] = None):
        self._data = np.zeros(0, np.float32) if data is None else np.array(data, np.float32).ravel().copy()

    @staticmethod
    def new() -> "MarkBuf":
        return MarkBuf()

    @staticmethod
    def generate_normal(length: int) -> "MarkBuf":
        """algorithm.rs:619-626: StandardNormal from a thread-local, non-deterministic RNG (host side)."""
        return MarkBuf(np.random.default_rng().standard_normal(length).astype(np.float32))

    @staticmethod
    def from_(data) -> "MarkBuf":            # `from` is a Python keyword
        return MarkBuf(data)

    def data(self) -> np.ndarray:
        return self._data

    def set_data(self, data):
        self._data = np.array(data, np.float32).ravel().copy()

    def __len__(self):
        return self._data.size


def _mark_data(m) -> np.ndarray:
    """The `Mark` trait (algorithm.rs:597-600, :659-666): anything exposing a f32 slice."""
    if isinstance(m, MarkBuf):
        return m.data()
    return np.ascontiguousarray(m, dtype=np.float32).ravel()


def _marks_c(marks):
    arrs = [np.ascontiguousarray(_mark_data(m), dtype=np.float32) for m in marks]
    ptrs = (C.c_void_p * max(len(arrs), 1))(*[a.ctypes.data for a in arrs])
    lens = (C.c_size_t * max(len(arrs), 1))(*[a.size for a in arrs])
    return arrs, ptrs, lens


# ---- Writer (algorithm.rs:285-433) -------------------------------------------------------------
class Writer:
    def __init__(self, image, config: Optional[WriteConfig] = None, ctx: Optional[Context] = None):
        """Writer::new (algorithm.rs:295-316): rgb -> yiq, DCT-II of the Y plane on the GPU."""
        self._ctx = ctx or default_context()
        self._lib = self._ctx._lib
        config = config or WriteConfig.default()
        rgb = _as_rgb(image)
        self.height, self.width = rgb.shape[:2]
        h = C.c_void_p()
        cfg = config._c()
        create = {np.dtype(np.uint8): self._lib.ssw_writer_create_rgb8,
                  np.dtype(np.uint16): self._lib.ssw_writer_create_rgb16}.get(rgb.dtype, self._lib.ssw_writer_create)
        check(create(self._ctx.handle, rgb.ctypes.data, self.width, self.height, C.byref(cfg), C.byref(h)), "Writer::new")
        self._h = h

    new = classmethod(lambda cls, image, config=None, ctx=None: cls(image, config, ctx))

    def coefficient_image(self) -> np.ndarray:
        out = np.empty((self.height, self.width), np.float32)
        check(self._lib.ssw_writer_coefficients(self._h, out.ctypes.data), "Writer::coefficient_image")
        return out

    def embed(self, marks):
        arrs, ptrs, lens = _marks_c(marks)
        check(self._lib.ssw_writer_embed(self._h, ptrs, lens, len(arrs)), "Writer::embed")

    def _out(self, out, dtype):
        if out is None:
            return np.empty((self.height, self.width, 3), dtype)
        if out.dtype != dtype or out.shape != (self.height, self.width, 3) or not out.flags.c_contiguous:
            raise ValueError(f"out must be a contiguous {np.dtype(dtype).name} array [H, W, 3]")
        return out

    def result(self, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Writer::result (algorithm.rs:361-379) -> f32 [H, W, 3]."""
        out = self._out(out, np.float32)
        check(self._lib.ssw_writer_result(self._h, out.ctypes.data), "Writer::result")
        return out

    def result_rgb8(self, out: Optional[np.ndarray] = None) -> np.ndarray:
        """`writer.result().into_rgb8()`: quantised on the device, u8 [H, W, 3]."""
        out = self._out(out, np.uint8)
        check(self._lib.ssw_writer_result_rgb8(self._h, out.ctypes.data), "Writer::result")
        return out

    def mark(self, marks, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Writer::mark (algorithm.rs:355-358) -> f32 [H, W, 3]."""
        arrs, ptrs, lens = _marks_c(marks)
        out = self._out(out, np.float32)
        check(self._lib.ssw_writer_mark(self._h, ptrs, lens, len(arrs), out.ctypes.data), "Writer::mark")
        return out

    def mark_rgb8(self, marks, out: Optional[np.ndarray] = None) -> np.ndarray:
        """`writer.mark(marks).into_rgb8()` (examples/main.rs:271-278): u8 [H, W, 3]."""
        arrs, ptrs, lens = _marks_c(marks)
        out = self._out(out, np.uint8)
        check(self._lib.ssw_writer_mark_rgb8(self._h, ptrs, lens, len(arrs), out.ctypes.data), "Writer::mark")
        return out

    def _copies(self, marks, out, dtype, fn, what):
        arrs = [_mark_data(m) for m in marks]
        if len({a.size for a in arrs}) > 1:
            raise ValueError("mark_copies: every mark must have the same length")
        n, k = len(arrs), (arrs[0].size if arrs else 0)
        m = np.ascontiguousarray(np.stack(arrs) if arrs else np.zeros((0, 0)), dtype=np.float32)
        shape = (n, self.height, self.width, 3)
        if out is None:
            out = np.empty(shape, dtype)
        elif out.dtype != dtype or out.shape != shape or not out.flags.c_contiguous:
            raise ValueError(f"out must be a contiguous {np.dtype(dtype).name} array [N, H, W, 3]")
        check(fn(self._h, m.ctypes.data, n, k, out.ctypes.data), what)
        return out

    def mark_copies(self, marks, out: Optional[np.ndarray] = None) -> np.ndarray:
        """Fingerprinting: for every mark m_i what `embed([m_i])` + `result()` would give on a clone of this writer as it
        stands (algorithm.rs:348-379; the loop of examples/main.rs:266-278 once per recipient) -> f32 [N, H, W, 3].  The
        shared transform runs once and each copy is a low-rank update on the GPU; the writer is neither consumed nor
        changed.  All marks must have one length (ValueError otherwise)."""
        return self._copies(marks, out, np.float32, self._lib.ssw_writer_mark_copies, "Writer::mark_copies")

    def mark_copies_rgb8(self, marks, out: Optional[np.ndarray] = None) -> np.ndarray:
        """mark_copies quantised like `into_rgb8()` on the device: u8 [N, H, W, 3]."""
        return self._copies(marks, out, np.uint8, self._lib.ssw_writer_mark_copies_rgb8, "Writer::mark_copies")

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._ctx.handle:
                self._lib.ssw_writer_destroy(self._h)
            self._h = None
        except Exception:
            pass


# ---- Reader (algorithm.rs:435-594) -------------------------------------------------------------
class Reader:
    def __init__(self, image, is_base: bool, config: Optional[ReadConfig], ctx: Optional[Context] = None):
        self._ctx = ctx or default_context()
        self._lib = self._ctx._lib
        rgb = _as_rgb(image)
        self.height, self.width = rgb.shape[:2]
        self.is_base = is_base
        h = C.c_void_p()
        cfg = config._c() if config is not None else None
        create = {np.dtype(np.uint8): self._lib.ssw_reader_create_rgb8,
                  np.dtype(np.uint16): self._lib.ssw_reader_create_rgb16}.get(rgb.dtype, self._lib.ssw_reader_create)
        check(create(self._ctx.handle, rgb.ctypes.data, self.width, self.height, int(is_base),
                     C.byref(cfg) if cfg is not None else None, C.byref(h)), "Reader::new_impl")
        self._h = h

    @staticmethod
    def base(image, config: Optional[ReadConfig] = None, ctx: Optional[Context] = None) -> "Reader":
        """Reader::base (algorithm.rs:462-464)."""
        return Reader(image, True, config or ReadConfig.default(), ctx)

    @staticmethod
    def derived(image, ctx: Optional[Context] = None, precision: int = Precision.F64) -> "ReaderDerived":
        """Reader::derived (algorithm.rs:469-471)."""
        return ReaderDerived(image, ctx, precision)

    def coefficients(self) -> np.ndarray:
        out = np.empty(self.height * self.width, np.float32)
        check(self._lib.ssw_reader_coefficients(self._h, out.ctypes.data), "Reader::coefficients")
        return out

    def indices(self, k: Optional[int] = None) -> np.ndarray:
        """Reader::indices (algorithm.rs:506-508); `k` limits the list to its first k entries."""
        n = self.height * self.width - 1
        k = n if k is None else int(k)
        out = np.empty(max(k, 0), np.uint64)
        check(self._lib.ssw_reader_indices(self._h, k, out.ctypes.data), "Reader::indices")
        return out

    def extract(self, derived: "ReaderDerived", extracted) -> np.ndarray:
        """Reader::extract (algorithm.rs:529-539).  `extracted` is the output buffer (numpy f32,
        written in place) or an int length; the filled array is returned."""
        out = np.empty(int(extracted), np.float32) if isinstance(extracted, (int, np.integer)) else extracted
        if out.dtype != np.float32 or not out.flags.c_contiguous:
            raise ValueError("extracted must be a contiguous float32 array")
        d = derived._reader if isinstance(derived, ReaderDerived) else derived
        check(self._lib.ssw_reader_extract(self._h, d._h, out.ctypes.data, out.size), "Reader::extract")
        return out

    def trace(self, suspects, marks, threshold: float = 6.0, k: Optional[int] = None, placements=None, base=None) -> "TraceResult":
        """Whose copy is each suspect?  Per 8-bit suspect image s: `self.extract(Reader.derived(s), k)`, then
        `Tester(ext).similarity(m)` for every stored mark m (algorithm.rs:529-539, :696-714; the `test` loop of
        examples/main.rs:369-415) as ONE call: this reader's transformed plane and index list are reused, the suspects
        stream to the GPU.  All marks must have one length (ValueError otherwise); `k` is only needed without marks.

        placements: None (every suspect has the original's shape, as before), or one entry per suspect, a `Placement` or
        None; suspects are then [h][w][3] or [h][w][4] arrays of any size and are restored on the device first (see
        `restore` for the rule).  `base`: the original's 8-bit pixels again -- the reader keeps the plane and the list,
        not the image -- needed as soon as a suspect has an alpha channel, covers less than the whole frame or is `Rotated`."""
        if not self.is_base:
            raise SswError(L.SSW_ERR_NOT_BASE, "Reader::trace")
        if placements is not None:
            turned = {}
            if any(isinstance(p, Rotated) for p in placements):          # turned copies: one angle search, one unrotate call
                suspects, placements, turned = _undo_rotated(base, suspects, placements, self._ctx)
            located_turned = {}
            if any(isinstance(p, Locate) and p.turned_range() for p in placements):      # cut-outs of a turned copy: found and laid back
                suspects, placements, located_turned = _undo_turned_cuts(base, suspects, placements, self._ctx)
            if any(isinstance(p, Locate) for p in placements):           # cut-outs at an unknown position: one locate call
                placements, _ = _resolve_locates(base, suspects, placements, self._ctx)
            arrs, ptrs, pl = _placed_suspects(suspects, placements, self.width, self.height)
            m, k = _trace_marks(marks, k)
            res = TraceResult.empty(len(arrs), m.shape[0], k)
            res.turned, res.located_turned = turned, located_turned
            b = None if base is None else _base_rgb8(base, self.width, self.height)
            check(self._lib.ssw_reader_trace_restored_host_rgb8(self._h, b.ctypes.data if b is not None else None, ptrs, pl, len(arrs), k,
                                                                *res._args(m, threshold)), "Reader::trace")
            return res
        arrs, ptrs, w, h = _frame_ptrs(suspects)
        if (w, h) != (self.width, self.height):
            raise SswError(L.SSW_ERR_LENGTH_MISMATCH, "Reader::trace")
        m, k = _trace_marks(marks, k)
        res = TraceResult.empty(len(arrs), m.shape[0], k)
        check(self._lib.ssw_reader_trace_host_rgb8(self._h, ptrs, len(arrs), k, *res._args(m, threshold)), "Reader::trace")
        return res

    def __del__(self):
        try:
            if getattr(self, "_h", None) and self._ctx.handle:
                self._lib.ssw_reader_destroy(self._h)
            self._h = None
        except Exception:
            pass


class ReaderDerived:
    """algorithm.rs:448-456: a Reader that can only be read from."""

    def __init__(self, image, ctx: Optional[Context] = None, precision: int = Precision.F64):
        cfg = ReadConfig(precision=precision)
        self._reader = Reader(image, False, cfg, ctx)

    new = classmethod(lambda cls, image, ctx=None, precision=Precision.F64: cls(image, ctx, precision))

    def coefficients(self) -> np.ndarray:
        return self._reader.coefficients()


# ---- the callers' loops over host images as one streaming call (examples/main.rs:271-278, :383-415) ----------------
def _frame_ptrs(images, w=None, h=None):
    """n 8-bit [H, W, 3] host images (a list, or one [n, H, W, 3] array) -> (kept-alive arrays, void* array, w, h)."""
    arrs = [np.ascontiguousarray(np.asarray(im)[:, :, :3]) for im in images]
    if not arrs:
        raise ValueError("no images")
    for a in arrs:
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape != arrs[0].shape:
            raise ValueError("images must be 8-bit [H, W, 3] arrays of one size")
    hh, ww = arrs[0].shape[:2]
    if (w, h) != (None, None) and (ww, hh) != (w, h):
        raise ValueError("image sizes differ")
    return arrs, (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs]), ww, hh


def mark_many(images, marks, config: Optional[WriteConfig] = None, ctx: Optional[Context] = None, out=None):
    """`for (image, mark) in ..: Writer::new(image, config).mark(&[&mark]).into_rgb8()` (examples/main.rs:271-278) as ONE
    streaming call over n 8-bit host images: ssw_batch_embed_host_rgb8.  marks: [n][k].  Returns / fills `out`, a list
    of n u8 [H, W, 3] arrays (pinned arrays from Context.pinned_empty are the DMA source / target themselves)."""
    ctx = ctx or default_context()
    config = config or WriteConfig.default()
    arrs, ptrs, w, h = _frame_ptrs(images)
    m = np.ascontiguousarray(np.stack([_mark_data(x) for x in marks]), dtype=np.float32)
    if m.ndim != 2 or m.shape[0] != len(arrs):
        raise ValueError("one mark of equal length per image")
    if out is None:
        out = [np.empty((h, w, 3), np.uint8) for _ in arrs]
    out = list(out)
    if len(out) != len(arrs):                   # the C side reads one output pointer per input frame
        raise ValueError("out: one output array per image")
    for o in out:
        if o.dtype != np.uint8 or o.shape != (h, w, 3) or not o.flags.c_contiguous:
            raise ValueError("out: contiguous u8 [H, W, 3] arrays")
    optrs = (C.c_void_p * len(out))(*[o.ctypes.data for o in out])
    cfg = config._c()
    check(ctx._lib.ssw_batch_embed_host_rgb8(ctx.handle, C.byref(cfg), ptrs, len(arrs), w, h, m.ctypes.data, m.shape[1], optrs),
          "ssw_batch_embed_host_rgb8")
    return out


def extract_many(base_images, derived_images, k: int, marks=None, config: Optional[ReadConfig] = None, ctx: Optional[Context] = None):
    """`Reader::base(b, config).extract(&Reader::derived(d), ..)` (+ `Tester::similarity` against marks[i]) per image pair
    (examples/main.rs:383-415) as ONE streaming call: ssw_batch_extract_host_rgb8.  Returns (extracted [n][k], sims [n] or None)."""
    ctx = ctx or default_context()
    config = config or ReadConfig.default()
    ba, bp, w, h = _frame_ptrs(base_images)
    if len(derived_images) != len(ba):          # checked before any pointer array is handed to the C side
        raise ValueError("one derived image per base image")
    da, dp, _, _ = _frame_ptrs(derived_images, w, h)
    n = len(ba)
    ext = np.empty((n, k), np.float32)
    m = sims = None
    if marks is not None:
        m = np.ascontiguousarray(np.stack([_mark_data(x) for x in marks]), dtype=np.float32)
        if m.shape != (n, k):
            raise ValueError("marks must be [n][k]")
        sims = np.empty(n, np.float32)
    cfg = config._c()
    check(ctx._lib.ssw_batch_extract_host_rgb8(ctx.handle, C.byref(cfg), bp, dp, n, w, h, k, ext.ctypes.data,
                                               m.ctypes.data if m is not None else None, sims.ctypes.data if sims is not None else None),
          "ssw_batch_extract_host_rgb8")
    return ext, sims


# ---- tracing: one original, many suspects, many stored marks (include/ssw.h: ssw_fingerprint_trace) -----------------
def _trace_marks(marks, k):
    arrs = [np.ascontiguousarray(_mark_data(x), dtype=np.float32) for x in (marks if marks is not None else [])]
    if len({a.size for a in arrs}) > 1:
        raise ValueError("trace: every mark must have the same length")
    if arrs and k is not None and int(k) != arrs[0].size:
        raise ValueError("trace: k differs from the marks' length")
    if not arrs and k is None:
        raise ValueError("trace: k is needed without marks")
    k = arrs[0].size if arrs else int(k)
    return (np.ascontiguousarray(np.stack(arrs)) if arrs else np.zeros((0, k), np.float32)), k


@dataclass
class TraceResult:
    """extracted [S][k]; sims [S][M] (the GEMM matrix, 1e-4 relative); best [S] (index of the mark a suspect carries most
    strongly, TraceResult.NONE without one -- e.g. the unmarked original, whose similarities are all NaN); best_sim [S]
    (Tester::similarity of that mark, exact); n_exceed [S] (marks above the threshold: 2 and more = colluders)."""
    extracted: np.ndarray
    sims: np.ndarray
    best: np.ndarray
    best_sim: np.ndarray
    n_exceed: np.ndarray
    threshold: float = 6.0
    turned: dict = field(default_factory=dict)      # {suspect: FoundAngle} of the `Rotated` entries whose angle was searched for
    located_turned: dict = field(default_factory=dict)      # {suspect: LocatedTurned} of the `Locate(turned=...)` entries
    NONE = L.TRACE_NONE

    @staticmethod
    def empty(n, n_marks, k) -> "TraceResult":
        return TraceResult(np.empty((n, k), np.float32), np.empty((n, n_marks), np.float32), np.full(n, L.TRACE_NONE, np.uint32),
                           np.full(n, np.nan, np.float32), np.zeros(n, np.uint32))

    def _args(self, m, threshold):
        """(marks, n_marks, threshold, extracted, sims, best, best_sim, n_exceed) of the C entry points."""
        self.threshold = float(threshold)
        if m.shape[0] == 0:
            return (None, 0, C.c_float(threshold), self.extracted.ctypes.data, None, None, None, None)
        return (m.ctypes.data, m.shape[0], C.c_float(threshold), self.extracted.ctypes.data, self.sims.ctypes.data,
                self.best.ctypes.data, self.best_sim.ctypes.data, self.n_exceed.ctypes.data)

    def matches(self, s: int) -> list:
        """Indices of the marks suspect s exceeds the threshold with (NaN never exceeds, algorithm.rs:677)."""
        return [int(j) for j in np.nonzero(self.sims[s] > np.float32(self.threshold))[0]]


# ---- tracing attacked copies: resized and cropped suspects are restored on the device (include/ssw.h: ssw_restore_rgb8) ----
@dataclass
class Placement:
    """Where a suspect lies in the original's frame: the rectangle at (x, y) of size w x h (None: see `restore`)."""
    x: int = 0
    y: int = 0
    w: Optional[int] = None
    h: Optional[int] = None


def _resolve_placement(p: Optional[Placement], sw: int, sh: int, channels: int, W: int, H: int) -> L.Placement:
    """The rule of `restore`: no rectangle size at (0, 0) on a suspect whose size differs from the original's = whole frame."""
    p = p or Placement()
    if (p.w is None) != (p.h is None):
        raise ValueError("Placement: w and h go together")
    if p.w is not None:
        pw, ph = int(p.w), int(p.h)
    elif (p.x, p.y) == (0, 0) and (sw, sh) != (W, H):
        pw, ph = W, H
    else:
        pw, ph = sw, sh
    if min(p.x, p.y) < 0 or pw <= 0 or ph <= 0:
        raise ValueError("Placement: negative position or empty rectangle")
    return L.Placement(sw, sh, channels, int(p.x), int(p.y), pw, ph)


def _base_rgb8(base, w=None, h=None) -> np.ndarray:
    b = np.ascontiguousarray(np.asarray(base)[:, :, :3])
    if b.dtype != np.uint8 or b.ndim != 3 or b.shape[2] != 3:
        raise ValueError("base must be an 8-bit [H, W, 3] image")
    if w is not None and (b.shape[1], b.shape[0]) != (w, h):
        raise ValueError("base: not the size of the reader's image")
    return b


def _placed_suspects(suspects, placements, W: int, H: int):
    """Suspects of any size with 3 or 4 channels + one placement each -> (kept-alive arrays, void* array, ssw_placement array)."""
    arrs = [np.ascontiguousarray(np.asarray(im)) for im in suspects]
    if not arrs:
        raise ValueError("no images")
    placements = list(placements)
    if len(placements) != len(arrs):
        raise ValueError("placements: one entry (a Placement or None) per suspect")
    for a in arrs:
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4) or 0 in a.shape:
            raise ValueError("suspects must be 8-bit [h, w, 3] or [h, w, 4] arrays")
    pl = (L.Placement * len(arrs))(*[_resolve_placement(p, a.shape[1], a.shape[0], a.shape[2], W, H) for a, p in zip(arrs, placements)])
    return arrs, (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs]), pl


# ---- locating cut-outs: the placement nobody told us (include/ssw.h: ssw_locate_rgb8) ---------------------------------------
@dataclass
class Locate:
    """A placement entry that says "find me": the suspect is a cut-out of the original at an unknown position; w x h is the
    size it had in the original's frame (None: its own size).  When that size is not known either: `widths=(lo, hi)`, the
    widths it may have had in the original, or `scale=(lo, hi)`, the same as factors of the suspect's own width (0.5: it was
    enlarged to twice its size after it was cut out) -- found by the scale ladder of ssw_locate_scaled_rgb8.  `turned=(lo, hi)`,
    or `turned=True` for +-10 degrees: the suspect is a cut-out of the frame TURNED by an unknown angle in that range -- what a
    photo editor's "straighten" leaves --, at the original's scale: angle and centre are found together (`locate_turned`) and the
    suspect is laid back into the frame (`restore_turned`).  `turned=` goes with none of the others.  `aspect=a`, 1 .. 4, beside
    `widths=` or `scale=`: the cut-out's sides were rounded on their own when it was scaled (480 x 333 halved is 240 x 166, not
    the 332 rows the kept aspect ratio gives back), so the sizes within a pixels of the ladder's answer are rescored in both
    dimensions (ssw_locate_free_rgb8).  0 or None: the ladder's answer as it is."""
    w: Optional[int] = None
    h: Optional[int] = None
    widths: Optional[Tuple[int, int]] = None
    scale: Optional[Tuple[float, float]] = None
    turned: Any = None
    aspect: Optional[int] = None

    def aspect_slack(self) -> int:
        """a of an `aspect=` entry, 0 for any other; ValueError for an a outside 0 .. 4 or an entry that has no range of widths."""
        if self.aspect is None:
            return 0
        if isinstance(self.aspect, bool) or int(self.aspect) != self.aspect or not 0 <= self.aspect <= L.LOCATE_FREE_MAX_SLACK:
            raise ValueError(f"Locate: aspect= is an integer from 0 to {L.LOCATE_FREE_MAX_SLACK}")
        if self.widths is None and self.scale is None:
            raise ValueError("Locate: aspect= goes with widths= or scale=, not with (w, h) or turned=")
        return int(self.aspect)

    def turned_range(self) -> Optional[Tuple[float, float]]:
        """(lo, hi) in degrees of a `turned=` entry, None for any other."""
        if self.turned is None or self.turned is False:
            return None
        if self.w is not None or self.h is not None or self.widths is not None or self.scale is not None or self.aspect is not None:
            raise ValueError("Locate: turned= goes with none of (w, h), widths=, scale= and aspect=")
        return _search((-10.0, 10.0) if self.turned is True else self.turned, "Locate(turned=)")

    def width_range(self, suspect_width: int) -> Optional[Tuple[int, int]]:
        """(wmin, wmax) of a ranged entry -- scale factors rounded outwards --, None for an entry of known size."""
        self.turned_range()                                      # (refuses turned= beside the others)
        self.aspect_slack()                                      # (refuses aspect= without a range)
        if self.widths is None and self.scale is None:
            return None
        if (self.widths is not None and self.scale is not None) or self.w is not None or self.h is not None:
            raise ValueError("Locate: one of (w, h), widths= and scale=")
        lo, hi = self.widths if self.widths is not None else self.scale
        if self.scale is not None:
            if not (0 < lo <= hi):
                raise ValueError("Locate: scale=(lo, hi) with 0 < lo <= hi")
            lo, hi = max(1, math.floor(lo * suspect_width)), math.ceil(hi * suspect_width)
        if int(lo) != lo or int(hi) != hi or not (0 < lo <= hi):
            raise ValueError("Locate: widths=(lo, hi), integers with 0 < lo <= hi")
        return int(lo), int(hi)


@dataclass
class Located:
    """Where a suspect lies: `placement`, a complete Placement(x, y, w, h) ready for `restore` / `trace_many`; `sad`, the sum
    of absolute luma differences there; `mean_abs_diff` = sad / (w * h) -- a few units for a true match of a marked copy.
    `size` is the (w, h) the suspect had in the original: given by the caller, or found by the scale ladder."""
    placement: Placement
    sad: int
    mean_abs_diff: float

    @property
    def size(self) -> Tuple[int, int]:
        return self.placement.w, self.placement.h


def _locate_sizes(arrs, sizes, W: int, H: int):
    """One (w, h) pair, Locate or None per suspect -> ssw_placement array with x = y = 0 and the size each suspect had."""
    sizes = list(sizes) if sizes is not None else [None] * len(arrs)
    if len(sizes) != len(arrs):
        raise ValueError("sizes: one entry (a Locate, a (w, h) pair or None) per suspect")
    out = []
    for a, z in zip(arrs, sizes):
        w, h = (z.w, z.h) if isinstance(z, Locate) else (z if z is not None else (None, None))
        if (w is None) != (h is None):
            raise ValueError("Locate: w and h go together")
        pw, ph = (int(w), int(h)) if w is not None else (a.shape[1], a.shape[0])
        if pw <= 0 or ph <= 0 or pw > W or ph > H:
            raise ValueError(f"Locate: a {pw}x{ph} rectangle does not fit the original ({W}x{H})")
        out.append(L.Placement(a.shape[1], a.shape[0], a.shape[2], 0, 0, pw, ph))
    return (L.Placement * len(out))(*out)


def locate(base, suspects, sizes=None, ctx: Optional[Context] = None) -> list:
    """Where in the original does each suspect lie?  A search over every translation on the device (ssw_locate_rgb8): integer
    luma differences, a coarse pass over all positions, the 8 best rescored at full resolution -- exactly reproducible, see
    include/ssw.h for the definition.  suspects: 8-bit [h, w, 3] or [h, w, 4] arrays (alpha is ignored: a mostly transparent
    cut-out is not supported).  sizes: None, or per suspect a `Locate(w, h)` / (w, h) pair / None -- the size the cut-out
    had in the original when it was scaled afterwards --, or a `Locate(widths=(lo, hi))` / `Locate(scale=(lo, hi))` when that
    size is unknown: those entries go through the scale ladder (ssw_locate_scaled_rgb8; aspect ratio kept, the smaller side at
    least 32) and `Located.size` says what was found; with `aspect=a` the sizes within a pixels of that answer are rescored in
    both dimensions (ssw_locate_free_rgb8), for thumbnails whose sides were rounded on their own.  Returns one `Located` per suspect.  A turned cut-out is `locate_turned`'s; a
    cut-out of a featureless region (the cat's grey background) is ambiguous."""
    ctx = ctx or default_context()
    b = _base_rgb8(base)
    H, W = b.shape[:2]
    arrs = [np.ascontiguousarray(np.asarray(im)) for im in suspects]
    if not arrs:
        return []
    for a in arrs:
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4) or 0 in a.shape:
            raise ValueError("suspects must be 8-bit [h, w, 3] or [h, w, 4] arrays")
    sizes = list(sizes) if sizes is not None else [None] * len(arrs)
    if len(sizes) != len(arrs):
        raise ValueError("sizes: one entry (a Locate, a (w, h) pair or None) per suspect")
    if any(isinstance(z, Locate) and z.turned_range() for z in sizes):
        raise ValueError("locate: a Locate(turned=...) entry is searched for with locate_turned")
    ranges = [z.width_range(a.shape[1]) if isinstance(z, Locate) else None for a, z in zip(arrs, sizes)]
    if any(r is not None for r in ranges):
        return _locate_mixed(ctx, b, arrs, sizes, ranges)
    pl = _locate_sizes(arrs, sizes, W, H)
    n = len(arrs)
    dev_base = ctx.to_device(b)
    dev = [ctx.to_device(a) for a in arrs]
    ptrs = (C.c_void_p * n)(*[d.ptr.value for d in dev])
    sad = (C.c_uint64 * n)()
    try:
        check(ctx._lib.ssw_locate_rgb8(ctx.handle, dev_base.ptr, W, H, ptrs, pl, n, sad), "ssw_locate_rgb8")
    finally:
        for d in dev + [dev_base]:
            d.free()
    return [Located(Placement(int(p.x), int(p.y), int(p.pw), int(p.ph)), int(s), int(s) / (int(p.pw) * int(p.ph))) for p, s in zip(pl, sad)]


def _locate_mixed(ctx, b, arrs, sizes, ranges) -> list:
    """`locate` with ranged entries: one ssw_locate_scaled_rgb8 call for those, one ssw_locate_rgb8 call for the others, and
    one ssw_locate_free_rgb8 call for the ranged entries with `aspect` > 0."""
    H, W = b.shape[:2]
    slack = [z.aspect_slack() if isinstance(z, Locate) else 0 for z in sizes]
    ranged = [i for i, r in enumerate(ranges) if r is not None and not slack[i]]
    free = [i for i, r in enumerate(ranges) if r is not None and slack[i]]
    fixed = [i for i, r in enumerate(ranges) if r is None]
    out = [None] * len(arrs)
    dev_base = ctx.to_device(b)
    dev = [ctx.to_device(a) for a in arrs]
    try:
        for idx, scaled in ((fixed, False), (ranged, True), (free, True)):
            if not idx:
                continue
            n = len(idx)
            ptrs = (C.c_void_p * n)(*[dev[i].ptr.value for i in idx])
            sad = (C.c_uint64 * n)()
            if scaled:
                pl = (L.Placement * n)(*[L.Placement(arrs[i].shape[1], arrs[i].shape[0], arrs[i].shape[2], 0, 0, 0, 0) for i in idx])
                rg = (L.ScaleRange * n)(*[L.ScaleRange(*ranges[i]) for i in idx])
                if idx is free:
                    sl = (C.c_uint32 * n)(*[slack[i] for i in idx])
                    check(ctx._lib.ssw_locate_free_rgb8(ctx.handle, dev_base.ptr, W, H, ptrs, pl, rg, sl, n, sad), "ssw_locate_free_rgb8")
                else:
                    check(ctx._lib.ssw_locate_scaled_rgb8(ctx.handle, dev_base.ptr, W, H, ptrs, pl, rg, n, sad), "ssw_locate_scaled_rgb8")
            else:
                pl = _locate_sizes([arrs[i] for i in idx], [sizes[i] for i in idx], W, H)
                check(ctx._lib.ssw_locate_rgb8(ctx.handle, dev_base.ptr, W, H, ptrs, pl, n, sad), "ssw_locate_rgb8")
            for i, p, s in zip(idx, pl, sad):
                out[i] = Located(Placement(int(p.x), int(p.y), int(p.pw), int(p.ph)), int(s), int(s) / (int(p.pw) * int(p.ph)))
    finally:
        for d in dev + [dev_base]:
            d.free()
    return out


def _resolve_locates(base, suspects, placements, ctx=None, locate_fn=None):
    """placements with `Locate` entries -> (placements with every Locate replaced by the Placement found, {index: Located}):
    ONE locate call for all of them; the other entries pass through untouched."""
    placements = list(placements)
    suspects = list(suspects)
    if len(placements) != len(suspects):
        raise ValueError("placements: one entry (a Placement, a Locate or None) per suspect")
    todo = [i for i, p in enumerate(placements) if isinstance(p, Locate)]
    if not todo:
        return placements, {}
    if base is None:
        raise ValueError("Locate entries need the original's pixels (base=)")
    found = (locate_fn or locate)(base, [suspects[i] for i in todo], [placements[i] for i in todo], ctx)
    for i, f in zip(todo, found):
        placements[i] = f.placement
    return placements, dict(zip(todo, found))


def restore(base, suspects, placements=None, ctx: Optional[Context] = None) -> list:
    """What tracing with `placements` does to each suspect before it extracts, as frames: the recipes of the reference's
    attack tests -- resize back with CatmullRom (tests/attack_resize.rs:31-36), then "complement the attacked image with the
    original" through Rgba::blend (tests/attack_crop.rs:56-70) -- on the device (ssw_restore_rgb8).  Returns one u8
    [H, W, 3] frame per suspect.

    base: the original, 8-bit [H, W, 3].  suspects: 8-bit [h, w, 3] or [h, w, 4] arrays of any size.  placements: None, or
    one entry per suspect, each a `Placement(x, y, w, h)` -- the rectangle of the original's frame the suspect covers; it is
    resized to w x h when its own size differs -- or None.  The rule for what is left out: a None entry, or a Placement
    without w / h at (0, 0), means "whole frame" when the suspect's size differs from the original's (a scaled copy), and
    "own size at (x, y)" otherwise (a cut-out, or an RGBA image of full size).  An alpha channel is filtered like a colour
    channel and blended over the original: alpha 0 keeps the original's pixel.  A `Locate(w, h)` entry is a cut-out whose
    position is not known: all such entries are found with one `locate` call first and then treated as that Placement; a
    `Locate(turned=...)` entry is found with `locate_turned` and comes back as `restore_turned` makes it."""
    ctx = ctx or default_context()
    b = _base_rgb8(base)
    H, W = b.shape[:2]
    suspects = list(suspects)
    if placements is not None and any(isinstance(p, Locate) and p.turned_range() for p in placements):
        suspects, placements, _ = _undo_turned_cuts(b, suspects, placements, ctx)
    if placements is not None and any(isinstance(p, Locate) for p in placements):
        placements, _ = _resolve_locates(b, suspects, placements, ctx)
    arrs, _, pl = _placed_suspects(suspects, placements if placements is not None else [None] * len(suspects), W, H)
    n, fb = len(arrs), W * H * 3
    dev_base, dev_out = ctx.to_device(b), ctx.alloc(n * fb)
    dev = [ctx.to_device(a) for a in arrs]
    ptrs = (C.c_void_p * n)(*[d.ptr.value for d in dev])
    check(ctx._lib.ssw_restore_rgb8(ctx.handle, dev_base.ptr, W, H, ptrs, pl, n, dev_out.ptr), "ssw_restore_rgb8")
    out = dev_out.to_host(np.uint8, (n, H, W, 3))
    for d in dev + [dev_base, dev_out]:
        d.free()
    return [out[i] for i in range(n)]


def trace_many(base, suspects, marks, k: Optional[int] = None, threshold: float = 6.0, config: Optional[ReadConfig] = None,
               ctx: Optional[Context] = None, placements=None) -> TraceResult:
    """`Reader::base(base, config)` once, then per suspect `extract` + `Tester::similarity` against every mark
    (examples/main.rs:369-415) as ONE streaming call over 8-bit host images: ssw_fingerprint_trace_host_rgb8.

    placements: None (every suspect has the original's shape, as before), or one entry per suspect, a `Placement` or None:
    suspects of any size with 3 or 4 channels are restored on the device first (ssw_fingerprint_trace_restored_host_rgb8;
    `restore` spells out the rule and returns the frames this call extracts from).  `Locate(w, h)` entries -- cut-outs at an
    unknown position -- are found with one `locate` call first.  `Rotated(angle)` entries -- copies of the original's size that
    were turned by a known angle -- are turned back with one `unrotate` call first and traced as whole frames; `Rotated()`
    entries, whose angle is not known, are searched for with one `find_angle` call before that (`TraceResult.turned` says what
    was found).  `Locate(turned=...)` entries -- cut-outs of a copy turned by an unknown angle -- are found with one `locate_turned`
    call per distinct range and laid back into the frame with one `restore_turned` call (`TraceResult.located_turned`)."""
    ctx = ctx or default_context()
    config = config or ReadConfig.default()
    if placements is not None:
        b = _base_rgb8(base)
        turned = {}
        if any(isinstance(p, Rotated) for p in placements):
            suspects, placements, turned = _undo_rotated(b, suspects, placements, ctx)
        located_turned = {}
        if any(isinstance(p, Locate) and p.turned_range() for p in placements):
            suspects, placements, located_turned = _undo_turned_cuts(b, suspects, placements, ctx)
        if any(isinstance(p, Locate) for p in placements):
            placements, _ = _resolve_locates(b, suspects, placements, ctx)
        arrs, ptrs, pl = _placed_suspects(suspects, placements, b.shape[1], b.shape[0])
        m, k = _trace_marks(marks, k)
        res = TraceResult.empty(len(arrs), m.shape[0], k)
        res.turned, res.located_turned = turned, located_turned
        cfg = config._c()
        check(ctx._lib.ssw_fingerprint_trace_restored_host_rgb8(ctx.handle, C.byref(cfg), b.ctypes.data, b.shape[1], b.shape[0], ptrs, pl,
                                                                len(arrs), k, *res._args(m, threshold)),
              "ssw_fingerprint_trace_restored_host_rgb8")
        return res
    b = np.ascontiguousarray(np.asarray(base)[:, :, :3])
    if b.dtype != np.uint8:
        raise ValueError("base must be an 8-bit [H, W, 3] image")
    arrs, ptrs, w, h = _frame_ptrs(suspects, b.shape[1], b.shape[0])
    m, k = _trace_marks(marks, k)
    res = TraceResult.empty(len(arrs), m.shape[0], k)
    cfg = config._c()
    check(ctx._lib.ssw_fingerprint_trace_host_rgb8(ctx.handle, C.byref(cfg), b.ctypes.data, ptrs, len(arrs), w, h, k,
                                                   *res._args(m, threshold)), "ssw_fingerprint_trace_host_rgb8")
    return res


# ---- identifying a suspect's original: an image catalogue (include/ssw.h: ssw_signature_rgb8, ssw_signature_match) -----------
IDENTIFY_MAX_DISTANCE = 8192


def _sig_frames(images):
    arrs = [np.ascontiguousarray(np.asarray(im)) for im in images]
    for a in arrs:
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4):
            raise ValueError("images must be 8-bit [h, w, 3] or [h, w, 4] arrays")
        if a.shape[0] < 32 or a.shape[1] < 32:
            raise ValueError(f"a {a.shape[1]}x{a.shape[0]} image is too small for a signature (32x32 at least)")
    return arrs


def signature(images, ctx: Optional[Context] = None) -> np.ndarray:
    """The signatures of 8-bit images of any sizes, [h, w, 3] or [h, w, 4] (alpha is ignored) -> uint8 [n][1024]: the rounded
    mean luma of the cells of a 32 x 32 grid, integers only (include/ssw.h states the definition); one call,
    ssw_signature_host_rgb8."""
    arrs = _sig_frames(images)
    out = np.empty((len(arrs), L.SIGNATURE_BYTES), np.uint8)
    if not arrs:
        return out
    ctx = ctx or default_context()
    ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    shapes = (L.ImageShape * len(arrs))(*[L.ImageShape(a.shape[1], a.shape[0], a.shape[2]) for a in arrs])
    check(ctx._lib.ssw_signature_host_rgb8(ctx.handle, ptrs, shapes, len(arrs), out.ctypes.data), "ssw_signature_host_rgb8")
    return out


class Catalogue:
    """The originals someone owns, as signatures: `add` them once, `save` the file, and `match` / `identify` name the original of
    a suspect picture -- the stage in front of `locate`, `restore` and `trace_many`, which all start from "here is the
    original".  The signatures stay on the device between `match` calls (uploaded again only after an `add`)."""

    def __init__(self, ctx: Optional[Context] = None):
        self._ctx = ctx
        self.names: List[str] = []
        self.marks_files: List[Optional[str]] = []
        self._sigs = np.zeros((0, L.SIGNATURE_BYTES), np.uint8)
        self._sizes = np.zeros((0, 2), np.uint32)
        self._dev: Optional[DeviceBuffer] = None
        self._dev_n = -1

    def __len__(self):
        return len(self.names)

    @property
    def signatures(self) -> np.ndarray:
        return self._sigs

    @property
    def sizes(self) -> np.ndarray:
        return self._sizes

    def add_signatures(self, names, signatures, sizes, marks_files=None) -> None:
        """Entries whose signatures are known already (a loaded file, another catalogue): no device work."""
        sig = np.ascontiguousarray(signatures, np.uint8).reshape(-1, L.SIGNATURE_BYTES)
        sizes = np.asarray(sizes, np.uint32).reshape(-1, 2)
        names = [str(x) for x in names]
        marks_files = list(marks_files) if marks_files is not None else [None] * len(names)
        if not (len(names) == len(marks_files) == sig.shape[0] == sizes.shape[0]):
            raise ValueError("Catalogue: names, signatures, sizes and marks_files differ in length")
        self.names += names
        self.marks_files += [str(m) if m else None for m in marks_files]
        self._sigs = np.concatenate([self._sigs, sig])
        self._sizes = np.concatenate([self._sizes, sizes])

    def add(self, name: str, image, marks_file: Optional[str] = None) -> None:
        self.add_many([name], [image], [marks_file])

    def add_many(self, names, images, marks_files=None) -> None:
        """`add` for several originals with one signature call."""
        arrs = _sig_frames(images)
        self.add_signatures(names, signature(arrs, self._context()), [(a.shape[1], a.shape[0]) for a in arrs], marks_files)

    def _context(self) -> Context:
        if self._ctx is None:
            self._ctx = default_context()
        return self._ctx

    def _resident(self) -> Optional[DeviceBuffer]:
        if self._dev_n != len(self):
            if self._dev is not None:
                self._dev.free()
            self._dev = self._context().to_device(self._sigs) if len(self) else None
            self._dev_n = len(self)
        return self._dev

    def match_signatures(self, signatures, top: int = 1) -> Tuple[np.ndarray, np.ndarray]:
        """(index [nq][top], distance [nq][top]) of the `top` nearest entries per query signature, nearest first, ties to the
        lower index; slots beyond the catalogue's size hold 0xFFFFFFFF in both (ssw_signature_match)."""
        if not 1 <= int(top) <= L.MATCH_TOP_MAX:
            raise ValueError(f"top must be 1 .. {L.MATCH_TOP_MAX}")
        q = np.ascontiguousarray(signatures, np.uint8).reshape(-1, L.SIGNATURE_BYTES)
        nq, top = q.shape[0], int(top)
        if nq == 0:
            return np.zeros((0, top), np.uint32), np.zeros((0, top), np.uint32)
        ctx = self._context()
        cat = self._resident()
        dq, dout = ctx.to_device(q), ctx.alloc(2 * nq * top * 4)
        try:
            check(ctx._lib.ssw_signature_match(ctx.handle, dq.ptr, nq, cat.ptr if cat is not None else None, len(self), top, dout.ptr,
                                               C.c_void_p(dout.ptr.value + nq * top * 4), None), "ssw_signature_match")
            both = dout.to_host(np.uint32, (2, nq, top))
        finally:
            dq.free()
            dout.free()
        return both[0], both[1]

    def match(self, suspects, top: int = 1) -> list:
        """Per suspect image the `top` nearest originals, nearest first: [[(name, distance, (w, h)), ...], ...] (fewer than
        `top` entries when the catalogue is smaller).  One signature call and one match call for all suspects."""
        idx, dist = self.match_signatures(signature(suspects, self._context()), top)
        return [[(self.names[i], int(d), (int(self._sizes[i][0]), int(self._sizes[i][1]))) for i, d in zip(row_i, row_d) if i != L.MATCH_NONE]
                for row_i, row_d in zip(idx, dist)]

    def save(self, path: str) -> None:
        from .storage import save_catalogue
        save_catalogue(path, self.names, self._sigs, self._sizes, self.marks_files)

    @staticmethod
    def load(path: str, ctx: Optional[Context] = None) -> "Catalogue":
        from .storage import load_catalogue
        names, sig, sizes, marks = load_catalogue(path)
        c = Catalogue(ctx)
        c.add_signatures(names, sig, sizes, marks)
        return c

    def __del__(self):
        try:
            if self._dev is not None:
                self._dev.free()
        except Exception:
            pass


@dataclass
class Identified:
    """`identify`'s answer for one suspect.  name: the original it is a copy of, or None when even the nearest entry is further
    than max_distance; nearest / distance / size / marks_file / index describe that nearest entry either way; candidates: the
    `top` nearest as (name, distance, (w, h)), nearest first."""
    name: Optional[str]
    nearest: Optional[str]
    distance: Optional[int]
    size: Optional[Tuple[int, int]]
    marks_file: Optional[str]
    index: Optional[int]
    candidates: list


def identify(catalogue: Catalogue, suspects, top: int = 1, max_distance: int = IDENTIFY_MAX_DISTANCE) -> list:
    """Which original is each suspect a copy of?  One `Identified` per suspect.  max_distance: the largest signature distance
    that still counts as "the same picture".  The default 8192 is a mean of 8 per cell; it lies between the largest distance
    measured for a genuine whole-frame copy (4715, a 640 x 444 photograph reduced to 64 x 44) and the smallest measured for an
    unrelated entry (15 640, the same photograph rolled by 40 columns) -- exactly that, not a guarantee.  Cut-outs are NOT
    identified (a cut-out is as far from its original as an unrelated picture), nor mirrored or turned copies."""
    idx, dist = catalogue.match_signatures(signature(suspects, catalogue._context()), top)
    out = []
    for row_i, row_d in zip(idx, dist):
        cands = [(catalogue.names[i], int(d), (int(catalogue.sizes[i][0]), int(catalogue.sizes[i][1]))) for i, d in zip(row_i, row_d)
                 if i != L.MATCH_NONE]
        if not cands:
            out.append(Identified(None, None, None, None, None, None, []))
            continue
        i, (name, d, size) = int(row_i[0]), cands[0]
        out.append(Identified(name if d <= max_distance else None, name, d, size, catalogue.marks_files[i], i, cands))
    return out


# ---- strength of a mark: visibility and collusion resistance (include/ssw.h: ssw_quality_rgb8, ssw_collude_rgb8) -------------
UPLOAD_GROUP_BYTES = 256 << 20      # frames the host wrappers keep on the device at a time (one frame's own size if that is more)


@dataclass
class Quality:
    """How far one copy is from its original (ssw_quality_rgb8): squared error per channel and of the luma, changed bytes and
    the largest byte difference -- integers; the derived figures are the caller's arithmetic and are made here."""
    sse: Tuple[int, int, int]
    sse_luma: int
    changed: int
    max_abs: int
    pixels: int

    @property
    def psnr(self) -> float:
        """10 log10(255^2 * 3 W H / (SSE_R + SSE_G + SSE_B)) in dB; inf for identical frames."""
        e = sum(self.sse)
        return math.inf if e == 0 else 10.0 * math.log10(255.0 ** 2 * 3 * self.pixels / e)

    @property
    def psnr_luma(self) -> float:
        return math.inf if self.sse_luma == 0 else 10.0 * math.log10(255.0 ** 2 * self.pixels / self.sse_luma)

    @property
    def changed_fraction(self) -> float:
        return self.changed / (3.0 * self.pixels) if self.pixels else 0.0


def _qualities(stats: np.ndarray, pixels: int) -> list:
    return [Quality((int(r[0]), int(r[1]), int(r[2])), int(r[3]), int(r[4]), int(r[5]), pixels) for r in stats]


def _frames_u8(images, what: str) -> list:
    arrs = [np.asarray(im) for im in images]
    for a in arrs:                                           # checked as they come: nothing is sliced away (an alpha channel is an error)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape != arrs[0].shape or a.size == 0:
            raise ValueError(f"{what}: 8-bit [H, W, 3] images of one size")
    return [np.ascontiguousarray(a) for a in arrs]


def _frames_of_side(images, what: str, user: str, side: int) -> list:
    """`_frames_u8` for `user` ("SSIM", "a JPEG attack"), which refuses frames with a side below `side`"""
    frames = _frames_u8(images, what)
    if frames and min(frames[0].shape[:2]) < side:
        raise ValueError(f"{what}: {user} needs frames of at least {side} x {side} pixels")
    return frames


def _upload_frames(ctx: Context, buf: "DeviceBuffer", arrs) -> "DeviceBuffer":
    for i, a in enumerate(arrs):
        check(ctx._lib.ssw_copy_to_dev(ctx.handle, C.c_void_p(buf.ptr.value + i * a.nbytes), a.ctypes.data, a.nbytes), "ssw_copy_to_dev")
    return buf


@contextmanager
def _owned(ctx: Context):
    """The device buffers of one host wrapper's call: yields `alloc`, the context's, and frees every buffer made through it on
    every way out of the `with` block -- an error from the library leaves nothing to `__del__`."""
    buffers = []

    def alloc(nbytes: int) -> "DeviceBuffer":
        buffers.append(ctx.alloc(nbytes))
        return buffers[-1]
    try:
        yield alloc
    finally:
        for d in buffers:
            d.free()


def _copies_against_originals(base, cp, what: str, ctx: Optional[Context], outputs, call) -> list:
    """The driver of `quality` and `ssim`.  base: one original, or one per copy of `cp` (checked here); the copies go up beside
    their originals in groups of at most UPLOAD_GROUP_BYTES of frames.  Per group call(ctx, dev_base, n_base, dev_copies, n,
    *dev_outputs) runs on device pointers, then every output comes down -- outputs: one (dtype, shape per copy) each.  Returns
    per group the list of its downloaded arrays, [n, *shape] each."""
    b = np.asarray(base) if not isinstance(base, (list, tuple)) else None
    bases = _frames_u8([base] if b is not None and b.ndim == 3 else base, what)
    if len(bases) not in (1, len(cp)) or bases[0].shape != cp[0].shape:
        raise ValueError(f"{what}: one original of the copies' size, or one per copy")
    ctx = ctx or default_context()
    fb, n, shared = cp[0].nbytes, len(cp), len(bases) == 1
    per = max(1, UPLOAD_GROUP_BYTES // (fb if shared else 2 * fb))
    groups = []
    with _owned(ctx) as alloc:
        dev_c = alloc(min(per, n) * fb)
        dev_o = [alloc(min(per, n) * int(np.prod(shape)) * np.dtype(dtype).itemsize) for dtype, shape in outputs]
        dev_b = _upload_frames(ctx, alloc(fb), bases) if shared else alloc(min(per, n) * fb)
        for g0 in range(0, n, per):
            g = cp[g0:g0 + per]
            _upload_frames(ctx, dev_c, g)
            if not shared:
                _upload_frames(ctx, dev_b, bases[g0:g0 + per])
            call(ctx, dev_b.ptr, 1 if shared else len(g), dev_c.ptr, len(g), *[d.ptr for d in dev_o])
            groups.append([d.to_host(dtype, (len(g),) + shape) for d, (dtype, shape) in zip(dev_o, outputs)])
    return groups


def quality(base, copies, ctx: Optional[Context] = None) -> list:
    """One `Quality` per copy.  base: the original, 8-bit [H, W, 3] -- or one original per copy (a list, or [n, H, W, 3]);
    copies: 8-bit images of that size.  One ssw_quality_rgb8 call per group of at most 256 MiB of frames."""
    cp = _frames_u8(copies, "quality")
    if not cp:
        return []
    h, w = cp[0].shape[:2]

    def call(ctx, dev_b, n_base, dev_c, n, dev_stats):
        check(ctx._lib.ssw_quality_rgb8(ctx.handle, dev_b, n_base, dev_c, n, w, h, dev_stats), "ssw_quality_rgb8")
    groups = _copies_against_originals(base, cp, "quality", ctx, [(np.uint64, (L.QUALITY_STATS,))], call)
    return [q for stats, in groups for q in _qualities(stats, w * h)]


@dataclass
class Ssim:
    """The structural similarity of one copy and its original (ssw_ssim_rgb8; include/ssw.h states the definition): the sum of
    the windows' fixed-point values (2^30 = identical), the worst window's value and index (wy * windows_x + wx; the first of
    equal ones) -- integers; the derived figures are the caller's arithmetic and are made here.  map: int32
    [windows_y, windows_x], the value of every window, when it was asked for."""
    sum: int
    worst: int
    worst_index: int
    windows_x: int
    windows_y: int
    map: Optional[np.ndarray] = None

    @property
    def mean(self) -> float:
        return self.sum / (L.SSIM_ONE * self.windows_x * self.windows_y)

    @property
    def worst_value(self) -> float:
        return self.worst / L.SSIM_ONE

    @property
    def worst_position(self) -> Tuple[int, int]:
        """pixel (x, y) of the worst window's upper left corner; the window is 8 x 8"""
        return 4 * (self.worst_index % self.windows_x), 4 * (self.worst_index // self.windows_x)


def _ssim_windows(w: int, h: int) -> Tuple[int, int]:
    return w // 4 - 1, h // 4 - 1


def _ssims(stats: np.ndarray, nx: int, ny: int, maps=None) -> list:
    """stats: u64 [n, 2] as ssw_ssim_rgb8 writes them"""
    stats = np.ascontiguousarray(stats, np.uint64)
    return [Ssim(int(s), (int(key) >> 32) - L.SSIM_ONE, int(key) & 0xFFFFFFFF, nx, ny, None if maps is None else maps[i])
            for i, (s, key) in enumerate(zip(stats.view(np.int64)[:, 0], stats[:, 1]))]


def ssim(base, copies, ctx: Optional[Context] = None, maps: bool = False) -> list:
    """One `Ssim` per copy.  base: the original, 8-bit [H, W, 3] -- or one original per copy (a list, or [n, H, W, 3]);
    copies: 8-bit images of that size, no side below 8.  maps: also the value of every window, as `Ssim.map`.  One
    ssw_ssim_rgb8 call per group of at most 256 MiB of frames."""
    cp = _frames_of_side(copies, "ssim", "SSIM", L.SSIM_MIN_SIDE)
    if not cp:
        return []
    h, w = cp[0].shape[:2]
    nx, ny = _ssim_windows(w, h)
    outputs = [(np.uint64, (L.SSIM_STATS,))] + ([(np.int32, (ny, nx))] if maps else [])       # the map: one more output per copy

    def call(ctx, dev_b, n_base, dev_c, n, dev_stats, dev_map=None):
        check(ctx._lib.ssw_ssim_rgb8(ctx.handle, dev_b, n_base, dev_c, n, w, h, dev_stats, dev_map), "ssw_ssim_rgb8")
    groups = _copies_against_originals(base, cp, "ssim", ctx, outputs, call)
    return [s for got in groups for s in _ssims(got[0], nx, ny, *got[1:])]


def _coalition(method, members, n_copies: int) -> L.Coalition:
    m = L.COLLUDE_METHODS.get(method.lower()) if isinstance(method, str) else int(method)
    if m is None or m not in L.COLLUDE_METHODS.values():
        raise ValueError(f"collude: unknown method {method!r} (one of {', '.join(L.COLLUDE_METHODS)})")
    members = [int(i) for i in members]
    if not 1 <= len(members) <= L.COLLUDE_MAX_MEMBERS or any(not 0 <= i < n_copies for i in members):
        raise ValueError(f"collude: 1 .. {L.COLLUDE_MAX_MEMBERS} members, each the index of a copy")
    return L.Coalition(m, len(members), (C.c_uint32 * L.COLLUDE_MAX_MEMBERS)(*members))


def _job_groups(job_frames, fb: int) -> list:
    """How jobs that read frames of `fb` bytes and write one each share the device: job_frames[j] are the frames job j reads.
    Returns the groups (used frames in first-use order, g0, g1) of consecutive jobs g0 .. g1 - 1.  A group always takes its
    first job; a further job joins while (frames used + its new frames + jobs + 1) * fb <= UPLOAD_GROUP_BYTES."""
    groups, g0 = [], 0
    while g0 < len(job_frames):
        used, g1 = {}, g0                                    # a dict as an ordered set
        while g1 < len(job_frames):
            more = [i for i in dict.fromkeys(job_frames[g1]) if i not in used]
            if g1 > g0 and (len(used) + len(more) + g1 - g0 + 1) * fb > UPLOAD_GROUP_BYTES:
                break
            used.update(dict.fromkeys(more))
            g1 += 1
        groups.append((list(used), g0, g1))
        g0 = g1
    return groups


def _run_jobs(ctx: Optional[Context], frames, job_frames, name: str, struct, local, base=None) -> list:
    """The runner of `collude`, `jpeg` and `filter`: the library call `name` (frames in, an array of `struct` jobs, one frame out
    per job) over the groups of `_job_groups`.  local(j, where): job j as a `struct` that names frame i as where[i], its place
    among the frames its group sent up.  base: the original, for a call that takes it in front of the frames (the rotation
    attack).  Returns one u8 [H, W, 3] frame per job, in order."""
    ctx = ctx or default_context()
    h, w = frames[0].shape[:2]
    fb, out = w * h * 3, []
    for used, g0, g1 in _job_groups(job_frames, fb):
        where = {i: j for j, i in enumerate(used)}
        jobs = (struct * (g1 - g0))(*[local(j, where) for j in range(g0, g1)])
        with _owned(ctx) as alloc:
            dev_f, dev_o = alloc(len(used) * fb), alloc((g1 - g0) * fb)
            _upload_frames(ctx, dev_f, [frames[i] for i in used])
            lead = () if base is None else (_upload_frames(ctx, alloc(fb), [base]).ptr,)
            check(getattr(ctx._lib, name)(ctx.handle, *lead, dev_f.ptr, len(used), w, h, jobs, g1 - g0, dev_o.ptr), name)
            out += list(dev_o.to_host(np.uint8, (g1 - g0, h, w, 3)))
    return out


def collude(copies, coalitions, ctx: Optional[Context] = None) -> list:
    """Forged copies out of several (ssw_collude_rgb8; include/ssw.h states the six definitions).  copies: 8-bit [H, W, 3]
    images of one size; coalitions: (method, members) pairs -- method "average", "median", "min", "max", "minmax" or "mosaic"
    (or the constant), members 1 .. 16 indices into `copies`, repeats allowed.  Returns one u8 [H, W, 3] frame per coalition,
    in order.  The coalitions go in groups whose members and results are at most 256 MiB on the device."""
    cp = _frames_u8(copies, "collude")
    co = [_coalition(m, mem, len(cp)) for m, mem in coalitions]
    if not co:
        return []
    members = [c.member[:c.count] for c in co]
    return _run_jobs(ctx, cp, members, "ssw_collude_rgb8", L.Coalition, lambda j, where: L.Coalition(
        co[j].method, co[j].count, (C.c_uint32 * L.COLLUDE_MAX_MEMBERS)(*[where[i] for i in members[j]])))


# An attack on single frames: the library call, its job struct and how a job is made of (frame, parameter) -- what `jpeg`,
# `filter` and the attack stage of `strength_report` need to know of it; a fourth entry, True: the call takes the original in
# front of the frames
_JPEG_ATTACK = ("ssw_jpeg_rgb8", L.JpegJob, L.JpegJob)
_FILTER_ATTACK = ("ssw_filter_rgb8", L.FilterJob, lambda frame, f: f.job(frame))


def _attack_every(ctx: Optional[Context], frames, params, attack, base=None) -> list:
    """Every frame under every parameter of `attack`, jobs in frame order: [len(frames)][len(params)] u8 [H, W, 3] frames."""
    name, struct, job = attack[:3]
    jobs = [(i, p) for i in range(len(frames)) for p in params]
    flat = _run_jobs(ctx, frames, [(i,) for i, _ in jobs], name, struct, lambda j, where: job(where[jobs[j][0]], jobs[j][1]), base)
    return [flat[i * len(params):(i + 1) * len(params)] for i in range(len(frames))]


def _jpeg_qualities(qualities, what: str) -> list:
    qs = list(qualities)
    if any(isinstance(q, bool) or not isinstance(q, (int, np.integer)) or not 1 <= q <= 100 for q in qs):
        raise ValueError(f"{what}: JPEG qualities are integers 1 .. 100")
    return [int(q) for q in qs]


def jpeg(images, qualities, ctx: Optional[Context] = None) -> list:
    """Every image as it comes back from a baseline JPEG of every quality (ssw_jpeg_rgb8; include/ssw.h states the steps): what
    PIL's save(f, "JPEG", quality=q) and open give, byte for byte, without a bitstream.  images: 8-bit [H, W, 3] of one size, no
    side below 8; qualities: integers 1 .. 100.  Returns [len(images)][len(qualities)] u8 [H, W, 3] frames.  The jobs go in
    groups whose frames and results are at most 256 MiB on the device."""
    frames, qs = _frames_of_side(images, "jpeg", "a JPEG attack", L.JPEG_MIN_SIDE), _jpeg_qualities(qualities, "jpeg")
    if not frames or not qs:
        return [[] for _ in frames]
    return _attack_every(ctx, frames, qs, _JPEG_ATTACK)


@dataclass(frozen=True)
class Filter:
    """One attack of ssw_filter_rgb8 (include/ssw.h states the definitions; they are Pillow's): make it with `Filter.blur`,
    `Filter.unsharp` or `Filter.median`.  `label` names it in reports: "blur 1.5", "unsharp 2,150,3", "median 3"."""
    kind: int
    radius: float = 0.0
    percent: int = 0
    threshold: int = 0

    @staticmethod
    def _radius(radius) -> float:
        if isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)):
            raise ValueError("Filter: the radius is a number")
        r = float(np.float32(radius)) if math.isfinite(radius) else math.nan
        if not 0.0 < r <= L.FILTER_RADIUS_MAX:                   # NaN fails too
            raise ValueError(f"Filter: a radius above 0 and at most {L.FILTER_RADIUS_MAX:g}")
        return r

    @classmethod
    def blur(cls, radius) -> "Filter":
        """ImageFilter.GaussianBlur(radius): radius is the Gaussian's sigma, 0 < radius <= 8"""
        return cls(L.FILTER_BLUR, cls._radius(radius))

    @classmethod
    def unsharp(cls, radius=2, percent=150, threshold=3) -> "Filter":
        """ImageFilter.UnsharpMask(radius, percent, threshold): percent 1 .. 1000, threshold 0 .. 255"""
        for v, lo, hi, what in ((percent, 1, 1000, "percent"), (threshold, 0, 255, "threshold")):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
                raise ValueError(f"Filter: an unsharp mask's {what} is an integer {lo} .. {hi}")
        return cls(L.FILTER_UNSHARP, cls._radius(radius), int(percent), int(threshold))

    @classmethod
    def median(cls) -> "Filter":
        """ImageFilter.MedianFilter(3)"""
        return cls(L.FILTER_MEDIAN3)

    @property
    def label(self) -> str:
        if self.kind == L.FILTER_BLUR:
            return f"blur {self.radius:g}"
        if self.kind == L.FILTER_UNSHARP:
            return f"unsharp {self.radius:g},{self.percent},{self.threshold}"
        return "median 3"

    def job(self, frame: int) -> L.FilterJob:
        return L.FilterJob(frame, self.kind, self.radius, self.percent, self.threshold)


def _filters(filters, what: str) -> list:
    fs = list(filters)
    if any(not isinstance(f, Filter) for f in fs):
        raise ValueError(f"{what}: filters are made with Filter.blur, Filter.unsharp or Filter.median")
    return fs


def filter(images, filters, ctx: Optional[Context] = None) -> list:
    """Every image under every filter (ssw_filter_rgb8; include/ssw.h states the definitions): what Pillow's GaussianBlur,
    UnsharpMask and MedianFilter(3) give, byte for byte.  images: 8-bit [H, W, 3] of one size, any size; filters: `Filter`
    objects.  Returns [len(images)][len(filters)] u8 [H, W, 3] frames.  The jobs go in groups whose frames and results are at
    most 256 MiB on the device."""
    frames, fs = _frames_u8(images, "filter"), _filters(filters, "filter")
    if not frames or not fs:
        return [[] for _ in frames]
    return _attack_every(ctx, frames, fs, _FILTER_ATTACK)


def _resample_filter(filter) -> int:
    f = L.RESAMPLE_FILTERS.get(filter.lower()) if isinstance(filter, str) else None
    if f is None:
        raise ValueError(f"unknown resample filter {filter!r} (one of {', '.join(L.RESAMPLE_FILTERS)})")
    return f


def _side(v, what: str) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= L.RESAMPLE_SIDE_MAX:
        raise ValueError(f"{what}: a side is an integer 1 .. {L.RESAMPLE_SIDE_MAX}")
    return int(v)


def resample(images, size, filter="bicubic", ctx: Optional[Context] = None) -> list:
    """Every image as PIL.Image.resize(size, filter) makes it, byte for byte (ssw_resample_rgb8; include/ssw.h states the
    definition).  images: 8-bit [H, W, 3] of one size; size: (nw, nh), sides 1 .. 65535; filter: "box", "bilinear", "bicubic" or
    "lanczos".  Returns one u8 [nh, nw, 3] frame per image.  The frames go in groups whose inputs and results are at most
    256 MiB on the device."""
    frames, f = _frames_u8(images, "resample"), _resample_filter(filter)
    nw, nh = (_side(v, "resample") for v in size)
    if not frames:
        return []
    ctx = ctx or default_context()
    h, w = frames[0].shape[:2]
    fb, ob, n, out = w * h * 3, nw * nh * 3, len(frames), []
    per = max(1, UPLOAD_GROUP_BYTES // (fb + ob))
    with _owned(ctx) as alloc:
        dev_i, dev_o = alloc(min(per, n) * fb), alloc(min(per, n) * ob)
        for g0 in range(0, n, per):
            g = frames[g0:g0 + per]
            _upload_frames(ctx, dev_i, g)
            check(ctx._lib.ssw_resample_rgb8(ctx.handle, dev_i.ptr, len(g), w, h, nw, nh, f, dev_o.ptr), "ssw_resample_rgb8")
            out += list(dev_o.to_host(np.uint8, (len(g), nh, nw, 3)))
    return out


@dataclass(frozen=True)
class Scale:
    """One attack of ssw_scale_attack_rgb8: the copy as PIL.Image.resize makes its thumbnail, brought back to the original's
    size as `trace` brings back a suspect of another size.  `Scale(factor, filter)`: the thumbnail has `size(w, h)`, sides
    rounded half up, 0 < factor <= 4; `Scale.to(nw, nh, filter)`: a thumbnail of that size whatever the frame's.  filter: "box",
    "bilinear", "bicubic" (the default) or "lanczos".  `label` names it in reports: "scale 0.5 bicubic", "scale 640x360 lanczos"."""
    factor: float = 0.0
    filter: str = "bicubic"
    nw: int = 0
    nh: int = 0

    def __post_init__(self):
        _resample_filter(self.filter)
        object.__setattr__(self, "filter", self.filter.lower())
        if self.nw or self.nh:
            if self.factor:
                raise ValueError("Scale: a factor or a size, not both")
            object.__setattr__(self, "nw", _side(self.nw, "Scale"))
            object.__setattr__(self, "nh", _side(self.nh, "Scale"))
            return
        f = self.factor
        if isinstance(f, bool) or not isinstance(f, (int, float, np.integer, np.floating)):
            raise ValueError("Scale: the factor is a number")
        if not (math.isfinite(f) and 0.0 < f <= L.SCALE_FACTOR_MAX):
            raise ValueError(f"Scale: a factor above 0 and at most {L.SCALE_FACTOR_MAX:g}")
        object.__setattr__(self, "factor", float(f))

    @classmethod
    def to(cls, nw, nh, filter="bicubic") -> "Scale":
        return cls(0.0, filter, _side(nw, "Scale"), _side(nh, "Scale"))

    def size(self, w: int, h: int) -> Tuple[int, int]:
        if self.nw:
            return self.nw, self.nh
        return max(1, int(w * self.factor + 0.5)), max(1, int(h * self.factor + 0.5))

    @property
    def label(self) -> str:
        return f"scale {self.nw}x{self.nh} {self.filter}" if self.nw else f"scale {self.factor:g} {self.filter}"

    def job(self, frame: int, w: int, h: int) -> L.ScaleJob:
        nw, nh = self.size(w, h)
        return L.ScaleJob(frame, nw, nh, L.RESAMPLE_FILTERS[self.filter])


def _scales(scales, what: str) -> list:
    sc = list(scales)
    if any(not isinstance(s, Scale) for s in sc):
        raise ValueError(f"{what}: scales are made with Scale(factor, filter) or Scale.to(nw, nh, filter)")
    return sc


def _scale_attack(w: int, h: int) -> tuple:
    """The attack of `_attack_every` and of the report's stage for frames of w x h: a scale job needs the frame's size"""
    return ("ssw_scale_attack_rgb8", L.ScaleJob, lambda frame, s: s.job(frame, w, h))


def scale_attack(images, scales, ctx: Optional[Context] = None) -> list:
    """Every image after every scale attack (ssw_scale_attack_rgb8): shrunk or enlarged as Pillow does it, then brought back to
    its size as `trace` would.  images: 8-bit [H, W, 3] of one size; scales: `Scale` objects.  Returns
    [len(images)][len(scales)] u8 [H, W, 3] frames.  The jobs go in groups whose frames and results are at most 256 MiB on the
    device."""
    frames, sc = _frames_u8(images, "scale_attack"), _scales(scales, "scale_attack")
    if not frames or not sc:
        return [[] for _ in frames]
    h, w = frames[0].shape[:2]
    if any(max(s.size(w, h)) > L.RESAMPLE_SIDE_MAX for s in sc):
        raise ValueError(f"scale_attack: a thumbnail's side is at most {L.RESAMPLE_SIDE_MAX}")
    return _attack_every(ctx, frames, sc, _scale_attack(w, h))


# ---- the rotation attack and its undoing (include/ssw.h: ssw_affine_rgb8, ssw_rotate_attack_rgb8, ssw_unrotate_rgb8) ---------
def _affine_filter(filter) -> int:
    f = L.AFFINE_FILTERS.get(filter.lower()) if isinstance(filter, str) else None
    if f is None:
        raise ValueError(f"unknown affine filter {filter!r} (one of {', '.join(L.AFFINE_FILTERS)})")
    return f


def _fill(fill, what: str) -> tuple:
    f = tuple(fill)
    if len(f) != 3 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= 255 for v in f):
        raise ValueError(f"{what}: the fill is three integers 0 .. 255")
    return tuple(int(v) for v in f)


def _angle(angle, what: str) -> float:
    if isinstance(angle, bool) or not isinstance(angle, (int, float, np.integer, np.floating)) or not math.isfinite(angle):
        raise ValueError(f"{what}: the angle is a finite number of degrees")
    return float(angle)


def rotation_matrix(angle: float, w: int, h: int) -> list:
    """The matrix PIL.Image.rotate(angle) hands to Image.transform for a w x h frame (expand=False, the default centre), number
    for number (include/ssw.h states it; csrc/affine_tables.hpp makes the same in C++)."""
    a = -math.radians(angle % 360.0)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = w / 2.0, h / 2.0
    m[2] = (m[0] * -cx + m[1] * -cy + 0.0) + cx
    m[5] = (m[3] * -cx + m[4] * -cy + 0.0) + cy
    return m


def affine(images, size, matrix, filter="bicubic", fill=(0, 0, 0), ctx: Optional[Context] = None) -> list:
    """Every image as PIL.Image.transform(size, AFFINE, matrix, filter, fillcolor=fill) makes it, byte for byte (ssw_affine_rgb8;
    include/ssw.h states the definition).  images: 8-bit [H, W, 3] of one size; size: (ow, oh), sides 1 .. 65535; matrix: six
    finite numbers; filter: "bilinear" or "bicubic".  Returns one u8 [oh, ow, 3] frame per image.  The frames go in groups whose
    inputs and results are at most 256 MiB on the device."""
    frames, f, fl = _frames_u8(images, "affine"), _affine_filter(filter), _fill(fill, "affine")
    ow, oh = (_side(v, "affine") for v in size)
    m = [float(v) for v in matrix]
    if len(m) != 6 or not all(math.isfinite(v) for v in m):
        raise ValueError("affine: the matrix is six finite numbers")
    if not frames:
        return []
    ctx = ctx or default_context()
    h, w = frames[0].shape[:2]
    fb, ob, n, out = w * h * 3, ow * oh * 3, len(frames), []
    per = max(1, UPLOAD_GROUP_BYTES // (fb + ob))
    cm, cf = (C.c_double * 6)(*m), (C.c_uint8 * 3)(*fl)
    with _owned(ctx) as alloc:
        dev_i, dev_o = alloc(min(per, n) * fb), alloc(min(per, n) * ob)
        for g0 in range(0, n, per):
            g = frames[g0:g0 + per]
            _upload_frames(ctx, dev_i, g)
            check(ctx._lib.ssw_affine_rgb8(ctx.handle, dev_i.ptr, len(g), w, h, ow, oh, cm, f, cf, dev_o.ptr), "ssw_affine_rgb8")
            out += list(dev_o.to_host(np.uint8, (len(g), oh, ow, 3)))
    return out


def rotate(images, angle, filter="bicubic", fill=(0, 0, 0), ctx: Optional[Context] = None) -> list:
    """Every image as PIL.Image.rotate(angle, filter, fillcolor=fill) makes it, byte for byte: `affine` with `rotation_matrix`."""
    frames = _frames_u8(images, "rotate")
    if not frames:
        return []
    h, w = frames[0].shape[:2]
    return affine(frames, (w, h), rotation_matrix(_angle(angle, "rotate"), w, h), filter, fill, ctx)


@dataclass(frozen=True)
class Rotate:
    """One attack of ssw_rotate_attack_rgb8: the copy as PIL.Image.rotate(angle, filter) makes it, turned back by the known
    angle and completed with the original as `trace` does it for a `Rotated(angle)` suspect.  angle: degrees counter-clockwise,
    as Pillow's; filter: "bilinear" or "bicubic" (the default).  `label` names it in reports: "rotate 0.5 bicubic".
    search: None (the default), or the range (lo, hi) of degrees within +-45 in which the tracer, who is NOT told the angle,
    searches for it (True: -10 .. 10) -- the copy is then turned back by the angle found (ssw_rotate_search_attack_rgb8;
    `strength_report` and `rotate_search_attack` read it, `job` does not); the label gains ", angle searched in -10..10"."""
    angle: float
    filter: str = "bicubic"
    search: Optional[Tuple[float, float]] = None

    def __post_init__(self):
        _affine_filter(self.filter)
        object.__setattr__(self, "filter", self.filter.lower())
        object.__setattr__(self, "angle", _angle(self.angle, "Rotate"))
        if self.search is not None:
            object.__setattr__(self, "search", _search(DEFAULT_ANGLE_SEARCH if self.search is True else self.search, "Rotate"))

    @property
    def label(self) -> str:
        searched = "" if self.search is None else f", angle searched in {self.search[0]:g}..{self.search[1]:g}"
        return f"rotate {self.angle:g} {self.filter}{searched}"

    def job(self, frame: int, w: int, h: int, fill=(0, 0, 0)) -> L.RotateJob:
        return L.RotateJob(frame, L.AFFINE_FILTERS[self.filter], (C.c_uint8 * 4)(*fill, 0), (C.c_double * 6)(*rotation_matrix(self.angle, w, h)),
                           (C.c_double * 6)(*rotation_matrix(-self.angle, w, h)))

    def kept(self, w: int, h: int) -> float:
        """The share of a w x h frame's pixels that the undoing takes from the rotated copy (the mask of include/ssw.h); the
        others are the original's.  Host arithmetic on the frame's geometry, a band of rows at a time."""
        F, B = rotation_matrix(self.angle, w, h), rotation_matrix(-self.angle, w, h)
        if F == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0] and B == F:
            return 1.0

        def point(m, X, Y):
            return m[0] * (X + 0.5) + m[1] * (Y + 0.5) + m[2], m[3] * (X + 0.5) + m[4] * (Y + 0.5) + m[5]

        def inside(x, y):
            return (x >= 0.0) & (x < w) & (y >= 0.0) & (y < h)

        count, X = 0, np.arange(w, dtype=np.float64)[None, :]
        for y0 in range(0, h, 256):
            Y = np.arange(y0, min(y0 + 256, h), dtype=np.float64)[:, None]
            xin, yin = point(B, X, Y)
            x, y = np.floor(xin - 0.5), np.floor(yin - 0.5)
            keep = inside(xin, yin) & (x - 1 >= 0) & (x + 2 <= w - 1) & (y - 1 >= 0) & (y + 2 <= h - 1)
            for cx in (x - 1, x + 2):
                for cy in (y - 1, y + 2):
                    keep &= inside(*point(F, cx, cy))
            count += int(keep.sum())
        return count / (w * h)


DEFAULT_ANGLE_SEARCH = (-10.0, 10.0)


def _search(search, what: str) -> Tuple[float, float]:
    """A range of angles (lo, hi) in degrees as ssw_find_angle_rgb8 takes it: finite, lo <= hi, within +-45."""
    try:
        lo, hi = search
        lo, hi = _angle(lo, what), _angle(hi, what)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: search=(lo, hi), two finite numbers of degrees") from None
    if not -45.0 <= lo <= hi <= 45.0:
        raise ValueError(f"{what}: search=(lo, hi) with -45 <= lo <= hi <= 45")
    return lo, hi


@dataclass(frozen=True)
class Rotated:
    """A placement entry that says "this suspect is the original's frame turned" (counter-clockwise, as PIL.Image.rotate does
    it): it is turned back on the device (ssw_unrotate_rgb8) and traced as a whole frame.  The suspect has the original's size
    and 3 channels.  `Rotated(angle)`: turned by `angle` degrees.  `Rotated()` or `Rotated(search=(lo, hi))`: the angle is not
    known and is searched for in the range first, among all such entries of a call at once (`find_angle`)."""
    angle: Optional[float] = None
    search: Tuple[float, float] = DEFAULT_ANGLE_SEARCH

    def __post_init__(self):
        if self.angle is not None:
            object.__setattr__(self, "angle", _angle(self.angle, "Rotated"))
        object.__setattr__(self, "search", _search(self.search, "Rotated"))


@dataclass
class FoundAngle:
    """By which angle a suspect was turned (ssw_find_angle_rgb8): `angle` = n / 32 degrees, counter-clockwise as
    PIL.Image.rotate's; `sad` the sum of absolute luma differences between the original turned by it and the suspect over the
    `count` pixels the turn keeps well inside the frame; `mean` = sad / count -- a few units for a true match of a marked copy."""
    angle: float
    n: int
    sad: int
    count: int
    mean: float


def find_angle(base, suspects, search=DEFAULT_ANGLE_SEARCH, ctx: Optional[Context] = None, rungs: bool = False):
    """By which angle was each suspect turned?  A search over the angle of a rotation about the centre on the device
    (ssw_find_angle_rgb8): integer luma differences between the original turned forward and the suspect, a ladder of angles 0.25
    degrees apart on 4 x 4 box means, the 4 best rungs refined in steps of 1/32 degree at full resolution -- exactly reproducible,
    see include/ssw.h for the definition.  base: the original, 8-bit [H, W, 3], both sides at least 32; suspects: 8-bit [H, W, 3]
    of that size; search: (lo, hi) in degrees, within +-45.  Returns one `FoundAngle` per suspect; with rungs=True also the
    ladder's sums, uint64 [n][rungs][2] = D, c.  A copy that was turned and cropped is `locate_turned`'s; one that was turned and
    scaled is not found."""
    lo, hi = _search(search, "find_angle")
    b = _frames_u8([base], "find_angle")[0]
    frames = _frames_u8(suspects, "find_angle")
    if frames and frames[0].shape != b.shape:
        raise ValueError("find_angle: a turned suspect has the original's size and 3 channels")
    h, w = b.shape[:2]
    if min(w, h) < L.ANGLE_MIN_SIDE or w * h > L.ANGLE_MAX_PIXELS:
        raise ValueError(f"find_angle: frames of at least {L.ANGLE_MIN_SIDE} x {L.ANGLE_MIN_SIDE} and at most 2^27 pixels")
    n_rungs = min(180, math.ceil(4.0 * hi)) - max(-180, math.floor(4.0 * lo)) + 1
    found, sums = [], np.zeros((len(frames), n_rungs, 2), np.uint64)
    if not frames:
        return (found, sums) if rungs else found
    ctx = ctx or default_context()
    fb, n = w * h * 3, len(frames)
    per = max(1, UPLOAD_GROUP_BYTES // fb)
    with _owned(ctx) as alloc:
        dev_b, dev_s = _upload_frames(ctx, alloc(fb), [b]), alloc(min(per, n) * fb)
        for g0 in range(0, n, per):
            g = frames[g0:g0 + per]
            _upload_frames(ctx, dev_s, g)
            got = (L.AngleFound * len(g))()
            part = np.zeros((len(g), n_rungs, 2), np.uint64)
            check(ctx._lib.ssw_find_angle_rgb8(ctx.handle, dev_b.ptr, dev_s.ptr, len(g), w, h, lo, hi, got, part.ctypes.data), "ssw_find_angle_rgb8")
            sums[g0:g0 + len(g)] = part
            found += [FoundAngle(int(f.n) / L.ANGLE_PER_DEGREE, int(f.n), int(f.sad), int(f.count), int(f.sad) / max(1, int(f.count))) for f in got]
    return (found, sums) if rungs else found


@dataclass
class LocatedTurned:
    """Where a cut-out of a turned copy lies and by which angle it was turned (ssw_locate_turned_rgb8): `angle` = n / 32 degrees,
    counter-clockwise as PIL.Image.rotate's; `centre`, the (x, y) of the suspect's centre in pixels of the original (a multiple
    of one half); `template`, the (w, h) of the turned-back part of the suspect that was compared; `sad`, the sum of absolute luma
    differences there; `mean_abs_diff` = sad / (w h of the template) -- a few units for a true match of a marked copy."""
    angle: float
    n: int
    centre: Tuple[float, float]
    template: Tuple[int, int]
    sad: int
    mean_abs_diff: float


def locate_turned(base, suspects, search=DEFAULT_ANGLE_SEARCH, ctx: Optional[Context] = None, rungs: bool = False):
    """Where does each suspect lie, and by which angle was it turned?  For cut-outs of a turned copy -- what "straighten" in a
    photo editor leaves: the frame turned, the wedges cropped away --, a search over angle and position together on the device
    (ssw_locate_turned_rgb8): per angle of a ladder 0.25 degrees apart the suspect is turned back about its own centre and its
    8 x 8 box means searched for in the original's, the 4 best rungs are refined in steps of 1/32 degree at full resolution --
    exactly reproducible, see include/ssw.h for the definition.  base: the original, 8-bit [H, W, 3]; suspects: 8-bit [h, w, 3]
    of any sizes, at the original's scale and without the attacker's fill; search: (lo, hi) in degrees, within +-45.  Returns
    one `LocatedTurned` per suspect; with rungs=True also the ladder's entries, uint64 [n][rungs][4] = D, n_j, x, y (a dropped
    rung: zeros).  A cut-out that was scaled as well is not found."""
    lo, hi = _search(search, "locate_turned")
    b = _base_rgb8(base)
    H, W = b.shape[:2]
    arrs = [np.ascontiguousarray(np.asarray(im)) for im in suspects]
    for a in arrs:
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or 0 in a.shape:
            raise ValueError("locate_turned: suspects are 8-bit [h, w, 3] arrays (RGBA is not supported)")
    n = len(arrs)
    n_rungs = min(180, math.ceil(4.0 * hi)) - max(-180, math.floor(4.0 * lo)) + 1
    entries = np.zeros((n, n_rungs, 4), np.uint64)
    if not arrs:
        return ([], entries) if rungs else []
    ctx = ctx or default_context()
    with _owned(ctx) as alloc:
        dev_b = _upload_frames(ctx, alloc(b.nbytes), [b])
        dev = [_upload_frames(ctx, alloc(a.nbytes), [a]) for a in arrs]
        ptrs = (C.c_void_p * n)(*[d.ptr.value for d in dev])
        shapes = (L.TurnedShape * n)(*[L.TurnedShape(a.shape[1], a.shape[0], 3) for a in arrs])
        got = (L.TurnedFound * n)()
        check(ctx._lib.ssw_locate_turned_rgb8(ctx.handle, dev_b.ptr, W, H, ptrs, shapes, n, lo, hi, got, entries.ctypes.data), "ssw_locate_turned_rgb8")
    found = [LocatedTurned(int(f.n) / L.ANGLE_PER_DEGREE, int(f.n), (int(f.x) + int(f.tw) / 2.0, int(f.y) + int(f.th) / 2.0), (int(f.tw), int(f.th)),
                           int(f.sad), int(f.sad) / (int(f.tw) * int(f.th))) for f in got]
    return (found, entries) if rungs else found


def restore_turned(base, suspects, found, ctx: Optional[Context] = None) -> list:
    """Cut-outs of a turned copy laid back into the original's frame (ssw_restore_turned_rgb8): what tracing a
    `Locate(turned=...)` entry extracts from.  found: per suspect a `LocatedTurned`, or an (angle, cx, cy) triple -- turned by
    `angle` degrees counter-clockwise, its centre at (cx, cy) pixels of the original.  The suspect is turned back and moved with
    Pillow's BICUBIC affine transform, exactly; where its footprint would need clamping, and outside it, the original's pixel
    stands.  Returns one u8 [H, W, 3] frame per suspect."""
    b = _base_rgb8(base)
    H, W = b.shape[:2]
    arrs = [np.ascontiguousarray(np.asarray(im)) for im in suspects]
    for a in arrs:
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or 0 in a.shape:
            raise ValueError("restore_turned: suspects are 8-bit [h, w, 3] arrays (RGBA is not supported)")
    found = list(found)
    if len(found) != len(arrs):
        raise ValueError("restore_turned: one LocatedTurned or (angle, cx, cy) per suspect")
    triples = [(f.angle, f.centre[0], f.centre[1]) if isinstance(f, LocatedTurned) else tuple(float(v) for v in f) for f in found]
    if any(len(t) != 3 or not all(math.isfinite(v) for v in t) for t in triples):
        raise ValueError("restore_turned: (angle, cx, cy), three finite numbers")
    if not arrs:
        return []
    ctx = ctx or default_context()
    n, fb = len(arrs), W * H * 3
    with _owned(ctx) as alloc:
        dev_b, dev_o = _upload_frames(ctx, alloc(fb), [b]), alloc(n * fb)
        dev = [_upload_frames(ctx, alloc(a.nbytes), [a]) for a in arrs]
        ptrs = (C.c_void_p * n)(*[d.ptr.value for d in dev])
        shapes = (L.TurnedShape * n)(*[L.TurnedShape(a.shape[1], a.shape[0], 3) for a in arrs])
        jobs = (L.TurnedJob * n)(*[L.TurnedJob(*t) for t in triples])
        check(ctx._lib.ssw_restore_turned_rgb8(ctx.handle, dev_b.ptr, W, H, ptrs, shapes, jobs, n, dev_o.ptr), "ssw_restore_turned_rgb8")
        return list(dev_o.to_host(np.uint8, (n, H, W, 3)))


def _undo_turned_cuts(base, suspects, placements, ctx, locate_fn=None, restore_fn=None):
    """placements with `Locate(turned=...)` entries -> (suspects, placements, {index: LocatedTurned}) with every such suspect laid
    back into the frame and its entry None: a whole frame of the original's size.  One `locate_turned` call per distinct range,
    one `restore_turned` call.  The other entries pass through untouched."""
    placements, suspects = list(placements), list(suspects)
    if len(placements) != len(suspects):
        raise ValueError("placements: one entry (a Placement, a Locate, a Rotated or None) per suspect")
    ranges = {i: p.turned_range() for i, p in enumerate(placements) if isinstance(p, Locate)}
    todo = [i for i, r in ranges.items() if r is not None]
    if not todo:
        return suspects, placements, {}
    if base is None:
        raise ValueError("Locate(turned=) entries need the original's pixels (base=)")
    b = _base_rgb8(base)
    found = {}
    for search in sorted({ranges[i] for i in todo}):
        idx = [i for i in todo if ranges[i] == search]
        found.update(zip(idx, (locate_fn or locate_turned)(b, [suspects[i] for i in idx], search, ctx)))
    for i, f in zip(todo, (restore_fn or restore_turned)(b, [suspects[i] for i in todo], [found[i] for i in todo], ctx)):
        suspects[i], placements[i] = f, None
    return suspects, placements, found


def _rotations(rotations, what: str) -> list:
    ro = list(rotations)
    if any(not isinstance(r, Rotate) for r in ro):
        raise ValueError(f"{what}: rotations are made with Rotate(angle, filter)")
    return ro


def _kept_shares(ctx: Context, rotations, w: int, h: int) -> list:
    """`Rotate.kept` of every rotation for a w x h frame, counted on the device (ssw_unrotate_kept): the same numbers"""
    if not rotations:
        return []
    jobs, counts = (L.RotateJob * len(rotations))(*[r.job(0, w, h) for r in rotations]), np.zeros(len(rotations), np.uint64)
    check(ctx._lib.ssw_unrotate_kept(ctx.handle, w, h, jobs, len(rotations), counts.ctypes.data), "ssw_unrotate_kept")
    return [int(c) / (w * h) for c in counts]


def _rotate_attack(w: int, h: int) -> tuple:
    """The attack of `_attack_every` and of the report's stage for frames of w x h: a rotation's matrices need the frame's size"""
    return ("ssw_rotate_attack_rgb8", L.RotateJob, lambda frame, r: r.job(frame, w, h), True)


def rotate_attack(base, images, rotations, ctx: Optional[Context] = None) -> list:
    """Every image after every rotation attack (ssw_rotate_attack_rgb8): turned as Pillow does it, then turned back and
    completed with `base`, the original, as `trace` would.  base: 8-bit [H, W, 3]; images: 8-bit [H, W, 3] of that size;
    rotations: `Rotate` objects.  Returns [len(images)][len(rotations)] u8 [H, W, 3] frames.  The jobs go in groups whose frames
    and results are at most 256 MiB on the device."""
    frames, ro = _frames_u8(images, "rotate_attack"), _rotations(rotations, "rotate_attack")
    if not frames or not ro:
        return [[] for _ in frames]
    b = _frames_u8([base], "rotate_attack")[0]
    if b.shape != frames[0].shape:
        raise ValueError("rotate_attack: the original has the images' size")
    h, w = b.shape[:2]
    return _attack_every(ctx, frames, ro, _rotate_attack(w, h), b)


def _found_angle(f) -> "FoundAngle":
    return FoundAngle(int(f.n) / L.ANGLE_PER_DEGREE, int(f.n), int(f.sad), int(f.count), int(f.sad) / max(1, int(f.count)))


def _search_ranges(rotations) -> list:
    """[(range, positions in `rotations`)] of the entries that carry a search, ranges in the order of their first entry"""
    ranges = {}
    for i, r in enumerate(rotations):
        if r.search is not None:
            ranges.setdefault(r.search, []).append(i)
    return list(ranges.items())


def rotate_search_attack(base, images, rotations, ctx: Optional[Context] = None) -> tuple:
    """Every image after every rotation attack when the tracer is NOT told the angle (ssw_rotate_search_attack_rgb8): turned as
    Pillow does it, the angle searched for on the device as `find_angle` does (all copies of a call at once: they share the
    original, so the original is turned once per candidate angle and compared with every copy), then turned back by the angle
    FOUND and completed with `base`.  rotations: `Rotate` objects; the range is each one's `search` (None: -10 .. 10), one library
    call per distinct range.  Returns (frames [len(images)][len(rotations)] u8 [H, W, 3], found [len(images)][len(rotations)]
    of `FoundAngle`).  Both sides at least 32."""
    frames, ro = _frames_u8(images, "rotate_search_attack"), _rotations(rotations, "rotate_search_attack")
    ro = [r if r.search is not None else Rotate(r.angle, r.filter, True) for r in ro]
    if not frames or not ro:
        return [[] for _ in frames], [[] for _ in frames]
    b = _frames_u8([base], "rotate_search_attack")[0]
    if b.shape != frames[0].shape:
        raise ValueError("rotate_search_attack: the original has the images' size")
    h, w = b.shape[:2]
    if min(w, h) < L.ANGLE_MIN_SIDE or w * h > L.ANGLE_MAX_PIXELS:
        raise ValueError(f"rotate_search_attack: frames of at least {L.ANGLE_MIN_SIDE} x {L.ANGLE_MIN_SIDE} and at most 2^27 pixels")
    ctx = ctx or default_context()
    fb = w * h * 3
    out, found = [[None] * len(ro) for _ in frames], [[None] * len(ro) for _ in frames]
    for (lo, hi), which in _search_ranges(ro):
        jobs = [(i, p) for i in range(len(frames)) for p in which]
        for used, g0, g1 in _job_groups([(i,) for i, _ in jobs], fb):
            where, n = {i: j for j, i in enumerate(used)}, g1 - g0
            arr = (L.RotateJob * n)(*[ro[p].job(where[i], w, h) for i, p in jobs[g0:g1]])
            got, kept = (L.AngleFound * n)(), np.zeros(n, np.uint64)
            with _owned(ctx) as alloc:
                dev_f, dev_o = alloc(len(used) * fb), alloc(n * fb)
                _upload_frames(ctx, dev_f, [frames[i] for i in used])
                dev_b = _upload_frames(ctx, alloc(fb), [b])
                check(ctx._lib.ssw_rotate_search_attack_rgb8(ctx.handle, dev_b.ptr, dev_f.ptr, len(used), w, h, arr, n, lo, hi, dev_o.ptr, None, got,
                                                             None, kept.ctypes.data), "ssw_rotate_search_attack_rgb8")
                for (i, p), frame, f in zip(jobs[g0:g1], dev_o.to_host(np.uint8, (n, h, w, 3)), got):
                    out[i][p], found[i][p] = frame, _found_angle(f)
    return out, found


# ---- the crop attack, placed or searched, also scaled (include/ssw.h: ssw_crop_attack_rgb8, ssw_crop_search_attack_rgb8) ------
def _ladder_height(pw: int, sw: int, sh: int) -> int:
    """ph(pw) of ssw_locate_scaled_rgb8: the height the ladder gives a piece of sw x sh at width pw"""
    return max(1, (2 * sh * pw + sw) // (2 * sw))


@dataclass(frozen=True)
class Crop:
    """One attack of ssw_crop_attack_rgb8 / ssw_crop_search_attack_rgb8: a rectangle cut out of the copy -- perhaps made a
    thumbnail as PIL.Image.resize makes it -- and laid over the original again, as the reference's crop test does it.
    `Crop(0.5)`: that fraction of both sides, cw = max(1, floor(W f + 0.5)) and ch likewise, centred: x = (W - cw) // 2,
    y = (H - ch) // 2; `anchor=(ax, ay)` in 0 .. 1 puts it elsewhere, x = floor((W - cw) ax): (0, 0) the top left corner, (0, 1)
    the bottom left.  `Crop.rect(x, y, cw, ch)`: that rectangle whatever the frame's size.  `scale=0.5` (a factor of the piece's
    sides, rounded as `Scale` rounds) or `to=(tw, th)` makes the piece a thumbnail with `filter` ("box", "bilinear", "bicubic",
    "lanczos").  search: None -- the tracer is told the rectangle; True -- it searches for it: the position of an unscaled piece
    (ssw_locate_rgb8), position and size of a thumbnail over the widths from its own up to the frame's
    (ssw_locate_scaled_rgb8); (wmin, wmax) -- over those widths.  `label` names it in reports: "crop 0.5", "crop 340,160,225x225",
    "crop 0.75 @ 0.5 lanczos"."""
    fraction: float = 0.0
    anchor: Tuple[float, float] = (0.5, 0.5)
    scale: float = 0.0
    to: Optional[Tuple[int, int]] = None
    filter: str = "bicubic"
    search: Any = None
    rectangle: Optional[Tuple[int, int, int, int]] = None

    def __post_init__(self):
        number = lambda v: not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and math.isfinite(v)
        whole = lambda v: not isinstance(v, bool) and isinstance(v, (int, np.integer))
        _resample_filter(self.filter)
        object.__setattr__(self, "filter", self.filter.lower())
        if self.rectangle is not None:
            r = tuple(self.rectangle)
            if self.fraction or len(r) != 4 or not all(whole(v) for v in r) or min(r[:2]) < 0 or min(r[2:]) < 1:
                raise ValueError("Crop.rect: x, y >= 0 and cw, ch >= 1, integers (and no fraction beside them)")
            object.__setattr__(self, "rectangle", tuple(int(v) for v in r))
        else:
            if not number(self.fraction) or not 0.0 < self.fraction <= 1.0:
                raise ValueError("Crop: a fraction above 0 and at most 1")
            object.__setattr__(self, "fraction", float(self.fraction))
        a = tuple(self.anchor) if isinstance(self.anchor, (tuple, list)) else ()
        if len(a) != 2 or not all(number(v) and 0.0 <= v <= 1.0 for v in a):
            raise ValueError("Crop: anchor=(ax, ay), both 0 .. 1")
        object.__setattr__(self, "anchor", (float(a[0]), float(a[1])))
        if self.to is not None:
            if self.scale:
                raise ValueError("Crop: scale= or to=, not both")
            if not isinstance(self.to, (tuple, list)) or len(self.to) != 2:
                raise ValueError("Crop: to=(tw, th)")
            object.__setattr__(self, "to", (_side(self.to[0], "Crop"), _side(self.to[1], "Crop")))
        elif self.scale:
            if not number(self.scale) or not 0.0 < self.scale <= L.SCALE_FACTOR_MAX:
                raise ValueError(f"Crop: scale= above 0 and at most {L.SCALE_FACTOR_MAX:g}")
            object.__setattr__(self, "scale", float(self.scale))
        s = self.search
        if s is False:
            object.__setattr__(self, "search", None)
        elif s is not None and s is not True:
            if not isinstance(s, (tuple, list)) or len(s) != 2 or not all(whole(v) for v in s) or not 0 < s[0] <= s[1]:
                raise ValueError("Crop: search=True or search=(wmin, wmax), integers with 0 < wmin <= wmax")
            object.__setattr__(self, "search", (int(s[0]), int(s[1])))

    @classmethod
    def rect(cls, x, y, cw, ch, **kwargs) -> "Crop":
        return cls(rectangle=(x, y, cw, ch), **kwargs)

    @property
    def scaled(self) -> bool:
        return bool(self.scale) or self.to is not None

    def rect_in(self, w: int, h: int) -> Tuple[int, int, int, int]:
        """(x, y, cw, ch) in a w x h frame; ValueError when an explicit rectangle leaves it"""
        if self.rectangle is not None:
            x, y, cw, ch = self.rectangle
            if x + cw > w or y + ch > h:
                raise ValueError(f"Crop: the rectangle {x},{y},{cw}x{ch} leaves the {w}x{h} frame")
            return self.rectangle
        cw, ch = max(1, int(w * self.fraction + 0.5)), max(1, int(h * self.fraction + 0.5))
        return int((w - cw) * self.anchor[0]), int((h - ch) * self.anchor[1]), cw, ch

    def thumb(self, w: int, h: int) -> Optional[Tuple[int, int]]:
        """(tw, th) of the thumbnail made of the piece in a w x h frame; None when it is not scaled"""
        if self.to is not None:
            return self.to
        if not self.scale:
            return None
        _, _, cw, ch = self.rect_in(w, h)
        return max(1, int(cw * self.scale + 0.5)), max(1, int(ch * self.scale + 0.5))

    def search_range(self, w: int, h: int) -> Optional[Tuple[int, int]]:
        """None: placed; (0, 0): the position of the piece at its own size is searched; (wmin, wmax): the scale ladder's widths.
        ValueError for a range the ladder refuses (a side below 32 at wmin, nothing that fits the frame)."""
        if self.search is None:
            return None
        t = self.thumb(w, h)
        if self.search is True and t is None:
            return 0, 0
        sw, sh = t or self.rect_in(w, h)[2:]
        lo, hi = (sw, w) if self.search is True else self.search
        if lo > hi or min(lo, _ladder_height(lo, sw, sh)) < L.LOCATE_SCALED_MIN_SIDE or lo > w or _ladder_height(lo, sw, sh) > h:
            raise ValueError(f"Crop: the widths {lo}..{hi} searched for a {sw}x{sh} piece need both sides at least "
                             f"{L.LOCATE_SCALED_MIN_SIDE} at the smallest and a smallest that fits the frame")
        return lo, hi

    @property
    def label(self) -> str:
        what = "{},{},{}x{}".format(*self.rectangle) if self.rectangle is not None else f"{self.fraction:g}"
        if self.anchor != (0.5, 0.5) and self.rectangle is None:
            what += f" anchor {self.anchor[0]:g},{self.anchor[1]:g}"
        if self.to is not None:
            what += f" @ {self.to[0]}x{self.to[1]} {self.filter}"
        elif self.scale:
            what += f" @ {self.scale:g} {self.filter}"
        return "crop " + what

    def job(self, frame: int, w: int, h: int) -> L.CropJob:
        tw, th = self.thumb(w, h) or (0, 0)
        return L.CropJob(frame, *self.rect_in(w, h), tw, th, L.RESAMPLE_FILTERS[self.filter] if tw else 0)


def _crops(crops, what: str, w: Optional[int] = None, h: Optional[int] = None) -> list:
    """The `Crop` objects of a call, each checked against the w x h frame when that is given: every ValueError comes from here"""
    cr = list(crops)
    if any(not isinstance(c, Crop) for c in cr):
        raise ValueError(f"{what}: crops are made with Crop(fraction) or Crop.rect(x, y, cw, ch)")
    if w is not None:
        for c in cr:
            c.rect_in(w, h)
            if max(c.thumb(w, h) or (0, 0)) > L.RESAMPLE_SIDE_MAX:
                raise ValueError(f"{what}: a thumbnail's side is at most {L.RESAMPLE_SIDE_MAX}")
            c.search_range(w, h)
    return cr


def _crop_attack(w: int, h: int) -> tuple:
    """The attack of the report's stage for frames of w x h: a crop's rectangle needs the frame's size; the original goes in front"""
    return ("ssw_crop_attack_rgb8", L.CropJob, lambda frame, c: c.job(frame, w, h), True)


def _crop_sizes(jobs) -> list:
    """(tw, th) of the T of every job: the thumbnail's size, or the piece's"""
    return [(int(j.tw), int(j.th)) if j.tw else (int(j.cw), int(j.ch)) for j in jobs]


def _crop_run(ctx: Optional[Context], what: str, base, images, crops, search: bool, thumbs: bool) -> tuple:
    """The runner of `crop_attack` and `crop_search_attack`: jobs in frame order over the groups of `_job_groups`.  Returns
    (frames, thumbs or None, found or None), each [len(images)][len(crops)]."""
    frames = _frames_u8(images, what)
    b = _frames_u8([base], what)[0] if frames else None
    if frames and b.shape != frames[0].shape:
        raise ValueError(f"{what}: the original has the images' size")
    cr = _crops(crops, what, *((b.shape[1], b.shape[0]) if frames else ()))
    out = [[None] * len(cr) for _ in frames]
    th, found = ([[None] * len(cr) for _ in frames] if thumbs else None), ([[None] * len(cr) for _ in frames] if search else None)
    if not frames or not cr:
        return [[] for _ in frames] if not cr else out, th, found
    ctx = ctx or default_context()
    h, w = b.shape[:2]
    fb = w * h * 3
    jobs = [(i, p) for i in range(len(frames)) for p in range(len(cr))]
    for used, g0, g1 in _job_groups([(i,) for i, _ in jobs], fb):
        where, n = {i: j for j, i in enumerate(used)}, g1 - g0
        arr = (L.CropJob * n)(*[cr[p].job(where[i], w, h) for i, p in jobs[g0:g1]])
        sizes = _crop_sizes(arr)
        with _owned(ctx) as alloc:
            dev_f, dev_o = alloc(len(used) * fb), alloc(n * fb)
            dev_t = alloc(sum(3 * a * c for a, c in sizes)) if thumbs else None
            _upload_frames(ctx, dev_f, [frames[i] for i in used])
            dev_b = _upload_frames(ctx, alloc(fb), [b])
            if search:
                rng = (L.CropSearch * n)(*[L.CropSearch(*cr[p].search_range(w, h)) for _, p in jobs[g0:g1]])
                got, sad = (L.Placement * n)(), np.zeros(n, np.uint64)
                check(ctx._lib.ssw_crop_search_attack_rgb8(ctx.handle, dev_b.ptr, dev_f.ptr, len(used), w, h, arr, rng, n, dev_o.ptr,
                                                           dev_t.ptr if thumbs else None, got, sad.ctypes.data),
                      "ssw_crop_search_attack_rgb8")
                for (i, p), f, s in zip(jobs[g0:g1], got, sad):
                    found[i][p] = Located(Placement(int(f.x), int(f.y), int(f.pw), int(f.ph)), int(s), int(s) / max(1, int(f.pw) * int(f.ph)))
            else:
                check(ctx._lib.ssw_crop_attack_rgb8(ctx.handle, dev_b.ptr, dev_f.ptr, len(used), w, h, arr, n, dev_o.ptr,
                                                    dev_t.ptr if thumbs else None), "ssw_crop_attack_rgb8")
            for (i, p), frame in zip(jobs[g0:g1], dev_o.to_host(np.uint8, (n, h, w, 3))):
                out[i][p] = frame
            if thumbs:
                flat, at = dev_t.to_host(np.uint8, (sum(3 * a * c for a, c in sizes),)), 0
                for (i, p), (a, c) in zip(jobs[g0:g1], sizes):
                    th[i][p], at = flat[at:at + 3 * a * c].reshape(c, a, 3), at + 3 * a * c
    return out, th, found


def crop_attack(base, images, crops, thumbs: bool = False, ctx: Optional[Context] = None):
    """Every image after every crop attack when the tracer is told the rectangle (ssw_crop_attack_rgb8): the rectangle cut out,
    made a thumbnail as Pillow does it when the `Crop` says so, brought back to its size and laid over `base`, the original, as
    `trace` with a `Placement` would.  base: 8-bit [H, W, 3]; images: 8-bit [H, W, 3] of that size; crops: `Crop` objects (a
    `search` of theirs is not read).  Returns [len(images)][len(crops)] u8 [H, W, 3] frames; with thumbs=True (frames, thumbs),
    thumbs the pieces as they would leak, u8 [th, tw, 3]: PIL's crop((x, y, x + cw, y + ch)).resize((tw, th), filter), byte for byte."""
    cr = [dataclasses.replace(c, search=None) if isinstance(c, Crop) else c for c in crops]
    out, th, _ = _crop_run(ctx, "crop_attack", base, images, cr, False, thumbs)
    return (out, th) if thumbs else out


def crop_search_attack(base, images, crops, ctx: Optional[Context] = None) -> tuple:
    """Every image after every crop attack when the tracer is NOT told where the piece came from (ssw_crop_search_attack_rgb8):
    cut, perhaps scaled, then placed where `locate` finds it -- the position of an unscaled piece, position and size of a
    thumbnail over each `Crop`'s widths (search=None is taken as True).  Returns (frames [len(images)][len(crops)] u8 [H, W, 3],
    found [len(images)][len(crops)] of `Located`)."""
    cr = [dataclasses.replace(c, search=True) if isinstance(c, Crop) and c.search is None else c for c in crops]
    out, _, found = _crop_run(ctx, "crop_search_attack", base, images, cr, True, False)
    return out, found


def unrotate(base, suspects, angles, ctx: Optional[Context] = None) -> list:
    """Every suspect turned back by its angle and completed with the original where the turn lost pixels (ssw_unrotate_rgb8;
    include/ssw.h states the mask): what tracing a `Rotated(angle)` entry extracts from.  base: the original, 8-bit [H, W, 3];
    suspects: 8-bit [H, W, 3] of that size; angles: one per suspect, the angle each was turned by.  Returns one u8 [H, W, 3]
    frame per suspect."""
    b = _frames_u8([base], "unrotate")[0]
    frames = _frames_u8(suspects, "unrotate")
    angles = [_angle(a, "unrotate") for a in angles]
    if len(angles) != len(frames):
        raise ValueError("unrotate: one angle per suspect")
    if not frames:
        return []
    if frames[0].shape != b.shape:
        raise ValueError("unrotate: a rotated suspect has the original's size and 3 channels")
    ctx = ctx or default_context()
    h, w = b.shape[:2]
    fb, n, out = w * h * 3, len(frames), []
    per = max(1, UPLOAD_GROUP_BYTES // (2 * fb))
    with _owned(ctx) as alloc:
        dev_b, dev_i, dev_o = _upload_frames(ctx, alloc(fb), [b]), alloc(min(per, n) * fb), alloc(min(per, n) * fb)
        for g0 in range(0, n, per):
            g = frames[g0:g0 + per]
            _upload_frames(ctx, dev_i, g)
            jobs = (L.RotateJob * len(g))(*[Rotate(a).job(i, w, h) for i, a in enumerate(angles[g0:g0 + per])])
            check(ctx._lib.ssw_unrotate_rgb8(ctx.handle, dev_b.ptr, dev_i.ptr, len(g), w, h, jobs, dev_o.ptr), "ssw_unrotate_rgb8")
            out += list(dev_o.to_host(np.uint8, (len(g), h, w, 3)))
    return out


def _undo_rotated(base, suspects, placements, ctx, find_fn=None, unrotate_fn=None):
    """placements with `Rotated` entries -> (suspects, placements, {index: FoundAngle}) with every such suspect turned back (one
    `unrotate` call) and its entry None: a whole frame of the original's size.  The entries without an angle are searched for
    first, all of one range with one `find_angle` call.  The other entries pass through untouched."""
    placements, suspects = list(placements), list(suspects)
    if len(placements) != len(suspects):
        raise ValueError("placements: one entry (a Placement, a Locate, a Rotated or None) per suspect")
    todo = [i for i, p in enumerate(placements) if isinstance(p, Rotated)]
    if not todo:
        return suspects, placements, {}
    if base is None:
        raise ValueError("Rotated entries need the original's pixels (base=)")
    b = _base_rgb8(base)
    turned = {i: np.asarray(suspects[i]) for i in todo}
    if any(a.dtype != np.uint8 or a.shape != b.shape for a in turned.values()):
        raise ValueError("Rotated: the suspect has the original's size and 3 channels")
    angles, found = {i: placements[i].angle for i in todo}, {}
    for search in sorted({placements[i].search for i in todo if placements[i].angle is None}):
        idx = [i for i in todo if placements[i].angle is None and placements[i].search == search]
        for i, f in zip(idx, (find_fn or find_angle)(b, [turned[i] for i in idx], search, ctx)):
            angles[i], found[i] = f.angle, f
    for i, f in zip(todo, (unrotate_fn or unrotate)(b, [turned[i] for i in todo], [angles[i] for i in todo], ctx)):
        suspects[i], placements[i] = f, None
    return suspects, placements, found


@dataclass
class Collusion:
    """What tracing made of one forgery: `size` colluders (the first `size` copies) pooled with `method`.  weakest_colluder: the
    smallest similarity among them; strongest_innocent: the largest among the other recipients (NaN when there are none);
    found / accused: colluders / innocents above the threshold."""
    method: str
    size: int
    weakest_colluder: float
    strongest_innocent: float
    found: int
    accused: int


@dataclass
class JpegResult:
    """What tracing made of the marked copies after a JPEG of `quality`.  survived: copies whose own mark still exceeds the
    threshold; weakest_own: the smallest similarity of a copy with its own mark; strongest_innocent: the largest with another
    recipient's (NaN when there is one copy); accused: (copy, other mark) pairs above the threshold; psnr_min / psnr_max: the
    compressed copies against the original, in dB; ssim_min / ssim_max: their mean SSIM (NaN unless the report was asked for it)."""
    quality: int
    survived: int
    weakest_own: float
    strongest_innocent: float
    accused: int
    psnr_min: float
    psnr_max: float
    ssim_min: float = math.nan
    ssim_max: float = math.nan


@dataclass
class FilterResult:
    """What tracing made of the marked copies after the filter `filter` (a `Filter.label`); the other fields as in `JpegResult`."""
    filter: str
    survived: int
    weakest_own: float
    strongest_innocent: float
    accused: int
    psnr_min: float
    psnr_max: float
    ssim_min: float = math.nan
    ssim_max: float = math.nan


@dataclass
class ScaleResult:
    """What tracing made of the marked copies after the scale attack `scale` (a `Scale.label`) with thumbnails of `size`
    (nw, nh); the other fields as in `JpegResult`."""
    scale: str
    size: Tuple[int, int]
    survived: int
    weakest_own: float
    strongest_innocent: float
    accused: int
    psnr_min: float
    psnr_max: float
    ssim_min: float = math.nan
    ssim_max: float = math.nan


@dataclass
class RotateResult:
    """What tracing made of the marked copies after the rotation attack `rotation` (a `Rotate.label`), turned back by the known
    angle; kept: the share of the frame's pixels the undoing took from the rotated copy (the rest is the original's); the other
    fields as in `JpegResult`.  For a rotation with a `search` the copies were turned back by the angle FOUND in that range:
    search = (lo, hi); found_min / found_max: the smallest and the largest angle found over the copies; worst_angle_error: the
    largest |found - angle|; kept: the smallest share over the copies."""
    rotation: str
    kept: float
    survived: int
    weakest_own: float
    strongest_innocent: float
    accused: int
    psnr_min: float
    psnr_max: float
    ssim_min: float = math.nan
    ssim_max: float = math.nan
    search: Optional[Tuple[float, float]] = None
    found_min: float = math.nan
    found_max: float = math.nan
    worst_angle_error: float = math.nan


@dataclass
class CropResult:
    """What tracing made of the marked copies after the crop attack `crop` (a `Crop.label`): size (cw, ch), rect (x, y, cw, ch),
    thumb (tw, th) when the piece was made a thumbnail, kept = cw ch / (W H); the other fields as in `JpegResult`.  For a crop
    with a `search` the piece was laid where the tracer's own search found it: search = (wmin, wmax) as the call got it, (0, 0)
    for the piece's own size; found: per copy (x, y, pw, ph); found_exact: how many copies got the true rectangle;
    worst_offset: the largest |x - true x|, |y - true y| over the copies; worst_size_error: the largest |pw - cw|, |ph - ch|."""
    crop: str
    size: Tuple[int, int]
    survived: int
    weakest_own: float
    strongest_innocent: float
    accused: int
    psnr_min: float
    psnr_max: float
    ssim_min: float = math.nan
    ssim_max: float = math.nan
    rect: Tuple[int, int, int, int] = (0, 0, 0, 0)
    thumb: Optional[Tuple[int, int]] = None
    kept: float = math.nan
    search: Optional[Tuple[int, int]] = None
    found: list = field(default_factory=list)
    found_exact: int = 0
    worst_offset: Tuple[int, int] = (0, 0)
    worst_size_error: Tuple[int, int] = (0, 0)


@dataclass
class StrengthRow:
    """`strength_report` for one alpha: the `Quality` of every copy, one `Collusion` per (method, size), methods outermost, and
    one `JpegResult` per JPEG quality asked for; ssim: the `Ssim` of every copy when the report was asked for it; filters: one
    `FilterResult` per filter asked for; scales: one `ScaleResult` per scale asked for; rotations: one `RotateResult` per rotation
    asked for; crops: one `CropResult` per crop asked for."""
    alpha: float
    quality: list
    collusions: list
    jpeg: list = field(default_factory=list)
    ssim: list = field(default_factory=list)
    filters: list = field(default_factory=list)
    scales: list = field(default_factory=list)
    rotations: list = field(default_factory=list)
    crops: list = field(default_factory=list)

    def collusion(self, method: str, size: int) -> Collusion:
        return next(c for c in self.collusions if (c.method, c.size) == (method, size))


def _collusion(method: str, size: int, sims: np.ndarray, threshold: float) -> Collusion:
    inside, outside = sims[:size], sims[size:]
    over = sims > np.float32(threshold)                      # NaN never exceeds (algorithm.rs:677)
    return Collusion(method, size, float(inside.min()), float(outside.max()) if outside.size else math.nan,
                     int(over[:size].sum()), int(over[size:].sum()))


def _attack_fold(sims: np.ndarray, qualities: list, threshold: float, ssims=()) -> tuple:
    """What `JpegResult` and `FilterResult` share, in their order: (survived, weakest_own, strongest_innocent, accused, psnr_min,
    psnr_max, ssim_min, ssim_max).  sims [copies][copies]: row c is copy c after the attack against every mark"""
    mean = [s.mean for s in ssims] or [math.nan]
    own, others = np.diagonal(sims), sims[~np.eye(len(sims), dtype=bool)]
    over = sims > np.float32(threshold)                      # NaN never exceeds (algorithm.rs:677)
    psnr = [q.psnr for q in qualities]
    return (int(np.diagonal(over).sum()), float(own.min()), float(others.max()) if others.size else math.nan,
            int(over.sum() - np.diagonal(over).sum()), min(psnr), max(psnr), min(mean), max(mean))


def _jpeg_result(quality: int, sims: np.ndarray, qualities: list, threshold: float, ssims=()) -> JpegResult:
    return JpegResult(quality, *_attack_fold(sims, qualities, threshold, ssims))


def _filter_result(label: str, sims: np.ndarray, qualities: list, threshold: float, ssims=()) -> FilterResult:
    return FilterResult(label, *_attack_fold(sims, qualities, threshold, ssims))


def _scale_result(label_size: tuple, sims: np.ndarray, qualities: list, threshold: float, ssims=()) -> ScaleResult:
    return ScaleResult(*label_size, *_attack_fold(sims, qualities, threshold, ssims))


def _rotate_result(label_kept: tuple, sims: np.ndarray, qualities: list, threshold: float, ssims=()) -> RotateResult:
    return RotateResult(*label_kept, *_attack_fold(sims, qualities, threshold, ssims))


def strength_report(image, alphas, k: int = 1000, copies: int = 8, sizes=(2, 4),
                    methods=("average", "median", "min", "max", "minmax", "mosaic"), threshold: float = 6.0,
                    config: Optional[WriteConfig] = None, seed=None, ctx: Optional[Context] = None, jpeg=(), ssim: bool = False,
                    filters=(), scales=(), rotations=(), crops=()) -> list:
    """The two questions to answer before a copy ships, per insertion strength: how visible is the mark, and how many
    recipients must pool their copies before tracing fails?  For each alpha (`config` with its alpha replaced; the default
    Option2 + Energy): `copies` marked copies of the 8-bit `image` (ssw_fingerprint_embed_rgb8), their distance from it
    (ssw_quality_rgb8), one forgery per (method, size) from the first `size` copies (one ssw_collude_rgb8 call) and one
    trace of all forgeries against all marks (ssw_fingerprint_trace_rgb8) -- device-resident: only the original and the
    marks go up, only statistics and similarities come down.  Marks: numpy.random.default_rng(seed)
    .standard_normal((copies, k)).astype(float32), the same for every alpha.  jpeg: JPEG qualities (1 .. 100); per alpha every
    copy is compressed at every quality (one ssw_jpeg_rgb8 call), all results are traced against all marks (one more
    ssw_fingerprint_trace_rgb8 call) and measured against the original (one more ssw_quality_rgb8 call): one `JpegResult` per
    quality in `StrengthRow.jpeg`.  ssim: also the structural similarity of every copy and its original (one ssw_ssim_rgb8 call per
    alpha, `StrengthRow.ssim`; one more on the JPEG results, `JpegResult.ssim_min` / `ssim_max`); no side below 8 then.
    filters: `Filter` objects; per alpha every copy goes through every filter (one ssw_filter_rgb8 call, filter-major), all
    results are traced against all marks and measured against the original (one more ssw_fingerprint_trace_rgb8 and
    ssw_quality_rgb8 call, and one ssw_ssim_rgb8 with `ssim`): one `FilterResult` per filter in `StrengthRow.filters`.
    scales: `Scale` objects; the same after the filters with one ssw_scale_attack_rgb8 call, scale-major: one `ScaleResult` per
    scale in `StrengthRow.scales` -- whether `trace` still names the recipient of a thumbnail that Pillow made.
    rotations: `Rotate` objects; the same after the scales with one ssw_rotate_attack_rgb8 call, rotation-major: one
    `RotateResult` per rotation in `StrengthRow.rotations` -- what `trace` finds in a copy that Pillow turned when it is told the angle.
    Rotations with a `search` (`Rotate(1.3, search=True)`) answer the publisher's question instead -- what is left when the
    tracer is NOT told the angle: after the call above, one ssw_rotate_search_attack_rgb8 call per distinct range turns the
    copies, searches for every copy's angle and turns it back by the angle found; then the same trace, quality and SSIM calls.
    Their rows stand in `StrengthRow.rotations` where they were given, with `found_min`, `found_max` and `worst_angle_error`.
    crops: `Crop` objects; the same after the rotations -- how much of the picture must a leak keep?  The crops without a
    `search` go in one ssw_crop_attack_rgb8 call, crop-major; those with one -- what is left when nobody tells the tracer where
    the piece came from -- in one ssw_crop_search_attack_rgb8 call; each followed by the same trace, quality and SSIM calls: one
    `CropResult` per crop in `StrengthRow.crops`, in the order given.
    Returns one `StrengthRow` per alpha."""
    jq, fl, sc = _jpeg_qualities(jpeg, "strength_report"), _filters(filters, "strength_report"), _scales(scales, "strength_report")
    ro = _rotations(rotations, "strength_report")
    img = _frames_of_side([image], "strength_report", "a JPEG attack", L.JPEG_MIN_SIDE if jq else 0)[0]
    cr = _crops(crops, "strength_report", img.shape[1], img.shape[0])
    if ssim:
        _frames_of_side([img], "strength_report", "SSIM", L.SSIM_MIN_SIDE)
    if any(r.search is not None for r in ro) and (min(img.shape[:2]) < L.ANGLE_MIN_SIDE or img.shape[0] * img.shape[1] > L.ANGLE_MAX_PIXELS):
        raise ValueError(f"strength_report: a searched rotation needs frames of at least {L.ANGLE_MIN_SIDE} x {L.ANGLE_MIN_SIDE} and at most 2^27 pixels")
    sizes, methods = [int(c) for c in sizes], [str(m).lower() for m in methods]
    if any(c > copies for c in sizes):
        raise ValueError("strength_report: a coalition cannot be larger than the number of copies")
    if any(not 1 <= c <= L.COLLUDE_MAX_MEMBERS for c in sizes) or copies < 1:
        raise ValueError(f"strength_report: coalitions of 1 .. {L.COLLUDE_MAX_MEMBERS} copies")
    plan = [(m, c) for m in methods for c in sizes]
    co = (L.Coalition * max(len(plan), 1))(*[_coalition(m, range(c), copies) for m, c in plan])
    ctx = ctx or default_context()
    config = config or WriteConfig.default()
    marks = np.random.default_rng(seed).standard_normal((copies, k)).astype(np.float32)
    h, w = img.shape[:2]
    fb, nf, windows = w * h * 3, len(plan), _ssim_windows(w, h)
    lib, rows = ctx._lib, []
    with _owned(ctx) as alloc:
        def trace(cfg, dev_frames, n, dev_e, dev_s):
            check(lib.ssw_fingerprint_trace_rgb8(ctx.handle, C.byref(cfg), dev_img.ptr, dev_frames.ptr, n, w, h, k, dev_marks.ptr, copies,
                                                 C.c_float(threshold), dev_e.ptr, dev_s.ptr, None, None, None), "ssw_fingerprint_trace_rgb8")

        def measure(dev_frames, n, dev_st):
            check(lib.ssw_quality_rgb8(ctx.handle, dev_img.ptr, 1, dev_frames.ptr, n, w, h, dev_st.ptr), "ssw_quality_rgb8")

        def ssims_of(dev_frames, n):
            check(lib.ssw_ssim_rgb8(ctx.handle, dev_img.ptr, 1, dev_frames.ptr, n, w, h, dev_ssim.ptr, None), "ssw_ssim_rgb8")
            return _ssims(dev_ssim.to_host(np.uint64, (n, L.SSIM_STATS)), *windows)

        def stage(attack, params):       # every copy under every parameter, parameter-major: the call, its jobs, their number, the results' buffers
            name, struct, job = attack[:3]
            n = len(params) * copies
            return (name if len(attack) == 3 else (name, True), (struct * n)(*[job(c, p) for p in params for c in range(copies)]), n,
                    [alloc(n * b) for b in (fb, k * 4, copies * 4, 8 * L.QUALITY_STATS)] if n else None)

        def attacked(cfg, made, labels, result, call=None):       # attack, trace, quality, the downloads, SSIM: one `result` per label
            name, jobs, n, (dev_frames, dev_e, dev_s, dev_st) = made
            name, lead = (name, ()) if isinstance(name, str) else (name[0], (dev_img.ptr,))       # the original in front
            if call is None:
                check(getattr(lib, name)(ctx.handle, *lead, dev_copies.ptr, copies, w, h, jobs, n, dev_frames.ptr), name)
            else:                                        # (the searched rotations: a call with answers of its own)
                call(jobs, n, dev_frames)
            trace(cfg, dev_frames, n, dev_e, dev_s)
            measure(dev_frames, n, dev_st)
            sims = dev_s.to_host(np.float32, (len(labels), copies, copies))
            q = _qualities(dev_st.to_host(np.uint64, (n, L.QUALITY_STATS)), w * h)
            s = ssims_of(dev_frames, n) if ssim else []
            return [result(label, sims[i], q[i * copies:(i + 1) * copies], threshold, s[i * copies:(i + 1) * copies])
                    for i, label in enumerate(labels)]

        dev_img, dev_marks = _upload_frames(ctx, alloc(img.nbytes), [img]), _upload_frames(ctx, alloc(marks.nbytes), [marks])
        dev_copies, dev_stats = alloc(copies * fb), alloc(copies * 8 * L.QUALITY_STATS)
        dev_forged, dev_ext, dev_sims = alloc(max(nf, 1) * fb), alloc(max(nf * k, 1) * 4), alloc(max(nf * copies, 1) * 4)
        jpeg_stage, filter_stage, scale_stage = stage(_JPEG_ATTACK, jq), stage(_FILTER_ATTACK, fl), stage(_scale_attack(w, h), sc)
        known = [i for i, r in enumerate(ro) if r.search is None]
        rotate_stage = stage(_rotate_attack(w, h), [ro[i] for i in known])
        # the searched rotations: per distinct range the positions in `ro`, the stage, the answers of its call
        search_stages = [(rng, which, stage(_rotate_attack(w, h), [ro[i] for i in which]), (L.AngleFound * (len(which) * copies))(),
                          np.zeros(len(which) * copies, np.uint64)) for rng, which in _search_ranges(ro)]
        # the crops: the placed ones and the searched ones, each kind one stage and one call; positions in `cr`
        placed, sought = [i for i, c in enumerate(cr) if c.search is None], [i for i, c in enumerate(cr) if c.search is not None]
        crop_stage, crop_search_stage = stage(_crop_attack(w, h), [cr[i] for i in placed]), stage(_crop_attack(w, h), [cr[i] for i in sought])
        crop_ranges = (L.CropSearch * max(1, len(sought) * copies))(*[L.CropSearch(*cr[i].search_range(w, h)) for i in sought for _ in range(copies)])
        crop_found, crop_sad = (L.Placement * max(1, len(sought) * copies))(), np.zeros(max(1, len(sought) * copies), np.uint64)
        dev_ssim = alloc(max([copies, jpeg_stage[2], filter_stage[2], scale_stage[2], rotate_stage[2], crop_stage[2], crop_search_stage[2]]
                             + [s[2][2] for s in search_stages]) * 8 * L.SSIM_STATS) if ssim else None
        kept = list(zip([ro[i].label for i in known], _kept_shares(ctx, [ro[i] for i in known], w, h)))

        def searched(cfg, rng, which, made, found, counts):      # one RotateResult per rotation of the range `rng`
            def call(jobs, n, dev_frames):
                check(lib.ssw_rotate_search_attack_rgb8(ctx.handle, dev_img.ptr, dev_copies.ptr, copies, w, h, jobs, n, rng[0], rng[1], dev_frames.ptr,
                                                        None, found, None, counts.ctypes.data), "ssw_rotate_search_attack_rgb8")

            def result(i, sims, q, threshold, s):
                angles = [int(f.n) / L.ANGLE_PER_DEGREE for f in found[i * copies:(i + 1) * copies]]
                return RotateResult(ro[which[i]].label, int(counts[i * copies:(i + 1) * copies].min()) / (w * h),
                                    *_attack_fold(sims, q, threshold, s), search=rng, found_min=min(angles), found_max=max(angles),
                                    worst_angle_error=max(abs(a - ro[which[i]].angle) for a in angles))
            return attacked(cfg, made, list(range(len(which))), result, call)

        def cropped(cfg, which, made, search):                   # one CropResult per crop of `which`, placed or searched
            def call(jobs, n, dev_frames):
                if search:
                    check(lib.ssw_crop_search_attack_rgb8(ctx.handle, dev_img.ptr, dev_copies.ptr, copies, w, h, jobs, crop_ranges, n, dev_frames.ptr,
                                                          None, crop_found, crop_sad.ctypes.data), "ssw_crop_search_attack_rgb8")
                else:
                    check(lib.ssw_crop_attack_rgb8(ctx.handle, dev_img.ptr, dev_copies.ptr, copies, w, h, jobs, n, dev_frames.ptr, None),
                          "ssw_crop_attack_rgb8")

            def result(i, sims, q, threshold, s):
                c = cr[which[i]]
                x, y, cw, ch = rect = c.rect_in(w, h)
                more = {}
                if search:
                    got = [(int(f.x), int(f.y), int(f.pw), int(f.ph)) for f in crop_found[i * copies:(i + 1) * copies]]
                    more = dict(search=c.search_range(w, h), found=got, found_exact=sum(g == rect for g in got),
                                worst_offset=(max(abs(g[0] - x) for g in got), max(abs(g[1] - y) for g in got)),
                                worst_size_error=(max(abs(g[2] - cw) for g in got), max(abs(g[3] - ch) for g in got)))
                return CropResult(c.label, (cw, ch), *_attack_fold(sims, q, threshold, s), rect=rect, thumb=c.thumb(w, h),
                                  kept=cw * ch / (w * h), **more)
            return attacked(cfg, made, list(range(len(which))), result, call)
        for alpha in alphas:
            cfg = L.Config(config.ordering.tag, config.insertion.tag, float(alpha), config.precision)
            check(lib.ssw_fingerprint_embed_rgb8(ctx.handle, C.byref(cfg), dev_img.ptr, w, h, dev_marks.ptr, copies, k, dev_copies.ptr, None),
                  "ssw_fingerprint_embed_rgb8")
            measure(dev_copies, copies, dev_stats)
            sims = np.zeros((0, copies), np.float32)
            if nf:
                check(lib.ssw_collude_rgb8(ctx.handle, dev_copies.ptr, copies, w, h, co, nf, dev_forged.ptr), "ssw_collude_rgb8")
                trace(cfg, dev_forged, nf, dev_ext, dev_sims)
                sims = dev_sims.to_host(np.float32, (nf, copies))
            q = _qualities(dev_stats.to_host(np.uint64, (copies, L.QUALITY_STATS)), w * h)
            rows.append(StrengthRow(float(alpha), q, [_collusion(m, c, sims[i], threshold) for i, (m, c) in enumerate(plan)]))
            if ssim:
                rows[-1].ssim = ssims_of(dev_copies, copies)
            if jq:
                rows[-1].jpeg = attacked(cfg, jpeg_stage, jq, _jpeg_result)
            if fl:
                rows[-1].filters = attacked(cfg, filter_stage, [f.label for f in fl], _filter_result)
            if sc:
                rows[-1].scales = attacked(cfg, scale_stage, [(s.label, s.size(w, h)) for s in sc], _scale_result)
            if ro:
                by_place = dict(zip(known, attacked(cfg, rotate_stage, kept, _rotate_result))) if known else {}
                for rng, which, made, found, counts in search_stages:
                    by_place.update(zip(which, searched(cfg, rng, which, made, found, counts)))
                rows[-1].rotations = [by_place[i] for i in range(len(ro))]
            if cr:
                by_place = dict(zip(placed, cropped(cfg, placed, crop_stage, False))) if placed else {}
                if sought:
                    by_place.update(zip(sought, cropped(cfg, sought, crop_search_stage, True)))
                rows[-1].crops = [by_place[i] for i in range(len(cr))]
    return rows


# ---- Tester (algorithm.rs:668-715) -------------------------------------------------------------
@dataclass
class Similarity:
    similarity: float

    def exceeds_sigma(self, n_sigma: float) -> bool:
        return self.similarity > n_sigma


class Tester:
    def __init__(self, extracted_watermark, ctx: Optional[Context] = None):
        self._e = np.ascontiguousarray(extracted_watermark, dtype=np.float32).ravel()
        self._ctx = ctx or default_context()

    new = classmethod(lambda cls, e, ctx=None: cls(e, ctx))

    def similarity(self, comparison_watermark) -> Similarity:
        m = np.ascontiguousarray(_mark_data(comparison_watermark), dtype=np.float32)
        out = C.c_float()
        check(self._ctx._lib.ssw_similarity(self._ctx.handle, self._e.ctypes.data, self._e.size, m.ctypes.data,
                                            m.size, C.byref(out)), "Tester::similarity")
        return Similarity(float(out.value))
