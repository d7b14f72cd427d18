"""A recording stand-in for libssw_hip.so, enough to run the host wrappers of the strength report (api.quality, ssim, collude,
jpeg, filter, strength_report) without a GPU, and the cases whose call record tests/golden/strength_calls_parent.json keeps.

Every call answers SSW_OK (or the status `fail` names for it) and is recorded as [name, arguments]: the context as "ctx", a
device pointer as ["dev", bytes of the allocation it points into, offset], a host pointer as "host", a scalar by value, a job
array or a configuration as the hex of its bytes.  ssw_dev_alloc hands out addresses that are never used twice and
ssw_copy_to_host zero-fills its destination; allocations and frees are kept beside the record (`allocs`, `live`), not in it."""
import ctypes as C

import numpy as np

from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd import api

HANDLE = 0xC0
FIRST_ADDRESS, ADDRESS_STEP = 1 << 56, 1 << 32       # above every host address; every allocation of the cases is far below the step


class FakeLib:
    def __init__(self, fail=None):
        self.fail = dict(fail or {})          # name -> status to answer instead of SSW_OK
        self.calls, self.allocs, self.live = [], [], {}
        self._sizes = {}                      # base address -> bytes, the freed ones included

    def __getattr__(self, name):
        if name not in L.SIGNATURES:
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def _pointer(self, value):
        if value is None:
            return None
        if value == HANDLE:
            return "ctx"
        base = value - (value - FIRST_ADDRESS) % ADDRESS_STEP
        if base in self._sizes:
            assert base in self.live, "a pointer into a freed allocation"
            assert value - base < self._sizes[base] or self._sizes[base] == 0
            return ["dev", self._sizes[base], value - base]
        return "host"

    def _argument(self, kind, a):
        if isinstance(a, (C.Array, C.Structure)):
            return bytes(a).hex()
        if hasattr(a, "_obj"):                # byref(...)
            return bytes(a._obj).hex()
        if kind is C.c_void_p:
            return self._pointer(a.value if isinstance(a, C.c_void_p) else a)
        if isinstance(a, C.c_float):
            return a.value
        return None if a is None else (float(a) if kind is C.c_float else int(a))

    def _call(self, name, args):
        kinds = L.SIGNATURES[name][1]
        assert len(args) == len(kinds), name
        if name == "ssw_ctx_destroy":
            return 0
        if name == "ssw_dev_alloc":
            base = FIRST_ADDRESS + len(self._sizes) * ADDRESS_STEP
            self._sizes[base] = self.live[base] = int(args[1])
            self.allocs.append(int(args[1]))
            args[2]._obj.value = base
            return 0
        if name == "ssw_dev_free":
            del self.live[args[1].value]
            return 0
        self.calls.append([name, [self._argument(k, a) for k, a in zip(kinds, args)]])
        if name == "ssw_copy_to_host":
            C.memset(args[1], 0, int(args[3]))
        return self.fail.get(name, 0)


def fake_context(fail=None):
    ctx = api.Context.__new__(api.Context)
    ctx._lib, ctx.handle, ctx.device_id = FakeLib(fail), C.c_void_p(HANDLE), 0
    return ctx


W, H = 24, 16
FB = W * H * 3


def frames(n, seed=0):
    return list(np.random.default_rng(seed).integers(0, 256, (n, H, W, 3), dtype=np.uint8))


def _report(ctx, **more):
    kw = dict(k=50, copies=3, sizes=(2,), methods=("average", "mosaic"), seed=1)
    kw.update(more)
    return api.strength_report(frames(1)[0], [0.02, 0.1], ctx=ctx, **kw)


COALITIONS = [("average", [0, 1]), ("median", [1, 1, 2]), ("mosaic", [3]), ("min", [2, 0, 3, 0]), ("max", [1]), ("minmax", [3, 2, 1, 0])]
QUALITIES = (90, 50, 10)
FILTERS = [api.Filter.blur(1.5), api.Filter.median(), api.Filter.unsharp()]

# name -> (UPLOAD_GROUP_BYTES or None for the default, the call on a context)
CASES = {
    "report_plain": (None, lambda ctx: _report(ctx)),
    "report_jpeg_filters_ssim": (None, lambda ctx: _report(ctx, jpeg=(75, 30), filters=[api.Filter.blur(1), api.Filter.median()], ssim=True)),
    "report_one_copy_jpeg": (None, lambda ctx: _report(ctx, copies=1, sizes=(), jpeg=(50,))),
    "quality_one_original": (2 * FB, lambda ctx: api.quality(frames(1)[0], frames(5, 1), ctx)),
    "quality_one_per_copy": (2 * FB, lambda ctx: api.quality(frames(5), frames(5, 1), ctx)),
    "ssim_maps_one_original": (2 * FB, lambda ctx: api.ssim(frames(1)[0], frames(5, 1), ctx, maps=True)),
    "ssim_maps_one_per_copy": (2 * FB, lambda ctx: api.ssim(frames(5), frames(5, 1), ctx, maps=True)),
    "collude_cap_5fb": (5 * FB, lambda ctx: api.collude(frames(4), COALITIONS, ctx)),
    "collude_cap_1": (1, lambda ctx: api.collude(frames(4), COALITIONS, ctx)),
}
for _name, _cap in (("default", None), ("5fb", 5 * FB), ("1", 1)):
    CASES[f"jpeg_cap_{_name}"] = (_cap, lambda ctx: api.jpeg(frames(4), QUALITIES, ctx))
    CASES[f"filter_cap_{_name}"] = (_cap, lambda ctx: api.filter(frames(4), FILTERS, ctx))


def run_case(name, ctx=None):
    """Runs one case on a fake context (a fresh one unless given); returns (the context's FakeLib, what the call returned)."""
    cap, call = CASES[name]
    ctx, before = ctx or fake_context(), api.UPLOAD_GROUP_BYTES
    try:
        if cap is not None:
            api.UPLOAD_GROUP_BYTES = cap
        return ctx._lib, call(ctx)
    finally:
        api.UPLOAD_GROUP_BYTES = before


def record(name):
    lib, _ = run_case(name)
    return {"calls": lib.calls, "allocs": sorted(lib.allocs), "live": len(lib.live)}


# ---- the strength command's output: hand-made rows ---------------------------------------------------------------------------
def cli_rows():
    nan, inf = float("nan"), float("inf")
    q = [api.Quality((120, 90, 300), 170, 400, 3, W * H), api.Quality((0, 0, 0), 0, 0, 0, W * H), api.Quality((7, 1, 2), 3, 9, 1, W * H)]
    s = [api.Ssim(14 * (1 << 30) - 12345, (1 << 29) + 77, 7, 5, 3), api.Ssim(15 * (1 << 30), 1 << 30, 0, 5, 3), api.Ssim(9 * (1 << 30), -5, 13, 5, 3)]
    with_ssim = api.StrengthRow(0.02, q, [api.Collusion("average", 2, 21.857, 1.304, 2, 0), api.Collusion("mosaic", 3, 5.5, nan, 1, 0),
                                          api.Collusion("min", 2, -0.25, 7.125, 0, 1)],
                                [api.JpegResult(75, 3, 18.26, 2.04, 0, 33.04, 35.96, 0.9512, 0.9749), api.JpegResult(10, 1, 3.949, 6.51, 2, 24.0, inf, 0.5, 1.0)],
                                s, [api.FilterResult("blur 1.5", 2, 5.05, nan, 0, 28.123, 29.0, 0.803, 0.81),
                                    api.FilterResult("unsharp 2,150,3", 3, 30.0, 6.04, 1, 31.5, inf, 0.9, 1.0)])
    without = api.StrengthRow(0.1, q[:1], [api.Collusion("median", 1, 9.0, nan, 1, 0)],
                              [api.JpegResult(50, 1, 12.345, nan, 0, 30.0, 30.0)], [], [api.FilterResult("median 3", 0, 1.5, nan, 3, 27.0, inf)])
    return [with_ssim, without, api.StrengthRow(0.5, q[1:2], [])]


def cli_output(as_json):
    """What cli.cmd_strength prints for `cli_rows` (strength_report and the image file are stood in for)."""
    import argparse
    import io
    from spread_spectrum_watermarking_amd import cli
    args = argparse.Namespace(file="cat.png", alpha=[0.02, 0.1, 0.5], length=50, copies=3, collude=[2], method=["average"], similarity_exceed=6.0,
                              jpeg=[75, 10], ssim=True, filters=[], json=as_json)
    before = cli.strength_report, cli._open_image
    cli.strength_report, cli._open_image = (lambda *a, **k: cli_rows()), (lambda path: None)
    try:
        out = io.StringIO()
        assert cli.cmd_strength(args, out) == 0
        return out.getvalue()
    finally:
        cli.strength_report, cli._open_image = before
