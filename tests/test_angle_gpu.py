"""ssw_find_angle_rgb8 on the GPU against the restatement of tests/test_angle_cpu.py: EQUALITY -- the answer's n, D and c and
every rung's (D, c) -- at the smallest shapes at which the kernels can go wrong (the minimum, odd sides, a pixel past a tile at
either factor, the largest angles and boxes, ties at every stage, the largest D, the 64-bit origin of a 20 000 pixel strip, a
device pointer one byte off), at the smallest ranges, on the cat, and through trace_many and the CLI."""
import ctypes as C
import functools
import io
import os

import numpy as np
import pytest
from PIL import Image

import gpu_util as G
from gpu_util import ctx, lib
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd import api, cli
from spread_spectrum_watermarking_amd._lib import check
from test_angle_cpu import ON_GRID, cat, find_angle_ref, marked_cat, rungs_ref, smooth, turned

pytestmark = pytest.mark.gpu


class Dev:
    """Device memory holding `a`, `off` bytes into its allocation"""

    def __init__(self, a, off=0):
        a = np.ascontiguousarray(a)
        self.buf, self.off = ctx().alloc(a.nbytes + off + 16), off
        check(lib().ssw_copy_to_dev(ctx().handle, self.ptr, a.ctypes.data, a.nbytes), "ssw_copy_to_dev")

    @property
    def ptr(self):
        return C.c_void_p(self.buf.ptr.value + self.off)

    def free(self):
        self.buf.free()


def dev_find(base, suspects, amin, amax, off=0, want_rungs=True):
    """-> ([(n, D, c)] per suspect, rungs [n][n_rungs][2]) of one call"""
    suspects = np.stack(suspects)
    n, h, w, _ = suspects.shape
    b, d = Dev(base, off), Dev(suspects, off)
    found = (L.AngleFound * n)()
    j0, j1 = rungs_ref(amin, amax)
    n_rungs = j1 - j0 + 1
    rungs = np.full((n, n_rungs, 2), 0xA5A5A5A5, np.uint64)
    try:
        check(lib().ssw_find_angle_rgb8(ctx().handle, b.ptr, d.ptr, n, w, h, amin, amax, found, rungs.ctypes.data if want_rungs else None),
              "ssw_find_angle_rgb8")
    finally:
        b.free(); d.free()
    assert all(f.n_rungs == n_rungs for f in found)
    return [(f.n, f.sad, f.count) for f in found], rungs


def same_as_ref(base, suspects, amin, amax, what, off=0):
    got, rungs = dev_find(base, suspects, amin, amax, off)
    refs = [find_angle_ref(base, s, amin, amax) for s in suspects]
    for i, (g, r) in enumerate(zip(got, refs)):
        want = np.asarray(r.rungs, np.uint64)
        bad = np.nonzero((rungs[i] != want).any(axis=1))[0]
        assert bad.size == 0, (what, i, "rung", int(bad[0]), rungs[i][bad[0]].tolist(), r.rungs[bad[0]])
        assert g == (r.n, r.D, r.c), (what, i, g, (r.n, r.D, r.c))
    return refs


# ---- shapes ------------------------------------------------------------------------------------------------------------------
SHAPES = [(32, 32, 4, "the minimum"), (33, 47, 4, "odd sides"), (65, 41, 2, "a pixel past a tile at f = 1"),
          (132, 36, 2, "a partial tile at f = 4"), (35, 130, 45, "a tall strip at the largest angles"), (96, 64, 45, "361 rungs")]


@pytest.mark.parametrize("w,h,r,why", SHAPES, ids=[f"{w}x{h}" for w, h, _, _ in SHAPES])
def test_shapes_equal_the_restatement(w, h, r, why):
    base = smooth(w, h)
    suspects = [turned(base, a) for a in (0.4 * r, -0.9 * r, 0.03125)]
    refs = same_as_ref(base, suspects, -r, r, why)
    assert len(refs[0].rungs) == 8 * r + 1


def test_a_flat_frame_ties_at_every_stage():
    flat = np.full((40, 52, 3), 93, np.uint8)
    r = same_as_ref(flat, [flat], -3, 3, "flat")[0]
    assert (r.n, r.D, r.kept) == (-96, 0, [0, 1, 2, 3])


def test_noise():
    base = np.random.default_rng(64).integers(0, 256, (64, 64, 3), dtype=np.uint8)
    same_as_ref(base, [turned(base, 1.5), turned(base, -3.0, "BILINEAR"), base], -4, 4, "noise")


def test_the_largest_difference():
    black, white = np.zeros((48, 40, 3), np.uint8), np.full((48, 40, 3), 255, np.uint8)
    r = same_as_ref(black, [white], -2, 2, "all-255 on all-0")[0]
    assert r.D == 255 * r.c


@pytest.mark.parametrize("w,h", [(20000, 32), (32, 20000)])
def test_a_long_strip_holds_the_64_bit_origin(w, h):
    """C p passes 2^31 at the strip's ends"""
    base = smooth(w, h)
    same_as_ref(base, [turned(base, 0.25), turned(base, -0.09375)], -0.5, 0.5, "strip")


def test_a_device_pointer_one_byte_off():
    base = smooth(65, 41, 3)
    same_as_ref(base, [turned(base, 1.0), turned(base, -1.75)], -2, 2, "one byte off", off=1)
    same_as_ref(base, [turned(base, 1.0)], -2, 2, "three bytes off", off=3)


# ---- ranges ------------------------------------------------------------------------------------------------------------------
def test_ranges_of_one_angle_two_rungs_and_the_truth_at_the_edge():
    base = smooth(96, 64)
    r = same_as_ref(base, [turned(base, 1.0)], 1.0, 1.0, "one angle")[0]
    assert len(r.rungs) == 1 and r.n == 32
    r = same_as_ref(base, [turned(base, 0.34375)], 0.3, 0.4, "two rungs")[0]
    assert len(r.rungs) == 2 and 8 <= r.n <= 16
    for edge in (-3.0, 3.0):
        r = same_as_ref(base, [turned(base, edge)], -3, 3, "the truth at the edge")[0]
        assert abs(r.n - 32 * edge) <= 32                                 # a 96 x 64 frame: within a degree; equality is the test


def test_without_the_rungs_the_answer_is_the_same():
    base = smooth(65, 41)
    sus = [turned(base, 0.5)]
    assert dev_find(base, sus, -2, 2, want_rungs=False)[0] == dev_find(base, sus, -2, 2)[0]


# ---- the cat -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("angle,filt,search", ON_GRID, ids=lambda v: str(v))
def test_the_cat_on_the_grid(angle, filt, search):
    r = same_as_ref(cat(), [turned(marked_cat(), angle, filt)], *search, "cat")[0]
    assert r.n == round(32 * angle)


def test_nine_suspects_with_nine_angles_in_one_call():
    angles = [-7.96875, -2.5, -0.15625, 0.0, 0.03125, 1.0, 3.4375, 5.0, 9.5]
    refs = same_as_ref(cat(), [turned(marked_cat(), a, "BILINEAR" if i % 2 else "BICUBIC") for i, a in enumerate(angles)], -10, 10, "nine")
    assert [r.n for r in refs] == [round(32 * a) for a in angles]


# ---- the public surface ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def leaked():
    """(base, marks, three marked copies of the cat turned by Pillow, their angles)"""
    base, angles = cat(), [1.0, -2.5, 0.6875]
    marks = np.random.default_rng(21).standard_normal((3, 1000)).astype(np.float32)
    copies = api.Writer(base, api.WriteConfig(), ctx()).mark_copies_rgb8(list(marks))
    return base, marks, [turned(c, a) for c, a in zip(copies, angles)], angles


def test_find_angle_python():
    base, _, sus, angles = leaked()
    found, rungs = api.find_angle(base, sus, ctx=ctx(), rungs=True)
    refs = [find_angle_ref(base, s, -10, 10) for s in sus]
    assert [(f.n, f.sad, f.count) for f in found] == [(r.n, r.D, r.c) for r in refs] and [f.angle for f in found] == angles
    assert np.array_equal(rungs, np.asarray([r.rungs for r in refs], np.uint64)) and all(f.mean == f.sad / f.count for f in found)
    assert [f.n for f in api.find_angle(base, sus[:1], search=(0.5, 1.5), ctx=ctx())] == [32]


def test_trace_many_with_searched_entries_is_the_trace_with_the_angles_found():
    base, marks, sus, angles = leaked()
    c = ctx()
    got = api.trace_many(base, sus, list(marks), ctx=c, placements=[api.Rotated()] * 3)
    assert sorted(got.turned) == [0, 1, 2] and [got.turned[i].angle for i in range(3)] == angles
    c.enable_timing(True)
    try:
        c.reset_timing()
        ref = api.trace_many(base, sus, list(marks), ctx=c, placements=[api.Rotated(got.turned[i].angle) for i in range(3)])
        c.synchronize()
        t = c.timing()
    finally:
        c.enable_timing(False)
    assert t["locate"]["launches"] == 0 and t["locate"]["ms"] == 0.0 and t["locate_coarse"]["launches"] == 0      # explicit angles: no search
    assert ref.turned == {}
    for name in ("extracted", "sims", "best", "best_sim", "n_exceed"):
        assert np.array_equal(getattr(got, name), getattr(ref, name), equal_nan=True), name
    assert list(got.best) == [0, 1, 2] and all(got.best_sim > 6.0), (got.best, got.best_sim)                      # it names each copy
    mixed = api.trace_many(base, sus, list(marks), ctx=c, placements=[api.Rotated(1.0), api.Rotated(search=(-3, 0)), api.Rotated()])
    assert sorted(mixed.turned) == [1, 2] and np.array_equal(mixed.sims, ref.sims, equal_nan=True)
    reader = api.Reader.base(base, ctx=c)
    handle = reader.trace(sus, list(marks), placements=[api.Rotated()] * 3, base=base)
    assert [handle.turned[i].n for i in range(3)] == [32, -80, 22] and list(handle.best) == [0, 1, 2]


def test_the_search_is_billed_to_locate():
    base, _, sus, _ = leaked()
    c = ctx()
    c.enable_timing(True)
    try:
        c.reset_timing()
        dev_find(base, sus, -10, 10)
        t = c.timing()
    finally:
        c.enable_timing(False)
    assert t["locate"]["launches"] >= 1 and t["locate"]["work"] > 0
    assert t["locate_coarse"]["launches"] == 1 and t["locate_coarse"]["work"] == 3 * 81 * (640 // 4) * (444 // 4)      # the ladder, nested
    assert all(v["launches"] == 0 for k, v in t.items() if k not in ("locate", "locate_coarse")), t


def test_cli_records_carry_turned(tmp_path):
    """fingerprint two copies of the cat, turn them with Pillow, trace them with --place FILE=rotate:? and its kin"""
    Image.fromarray(cat()).save(tmp_path / "base.png")
    assert cli.main(["fingerprint", str(tmp_path / "base.png"), "--copies", "2", "-d", "copy"]) == 0
    copies = [np.asarray(Image.open(tmp_path / f"base_fp{i}.png").convert("RGB")) for i in range(2)]
    names = [str(tmp_path / f"leak{i}.png") for i in range(3)]
    for name, (c, a) in zip(names, ((0, 1.0), (1, -2.5), (0, 0.6875))):
        Image.fromarray(turned(copies[c], a)).save(name)
    out = io.StringIO()
    args = cli.build_parser().parse_args(["trace", str(tmp_path / "base.png"), "--suspects", *names, "--marks", str(tmp_path / "base_fp.json"),
                                          "--place", f"{names[0]}=rotate:?", "--place", f"{names[1]}=rotate:-4..0", "--place", f"{names[2]}=rotate:0.6875"])
    assert cli.cmd_trace(args, out) == 0
    text = out.getvalue()
    assert text.count("  Turned: ") == 2 and text.count("  Matches: true") == 3, text
    assert '  Turned: "1 (mean luma difference ' in text and '  Turned: "-2.5 (mean luma difference ' in text, text
    assert text.count("turned back by the angle found") == 2 and "turned back by 0.6875 degrees" in text, text
    assert [ln for ln in text.splitlines() if ln.startswith("  Description")] == ['  Description: "copy #0"', '  Description: "copy #1"', '  Description: "copy #0"'], text


# ---- errors ------------------------------------------------------------------------------------------------------------------
def test_errors():
    z = np.zeros((40, 40, 3), np.uint8)
    b, d = Dev(z), Dev(z[None])
    found, h = (L.AngleFound * 1)(), ctx().handle
    f = lib().ssw_find_angle_rgb8
    try:
        assert f(h, b.ptr, d.ptr, 1, 31, 40, -1.0, 1.0, found, None) == L.SSW_ERR_BAD_DIMS
        assert f(h, b.ptr, d.ptr, 1, 40, 31, -1.0, 1.0, found, None) == L.SSW_ERR_BAD_DIMS
        assert f(h, b.ptr, d.ptr, 1, 40, 40, 1.0, -1.0, found, None) == L.SSW_ERR_BAD_ARG
        assert f(h, b.ptr, d.ptr, 1, 40, 40, -45.5, 1.0, found, None) == L.SSW_ERR_BAD_ARG
        assert f(h, b.ptr, d.ptr, 1, 40, 40, 0.0, 45.25, found, None) == L.SSW_ERR_BAD_ARG
        assert f(h, b.ptr, d.ptr, 1, 40, 40, float("nan"), 1.0, found, None) == L.SSW_ERR_BAD_ARG
        assert f(h, b.ptr, d.ptr, 1, 40, 40, 0.0, float("inf"), found, None) == L.SSW_ERR_BAD_ARG
        assert f(h, None, d.ptr, 1, 40, 40, -1.0, 1.0, found, None) == L.SSW_ERR_BAD_ARG
        assert f(h, b.ptr, None, 1, 40, 40, -1.0, 1.0, found, None) == L.SSW_ERR_BAD_ARG
        assert f(h, b.ptr, d.ptr, 1, 40, 40, -1.0, 1.0, None, None) == L.SSW_ERR_BAD_ARG
        assert f(None, b.ptr, d.ptr, 1, 40, 40, -1.0, 1.0, found, None) == L.SSW_ERR_BAD_ARG
        assert f(h, b.ptr, d.ptr, 1, 1 << 14, (1 << 13) + 1, -1.0, 1.0, found, None) == L.SSW_ERR_UNSUPPORTED
        assert f(h, None, None, 0, 0, 0, 5.0, -5.0, None, None) == L.SSW_OK                 # n == 0 is checked first
        assert f(h, b.ptr, d.ptr, 1, 40, 40, -1.0, 1.0, found, None) == L.SSW_OK and found[0].n_rungs == 9 and found[0].sad == 0
    finally:
        b.free(); d.free()
