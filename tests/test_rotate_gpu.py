"""ssw_affine_rgb8, ssw_rotate_attack_rgb8 and ssw_unrotate_rgb8 on the device against `affine_ref` and `unrotate_ref`, the numpy
restatements of tests/test_rotate_cpu.py (themselves checked there against Pillow byte for byte): every comparison is
np.array_equal or equality of float32 bits, there is no tolerance.  Shapes are the smallest at which the kernels can go wrong: a
single pixel, a single row and a single column, odd sides, every width from 61 to 68 (row bytes modulo 4, the edge of a 32-pixel
tile), more than one tile in both axes, two strips that cross many tiles in one axis, matrices whose box of source pixels fits
the LDS and matrices at which it does not, a device pointer one byte off, more jobs than one workspace group."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest
from PIL import Image

import gpu_util as G
from conftest import ROOT
from gpu_util import ctx, lib
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd import api, cli
from spread_spectrum_watermarking_amd._lib import check
from test_rotate_cpu import (ANGLES, BICUBIC, BILINEAR, BLACK, IDENTITY, MAGENTA, NAMES, SHEAR_MILD, affine_ref, cat, general_matrices, noise,
                             pil_rotate, rotate_ref, rotation_matrix_ref, small_frames, unrotate_mask_ref, unrotate_ref)

pytestmark = pytest.mark.gpu

LIBDIR = os.path.join(ROOT, "spread_spectrum_watermarking_amd", "lib")
SENTINEL = 0xA5


class Dev:
    """Device memory holding `data` (an array, or a number of bytes filled with SENTINEL) `off` bytes into its allocation."""

    def __init__(self, data, off=0):
        a = np.full(data, SENTINEL, np.uint8) if isinstance(data, int) else np.ascontiguousarray(data)
        self.buf, self.off, self.nbytes = ctx().alloc(a.nbytes + off + 16), off, a.nbytes
        if a.nbytes:
            check(lib().ssw_copy_to_dev(ctx().handle, self.ptr, a.ctypes.data, a.nbytes), "ssw_copy_to_dev")

    @property
    def ptr(self):
        return C.c_void_p(self.buf.ptr.value + self.off)

    def host(self, dtype, shape):
        out = np.empty(shape, dtype)
        if out.nbytes:
            check(lib().ssw_copy_to_host(ctx().handle, out.ctypes.data, self.ptr, out.nbytes), "ssw_copy_to_host")
        return out

    def free(self):
        self.buf.free()


def c_matrix(m):
    return (C.c_double * 6)(*m)


def dev_affine(frames, size, m, filt, fill=BLACK, off_in=0, off_out=0):
    """frames [n, h, w, 3] -> [n, oh, ow, 3]; checks the SENTINEL byte behind the last frame and that the input is unchanged."""
    n, h, w, _ = frames.shape
    ow, oh = size
    d, o = Dev(frames, off_in), Dev(n * oh * ow * 3 + 1, off_out)
    check(lib().ssw_affine_rgb8(ctx().handle, d.ptr, n, w, h, ow, oh, c_matrix(m), filt, (C.c_uint8 * 3)(*fill), o.ptr), "ssw_affine_rgb8")
    out = o.host(np.uint8, (n * oh * ow * 3 + 1,))
    assert np.array_equal(d.host(np.uint8, frames.shape), frames), "the call changed its input"
    d.free(); o.free()
    assert out[-1] == SENTINEL, "a byte behind the last frame was written"
    return out[:-1].reshape(n, oh, ow, 3)


def lds_form(w, h, m):
    form, bw, bh = C.c_int(-1), C.c_uint32(), C.c_uint32()
    check(lib().ssw_affine_plan(w, h, c_matrix(m), C.byref(form), C.byref(bw), C.byref(bh)), "ssw_affine_plan")
    assert form.value in (0, 1) and 1 <= bw.value <= w and 1 <= bh.value <= h
    return form.value == 1


def job(frame, angle, filt, fill, w, h):
    return L.RotateJob(frame, filt, (C.c_uint8 * 4)(*fill, 0), c_matrix(rotation_matrix_ref(angle, w, h)), c_matrix(rotation_matrix_ref(-angle, w, h)))


def jobs_c(jobs, w, h):
    """jobs: (frame, angle, filter, fill)"""
    return (L.RotateJob * max(len(jobs), 1))(*[job(*j, w, h) for j in jobs])


def dev_rotate_attack(base, frames, jobs, extra=0):
    n, h, w, _ = frames.shape
    b, d, o = Dev(base), Dev(frames), Dev((len(jobs) + extra) * h * w * 3)
    check(lib().ssw_rotate_attack_rgb8(ctx().handle, b.ptr, d.ptr, n, w, h, jobs_c(jobs, w, h), len(jobs), o.ptr), "ssw_rotate_attack_rgb8")
    out = o.host(np.uint8, (len(jobs) + extra, h, w, 3))
    assert np.array_equal(d.host(np.uint8, frames.shape), frames) and np.array_equal(b.host(np.uint8, base.shape), base), "the call changed its input"
    b.free(); d.free(); o.free()
    return out


def dev_unrotate(base, suspects, jobs):
    """jobs: (suspect, angle)"""
    n, h, w, _ = suspects.shape
    b, d, o = Dev(base), Dev(suspects), Dev(n * h * w * 3 + 1)
    cj = jobs_c([(s, a, 7, (9, 9, 9)) for s, a in jobs], w, h)                    # filter and fill are not read
    check(lib().ssw_unrotate_rgb8(ctx().handle, b.ptr, d.ptr, n, w, h, cj, o.ptr), "ssw_unrotate_rgb8")
    out = o.host(np.uint8, (n * h * w * 3 + 1,))
    b.free(); d.free(); o.free()
    assert out[-1] == SENTINEL
    return out[:-1].reshape(n, h, w, 3)


def original_of(frame):
    return (255 - frame)[::-1].copy()


# ---- the transform -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,frame", small_frames(), ids=lambda v: v if isinstance(v, str) else "")
def test_rotations_equal_the_restatement(name, frame):
    h, w = frame.shape[:2]
    for angle in ANGLES:
        for filt in (BILINEAR, BICUBIC):
            for fill in (BLACK, MAGENTA):
                got = dev_affine(frame[None], (w, h), rotation_matrix_ref(angle, w, h), filt, fill)[0]
                assert np.array_equal(got, rotate_ref(frame, angle, filt, fill)), (name, angle, NAMES[filt], fill)


@pytest.mark.parametrize("w,h", [(128, 72), (53, 37), (131, 75)])
def test_general_matrices_equal_the_restatement(w, h):
    frame = noise(w, h, 3)
    for name, m, size in general_matrices(w, h) + [("mild shear", SHEAR_MILD, (w, h))]:
        for filt in (BILINEAR, BICUBIC):
            got = dev_affine(frame[None], size, m, filt, MAGENTA)[0]
            assert np.array_equal(got, affine_ref(frame, size, m, filt, MAGENTA)), (name, NAMES[filt])


def test_a_batch_of_three_one_byte_off():
    w, h = 53, 37
    frames = np.stack([noise(w, h, s) for s in (1, 2, 3)])
    for angle, filt in ((1, BICUBIC), (30, BILINEAR), (-7.5, BICUBIC)):
        m = rotation_matrix_ref(angle, w, h)
        want = np.stack([affine_ref(f, (w, h), m, filt, MAGENTA) for f in frames])
        for off_in, off_out in ((1, 0), (0, 1), (1, 1), (3, 2)):
            assert np.array_equal(dev_affine(frames, (w, h), m, filt, MAGENTA, off_in, off_out), want), (angle, off_in, off_out)


@pytest.mark.parametrize("w", range(61, 69))
def test_every_width_modulo_four_and_the_tile_edge(w):
    h = 19
    frames = np.stack([noise(w, h, 5), noise(w, h, 6)])
    for angle in (1, 30):
        for filt in (BILINEAR, BICUBIC):
            m = rotation_matrix_ref(angle, w, h)
            got = dev_affine(frames, (w, h), m, filt, MAGENTA)
            for i in range(2):
                assert np.array_equal(got[i], affine_ref(frames[i], (w, h), m, filt, MAGENTA)), (w, angle, NAMES[filt], i)
    # the same widths as the output's of another size
    m = [0.9, 0.1, 0.25, -0.1, 0.9, 2.0]
    got = dev_affine(noise(40, 23, 7)[None], (w, 11), m, BICUBIC)[0]
    assert np.array_equal(got, affine_ref(noise(40, 23, 7), (w, 11), m, BICUBIC))


@pytest.mark.parametrize("w,h", [(1024, 16), (16, 1024)])
def test_strips_that_cross_many_tiles(w, h):
    frame = noise(w, h, 9)
    for angle, filt in ((1, BICUBIC), (45, BILINEAR), (90.5, BICUBIC)):
        got = dev_affine(frame[None], (w, h), rotation_matrix_ref(angle, w, h), filt)[0]
        assert np.array_equal(got, rotate_ref(frame, angle, filt)), (angle, NAMES[filt])


def test_the_global_form_where_the_box_does_not_fit():
    w, h = 197, 131
    frame = noise(w, h)
    (_, shrink, small), _, (_, shear, _) = general_matrices(w, h)
    assert not lds_form(w, h, shrink) and not lds_form(w, h, shear)
    assert all(lds_form(w, h, rotation_matrix_ref(a, w, h)) for a in ANGLES) and lds_form(w, h, SHEAR_MILD)
    assert not lds_form(1024, 16, [1.0, 60.0, 0.0, 0.0, 1.0, 0.0]) and lds_form(1024, 16, rotation_matrix_ref(45, 1024, 16))
    for m, size in ((shrink, small), (shear, (w, h)), (SHEAR_MILD, (w, h))):
        for filt in (BILINEAR, BICUBIC):
            got = dev_affine(np.stack([frame, frame[::-1]]), size, m, filt, MAGENTA)
            assert np.array_equal(got[0], affine_ref(frame, size, m, filt, MAGENTA)), (m, NAMES[filt])
            assert np.array_equal(got[1], affine_ref(frame[::-1], size, m, filt, MAGENTA)), (m, NAMES[filt])


# ---- the attack --------------------------------------------------------------------------------------------------------------
def attack_ref(base, frames, f, angle, filt, memo):
    key = (f, angle, filt)
    if key not in memo:
        memo[key] = unrotate_ref(base, rotate_ref(frames[f], angle, filt, MAGENTA), angle)
    return memo[key]


def test_attack_jobs_in_mixed_order_with_repeats_both_filters_and_two_fills():
    w, h = 53, 37
    frames = np.stack([noise(w, h, s) for s in range(4)])
    base = original_of(frames[0])
    kinds = [(0.25, BICUBIC, BLACK), (0.25, BICUBIC, MAGENTA), (30, BILINEAR, BLACK), (30, BILINEAR, MAGENTA), (-7.5, BICUBIC, BLACK), (0, BICUBIC, BLACK),
             (180.3, BILINEAR, MAGENTA), (90, BICUBIC, BLACK)]
    rng = np.random.default_rng(5)
    jobs = [(int(rng.integers(0, 4)),) + kinds[int(rng.integers(0, len(kinds)))] for _ in range(24)]
    jobs[3], jobs[4], jobs[5] = (3,) + kinds[0], (3,) + kinds[0], (1,) + kinds[0]           # a batch of three, a frame twice in it
    jobs[10], jobs[11] = (2,) + kinds[0], (2,) + kinds[1]                                    # the two fills: equal output
    jobs[20], jobs[23] = (1,) + kinds[5], (3,) + kinds[0]                                    # angle 0; a repeat far apart
    out = dev_rotate_attack(base, frames, jobs, extra=1)
    memo = {}
    for i, (f, angle, filt, _) in enumerate(jobs):
        assert np.array_equal(out[i], attack_ref(base, frames, f, angle, filt, memo)), (i, jobs[i])
    assert np.array_equal(out[10], out[11]) and np.array_equal(out[20], frames[1])           # angle 0 gives back the copy unchanged
    assert np.all(out[24] == SENTINEL)
    for i in (0, 4, 23):                                                                     # alone = inside the batch
        assert np.array_equal(dev_rotate_attack(base, frames, [jobs[i]])[0], out[i]), i


def test_forty_jobs_are_more_than_one_workspace_group():
    w, h = 197, 131
    frames = np.stack([noise(w, h, s) for s in range(3)])
    base = original_of(frames[1])
    jobs = [(i % 3, 1.0, BICUBIC, BLACK) for i in range(40)]                                 # one batch: groups of 32 and 8
    out = dev_rotate_attack(base, frames, jobs, extra=1)
    memo = {}
    for i in range(40):
        assert np.array_equal(out[i], attack_ref(base, frames, i % 3, 1.0, BICUBIC, memo)), i
    assert np.all(out[40] == SENTINEL)
    mask = unrotate_mask_ref(w, h, 1.0)
    assert np.array_equal(out[0][~mask], base[~mask]) and 0.9 < mask.mean() < 1.0


# ---- the undoing -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(53, 37), (40, 9), (197, 131), (64, 33)])
def test_undoing_what_pillow_rotated(w, h):
    frame = noise(w, h, 4)
    base = original_of(frame)
    cases = [(a, f) for a in (0.25, 1, 2, 5, -7.5, 30, 45, 90.5, 180.3, 0) for f in (BILINEAR, BICUBIC)]
    suspects = np.stack([pil_rotate(frame, a, f, MAGENTA) for a, f in cases])
    jobs = [(i, a) for i, (a, _) in enumerate(cases)]
    order = list(reversed(jobs))                                                             # suspects in another order than the results
    got = dev_unrotate(base, suspects, order)
    for (s, a), g in zip(order, got):
        assert np.array_equal(g, unrotate_ref(base, suspects[s], a)), (a, cases[s])
    assert np.array_equal(got[0], suspects[len(cases) - 1]) and np.array_equal(got[1], suspects[len(cases) - 2])      # angle 0


def test_the_kept_share_is_counted_on_the_device():
    kept, hd = lib().ssw_unrotate_kept, ctx().handle
    for w, h in ((53, 37), (40, 9), (7, 1), (197, 131), (640, 444), (1024, 16)):
        angles = [0.25, 1, -7.5, 30, 45, 90.5, 180.3, 0]
        counts = np.full(len(angles) + 1, 77, np.uint64)
        check(kept(hd, w, h, jobs_c([(5, a, 9, BLACK) for a in angles], w, h), len(angles), counts.ctypes.data), "ssw_unrotate_kept")
        assert counts.tolist() == [int(unrotate_mask_ref(w, h, a).sum()) for a in angles[:-1]] + [w * h, 77], (w, h)
    assert api._kept_shares(ctx(), [api.Rotate(1.0), api.Rotate(30, "bilinear")], 640, 444) == [api.Rotate(1.0).kept(640, 444), api.Rotate(30).kept(640, 444)]
    one, good = np.zeros(1, np.uint64), jobs_c([(0, 1.0, BICUBIC, BLACK)], 16, 8)
    assert kept(hd, 16, 8, None, 0, None) == L.SSW_OK and kept(None, 16, 8, good, 1, one.ctypes.data) == L.SSW_ERR_BAD_ARG
    assert kept(hd, 16, 8, None, 1, one.ctypes.data) == L.SSW_ERR_BAD_ARG and kept(hd, 16, 8, good, 1, None) == L.SSW_ERR_BAD_ARG
    assert kept(hd, 0, 8, good, 1, one.ctypes.data) == L.SSW_ERR_BAD_DIMS and kept(hd, 16, 65536, good, 1, one.ctypes.data) == L.SSW_ERR_BAD_DIMS
    good[0].back[3] = float("nan")
    assert kept(hd, 16, 8, good, 1, one.ctypes.data) == L.SSW_ERR_BAD_ARG


# ---- status codes ------------------------------------------------------------------------------------------------------------
def test_status_codes_and_nothing_enqueued():
    af, ra, ur, hd = lib().ssw_affine_rgb8, lib().ssw_rotate_attack_rgb8, lib().ssw_unrotate_rgb8, ctx().handle
    w, h = 16, 8
    fb = w * h * 3
    frames = np.stack([noise(w, h, s) for s in range(3)])
    base = original_of(frames[0])
    b, d, o = Dev(base), Dev(frames), Dev(3 * fb)
    untouched = lambda: np.all(o.host(np.uint8, (3 * fb,)) == SENTINEL)
    m, fill = c_matrix(rotation_matrix_ref(1.0, w, h)), (C.c_uint8 * 3)(1, 2, 3)
    good = jobs_c([(0, 1.0, BICUBIC, BLACK), (2, 30, BILINEAR, MAGENTA)], w, h)
    # nothing to do comes first
    assert af(hd, None, 0, 0, 0, 0, 0, None, 99, None, None) == L.SSW_OK
    assert ra(hd, None, None, 0, 0, 0, None, 0, None) == L.SSW_OK and ur(hd, None, None, 0, 0, 0, None, None) == L.SSW_OK
    assert ra(hd, b.ptr, d.ptr, 3, w, h, good, 0, o.ptr) == L.SSW_OK
    # a null pointer
    assert af(None, d.ptr, 2, w, h, w, h, m, BICUBIC, fill, o.ptr) == L.SSW_ERR_BAD_ARG
    for args in ((None, 2, w, h, w, h, m, BICUBIC, fill, o.ptr), (d.ptr, 2, w, h, w, h, None, BICUBIC, fill, o.ptr),
                 (d.ptr, 2, w, h, w, h, m, BICUBIC, None, o.ptr), (d.ptr, 2, w, h, w, h, m, BICUBIC, fill, None)):
        assert af(hd, *args) == L.SSW_ERR_BAD_ARG
    assert ra(None, b.ptr, d.ptr, 3, w, h, good, 2, o.ptr) == L.SSW_ERR_BAD_ARG
    for args in ((None, d.ptr, 3, w, h, good, 2, o.ptr), (b.ptr, None, 3, w, h, good, 2, o.ptr), (b.ptr, d.ptr, 3, w, h, None, 2, o.ptr),
                 (b.ptr, d.ptr, 3, w, h, good, 2, None)):
        assert ra(hd, *args) == L.SSW_ERR_BAD_ARG
    assert ur(None, b.ptr, d.ptr, 2, w, h, good, o.ptr) == L.SSW_ERR_BAD_ARG
    for args in ((None, d.ptr, 2, w, h, good, o.ptr), (b.ptr, None, 2, w, h, good, o.ptr), (b.ptr, d.ptr, 2, w, h, None, o.ptr),
                 (b.ptr, d.ptr, 2, w, h, good, None)):
        assert ur(hd, *args) == L.SSW_ERR_BAD_ARG
    # an unknown filter
    for bad in (2, -1):
        assert af(hd, d.ptr, 2, w, h, w, h, m, bad, fill, o.ptr) == L.SSW_ERR_BAD_ARG, bad
    for bad in (2, 0xFFFFFFFF):
        assert ra(hd, b.ptr, d.ptr, 3, w, h, jobs_c([(0, 1.0, BICUBIC, BLACK), (1, 1.0, bad, BLACK)], w, h), 2, o.ptr) == L.SSW_ERR_BAD_ARG, bad
    # frame >= n_frames, behind a good job
    for bad in (3, 0xFFFFFFFF):
        assert ra(hd, b.ptr, d.ptr, 3, w, h, jobs_c([(0, 1.0, BICUBIC, BLACK), (bad, 1.0, BICUBIC, BLACK)], w, h), 2, o.ptr) == L.SSW_ERR_BAD_ARG, bad
    assert ra(hd, b.ptr, d.ptr, 2, w, h, good, 2, o.ptr) == L.SSW_ERR_BAD_ARG                # frame 2 of 2 frames
    assert ur(hd, b.ptr, d.ptr, 2, w, h, good, o.ptr) == L.SSW_ERR_BAD_ARG                   # suspect 2 of 2 suspects
    # a matrix entry that is not finite
    for k in range(6):
        for v in (float("nan"), float("inf"), -float("inf")):
            bad_m = rotation_matrix_ref(1.0, w, h)
            bad_m[k] = v
            assert af(hd, d.ptr, 2, w, h, w, h, c_matrix(bad_m), BICUBIC, fill, o.ptr) == L.SSW_ERR_BAD_ARG, (k, v)
            for field in ("forward", "back"):
                js = jobs_c([(0, 1.0, BICUBIC, BLACK), (1, 1.0, BICUBIC, BLACK)], w, h)
                getattr(js[1], field)[k] = v
                assert ra(hd, b.ptr, d.ptr, 3, w, h, js, 2, o.ptr) == L.SSW_ERR_BAD_ARG, (field, k, v)
                assert ur(hd, b.ptr, d.ptr, 2, w, h, js, o.ptr) == L.SSW_ERR_BAD_ARG, (field, k, v)
    # outputs that overlap inputs
    inside = C.c_void_p(d.ptr.value + fb)
    assert af(hd, d.ptr, 3, w, h, w, h, m, BICUBIC, fill, inside) == L.SSW_ERR_BAD_ARG
    assert af(hd, d.ptr, 3, w, h, w, h, m, BICUBIC, fill, d.ptr) == L.SSW_ERR_BAD_ARG
    assert ra(hd, b.ptr, d.ptr, 3, w, h, good, 2, inside) == L.SSW_ERR_BAD_ARG and ra(hd, b.ptr, d.ptr, 3, w, h, good, 2, b.ptr) == L.SSW_ERR_BAD_ARG
    two = jobs_c([(0, 1.0, BICUBIC, BLACK), (1, 30, BICUBIC, BLACK)], w, h)
    assert ur(hd, b.ptr, d.ptr, 2, w, h, two, inside) == L.SSW_ERR_BAD_ARG and ur(hd, b.ptr, d.ptr, 2, w, h, two, b.ptr) == L.SSW_ERR_BAD_ARG
    ctx().synchronize()
    assert np.array_equal(d.host(np.uint8, frames.shape), frames) and np.array_equal(b.host(np.uint8, base.shape), base)
    # a side of 0 or above 65535
    for ww, hh, ow, oh in ((0, 8, 8, 4), (16, 0, 8, 4), (16, 8, 0, 4), (16, 8, 8, 0), (65536, 8, 8, 4), (16, 65536, 8, 4), (16, 8, 65536, 4), (16, 8, 8, 65536)):
        assert af(hd, d.ptr, 2, ww, hh, ow, oh, m, BICUBIC, fill, o.ptr) == L.SSW_ERR_BAD_DIMS, (ww, hh, ow, oh)
    for ww, hh in ((0, 8), (16, 0), (65536, 8), (16, 65536)):
        assert ra(hd, b.ptr, d.ptr, 3, ww, hh, good, 2, o.ptr) == L.SSW_ERR_BAD_DIMS and ur(hd, b.ptr, d.ptr, 2, ww, hh, two, o.ptr) == L.SSW_ERR_BAD_DIMS
    ctx().synchronize()
    assert untouched()
    # ... and the good calls do run
    assert ra(hd, b.ptr, d.ptr, 3, w, h, good, 2, o.ptr) == L.SSW_OK
    got = o.host(np.uint8, (3, h, w, 3))
    assert np.array_equal(got[0], unrotate_ref(base, rotate_ref(frames[0], 1.0, BICUBIC), 1.0))
    assert np.array_equal(got[1], unrotate_ref(base, rotate_ref(frames[2], 30, BILINEAR), 30)) and np.all(got[2] == SENTINEL)
    m6, form = c_matrix(IDENTITY), C.c_int()
    assert lib().ssw_affine_plan(w, h, None, C.byref(form), None, None) == L.SSW_ERR_BAD_ARG and lib().ssw_affine_plan(0, h, m6, C.byref(form), None, None) == L.SSW_ERR_BAD_DIMS
    assert lib().ssw_affine_plan(w, h, m6, C.byref(form), None, None) == L.SSW_OK and form.value == 1
    assert lib().ssw_rotation_matrix(1.0, w, h, None) == L.SSW_ERR_BAD_ARG and lib().ssw_rotation_matrix(float("nan"), w, h, m6) == L.SSW_ERR_BAD_ARG
    assert lib().ssw_rotation_matrix(1.0, w, h, m6) == L.SSW_OK and list(m6) == rotation_matrix_ref(1.0, w, h)
    b.free(); d.free(); o.free()


# ---- timing ------------------------------------------------------------------------------------------------------------------
def test_timed_as_convert_and_resize_with_the_stated_bytes():
    w, h = 57, 41
    frames = np.stack([noise(w, h, s) for s in range(3)])
    base = original_of(frames[0])
    c = ctx()
    c.enable_timing(True)
    try:
        c.reset_timing()
        dev_affine(frames, (20, 30), [2.0, 0.0, 0.0, 0.0, 1.0, 0.0], BICUBIC)
        t = c.timing()
        assert t["convert"]["launches"] >= 1 and t["convert"]["work"] == 3 * (3 * w * h + 3 * 20 * 30)
        assert all(v["launches"] == 0 for k, v in t.items() if k != "convert")
        c.reset_timing()
        dev_rotate_attack(base, frames, [(0, 1.0, BICUBIC, BLACK), (2, 1.0, BICUBIC, BLACK), (1, 30, BILINEAR, BLACK)])
        t = c.timing()
        assert t["convert"]["work"] == 3 * 6 * w * h and t["resize"]["work"] == 3 * 6 * w * h
        assert all(v["launches"] == 0 for k, v in t.items() if k not in ("convert", "resize"))
        c.reset_timing()
        dev_unrotate(base, frames, [(0, 1.0), (1, 1.0), (2, 2.0)])
        t = c.timing()
        assert t["resize"]["work"] == 3 * 6 * w * h and all(v["launches"] == 0 for k, v in t.items() if k != "resize")
    finally:
        c.enable_timing(False)


# ---- the Python wrappers -----------------------------------------------------------------------------------------------------
def test_python_wrappers_in_one_group_and_in_many(monkeypatch):
    w, h = 40, 24
    images = [noise(w, h, 20 + i) for i in range(4)]
    base = original_of(images[0])
    rotations = [api.Rotate(0.5), api.Rotate(30, "bilinear"), api.Rotate(0)]
    want = [[unrotate_ref(base, rotate_ref(im, r.angle, L.AFFINE_FILTERS[r.filter]), r.angle) for r in rotations] for im in images]
    turned = [rotate_ref(im, 5, BILINEAR, MAGENTA) for im in images]
    small = [affine_ref(im, (13, 7), [3.0, 0.0, 0.5, 0.0, 3.0, 0.25], BICUBIC) for im in images]
    undone = [unrotate_ref(base, t, 5) for t in turned]
    for cap in (api.UPLOAD_GROUP_BYTES, 5 * h * w * 3, 1):                                   # one group | frames and jobs split | a job a group
        monkeypatch.setattr(api, "UPLOAD_GROUP_BYTES", cap)
        got = api.rotate_attack(base, images, rotations, ctx())
        assert len(got) == 4 and all(len(g) == 3 for g in got)
        for i in range(4):
            for j in range(3):
                assert np.array_equal(got[i][j], want[i][j]), (cap, i, j)
        assert all(np.array_equal(a, b) for a, b in zip(api.rotate(images, 5, "bilinear", MAGENTA, ctx()), turned)), cap
        assert all(np.array_equal(a, b) for a, b in zip(api.affine(images, (13, 7), [3.0, 0.0, 0.5, 0.0, 3.0, 0.25], ctx=ctx()), small)), cap
        assert all(np.array_equal(a, b) for a, b in zip(api.unrotate(base, turned, [5] * 4, ctx()), undone)), cap
    assert np.array_equal(want[1][2], images[1])
    with pytest.raises(ValueError):
        api.trace_many(base, [np.zeros((h, w, 4), np.uint8)], [np.zeros(4, np.float32)], ctx=ctx(), placements=[api.Rotated(1.0)])
    with pytest.raises(ValueError):
        api.trace_many(base, [np.zeros((h, w + 1, 3), np.uint8)], [np.zeros(4, np.float32)], ctx=ctx(), placements=[api.Rotated(1.0)])


# ---- the report --------------------------------------------------------------------------------------------------------------
def same(a, b):
    return a == b or (a != a and b != b)


def test_strength_report_equals_the_chain_through_the_host():
    """Field for field against mark_copies_rgb8 -> api.rotate_attack -> trace_many -> api.quality -> api.ssim."""
    image = cat()
    alphas, n, k = [0.02, 0.1], 3, 200
    rotations = [api.Rotate(0.5), api.Rotate(2, "bilinear")]
    c = ctx()
    rows = api.strength_report(image, alphas, copies=n, k=k, sizes=(2,), rotations=rotations, ssim=True, seed=3, ctx=c)
    plain = api.strength_report(image, alphas, copies=n, k=k, sizes=(2,), ssim=True, seed=3, ctx=c)
    marks = np.random.default_rng(3).standard_normal((n, k)).astype(np.float32)
    for r, p in zip(rows, plain):
        assert (r.alpha, r.quality, r.collusions, r.jpeg, r.ssim, r.filters, r.scales) == (p.alpha, p.quality, p.collusions, p.jpeg, p.ssim, p.filters, p.scales)
        assert p.rotations == []
        copies = api.Writer(image, api.WriteConfig(insertion=api.Insertion.Option2(r.alpha)), c).mark_copies_rgb8(list(marks))
        per_copy = api.rotate_attack(image, list(copies), rotations, c)
        attacked = [per_copy[i][j] for j in range(len(rotations)) for i in range(n)]
        traced = api.trace_many(image, attacked, list(marks), threshold=6.0, config=api.ReadConfig(extraction=api.Extraction.Option2(r.alpha)), ctx=c)
        quality, ssims = api.quality(image, attacked, c), api.ssim(image, attacked, c)
        assert [j.rotation for j in r.rotations] == ["rotate 0.5 bicubic", "rotate 2 bilinear"]
        assert [j.kept for j in r.rotations] == [unrotate_mask_ref(640, 444, a).mean() for a in (0.5, 2)]
        for i, j in enumerate(r.rotations):
            sims = np.asarray(traced.sims[i * n:(i + 1) * n])
            own, others = np.diagonal(sims), sims[~np.eye(n, dtype=bool)]
            psnr = [q.psnr for q in quality[i * n:(i + 1) * n]]
            mean = [s.mean for s in ssims[i * n:(i + 1) * n]]
            print(f"alpha {r.alpha}: {j}")
            assert same(j.weakest_own, float(own.min())) and same(j.strongest_innocent, float(others.max())), (r.alpha, j)
            assert j.survived == int((own > np.float32(6.0)).sum()) and j.accused == int((others > np.float32(6.0)).sum()), (r.alpha, j)
            assert (j.psnr_min, j.psnr_max) == (min(psnr), max(psnr)), (r.alpha, j)
            assert (j.ssim_min, j.ssim_max) == (min(mean), max(mean)), (r.alpha, j)


def test_the_report_says_what_trace_finds_in_a_copy_pillow_rotated():
    """The claim the feature makes: for alpha 0.1 and Rotate(1.0), copy c turned by PIL.Image.rotate(1.0, BICUBIC) itself and handed
    to trace_many with Rotated(1.0) has the similarities of row c of the report's matrix -- exactly, in float32 bits."""
    image = cat()
    n, k, alpha = 3, 1000, 0.1
    c = ctx()
    marks = np.random.default_rng(3).standard_normal((n, k)).astype(np.float32)
    copies = api.Writer(image, api.WriteConfig(insertion=api.Insertion.Option2(alpha)), c).mark_copies_rgb8(list(marks))
    # the report's matrix: the report keeps only its folds, so the same device chain is run here on the copies
    attacked = [a[0] for a in api.rotate_attack(image, list(copies), [api.Rotate(1.0)], c)]
    cfg = api.ReadConfig(extraction=api.Extraction.Option2(alpha))
    matrix = np.asarray(api.trace_many(image, attacked, list(marks), threshold=6.0, config=cfg, ctx=c).sims, np.float32)
    row = api.strength_report(image, [alpha], copies=n, k=k, sizes=(2,), rotations=[api.Rotate(1.0)], seed=3, ctx=c)[0].rotations[0]
    own, others = np.diagonal(matrix), matrix[~np.eye(n, dtype=bool)]
    assert row.weakest_own == float(own.min()) and row.strongest_innocent == float(others.max()) and row.kept == 278328 / (640 * 444)
    turned = [np.asarray(Image.fromarray(copies[i]).rotate(1.0, resample=Image.BICUBIC)) for i in range(n)]
    for i in range(n):
        sims = np.asarray(api.trace_many(image, [turned[i]], list(marks), threshold=6.0, config=cfg, ctx=c, placements=[api.Rotated(1.0)]).sims, np.float32)[0]
        print(f"copy {i}: turned by Pillow {sims.tolist()} report {matrix[i].tolist()}")
        assert sims.tobytes() == matrix[i].tobytes(), i
    # a reader's trace, and a call that mixes a turned copy with one that is not
    reader = api.Reader.base(image, cfg, c)
    both = reader.trace([turned[1], copies[2]], list(marks), placements=[api.Rotated(1.0), None], base=image)
    assert np.asarray(both.sims, np.float32)[0].tobytes() == matrix[1].tobytes()
    print(f"report row: {row}")


def test_cli_strength_prints_the_rotation_rows_and_trace_turns_back(tmp_path, capsys):
    image = cat()
    path = str(tmp_path / "cat.png")
    Image.fromarray(image).save(path)
    args = ["strength", path, "--alpha", "0.1", "--copies", "3", "--collude", "2", "--method", "average", "-n", "200", "--rotate", "0.5", "2:bilinear", "-1"]
    assert cli.main(args) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[3].startswith("  average of 2: found 2/2") and len(lines) == 7
    row = r"  %s: own mark found \d/3, weakest -?\d+\.\d, strongest innocent -?\d+\.\d(, \d innocent accused)?, \d\d\.\d \.\. \d\d\.\d dB, \d\d\.\d %% kept"
    for line, label in zip(lines[4:], ("rotate 0.5 bicubic", "rotate 2 bilinear", "rotate -1 bicubic")):
        assert re.fullmatch(row % re.escape(label), line), line
    assert lines[6].endswith(", 97.9 % kept")
    assert cli.main(args + ["--json"]) == 0
    doc = json.loads(capsys.readouterr().out)
    assert [s["rotation"] for s in doc[0]["rotations"]] == ["rotate 0.5 bicubic", "rotate 2 bilinear", "rotate -1 bicubic"]
    assert sorted(doc[0]["rotations"][0]) == ["accused", "kept", "psnr_max", "psnr_min", "rotation", "strongest_innocent", "survived", "weakest_own"]
    assert doc[0]["rotations"][2]["kept"] == 278328 / (640 * 444) and "scales" not in doc[0]
    assert cli.parse_place("leak.png=rotate:1.5") == ("leak.png", api.Rotated(1.5)) and cli.parse_place("a=b.png=3,4")[1] == api.Placement(3, 4)
    with pytest.raises(ValueError):
        cli.parse_place("leak.png=rotate:much")


# ---- the C++ wrappers --------------------------------------------------------------------------------------------------------
def test_cpp_wrappers_equal_the_c_calls(tmp_path):
    exe = str(tmp_path / "rotate_wrappers_test")
    done = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "rotate_wrappers_test.cpp"), "-o", exe,
                           "-L", LIBDIR, "-lssw_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True, text=True)
    assert done.stderr == "", done.stderr
    out = subprocess.run([exe], capture_output=True, text=True)
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0 and lines[-1] == "ok", out.stdout + out.stderr
    assert [float.fromhex(v) for v in lines[0].split()] == rotation_matrix_ref(1.5, 33, 17)
