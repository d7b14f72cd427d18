"""The rotation attack's reference and its surfaces, without a GPU.  `affine_ref` is the numpy restatement of Pillow's affine
transform with a BILINEAR or BICUBIC filter (Geometry.c) and `rotation_matrix_ref` of the matrix PIL.Image.rotate makes -- the
definition include/ssw.h states, which the device results must EQUAL (tests/test_rotate_gpu.py imports them).  They are checked
here byte for byte against Pillow itself; `unrotate_ref` and `unrotate_mask_ref` restate the undoing, checked for independence
of the fill colour and against Pillow under the mask; then the host's matrices and tile plans against Python's numbers."""
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image

from conftest import ROOT
from spread_spectrum_watermarking_amd import api
from test_jpeg_cpu import cat_image

BILINEAR, BICUBIC = 0, 1
NAMES = {BILINEAR: "bilinear", BICUBIC: "bicubic"}
PIL_FILTER = {BILINEAR: Image.BILINEAR, BICUBIC: Image.BICUBIC}
BLACK, MAGENTA = (0, 0, 0), (255, 0, 255)
IDENTITY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def rotation_matrix_ref(angle, w, h):
    a = -math.radians(angle % 360.0)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = w / 2.0, h / 2.0
    m[2] = (m[0] * -cx + m[1] * -cy + 0.0) + cx
    m[5] = (m[3] * -cx + m[4] * -cy + 0.0) + cy
    return m


def sample_points(m, X, Y):
    """numpy evaluates one operation per call and rounds each: the sums below are the definition's, from the left"""
    px, py = X + 0.5, Y + 0.5
    return m[0] * px + m[1] * py + m[2], m[3] * px + m[4] * py + m[5]


def inside(xin, yin, w, h):
    return ~((xin < 0.0) | (xin >= w) | (yin < 0.0) | (yin >= h))


def base_positions(m, w, h, ow, oh):
    """(inside [oh, ow], x, y, dx, dy of the inside pixels, flat): steps 1 to 3"""
    X, Y = np.arange(ow, dtype=np.float64)[None, :], np.arange(oh, dtype=np.float64)[:, None]
    xin, yin = sample_points(m, X, Y)
    xin, yin = np.broadcast_arrays(xin, yin)
    ok = inside(xin, yin, w, h)
    xs, ys = xin[ok] - 0.5, yin[ok] - 0.5
    fx, fy = np.floor(xs), np.floor(ys)
    return ok, fx.astype(np.int64), fy.astype(np.int64), xs - fx, ys - fy


def _lerp(a, b, d):
    return a + (b - a) * d


def _cubic(a, b, c, d, t):
    p1, p2, p3, p4 = b, -a + c, 2 * (a - b) + c - d, -a + b - c + d
    return p1 + t * (p2 + t * (p3 + t * p4))


def affine_ref(frame, size, m, filt, fill=BLACK):
    """frame u8 [h, w, 3] -> u8 [oh, ow, 3]: Image.transform(size, AFFINE, m, filt, fillcolor=fill)"""
    h, w = frame.shape[:2]
    ow, oh = size
    ok, x, y, dx, dy = base_positions(m, w, h, ow, oh)
    src = frame.astype(np.float64)
    dx, dy = dx[:, None], dy[:, None]
    XC, YC = (lambda i: np.clip(i, 0, w - 1)), (lambda j: np.clip(j, 0, h - 1))
    if filt == BILINEAR:
        x0, x1 = XC(x), XC(x + 1)
        v1 = _lerp(src[YC(y), x0], src[YC(y), x1], dx)
        below = ((y + 1 >= 0) & (y + 1 < h))[:, None]
        v2 = np.where(below, _lerp(src[YC(y + 1), x0], src[YC(y + 1), x1], dx), v1)
        got = np.trunc(_lerp(v1, v2, dy)).astype(np.uint8)
    else:
        cols = [XC(x - 1), XC(x), XC(x + 1), XC(x + 2)]
        row = lambda j: _cubic(*[src[YC(j), c] for c in cols], dx)
        valid = lambda j: ((j >= 0) & (j < h))[:, None]
        v1 = row(y - 1)
        v2 = np.where(valid(y), row(y), v1)
        v3 = np.where(valid(y + 1), row(y + 1), v2)
        v4 = np.where(valid(y + 2), row(y + 2), v3)
        v = _cubic(v1, v2, v3, v4, dy)
        got = np.where(v <= 0.0, 0, np.where(v >= 255.0, 255, np.trunc(np.clip(v, 0.0, 255.0)))).astype(np.uint8)
    out = np.empty((oh, ow, 3), np.uint8)
    out[:] = np.asarray(fill, np.uint8)
    out[ok] = got
    return out


def rotate_ref(frame, angle, filt, fill=BLACK):
    h, w = frame.shape[:2]
    return affine_ref(frame, (w, h), rotation_matrix_ref(angle, w, h), filt, fill)


@functools.lru_cache(maxsize=512)
def unrotate_mask_ref(w, h, angle):
    """bool [h, w]: where the undoing keeps the turned-back pixel"""
    F, B = rotation_matrix_ref(angle, w, h), rotation_matrix_ref(-angle, w, h)
    X, Y = np.arange(w, dtype=np.float64)[None, :], np.arange(h, dtype=np.float64)[:, None]
    xin, yin = sample_points(B, X, Y)
    xin, yin = np.broadcast_arrays(xin, yin)
    x, y = np.floor(xin - 0.5), np.floor(yin - 0.5)
    keep = inside(xin, yin, w, h) & (x - 1 >= 0) & (x + 2 <= w - 1) & (y - 1 >= 0) & (y + 2 <= h - 1)
    for cx in (x - 1, x + 2):
        for cy in (y - 1, y + 2):
            keep = keep & inside(*sample_points(F, cx, cy), w, h)
    return keep


def is_copy(w, h, angle):
    return rotation_matrix_ref(angle, w, h) == IDENTITY and rotation_matrix_ref(-angle, w, h) == IDENTITY


def unrotate_ref(base, attacked, angle):
    """The restored frame: the attacked one turned back (BICUBIC) where the mask holds, the original elsewhere; angle 0: a copy"""
    h, w = base.shape[:2]
    if is_copy(w, h, angle):
        return attacked.copy()
    U = affine_ref(attacked, (w, h), rotation_matrix_ref(-angle, w, h), BICUBIC)
    return np.where(unrotate_mask_ref(w, h, angle)[:, :, None], U, base)


# ---- cases -------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (7, 1), (1, 7), (3, 2), (5, 7), (64, 33), (53, 37), (200, 9), (197, 131), (33, 33)]      # (w, h); 33 x 33: the square of 90 and 270
ANGLES = [0, 0.1, 0.25, 1, -7.5, 30, 45, 90, 180, 180.3, 270, 270.5, 359]


def noise(w, h, seed=0):
    return np.random.default_rng(1000 * w + h + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def checkerboard(w=37, h=100):
    yy, xx = np.mgrid[:h, :w]
    return np.repeat((((xx + yy) % 2) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


def small_frames():
    """(name, frame) of every frame of the first test but the cat"""
    out = [(f"{w}x{h}", noise(w, h)) for w, h in SIZES]
    return out + [("checkerboard", checkerboard()), ("white", np.full((21, 30, 3), 255, np.uint8))]


@functools.lru_cache(maxsize=1)
def cat():
    return cat_image()


def general_matrices(w, h):
    """(name, matrix, output size) of the three transforms that are no rotation"""
    return [("shrink8", [8.0, 0.0, 0.0, 0.0, 8.0, 0.0], (16, 9)),
            ("enlarge3", [1 / 3, 0.0, 0.0, 0.0, 1 / 3, 0.0], (3 * w, 3 * h)),
            ("shear", [1.0, 60.0, -0.75 * w - 40.0, 1.0, 1.0, -3.5], (w, h))]


SHEAR_MILD = [1.0, 0.4, -11.25, 0.125, 1.0, -3.5]           # most of the output inside: the LDS form's turn at a shear


def pil_rotate(frame, angle, filt, fill=BLACK):
    return np.asarray(Image.fromarray(frame).rotate(angle, resample=PIL_FILTER[filt], fillcolor=fill))


def pil_affine(frame, size, m, filt, fill=BLACK):
    return np.asarray(Image.fromarray(frame).transform(size, Image.AFFINE, m, resample=PIL_FILTER[filt], fillcolor=fill))


# ---- 1. the restatement is Pillow ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,frame", small_frames() + [("cat", None)], ids=lambda v: v if isinstance(v, str) else "")
def test_affine_ref_is_pil_rotate(name, frame):
    frame = cat() if frame is None else frame
    for angle in ANGLES:
        for filt in (BILINEAR, BICUBIC):
            for fill in (BLACK, MAGENTA):
                assert np.array_equal(rotate_ref(frame, angle, filt, fill), pil_rotate(frame, angle, filt, fill)), (name, angle, NAMES[filt], fill)


def test_the_formula_gives_pillows_transposes_their_bytes():
    """Pillow answers 0 and 180 degrees, and 90 and 270 on a square frame, with a copy or a transpose; the formula needs no
    routing for them: it lands on pixel centres and gives the same bytes."""
    sq, ob = noise(33, 33), noise(64, 33)
    for filt in (BILINEAR, BICUBIC):
        assert np.array_equal(rotate_ref(ob, 0, filt), ob) and np.array_equal(rotate_ref(ob, 360.0, filt), ob)
        assert np.array_equal(rotate_ref(ob, 180, filt), ob[::-1, ::-1])
        assert np.array_equal(rotate_ref(sq, 90, filt), np.asarray(Image.fromarray(sq).transpose(Image.ROTATE_90)))
        assert np.array_equal(rotate_ref(sq, 270, filt), np.asarray(Image.fromarray(sq).transpose(Image.ROTATE_270)))


@pytest.mark.parametrize("w,h", [(128, 72), (53, 37), (131, 75)])
def test_affine_ref_is_pil_transform(w, h):
    frame = noise(w, h, 3)
    for name, m, size in general_matrices(w, h) + [("mild shear", SHEAR_MILD, (w, h))]:
        for filt in (BILINEAR, BICUBIC):
            for fill in (BLACK, MAGENTA):
                got = affine_ref(frame, size, m, filt, fill)
                assert np.array_equal(got, pil_affine(frame, size, m, filt, fill)), (name, NAMES[filt], fill)
        if name == "shear":                                             # most of the output lies outside
            outside = np.all(got == np.asarray(MAGENTA, np.uint8), axis=2).mean()
            assert 0.5 < outside < 1.0, outside


# ---- 2. the undoing does not see the fill ----------------------------------------------------------------------------------
def undo_case(frame, angle, filt):
    h, w = frame.shape[:2]
    base = (255 - frame)[::-1].copy()                                   # an "original" that differs everywhere: the mask shows
    black, magenta = pil_rotate(frame, angle, filt, BLACK), pil_rotate(frame, angle, filt, MAGENTA)
    a, b = unrotate_ref(base, black, angle), unrotate_ref(base, magenta, angle)
    assert np.array_equal(a, b), "the fill shows"
    if is_copy(w, h, angle):
        assert np.array_equal(a, black)
        return
    mask = unrotate_mask_ref(w, h, angle)
    back = pil_rotate(magenta, -angle, BICUBIC, (0, 255, 0))
    assert np.array_equal(a[mask], back[mask]) and np.array_equal(a[~mask], base[~mask])


@pytest.mark.parametrize("name,frame", small_frames() + [("cat", None)], ids=lambda v: v if isinstance(v, str) else "")
def test_the_undoing_is_independent_of_the_fill(name, frame):
    frame = cat() if frame is None else frame
    for angle in ANGLES:
        for filt in (BILINEAR, BICUBIC):
            undo_case(frame, angle, filt)


UNDO_ANGLES = [0.25, 1, 2, 5, -7.5, 30, 45, 90.5, 180.3]


@pytest.mark.parametrize("which", ["cat", "53x37", "40x9"])
def test_the_undoing_on_the_cases_the_rule_was_found_on(which):
    frame = cat() if which == "cat" else noise(*[int(v) for v in which.split("x")])
    for angle in UNDO_ANGLES:
        for filt in (BILINEAR, BICUBIC):
            undo_case(frame, angle, filt)


def test_the_mask_of_the_cat_at_one_degree():
    mask = unrotate_mask_ref(640, 444, 1)
    assert mask.shape == (444, 640) and int(mask.sum()) == 278328 and round(100 * mask.mean(), 2) == 97.95
    assert api.Rotate(1.0).kept(640, 444) == 278328 / (640 * 444) and api.Rotate(0).kept(640, 444) == 1.0
    for w, h, angle in ((53, 37, 30), (40, 9, -7.5), (7, 1, 45), (197, 131, 90.5)):
        assert api.Rotate(angle).kept(w, h) == unrotate_mask_ref(w, h, angle).mean(), (w, h, angle)


# ---- 3. the host's tables ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tables_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("affine") / "affine_tables_test")
    done = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "spread_spectrum_watermarking_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "affine_tables_test.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    assert done.stderr == "", done.stderr
    return exe


def golden_angles():
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "rotation_angles.json")))
    return [float.fromhex(a) for a in doc["angles"]]


def test_the_committed_angles_are_the_generators():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import rotation_angles
    finally:
        sys.path.pop(0)
    angles = golden_angles()
    assert angles == rotation_angles.angles() and len(angles) == 64
    assert sum(a < 0 for a in angles) >= 10 and 0.1 in angles and math.nextafter(90.0, 0.0) in angles


@pytest.mark.parametrize("w,h", [(640, 444), (197, 131), (1, 1), (3840, 2160)])
def test_host_matrices_are_pythons_bit_for_bit(tables_exe, w, h):
    angles = golden_angles()
    out = subprocess.run([tables_exe, "matrix", str(w), str(h)] + [a.hex() for a in angles], check=True, capture_output=True, text=True).stdout
    lines = out.splitlines()
    assert len(lines) == 64
    for angle, line in zip(angles, lines):
        got = [float.fromhex(v) for v in line.split()]
        for m in (rotation_matrix_ref(angle, w, h), api.rotation_matrix(angle, w, h)):
            assert [v.hex() for v in got] == [v.hex() for v in m], angle         # (hex: -0.0 is not 0.0)


def host_plan(exe, w, h, ow, oh, m):
    out = subprocess.run([exe, "plan", str(w), str(h), str(ow), str(oh)] + [float(v).hex() for v in m], check=True, capture_output=True, text=True).stdout
    lines = [[int(v) for v in line.split()] for line in out.splitlines()]
    return lines[0], lines[1:]


def test_host_tile_plans_hold_every_tap(tables_exe):
    w, h = 197, 131
    cases = [(rotation_matrix_ref(a, w, h), (w, h)) for a in (0.25, 1, 30, 45, 90.5)] + [([8.0, 0.0, 0.0, 0.0, 8.0, 0.0], (16, 9))]
    cases += [(rotation_matrix_ref(-1, w, h), (w, h)), (SHEAR_MILD, (w, h))]
    for m, (ow, oh) in cases:
        (lds, box_w, box_h, pitch, lds_bytes), tiles = host_plan(tables_exe, w, h, ow, oh, m)
        assert len(tiles) == -(-ow // 32) * -(-oh // 8)
        assert pitch % 4 == 0 and pitch >= 3 * box_w and lds_bytes == pitch * box_h and lds == (lds_bytes <= 16384)
        ok, x, y, _, _ = base_positions(m, w, h, ow, oh)
        X = np.broadcast_to(np.arange(ow)[None, :], (oh, ow))[ok]
        Y = np.broadcast_to(np.arange(oh)[:, None], (oh, ow))[ok]
        lo_x, hi_x = np.clip(x - 1, 0, w - 1), np.clip(x + 2, 0, w - 1)         # the taps of BICUBIC; BILINEAR's lie among them
        lo_y, hi_y = np.clip(y - 1, 0, h - 1), np.clip(y + 2, 0, h - 1)
        seen = 0
        for X0, Y0, x0, y0, bw, bh in tiles:
            assert 1 <= bw <= box_w and 1 <= bh <= box_h and 0 <= x0 and x0 + bw <= w and 0 <= y0 and y0 + bh <= h, (m, X0, Y0)
            t = (X >= X0) & (X < X0 + 32) & (Y >= Y0) & (Y < Y0 + 8)
            seen += int(t.sum())
            if t.any():
                assert lo_x[t].min() >= x0 and hi_x[t].max() < x0 + bw and lo_y[t].min() >= y0 and hi_y[t].max() < y0 + bh, (m, X0, Y0)
        assert seen == int(ok.sum())
    assert host_plan(tables_exe, w, h, 16, 9, [8.0, 0.0, 0.0, 0.0, 8.0, 0.0])[0][0] == 0          # the shrink by 8 takes the global form
    assert host_plan(tables_exe, w, h, w, h, general_matrices(w, h)[2][1])[0][0] == 0             # and so does the strong shear
    assert host_plan(tables_exe, w, h, w, h, rotation_matrix_ref(45, w, h))[0][0] == 1            # no rotation does


# ---- the surfaces ------------------------------------------------------------------------------------------------------------
def test_python_surface_without_a_gpu():
    assert api.Rotate(0.5).label == "rotate 0.5 bicubic" and api.Rotate(2, "Bilinear").label == "rotate 2 bilinear"
    assert api.Rotate(-1).label == "rotate -1 bicubic"
    j = api.Rotate(1.0, "bilinear").job(3, 640, 444)
    assert (j.frame, j.filter, list(j.fill)) == (3, 0, [0, 0, 0, 0])
    assert list(j.forward) == rotation_matrix_ref(1.0, 640, 444) and list(j.back) == rotation_matrix_ref(-1.0, 640, 444)
    for bad in (lambda: api.Rotate(1, "lanczos"), lambda: api.Rotate(float("nan")), lambda: api.Rotate("1"), lambda: api.Rotated(float("inf")),
                lambda: api.strength_report(np.zeros((8, 8, 3), np.uint8), [0.1], rotations=[1.0]),
                lambda: api.affine([np.zeros((8, 8, 3), np.uint8)], (8, 8), [1, 0, 0, 0, 1]),
                lambda: api.affine([np.zeros((8, 8, 3), np.uint8)], (8, 8), IDENTITY, fill=(0, 0, 256)),
                lambda: api.unrotate(np.zeros((8, 8, 3), np.uint8), [np.zeros((8, 9, 3), np.uint8)], [1.0]),
                lambda: api._undo_rotated(np.zeros((8, 8, 3), np.uint8), [np.zeros((8, 8, 4), np.uint8)], [api.Rotated(1.0)], None),
                lambda: api._undo_rotated(None, [np.zeros((8, 8, 3), np.uint8)], [api.Rotated(1.0)], None)):
        with pytest.raises(ValueError):
            bad()
    assert api.affine([], (8, 8), IDENTITY) == [] and api.rotate([], 1.0) == [] and api.unrotate(np.zeros((8, 8, 3), np.uint8), [], []) == []
