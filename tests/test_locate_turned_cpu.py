"""Locating cut-outs of a turned copy (ssw_locate_turned_rgb8): the parts that need no GPU.  `locate_turned_ref` is the numpy
restatement of the definition include/ssw.h states -- integers only, so the device results must EQUAL it
(tests/test_locate_turned_gpu.py imports it from here); `restore_turned_ref` restates the restoring step.  Checked here: the
eight cases the constants were chosen on (the marked cat turned by Pillow and cropped), the recorded answers, the host's table
of template sizes and restoring matrices against Python's, and the argument checks of the Python layer."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest
from PIL import Image

from conftest import GOLDEN, ROOT
from test_angle_cpu import PER_DEGREE, angle_table_ref, rungs_ref
from test_locate_cpu import locate_ref, luma
from test_locate_scale_cpu import box8
from test_rotate_cpu import BICUBIC, affine_ref, base_positions, rotation_matrix_ref

STEP, STRIDE, BOX, KEEP, NEAR, NEAR_XY, SIDE_MIN = 8, 4, 8, 4, 7, 8, 32
FILL = (200, 30, 90)


# ---- the definition of include/ssw.h (ssw_locate_turned_rgb8), restated ----------------------------------------------------------
def sample_ref(sw, sh, n, tw, th, X, Y):
    """(X0, Y0, fx, fy) of the template pixels (X, Y) (int64 arrays) of angle n at size tw x th"""
    C, S = angle_table_ref(n)
    p, q = 2 * X + 1 - tw, 2 * Y + 1 - th
    Rx, Ry = (sw - 1) * 65536 + C * p - S * q, (sh - 1) * 65536 + S * p + C * q
    return Rx >> 17, Ry >> 17, (Rx >> 9) & 255, (Ry >> 9) & 255


@functools.lru_cache(maxsize=None)
def template_size_ref(sw, sh, n):
    """(tw, th) of angle n for a suspect sw x sh, None when no size has its four corners valid"""
    for i in range(sw // 8, 0, -1):
        tw, th = 8 * i, 8 * max(1, (2 * i * sh + sw) // (2 * sw))
        corners = [sample_ref(sw, sh, n, tw, th, X, Y) for X in (0, tw - 1) for Y in (0, th - 1)]          # (plain integers)
        if all(0 <= X0 <= sw - 2 and 0 <= Y0 <= sh - 2 for X0, Y0, _, _ in corners):
            return tw, th
    return None


def usable_size_ref(W, H, sw, sh, n):
    """The template size of angle n, None when the angle is dropped"""
    size = template_size_ref(sw, sh, n)
    return None if size is None or min(size) < SIDE_MIN or size[0] > W or size[1] > H else size


def template_ref(ls, n, tw, th):
    """T [th, tw] int64: the suspect's luma ls turned back by n / 32 degrees about its own centre"""
    sh, sw = ls.shape
    X, Y = np.arange(tw, dtype=np.int64)[None, :], np.arange(th, dtype=np.int64)[:, None]
    x, y, fx, fy = sample_ref(sw, sh, n, tw, th, X, Y)
    assert ((x >= 0) & (x <= sw - 2) & (y >= 0) & (y <= sh - 2)).all()          # the corners bound every tap
    return ((256 - fx) * (256 - fy) * ls[y, x] + fx * (256 - fy) * ls[y, x + 1] + (256 - fx) * fy * ls[y + 1, x] + fx * fy * ls[y + 1, x + 1] + 32768) >> 16


def boxes_ref(t):
    """T_j: the 8 x 8 box means of a template at multiples of 8"""
    th, tw = t.shape
    return (t.reshape(th // 8, 8, tw // 8, 8).sum(axis=(1, 3)) + 32) >> 6


def ladder_ref(base, s, j0, j1):
    """Per rung None (dropped) or (D, n_j, x, y, tw, th): the smallest (D, y, x) of the rung's box search"""
    H, W = base.shape[:2]
    sh, sw = s.shape[:2]
    ls = luma(s)
    b8 = box8(luma(base))[::STRIDE, ::STRIDE]
    out = []
    for j in range(j0, j1 + 1):
        size = usable_size_ref(W, H, sw, sh, STEP * j)
        if size is None:
            out.append(None)
            continue
        tw, th = size
        t = boxes_ref(template_ref(ls, STEP * j, tw, th))
        nx, ny = (W - tw) // STRIDE + 1, (H - th) // STRIDE + 1
        d = np.zeros((ny, nx), np.int64)
        for k in range(t.shape[0]):
            for i in range(t.shape[1]):
                d += np.abs(b8[2 * k:2 * k + ny, 2 * i:2 * i + nx] - t[k, i])
        idx = int(np.argmin(d.ravel()))                                # the first minimum in (y, x) order
        out.append((int(d.ravel()[idx]), t.size, STRIDE * (idx % nx), STRIDE * (idx // nx), tw, th))
    return out


def kept_ref(rungs):
    """The 4 rungs (indices j - j0, best first) with the smallest D / n_j, cross-multiplied, ties to the smaller j"""
    live = [i for i, r in enumerate(rungs) if r is not None]
    cmp = lambda a, b: (rungs[a][0] * rungs[b][1] > rungs[b][0] * rungs[a][1]) - (rungs[a][0] * rungs[b][1] < rungs[b][0] * rungs[a][1]) or a - b
    return sorted(live, key=functools.cmp_to_key(cmp))[:KEEP]


def refine_jobs_ref(rungs, kept, W, H, sw, sh, j0, j1):
    """(n, tw, th, window) of every windowed search of the refinement: each n once, with the kept rung of best rank"""
    jobs, seen = [], set()
    for i in kept:
        _, _, xj, yj, twj, thj = rungs[i]
        for n in range(STEP * (j0 + i) - NEAR, STEP * (j0 + i) + NEAR + 1):
            if n < STEP * j0 or n > STEP * j1 or n in seen:
                continue
            seen.add(n)
            size = usable_size_ref(W, H, sw, sh, n)
            if size is None:
                continue
            tw, th = size
            cx, cy = (2 * xj + twj - tw) >> 1, (2 * yj + thj - th) >> 1
            win = (max(0, cx - NEAR_XY), min(W - tw, cx + NEAR_XY), max(0, cy - NEAR_XY), min(H - th, cy + NEAR_XY))
            if win[0] <= win[1] and win[2] <= win[3]:                   # (an empty window: the angle is not searched)
                jobs.append((n, tw, th, win))
    return jobs


class TurnedRef:
    def __init__(self, n, x, y, tw, th, sad, j0, j1, rungs, kept):
        self.n, self.x, self.y, self.tw, self.th, self.sad, self.j0, self.j1, self.rungs, self.kept = n, x, y, tw, th, sad, j0, j1, rungs, kept
        self.angle, self.centre, self.n_rungs = n / PER_DEGREE, (2 * x + tw, 2 * y + th), j1 - j0 + 1

    def answer(self):
        return (self.n, self.x, self.y, self.tw, self.th, self.sad)

    def rung_rows(self):
        """[n_rungs][4]: D, n_j, x, y of every rung, a dropped one all zero -- what the call reports"""
        return [[0, 0, 0, 0] if r is None else list(r[:4]) for r in self.rungs]


def locate_turned_ref(base, s, amin, amax):
    """The answer, every rung's entry and the kept rungs; ValueError is the C side's SSW_ERR_BAD_DIMS (every rung dropped)"""
    H, W = base.shape[:2]
    sh, sw = s.shape[:2]
    j0, j1 = rungs_ref(amin, amax)
    rungs = ladder_ref(base, s, j0, j1)
    kept = kept_ref(rungs)
    if not kept:
        raise ValueError("every rung is dropped")
    ls, best = luma(s), None
    for n, tw, th, win in refine_jobs_ref(rungs, kept, W, H, sw, sh, j0, j1):
        t = template_ref(ls, n, tw, th).astype(np.uint8)
        x, y, sad = locate_ref(base, np.repeat(t[:, :, None], 3, axis=2), window=win)      # the luma of a grey pixel is its value
        if best is None or (sad * best[3] * best[4], n, y, x) < (best[5] * tw * th, best[0], best[2], best[1]):
            best = (n, x, y, tw, th, sad)
    return TurnedRef(*best, j0, j1, rungs, kept)


def restore_matrix_ref(angle, cx, cy, sw, sh):
    b = rotation_matrix_ref(-angle, 0, 0)
    return [b[0], b[1], (b[0] * -cx + b[1] * -cy + 0.0) + sw / 2.0, b[3], b[4], (b[3] * -cx + b[4] * -cy + 0.0) + sh / 2.0]


def restore_turned_ref(base, s, angle, cx, cy):
    """The restored frame: the suspect laid back into the original's frame (BICUBIC) where its footprint needs no clamping, the
    original elsewhere.  angle in degrees, (cx, cy) the suspect's centre in pixels of the original."""
    H, W = base.shape[:2]
    sh, sw = s.shape[:2]
    m = restore_matrix_ref(angle, cx, cy, sw, sh)
    ok, x, y, _, _ = base_positions(m, sw, sh, W, H)
    keep = np.zeros((H, W), bool)
    keep[ok] = (x - 1 >= 0) & (x + 2 <= sw - 1) & (y - 1 >= 0) & (y + 2 <= sh - 1)
    return np.where(keep[:, :, None], affine_ref(s, (W, H), m, BICUBIC), base)


# ---- the cases: (turned by, crop x, y, w, h) of the marked cat -------------------------------------------------------------------
CASES = [(3.3, 120, 90, 400, 300), (-7.9, 200, 100, 320, 256), (0.7, 60, 40, 500, 360), (9.6, 250, 150, 200, 160),
         (0.0, 161, 61, 400, 320), (1.0, 300, 200, 128, 96), (-2.5, 0, 0, 640, 444), (5.0, 37, 21, 333, 251)]
WHOLE_PIXEL = [(0.0, 161, 61, 400, 320), (-2.5, 0, 0, 640, 444)]     # the true centre is a whole pixel
# The restatement answers -8.03125 here, 4.2 / 32 degrees from the truth (its centre is within 0.9 half pixels): the answer is
# recorded and only the equality is asserted -- no constant was moved.
OUTSIDE_THE_ANGLE_LIMIT = [(-7.9, 200, 100, 320, 256)]
SEARCH = (-10, 10)
ANSWERS = os.path.join(GOLDEN, "locate_turned_answers.json")         # what the restatement answers, recorded: the GPU tests compare with it


def name_of(c):
    return "%g@%d,%d %dx%d" % c


@functools.lru_cache(maxsize=1)
def cat():
    g = np.load(os.path.join(GOLDEN, "cat_decoded_u8.npz"))
    return g["cat"], g["watermarked_with_1"]


def turned_cut(frame, angle, x, y, w, h):
    t = np.asarray(Image.fromarray(frame).rotate(angle, resample=Image.BICUBIC, fillcolor=FILL))
    return np.ascontiguousarray(t[y:y + h, x:x + w])


def true_centre(W, H, angle, x, y, w, h):
    """Where the cut-out's centre lay in the original, in half pixels: Pillow's matrix maps output to input positions"""
    m = rotation_matrix_ref(angle, W, H)
    cx, cy = x + w / 2.0, y + h / 2.0
    return 2 * (m[0] * cx + m[1] * cy + m[2]), 2 * (m[3] * cx + m[4] * cy + m[5])


@functools.lru_cache(maxsize=None)
def found(c):
    base, marked = cat()
    return locate_turned_ref(base, turned_cut(marked, *c), *SEARCH)


def recorded():
    with open(ANSWERS) as f:
        return json.load(f)


# ---- what it finds ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=name_of)
def test_the_eight_cases_are_found(c):
    """The first run of this search with the constants of the issue (rung step 0.25 degrees, stride 4, box 8, 4 kept, +-7, +-8)"""
    base, _ = cat()
    f = found(c)
    tx, ty = true_centre(base.shape[1], base.shape[0], *c)
    print(name_of(c), "->", f.angle, f.centre, "truth", c[0], (round(tx, 2), round(ty, 2)), "mean", round(f.sad / (f.tw * f.th), 2),
          "template", (f.tw, f.th), "kept", [(f.j0 + i) / 4 for i in f.kept])
    rec = recorded()[name_of(c)]
    assert list(f.answer()) == rec["answer"] and f.rung_rows() == rec["rungs"]
    if c not in OUTSIDE_THE_ANGLE_LIMIT:
        assert abs(f.n - 32 * c[0]) <= 4
    assert abs(f.centre[0] - tx) <= 2 and abs(f.centre[1] - ty) <= 2
    assert any(abs((f.j0 + i) / 4 - c[0]) <= 0.25 for i in f.kept)
    if c in WHOLE_PIXEL:
        assert f.n == 32 * c[0] and f.centre == (tx, ty)


def test_the_recorded_file_holds_these_cases_only():
    assert sorted(recorded()) == sorted(name_of(c) for c in CASES)


# ---- the parts of the definition -------------------------------------------------------------------------------------------------
def test_template_sizes():
    assert template_size_ref(640, 444, 0) == (632, 440)                # X0 = X + (sw - tw) / 2 <= sw - 2
    assert template_size_ref(64, 64, 0) == (56, 56) and template_size_ref(64, 64, 1440) == (40, 40) and template_size_ref(64, 64, -1440) == (40, 40)
    assert template_size_ref(70, 66, 0) == (64, 64)
    assert template_size_ref(1000, 64, 0) == (936, 56)
    assert usable_size_ref(2000, 2000, 1000, 64, 320) is None and usable_size_ref(2000, 2000, 1000, 64, 80) is not None
    assert usable_size_ref(640, 444, 640, 444, 0) == (632, 440) and usable_size_ref(600, 444, 640, 444, 0) is None
    assert template_size_ref(8, 8, 0) is None or template_size_ref(8, 8, 0)[0] < SIDE_MIN
    for sw, sh in ((64, 64), (333, 251), (1000, 64)):                  # a smaller size of the same angle is valid too: "largest" is a threshold
        for n in (-1440, -77, 0, 5, 640):
            size = template_size_ref(sw, sh, n)
            if size:
                ls = np.zeros((sh, sw), np.int64)
                template_ref(ls, n, *size)                              # asserts every tap inside


def test_the_template_of_angle_zero_is_the_centred_cut():
    ls = luma(np.random.default_rng(5).integers(0, 256, (66, 70, 3), dtype=np.uint8))
    assert (template_ref(ls, 0, 64, 64) == ls[1:65, 3:67]).all()
    odd = template_ref(ls, 0, 56, 56)                                   # 70 - 56 even, 66 - 56 even as well: whole pixels again
    assert (odd == ls[5:61, 7:63]).all()


def test_ties_go_to_the_smaller_index_at_every_stage():
    flat = np.full((80, 96, 3), 93, np.uint8)
    f = locate_turned_ref(flat, flat[:64, :64], -1, 1)
    assert f.kept == [0, 1, 2, 3] and all(r[0] == 0 and r[2:4] == (0, 0) for r in f.rungs)
    assert f.n == -32 and (f.x, f.y, f.sad) == (0, 0, 0)


def test_every_rung_dropped_is_an_error():
    base = np.zeros((64, 64, 3), np.uint8)
    with pytest.raises(ValueError):
        locate_turned_ref(base, np.zeros((30, 30, 3), np.uint8), -1, 1)          # templates below 32
    with pytest.raises(ValueError):
        locate_turned_ref(base, np.zeros((200, 200, 3), np.uint8), -1, 1)        # templates larger than the frame


def test_restoring_an_unturned_cut_out_gives_its_inner_pixels_back():
    base, marked = cat()
    s = marked[61:381, 161:561]
    r = restore_turned_ref(base, s, 0.0, 161 + 200.0, 61 + 160.0)
    want = base.copy()
    want[62:379, 162:559] = marked[62:379, 162:559]                     # the footprint x-1 .. x+2 stays inside the suspect
    assert (r == want).all()
    assert (restore_turned_ref(base, s[:3, :5], 3.0, 100.0, 100.0) == base).all()          # three rows hold no footprint: the mask is empty
    assert (restore_turned_ref(base, s[:1, :1], 0.0, 100.5, 100.5) == base).all()


# ---- the host's tables against Python's ------------------------------------------------------------------------------------------
SHAPES = [(64, 64), (70, 66), (1000, 64), (640, 444), (67, 65), (33, 200)]
MATRICES = [(3.3125, 319.0, 240.0, 400, 300), (-8.03125, 360.5, 222.25, 320, 256), (0.0, 10.0, 7.5, 5, 4), (45.0, -3.0, 900.5, 64, 64),
            (-0.03125, 32768.0, 1.0, 65535, 1)]


@pytest.fixture(scope="module")
def tables_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("turned_tables") / "turned_tables_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "spread_spectrum_watermarking_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "turned_tables_test.cpp"), "-o", exe], check=True)
    return exe


def check_tables(exe):
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n")
    sizes = {}
    mats = []
    for ln in lines:
        p = ln.split()
        if p and p[0] == "size":
            sizes[tuple(int(v) for v in p[1:4])] = (int(p[4]), int(p[5]))
        if p and p[0] == "matrix":
            mats.append([float.fromhex(v) for v in p[1:]])
    assert len(sizes) == len(SHAPES) * 2881
    for sw, sh in SHAPES:
        for n in range(-1440, 1441):
            assert sizes[(sw, sh, n)] == (template_size_ref(sw, sh, n) or (0, 0)), (sw, sh, n)
    assert mats == [restore_matrix_ref(*m) for m in MATRICES]


def test_host_tables_are_pythons(tables_exe):
    check_tables(tables_exe)


def test_host_tables_under_sanitizers(tmp_path):
    exe = str(tmp_path / "turned_tables_san")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "spread_spectrum_watermarking_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "turned_tables_test.cpp"),
                    "-o", exe], check=True)
    check_tables(exe)


# ---- the Python layer without a GPU ----------------------------------------------------------------------------------------------
def test_argument_errors_of_the_python_layer():
    from spread_spectrum_watermarking_amd import api
    base = np.zeros((80, 96, 3), np.uint8)
    s = np.zeros((64, 64, 3), np.uint8)
    for search in ((2, 1), (-46, 0), (0, 45.5), (float("nan"), 1), (1,), "wide"):
        with pytest.raises(ValueError):
            api.locate_turned(base, [s], search)
    for bad in (np.zeros((64, 64, 4), np.uint8), np.zeros((64, 64), np.uint8), np.zeros((64, 64, 3), np.float32), np.zeros((0, 64, 3), np.uint8)):
        with pytest.raises(ValueError):
            api.locate_turned(base, [bad])
        with pytest.raises(ValueError):
            api.restore_turned(base, [bad], [(0.0, 1.0, 1.0)])
    assert api.locate_turned(base, []) == [] and api.restore_turned(base, [], []) == []
    found, entries = api.locate_turned(base, [], (-1, 1), rungs=True)
    assert found == [] and entries.shape == (0, 9, 4)
    for triples in ([], [(1.0, 2.0)], [(float("inf"), 1.0, 1.0)], [(0.0, 1.0, 1.0), (0.0, 1.0, 1.0)]):
        with pytest.raises(ValueError):
            api.restore_turned(base, [s], triples)
    assert api.Locate(turned=True).turned_range() == (-10.0, 10.0) and api.Locate(turned=(-3, 4.5)).turned_range() == (-3.0, 4.5)
    assert api.Locate(64, 64).turned_range() is None and api.Locate().turned_range() is None
    for bad in (api.Locate(w=64, h=64, turned=True), api.Locate(widths=(60, 70), turned=True), api.Locate(scale=(0.5, 1.0), turned=(-1, 1))):
        with pytest.raises(ValueError):
            bad.turned_range()
        with pytest.raises(ValueError):
            bad.width_range(64)
    with pytest.raises(ValueError):
        api.Locate(turned=(5, -5)).turned_range()


def test_turned_entries_are_resolved_by_one_search_per_range_and_one_restoring():
    from spread_spectrum_watermarking_amd import api
    base = np.arange(80 * 96 * 3, dtype=np.uint8).reshape(80, 96, 3)
    sus = [np.full((40 + i, 50 + i, 3), i, np.uint8) for i in range(5)]
    pl = [api.Locate(turned=True), api.Placement(1, 2), api.Locate(turned=(-3, 3)), api.Locate(turned=(-10, 10)), api.Locate(40, 44)]
    calls = []

    def locate_fn(b, s, search, ctx):
        calls.append(("locate", search, [int(a[0, 0, 0]) for a in s]))
        return [api.LocatedTurned(1.5, 48, (30.0 + a[0, 0, 0], 20.5), (32, 32), 7, 7 / 1024) for a in s]

    def restore_fn(b, s, found, ctx):
        calls.append(("restore", [int(a[0, 0, 0]) for a in s], [f.centre[0] for f in found]))
        return [np.full_like(b, 100 + a[0, 0, 0]) for a in s]

    out_s, out_p, found = api._undo_turned_cuts(base, sus, pl, None, locate_fn, restore_fn)
    assert calls == [("locate", (-10.0, 10.0), [0, 3]), ("locate", (-3.0, 3.0), [2]), ("restore", [0, 2, 3], [30.0, 32.0, 33.0])]
    assert sorted(found) == [0, 2, 3] and all(isinstance(f, api.LocatedTurned) for f in found.values())
    assert [out_p[i] for i in (0, 2, 3)] == [None] * 3 and out_p[1] is pl[1] and out_p[4] is pl[4]
    assert all(out_s[i].shape == base.shape and out_s[i][0, 0, 0] == 100 + i for i in (0, 2, 3)) and out_s[1] is sus[1] and out_s[4] is sus[4]
    same = api._undo_turned_cuts(base, sus[:2], [None, api.Locate(40, 41)], None, locate_fn, restore_fn)
    assert same[2] == {} and len(calls) == 3                            # no such entry: nothing is called
    with pytest.raises(ValueError):
        api._undo_turned_cuts(None, sus[:1], [api.Locate(turned=True)], None, locate_fn, restore_fn)


# ---- the C++ wrappers over a stub ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_cpp_wrappers_against_a_stub(tmp_path, sanitize):
    """wm::locate_turned and wm::restore_turned (include/ssw_turned.hpp) over a stub of the C functions: argument order, vector
    sizes, suspects of mixed sizes, a thrown status with nothing left alive -- a stand-alone program, plain and under ASan/UBSan"""
    from test_angle_cpu import build_exe
    exe = build_exe(tmp_path, "turned_wrappers_test", ["turned_wrappers_test.cpp", "turned_stub.cpp", "ssw_stub.cpp"], sanitize)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
    assert out.stdout.splitlines()[-1] == "turned wrappers: ok"
