"""Hard inputs for the free-aspect rescoring (csrc/locate_free.hip, run through the diagnostic ssw_locate_free_sums_rgb8, which
starts the stage wherever the caller says and hands back every sum): the tie-heavy and saturated frames of tests/locate_cases.py,
starts laid on every edge of the frame, and suspects whose sizes reach the tiles `free_pick_tile` has.  numpy only:
tests/test_locate_free_hard_cpu.py pins what the tables claim to reach (the tiles come from tests/cpp/locate_free_plan_test.cpp)
and the answers the content decides, by the restatement alone; tests/test_locate_free_hard_gpu.py runs the same cases on the device.

A case is one base frame, one suspect and one start.  The start is the table's; the rectangle the suspect was cut from is the
start minus `off` = (dpw, dph, dx, dy), so with off != 0 the winner is not the centre slot.

  T  tile edges: starts of 36 x 36, 64 x 64, 128 x 64, 128 x 128 (and 64 x 32 for the tiles of 32 columns) with slack 4 -- the sizes
     meet every pw mod 4 and cross k oxb, k oyb of every tile -- and per start suspects at its own size (the plain front is one
     item of the 81), halved, doubled, x 3, x 0.95 and x 1/3 where no side of the suspect passes 136, RGB and RGBA, + a 126 x 36
     suspect of the 36 x 36 start (3.5 times as wide: its sizes up to 36 columns get the tile of 32 x 32, one tile at 32 x 32); the two
     suspects of the 64 x 32 start are 256 x 128 RGBA and 128 x 64 RGB.
  W  windows and the frame's edge, on one base per W mod 4: x0 in {0, 3, 4, W - pw0 - 3, W - pw0} and y0 likewise, the four corners,
     pw0 = W, ph0 = H, ph0 = 33 (heights stop at 32), wmin = wmax = pw0, slacks 1 to 4, a flat and a foreign suspect whose ties
     are decided inside a clipped window; + a 160 x 32 base whose one size has one position.
  X  contents: three shapes -- the plain front, a resized RGB suspect, a resized RGBA one -- on all eight contents, started at the truth."""
import os
import subprocess
from collections import namedtuple
from functools import lru_cache

import numpy as np

import locate_cases as LC
from conftest import ROOT
from oracle import oracle as O
from test_locate_free_cpu import NEAR, free_sizes, free_window, locate_free_ref
from test_locate_scale_cpu import with_alpha

SIDE = 2 * NEAR + 1
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
CONTENTS = ("noise", "binary", "flat", "periodic", "rows", "columns") + LC.FOREIGN

# name, table, base W x H, content, variant (exact / noisy / resized / foreign), rect (x, y, pw, ph) of the cut, size (sw, sh) of the
# suspect, channels, start (pw0, ph0, x0, y0), wmin, wmax, slack
Case = namedtuple("Case", "name table W H content variant rect size channels start wmin wmax slack")


def _case(table, name, W, H, content, start, size=None, channels=3, off=(0, 0, 0, 0), noisy=False, slack=4, widths=None):
    pw0, ph0, x0, y0 = start
    rect = (x0 - off[2], y0 - off[3], pw0 - off[0], ph0 - off[1])
    size = size or rect[2:]
    variant = "foreign" if content in LC.FOREIGN else "resized" if size != rect[2:] else "noisy" if noisy else "exact"
    assert 0 <= rect[0] <= W - rect[2] and 0 <= rect[1] <= H - rect[3] and 0 <= x0 <= W - pw0 and 0 <= y0 <= H - ph0, name
    wmin, wmax = widths or (max(32, pw0 - 8), min(W, pw0 + 8))
    return Case("%s %s" % (table, name), table, W, H, content, variant, rect, tuple(size), channels, tuple(start), wmin, wmax, slack)


def _seeded(table, W, H, pw, ph, margin=8):
    """A start at least `margin` inside the frame on every side, so that a table T start and its offsets stay unclipped."""
    rng = np.random.default_rng([ord(table), W, H, pw, ph])
    return int(rng.integers(margin, W - pw - margin + 1)), int(rng.integers(margin, H - ph - margin + 1))


# ---- T: (start size, base, [(what, suspect size, channels, content, off, noisy)]) ---------------------------------------------
_T = [((36, 36), (161, 97), [("own", (36, 36), 3, "noise", (0, 0, 0, 0), False),
                             ("halved", (18, 18), 3, "binary", (2, -3, 4, -4), False),
                             ("doubled rgba", (72, 72), 4, "noise", (0, 0, 0, 0), False),
                             ("x3", (108, 108), 3, "periodic", (-4, 4, -1, 2), False),
                             ("x0.95 rgba", (34, 34), 4, "binary", (0, 0, 0, 0), False),
                             # 3.5 times as wide: 14 or more horizontal taps leave no tile of 64 columns -> 32 x 32, one tile at 32 x 32
                             ("x3.5 wide", (126, 36), 3, "noise", (0, 0, 0, 0), False)]),
      ((64, 64), (202, 120), [("own noisy", (64, 64), 3, "rows", (0, 0, 2, -2), True),
                              ("halved rgba", (32, 32), 4, "noise", (0, 0, 0, 0), False),
                              ("doubled", (128, 128), 3, "binary", (-3, 2, -4, 4), False),
                              ("x0.95 rgba", (61, 61), 4, "columns", (0, 0, 0, 0), False)]),
      ((128, 64), (243, 131), [("own rgba", (128, 64), 4, "noise", (0, 0, 4, 4), False),
                               ("halved", (64, 32), 3, "periodic", (0, 0, 0, 0), False),
                               ("x0.95", (122, 61), 3, "noise", (-2, 0, 0, 3), False)]),
      ((128, 128), (300, 200), [("own", (128, 128), 3, "binary", (0, 0, 0, 0), False),
                                ("halved rgba", (64, 64), 4, "noise", (3, -4, -2, 1), False),
                                ("x0.95 rgba", (122, 122), 4, "noise", (0, 0, 0, 0), False),
                                ("x1/3", (43, 43), 3, "noise", (0, 0, 0, 0), False)]),
      ((64, 32), (160, 96), [("x4 rgba", (256, 128), 4, "noise", (0, 0, 0, 0), False),
                             ("doubled", (128, 64), 3, "binary", (0, 0, 1, -1), False)])]


def _table_t():
    out = []
    for (pw0, ph0), (W, H), suspects in _T:
        x0, y0 = _seeded("T", W, H, pw0, ph0)
        for what, size, ch, content, off, noisy in suspects:
            out.append(_case("T", "%dx%d %s %s" % (pw0, ph0, what, content), W, H, content, (pw0, ph0, x0, y0), size, ch, off, noisy))
    return out


# ---- W ---------------------------------------------------------------------------------------------------------------------------
W_BASES = ((160, 96), (161, 97), (162, 98), (163, 99))
W_CONTENTS = ("noise", "binary", "periodic", "noise")


def _table_w():
    out = []
    for b, ((W, H), content) in enumerate(zip(W_BASES, W_CONTENTS)):
        pw0, ph0 = 40 + b, 36 + b
        spots = [(0, 0), (3, 3), (4, 4), (W - pw0 - 3, H - ph0 - 3), (W - pw0, H - ph0), (W - pw0, 0), (0, H - ph0)]
        for i, (x0, y0) in enumerate(spots):
            half = i % 2 == 1                                            # every other start: a resized suspect, RGBA on two of the bases
            out.append(_case("W", "%dx%d at %d,%d a%d" % (W, H, x0, y0, 1 + (i + b) % 4), W, H, content, (pw0, ph0, x0, y0),
                             (pw0 // 2, ph0 // 2) if half else None, 4 if half and b % 2 else 3, slack=1 + (i + b) % 4))
        out.append(_case("W", "%dx%d pw0 = W" % (W, H), W, H, content, (W, 40, 0, 10 + b), (W // 2, 20), 3, widths=(W - 8, W + 8)))
        out.append(_case("W", "%dx%d ph0 = H" % (W, H), W, H, content, (44, H, 20 + b, 0), None, 4))
        out.append(_case("W", "%dx%d ph0 = 33" % (W, H), W, H, content, (48, 33, 50 + b, 30), None, 3))
        out.append(_case("W", "%dx%d wmin = wmax" % (W, H), W, H, content, (52, 40, 60 + b, 20), (26, 20), 3 + b % 2, widths=(52, 52)))
        # ties decided inside clipped windows: the first position of the first size that is scored
        out.append(_case("W", "%dx%d flat corner" % (W, H), W, H, "flat", (pw0, ph0, W - pw0, H - ph0)))
        out.append(_case("W", "%dx%d foreign corner" % (W, H), W, H, LC.FOREIGN[b % 2], (pw0, ph0, 2, H - ph0 - 1), (pw0 // 2, ph0 // 2), 4))
    out.append(_case("W", "160x32 one size, one position", 160, 32, "noise", (160, 32, 0, 0), (80, 16), 3, widths=(160, 160)))
    return out


# ---- X: (what, start size, suspect size, channels, slack) on a 162 x 98 base ------------------------------------------------------
X_BASE = (162, 98)
# the width ranges are ones the ladder takes too (min(wmin, ph(wmin)) >= 32), for the cases that also go through the public call
X_SHAPES = (("plain", (40, 36), None, 3, 2, (36, 48)), ("resized", (64, 48), (32, 24), 3, 2, (56, 72)), ("rgba", (48, 40), (72, 60), 4, 3, (40, 56)))


def _table_x():
    W, H = X_BASE
    return [_case("X", "%s %s" % (what, content), W, H, content, (pw0, ph0) + _seeded("X", W, H, pw0, ph0), size, ch, slack=a, widths=widths)
            for content in CONTENTS for what, (pw0, ph0), size, ch, a, widths in X_SHAPES]


CASES = _table_t() + _table_w() + _table_x()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def names(table=None):
    return [c.name for c in CASES if table is None or c.table == table]


# ---- pixels ----------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def pixels(name):
    """-> (base [H, W, 3], suspect [sh, sw, channels]); left unchanged by every test."""
    c = BY_NAME[name]
    if c.variant == "foreign":
        lo, hi = (0, 255) if c.content == LC.FOREIGN[0] else (255, 0)
        base, s = np.full((c.H, c.W, 3), lo, np.uint8), np.full((c.size[1], c.size[0], 3), hi, np.uint8)
    else:
        base = LC.frame(c.content, c.H, c.W, seed=ord(c.table))
        s = LC.cut(base, *c.rect)
        if c.variant == "noisy":
            s = LC.noisy(s, len(name))
        if c.variant == "resized":
            s = O.resize_rgb8(s, *c.size)
    if c.channels == 4:
        s = with_alpha(s, len(name))
    for a in (base, s):
        a.setflags(write=False)
    return base, s


# ---- what the stage does with a case ---------------------------------------------------------------------------------------------
def items(c):
    """[(pw, ph, (xa, xb, ya, yb))] of the sizes that are scored, in the stage's order (free_sizes, free_window)."""
    a0 = c.start + (0,)
    out = []
    for pw, ph in free_sizes(a0, c.W, c.H, c.wmin, c.wmax, c.slack):
        win = free_window(a0, c.W, c.H, pw, ph)
        if win[0] <= win[1] and win[2] <= win[3]:
            out.append((pw, ph, win))
    return out


def slot_of(start, a, pw, ph, x, y):
    """(size slot, position slot) of host_sums: relative to the unclipped start."""
    pw0, ph0, x0, y0 = start[:4]
    return (pw - pw0 + a) * (2 * a + 1) + (ph - ph0 + a), SIDE * (y - y0 + NEAR) + (x - x0 + NEAR)


def slot(c, pw, ph, x, y):
    return slot_of(c.start, c.slack, pw, ph, x, y)


def candidate(start, a, size_slot, pos_slot):
    """(pw, ph, x, y) of a slot: slot_of's inverse."""
    pw0, ph0, x0, y0 = start[:4]
    return pw0 - a + size_slot // (2 * a + 1), ph0 - a + size_slot % (2 * a + 1), x0 - NEAR + pos_slot % SIDE, y0 - NEAR + pos_slot // SIDE


def sums_array(start, a, scores):
    """host_sums as include/ssw.h lays it out, from the `scores` of locate_free_ref(..., details=True): all ones where nothing is scored."""
    sums = np.full(((2 * a + 1) ** 2, SIDE * SIDE), EMPTY, np.uint64)
    for (pw, ph, x, y), sad in scores.items():
        sums[slot_of(start, a, pw, ph, x, y)] = sad
    return sums


@lru_cache(maxsize=None)
def reference(name):
    """-> (sums [(2a + 1)^2][81] u64, all ones where nothing is scored; answer (pw, ph, x, y, sad)) of
    locate_free_ref(..., start=..., details=True); the start and 0 when no size is scored at all.  Computed once per case."""
    c = BY_NAME[name]
    base, s = pixels(name)
    best, _, scores = locate_free_ref(base, s, c.wmin, c.wmax, c.slack, start=c.start + (0,), details=True)
    sums = sums_array(c.start, c.slack, scores)
    assert len(scores) == sum((w[1] - w[0] + 1) * (w[3] - w[2] + 1) for _, _, w in items(c))
    sums.setflags(write=False)
    return sums, (best if best is not None else c.start + (0,))


def truth(c):
    """(pw, ph, x, y, sad) that the definition gives where the content decides it, else None
    (tests/test_locate_free_hard_cpu.py confirms each rule with the restatement):
      flat, foreign:  every scored candidate ties -> the first scored size (the smallest pw, then ph) at its window's first
                      position; SAD 0, or 255 pw ph (the oracle's resize keeps a flat 255 suspect at 255 exactly)
      rows, unscaled exact cut:     every pw and x ties at the cut's own height and row -> smallest pw, own ph, xa, the true y
      columns, unscaled exact cut:  -> own pw, smallest ph, the true x, ya
      noise, binary, periodic, exact or resized, started at the truth: the truth; SAD 0 when unscaled"""
    its = items(c)
    x, y, pw, ph = c.rect
    if not its:
        return None
    if c.content == "flat" or c.variant == "foreign":
        p, q, w = its[0]
        return p, q, w[0], w[2], (255 * p * q if c.variant == "foreign" else 0)
    if c.variant == "exact" and c.content == "rows":
        at = [(p, w) for p, q, w in its if q == ph and w[2] <= y <= w[3]]
        return (at[0][0], ph, at[0][1][0], y, 0) if at else None
    if c.variant == "exact" and c.content == "columns":
        at = [(q, w) for p, q, w in its if p == pw and w[0] <= x <= w[1]]
        return (pw, at[0][0], x, at[0][1][2], 0) if at else None
    if c.content in ("noise", "binary", "periodic") and c.variant in ("exact", "resized") and c.start == (pw, ph, x, y):
        return (pw, ph, x, y, 0 if c.variant == "exact" else None)
    return None


# ---- the tiles: tests/cpp/locate_free_plan_test.cpp ------------------------------------------------------------------------------
def build_plan_program(directory):
    """Built the way tests/test_locate_free_cpp_cpu.py builds locate_free_tile_test: hipcc against libssw_hip.so."""
    libdir = os.path.join(ROOT, "spread_spectrum_watermarking_amd", "lib")
    exe = os.path.join(str(directory), "locate_free_plan_test")
    subprocess.run(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "--offload-arch=gfx950", os.path.join(ROOT, "tests", "cpp", "locate_free_plan_test.cpp"),
                    "-I", os.path.join(ROOT, "spread_spectrum_watermarking_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                    "-o", exe, "-L", libdir, "-lssw_hip", f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


Tile = namedtuple("Tile", "oyb oxb tiles_x tiles_y lds")


def tiles(exe, cases):
    """{case name: [Tile of every item, in items()'s order]}: one run of the program over every item of `cases`."""
    lines = ["%d %d %d %d %d" % (c.size[0], c.size[1], c.channels, pw, ph) for c in cases for pw, ph, _ in items(c)]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(lines) and "none" not in out and "bad line" not in out, out[-3:]
    it, got = iter(out), {}
    for c in cases:
        got[c.name] = [Tile(*(int(v) for v in next(it).split())) for _ in items(c)]
    return got
