"""Hard inputs for the cut-out search (csrc/locate.hip): tie-heavy and saturated frames, the suspect variants cut from them,
and the tables of shapes that sit on the edges of the coarse kernel's template chunk, of its candidate tile and of the eight
rounds of the top-k.  numpy only: tests/test_locate_hard_cpu.py pins what every table claims to reach -- against the constants
read out of locate.hip -- and the tie structure of every content by the restatement alone; tests/test_locate_hard_gpu.py runs
the same cases on the device.

A case is (table, W, H, content): one base frame and every suspect of the table that is searched in it (all rectangles x
variants), so one `locate` call carries them all."""
import os
import re
from collections import namedtuple
from functools import lru_cache

import numpy as np

from conftest import ROOT
from oracle import oracle as O
from test_jpeg_cpu import content as jpeg_content

SOURCE = os.path.join(ROOT, "spread_spectrum_watermarking_amd", "csrc", "locate.hip")


# ---- the constants of locate.hip and the arithmetic of plan_items / coarse_desc / locate_coarse_kernel --------------------------
@lru_cache(maxsize=None)
def constants():
    """LOC_* of csrc/locate.hip, + TOPK_PER_BLOCK / TOPK_BLOCKS: the candidates one sweep of locate_topk_kernel's grid covers."""
    text = open(SOURCE).read()
    c = {k: int(v) for k, v in re.findall(r"\b(LOC_[A-Z]+) = (\d+)\b", text)}
    m = re.search(r"topk_blocks\(uint32_t max_n\) \{ return [^;]*\+ (\d+)\) / (\d+), (\d+)\); \}", text)
    assert m and int(m.group(1)) + 1 == int(m.group(2)), "topk_blocks: not the expression this file knows"
    c["TOPK_PER_BLOCK"], c["TOPK_BLOCKS"] = int(m.group(2)), int(m.group(3))
    for name in ("LOC_BATCH", "LOC_TOP", "LOC_TX", "LOC_TY", "LOC_YPL", "LOC_JB", "LOC_KW"):
        assert name in c, name
    return c


Plan = namedtuple("Plan", "f tw th nx ny tiles_x tiles_y phases")        # phases: [(px, py, nxp, nyp)] in the kernel's order


def plan(W, H, pw, ph):
    """What plan_items, coarse_desc and the head of locate_coarse_kernel compute for a pw x ph suspect in a W x H frame."""
    c = constants()
    f = 4 if min(pw, ph) >= 64 else 1
    tw, th = (pw // 4, ph // 4) if f == 4 else (pw, ph)
    nx, ny = W - pw + 1, H - ph + 1
    up = lambda v, a: (v + a - 1) // a
    tiles_x, tiles_y = up(up(nx, f), c["LOC_TX"]), up(up(ny, f), c["LOC_TY"])
    phases = [(p % f, p // f, up(nx - p % f, f) if nx > p % f else 0, up(ny - p // f, f) if ny > p // f else 0) for p in range(f * f)]
    return Plan(f, tw, th, nx, ny, tiles_x, tiles_y, phases)


def chunk_bytes():
    return 4 * constants()["LOC_KW"]


# ---- contents ---------------------------------------------------------------------------------------------------------------------
CONTENTS = ("noise", "binary", "cat+noise", "flat", "periodic", "rows", "columns")
FOREIGN = ("foreign 255 over 0", "foreign 0 over 255")       # not a frame of its own kind: an all-0 / all-255 base, see `case`
CELL_W, CELL_H = 16, 8


def frame(kind, h, w, seed=0):
    """[h, w, 3] u8.  noise / binary / cat+noise: tests/test_jpeg_cpu.py's.  flat: one colour -- every candidate ties at every
    stage.  periodic: a random 8-row x 16-column cell, tiled -- exact ties at every (16, 8) shift.  rows / columns: each row /
    column one random colour -- every x / every y ties."""
    if kind in ("noise", "binary", "cat+noise"):
        return np.ascontiguousarray(jpeg_content(kind, h, w, seed))
    rng = np.random.default_rng([seed, h, w, CONTENTS.index(kind)])
    if kind == "flat":
        return np.ascontiguousarray(np.broadcast_to(rng.integers(0, 256, 3, dtype=np.uint8), (h, w, 3)))
    if kind == "periodic":
        cell = rng.integers(0, 256, (CELL_H, CELL_W, 3), dtype=np.uint8)
        return np.ascontiguousarray(np.tile(cell, (-(-h // CELL_H), -(-w // CELL_W), 1))[:h, :w])
    if kind == "rows":
        return np.ascontiguousarray(np.broadcast_to(rng.integers(0, 256, (h, 1, 3), dtype=np.uint8), (h, w, 3)))
    if kind == "columns":
        return np.ascontiguousarray(np.broadcast_to(rng.integers(0, 256, (1, w, 3), dtype=np.uint8), (h, w, 3)))
    raise KeyError(kind)


# ---- suspect variants -------------------------------------------------------------------------------------------------------------
def cut(img, x, y, w, h):
    return np.ascontiguousarray(img[y:y + h, x:x + w])


def noisy(c, seed):
    """The cut plus integers in [-2, 2], clipped: on periodic / rows / columns content, ties with a non-zero SAD."""
    n = np.random.default_rng([seed, 77]).integers(-2, 3, c.shape)
    return np.clip(c.astype(np.int16) + n, 0, 255).astype(np.uint8)


# ---- case tables: (W, H, pw, ph) --------------------------------------------------------------------------------------------------
def _on(W, H, sizes):
    return [(W, H, pw, ph) for pw, ph in sizes]


TABLES = {
    # A. template chunk edges, f = 1
    "A": _on(200, 150, [(1, 1), (2, 7), (3, 8), (4, 9), (5, 16), (61, 17), (63, 8), (64, 8), (65, 9), (67, 1), (127, 7), (128, 16),
                        (129, 17), (131, 63), (63, 131), (64, 63), (63, 64)]),
    # B. template chunk edges, f = 4, W % 4 == 3
    "B": _on(331, 141, [(64, 64), (67, 71), (68, 64), (71, 68), (252, 64), (255, 67), (256, 68), (259, 71), (260, 64)]),
    # C. candidate tile edges, f = 1: base (nx + 15) x (ny + 15), suspect 16 x 16
    "C": [(nx + 15, ny + 15, 16, 16) for nx, ny in ((63, 31), (64, 32), (65, 33), (129, 65), (64, 33), (65, 32))],
    # D. candidate tile edges, f = 4: base (nx + 63) x (ny + 63), suspect 64 x 64
    "D": [(nx + 63, ny + 63, 64, 64) for nx, ny in ((253, 125), (256, 128), (257, 129), (260, 132), (261, 133), (257, 128), (256, 129))],
    # E. 1, 2, 3, 7, 8, 9 and 9 candidates, for both f
    "E": _on(40, 30, [(40, 30), (39, 30), (40, 28), (34, 30), (33, 30), (32, 30), (38, 28)])
         + _on(72, 70, [(72, 70), (71, 70), (72, 68), (66, 70), (65, 70), (64, 70), (70, 68)]),
    # F. more candidates than one sweep of the top-k grid
    "F": [(1100, 1000, 8, 8)],
}
TABLE_CONTENTS = {t: CONTENTS + FOREIGN for t in "ABCDE"}
TABLE_CONTENTS["F"] = ("flat", "rows", "noise")
# G. known-size resized suspects (sizes=): (pw, ph) of an f = 1 and an f = 4 target on table A's base, each halved, doubled and
# scaled by 3 / 2 before it is handed in, + the halved f = 4 one as RGBA.  binary: CatmullRom overshoots 0 / 255 in both directions,
# so the restore resize clamps at both ends before the search sees the frame.
G_BASE = (200, 150)
G_TARGETS = ((48, 36), (96, 72))
G_SCALES = (("halved", 1, 2), ("doubled", 2, 1), ("x 3/2", 3, 2))
G_CONTENTS = ("binary", "noise")


def bases(table):
    """The (W, H) of a table, each once, in the table's order."""
    out = []
    for W, H, _, _ in TABLES[table]:
        if (W, H) not in out:
            out.append((W, H))
    return out


def ids():
    """(table, W, H, content) of every case of the tables A to F."""
    return [(t, W, H, c) for t in TABLES for W, H in bases(t) for c in TABLE_CONTENTS[t]]


def position(table, W, H, pw, ph):
    """Where the table's pw x ph rectangle is cut from its W x H base: seeded, anywhere it fits."""
    rng = np.random.default_rng([ord(table), W, H, pw, ph])
    return int(rng.integers(0, W - pw + 1)), int(rng.integers(0, H - ph + 1))


Suspect = namedtuple("Suspect", "name rect variant pixels size")         # rect: (x, y, pw, ph) of the cut; size: sizes= entry or None


@lru_cache(maxsize=4)
def case(table, W, H, content):
    """-> (base [H, W, 3], [Suspect]) of one id of the tables A to F: every rectangle of the table on this base, exact and
    noisy; for the two foreign contents one all-255 (all-0) suspect per rectangle over an all-0 (all-255) base."""
    rects = [position(table, W, H, pw, ph) + (pw, ph) for w_, h_, pw, ph in TABLES[table] if (w_, h_) == (W, H)]
    if content in FOREIGN:
        lo, hi = (0, 255) if content == FOREIGN[0] else (255, 0)
        base = np.full((H, W, 3), lo, np.uint8)
        return base, [Suspect("%dx%d foreign" % r[2:], r, "foreign", np.full((r[3], r[2], 3), hi, np.uint8), None) for r in rects]
    base = frame(content, H, W, seed=ord(table))
    sus = []
    for i, r in enumerate(rects):
        c = cut(base, *r)
        sus.append(Suspect("%dx%d exact" % r[2:], r, "exact", c, None))
        sus.append(Suspect("%dx%d noisy" % r[2:], r, "noisy", noisy(c, i), None))
    return base, sus


@lru_cache(maxsize=2)
def case_g(content):
    """-> (base, [Suspect]) of table G: 2 targets x 3 scales, + one RGBA form with random alpha (its answer: the RGB one's)."""
    W, H = G_BASE
    base = frame(content, H, W, seed=ord("G"))
    sus = []
    for pw, ph in G_TARGETS:
        r = position("G", W, H, pw, ph) + (pw, ph)
        for name, num, den in G_SCALES:
            s = O.resize_rgb8(cut(base, *r), pw * num // den, ph * num // den)
            sus.append(Suspect("%dx%d %s" % (pw, ph, name), r, "resized", s, (pw, ph)))
    half = sus[len(G_SCALES)]                                              # the f = 4 target, halved
    alpha = np.random.default_rng(5).integers(0, 256, half.pixels.shape[:2] + (1,), dtype=np.uint8)
    sus.append(Suspect(half.name + " rgba", half.rect, "resized", np.ascontiguousarray(np.concatenate([half.pixels, alpha], 2)), half.size))
    return base, sus


# ---- the scale ladder (ssw_locate_scaled_rgb8): name -> (size of the cut, size it is resized to or None, (wmin, wmax)) -------------
LADDER_BASE = (320, 192)
LADDER_CONTENTS = ("noise", "binary", "flat", "periodic", "rows", "columns")
LADDER = {"160x96 halved": ((160, 96), (80, 48), (120, 200)),
          "129x65 unscaled": ((129, 65), None, (100, 140)),
          "48x40 doubled": ((48, 40), (96, 80), (40, 72))}


def ladder_case(content, name):
    """-> (base, suspect, wmin, wmax, (x, y, pw, ph) of the cut)"""
    W, H = LADDER_BASE
    (pw, ph), size, (lo, hi) = LADDER[name]
    base = frame(content, H, W, seed=ord("L"))
    r = position("L", W, H, pw, ph) + (pw, ph)
    c = cut(base, *r)
    return base, (O.resize_rgb8(c, *size) if size else c), lo, hi, r


# ---- what the search must answer where the content decides it ----------------------------------------------------------------------
MIN_UNIQUE = 14     # pixels of noise / binary (8 lumas: 42 bits) that occur once in a frame of < 2^21 positions, near enough


def truth(content, s):
    """(x, y, sad) that the definition gives for suspect `s` of a `content` base, or None where the content does not decide it.
    tests/test_locate_hard_cpu.py confirms each rule with the restatement.
      flat, exact:      every candidate has D = SAD = 0 -> the first, (0, 0)
      periodic, exact:  a cut that spans a whole cell matches at the (16, 8) shifts only -> the first of them
      rows, exact:      every x ties, the rows (4 or more: 32 bits of luma) occur once -> (0, y)
      columns, exact:   every y ties -> (x, 0)
      foreign:          every candidate ties at the largest difference -> (0, 0), 255 per pixel
      noise, binary, cat+noise, exact: the bytes occur once -> (x, y) with SAD 0
    A noisy cut ties too, but which tied position wins depends on its noise: equality with the restatement is its check."""
    x, y, pw, ph = s.rect
    if s.variant == "foreign":
        return 0, 0, 255 * pw * ph
    if s.variant != "exact":
        return None
    if content == "flat":
        return 0, 0, 0
    if content == "periodic":
        return (x % CELL_W, y % CELL_H, 0) if pw >= CELL_W and ph >= CELL_H else None
    if content == "rows":
        return (0, y, 0) if ph >= 4 else None
    if content == "columns":
        return (x, 0, 0) if pw >= 4 else None
    return (x, y, 0) if pw * ph >= MIN_UNIQUE else None
