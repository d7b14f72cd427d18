"""Locating scaled cut-outs whose aspect ratio was not kept exactly (ssw_locate_free_rgb8): the parts that need no GPU -- the
numpy restatement of the definition in include/ssw.h (the yardstick of tests/test_locate_free_gpu.py, which imports it from
here), built from `locate_scaled_ref`, `restored` and `luma` of the files that check those; what it finds on the reference's
photograph (recorded in tests/golden/locate_free_answers.json by tests/golden/gen_locate_free.py); `Locate(aspect=...)`, the
CLI's --locate FILE=W0..W1~A, and the library calls `locate` makes, on a recording stand-in.

The record holds, per case and slack, the ladder's answer, the free answer and its SAD.  A full ladder over 240 .. 640 takes
the restatement 4 - 12 s, so the tests here run it for FOUR of the twelve crop thumbnails, one per answer the ladder gives
(and for the short ranges); for the others the stage is re-derived from the recorded ladder answer, which the generator took from the full restatement."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import fake_ssw
from conftest import GOLDEN, ROOT
from oracle import oracle as O
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd import api, cli
from test_locate_cpu import cat, cut, luma, restored
from test_locate_scale_cpu import EXTRA, SIX, locate_scaled_ref, with_alpha
from test_locate_scale_cpu import case as scale_case
from test_locate_scale_cpu import recorded as scale_recorded

NEAR, SLACK_MAX, MIN_SIDE = 4, 4, 32
ANSWERS = os.path.join(GOLDEN, "locate_free_answers.json")


# ---- the definition of include/ssw.h (ssw_locate_free_rgb8), restated -----------------------------------------------------------
def free_sizes(a0, W, H, wmin, wmax, a):
    """Step 2: the sizes, in the order (pw, ph)."""
    pw0, ph0 = a0[:2]
    return [(pw, ph) for pw in range(max(pw0 - a, wmin, MIN_SIDE), min(pw0 + a, wmax, W) + 1)
            for ph in range(max(ph0 - a, MIN_SIDE), min(ph0 + a, H) + 1)]


def free_window(a0, W, H, pw, ph):
    """Step 3: (x_first, x_last, y_first, y_last) of one size; empty when first > last."""
    x0, y0 = a0[2:4]
    return max(0, x0 - NEAR), min(W - pw, x0 + NEAR), max(0, y0 - NEAR), min(H - ph, y0 + NEAR)


def locate_free_ref(base, s, wmin, wmax, a, start=None, details=False):
    """-> (pw, ph, x, y, sad): the smallest sad / (pw ph), ties to the smaller pw, then ph, then y, then x.  start: the
    ladder's answer A0 when the caller already has it, else `locate_scaled_ref` runs."""
    if not 1 <= a <= SLACK_MAX:
        raise ValueError("slack")
    H, W = base.shape[:2]
    a0 = tuple(start) if start is not None else locate_scaled_ref(base, s, wmin, wmax)
    lo = luma(base).astype(np.int32)
    best, scores = None, {}
    for pw, ph in free_sizes(a0, W, H, wmin, wmax, a):
        xa, xb, ya, yb = free_window(a0, W, H, pw, ph)
        if xa > xb or ya > yb:
            continue
        lr = luma(restored(s, pw, ph)).astype(np.int32)
        for y in range(ya, yb + 1):
            for x in range(xa, xb + 1):
                sad = int(np.abs(lr - lo[y:y + ph, x:x + pw]).sum())
                scores[(pw, ph, x, y)] = sad
                if best is None or sad * best[0] * best[1] < best[4] * pw * ph:        # visited in (pw, ph, y, x) order: ties keep the first
                    best = (pw, ph, x, y, sad)
    return (best, a0, scores) if details else best


# ---- the cases: name -> (base, suspect, wmin, wmax, truth (x, y, w, h) or None) ----------------------------------------------------
@functools.lru_cache(maxsize=None)
def crop_thumb(th, copy, alpha):
    """The 480 x 333 piece at 80,55 of marked copy `copy` (the crop rows' copies: k = 1000, default_rng(3)), halved by
    Pillow's BICUBIC to 240 x th"""
    from test_crop_cpu import marked_copies
    from test_resample_cpu import FILTERS, resample_ref
    return resample_ref(cut(marked_copies(alpha)[copy], 80, 55, 480, 333), 240, th, FILTERS["bicubic"])


CROPS = ["crop 240x%d copy %d alpha %s" % (th, c, al) for th in (166, 167) for c in range(3) for al in (0.1, 0.02)]
# (rectangle, thumbnail, range): the oracle's CatmullRom makes the thumbnail
OFF_ASPECT = {"407x326 -> 203x163": ((161, 61, 407, 326), (203, 163), (391, 423)),
              "400x320 -> 200x159": ((161, 61, 400, 320), (200, 159), (300, 500)),
              "400x320 -> 200x158": ((161, 61, 400, 320), (200, 158), (300, 500)),
              "400x320 -> 203x160": ((161, 61, 400, 320), (203, 160), (300, 500)),
              "corner 300x200 -> 151x100": ((340, 244, 300, 200), (151, 100), (200, 400)),
              "background 300x200 -> 150x101": ((0, 0, 300, 200), (150, 101), (200, 400)),      # the known limit: recorded, not the truth
              "34x34 unscaled": ((300, 150, 34, 34), None, (32, 56)),
              # enlargement factors whose cheapest resize tile leaves no room for the window: the tile is chosen with it counted
              "x3: 480x333 -> 160x111": ((80, 55, 480, 333), (160, 111), (456, 504)),
              "x0.95: 300x200 -> 316x211": ((170, 120, 300, 200), (316, 211), (284, 316)),
              "rgba x1.2: 360x240 -> 300x200": ((150, 100, 360, 240), (300, 200), (340, 380))}
# the slacks recorded per case; every other case: 2
SLACKS = {"400x320 -> 203x160": (2, 4), "34x34 unscaled": (4,), "crop 240x166 copy 0 alpha 0.02": (2, 4), "crop 240x167 copy 0 alpha 0.02": (2, 4)}
# exact with the first slack listed ("400x320 -> 203x160": only with 4)
EXACT = CROPS + ["407x326 -> 203x163", "400x320 -> 200x159", "400x320 -> 200x158", "corner 300x200 -> 151x100",
                 "x3: 480x333 -> 160x111", "x0.95: 300x200 -> 316x211", "rgba x1.2: 360x240 -> 300x200"]
ALL = CROPS + list(OFF_ASPECT) + list(SIX) + EXTRA


def slacks(name):
    return SLACKS.get(name, (2,))


def case(name):
    if name in SIX or name in EXTRA:
        return scale_case(name)
    base, marked = cat()
    if name.startswith("crop "):
        _, size, _, c, _, al = name.split()
        from test_jpeg_cpu import cat_image
        return cat_image(), crop_thumb(int(size.split("x")[1]), int(c), float(al)), 240, 640, (80, 55, 480, 333)
    rect, size, rng = OFF_ASPECT[name]
    s = cut(marked, *rect)
    s = O.resize_rgb8(s, *size) if size else s
    return base, (with_alpha(s, 5) if name.startswith("rgba ") else s), rng[0], rng[1], rect


def recorded():
    with open(ANSWERS) as f:
        return {k: {int(a): (tuple(v["ladder"]), tuple(v["free"])) for a, v in by.items()} for k, by in json.load(f).items()}


# ---- what it finds ----------------------------------------------------------------------------------------------------------
def check(name, a, got, a0, truth):
    ladder, free = recorded()[name][a]
    print(name, "a", a, "ladder", a0, "->", got, "truth", truth)
    assert a0 == ladder and got == free
    assert got[4] * a0[0] * a0[1] <= a0[4] * got[0] * got[1]                   # A0 is a candidate
    if name in EXACT and (name != "400x320 -> 203x160" or a == 4):
        x, y, w, h = truth
        assert got[:4] == (w, h, x, y)


# one thumbnail per pattern of ladder answer: 480x332 at 80,56, 481x333 at 79,55, 479x333 at 81,55, 480x334 at 80,54
FULL_CROPS = ["crop 240x166 copy 0 alpha 0.02", "crop 240x166 copy 1 alpha 0.1", "crop 240x167 copy 0 alpha 0.02", "crop 240x167 copy 1 alpha 0.02"]


@pytest.mark.parametrize("name", FULL_CROPS + list(OFF_ASPECT))
def test_the_full_restatement(name):
    """Ladder and stage from the suspect alone.  480 x 333 halved to 240 x 166: the ladder answers 480 x 332 at 80,56, the
    stage the truth.  The background piece is the documented ambiguous case: recorded, not the truth."""
    base, s, lo, hi, truth = case(name)
    a0 = None
    for a in slacks(name):
        got, a0, _ = locate_free_ref(base, s, lo, hi, a, start=a0, details=True)
        check(name, a, got, a0, truth)
    if name == "background 300x200 -> 150x101":
        assert recorded()[name][2][1][:4] != (300, 200, 0, 0)
    if name == "34x34 unscaled":                                                # the sizes are clipped at 32: 32 .. 38, not 30 .. 38
        assert a0[:4] == (34, 34, 300, 150) and free_sizes(a0, 640, 444, lo, hi, 4)[0] == (32, 32) and len(free_sizes(a0, 640, 444, lo, hi, 4)) == 49


@pytest.mark.parametrize("name", [c for c in CROPS if c not in FULL_CROPS])
def test_the_crop_thumbnails_from_their_recorded_ladder_answers(name):
    """The other eight thumbnails: the stage re-derived from the ladder answer the generator recorded from the full
    restatement.  Every one becomes 480 x 333 at 80,55."""
    base, s, lo, hi, truth = case(name)
    for a in slacks(name):
        ladder = recorded()[name][a][0]
        check(name, a, locate_free_ref(base, s, lo, hi, a, start=ladder), ladder, truth)


@pytest.mark.parametrize("name", list(SIX) + EXTRA)
def test_the_recorded_ladder_cases_keep_their_rectangle(name):
    """The 15 cases of locate_scale_answers.json (checked against the ladder's restatement by tests/test_locate_scale_cpu.py):
    with a = 2 the stage answers the same rectangle wherever the ladder was exact, and never a worse one."""
    base, s, lo, hi, (x, y, w, h) = case(name)
    ladder = scale_recorded()[name]
    got = locate_free_ref(base, s, lo, hi, 2, start=ladder)
    check(name, 2, got, ladder, None)
    if ladder[:4] == (w, h, x, y):
        assert got == ladder
    if name == "rgba":
        assert got == recorded()["narrow rgb"][2][1]


def test_sizes_windows_and_ties():
    assert free_sizes((480, 332, 80, 56, 0), 640, 444, 240, 640, 2) == [(pw, ph) for pw in range(478, 483) for ph in range(330, 335)]
    assert len(free_sizes((480, 332, 80, 56, 0), 640, 444, 240, 640, 4)) == 81
    assert free_sizes((400, 320, 0, 0, 0), 640, 444, 400, 400, 1) == [(400, 319), (400, 320), (400, 321)]            # wmin == wmax
    assert free_sizes((639, 443, 0, 0, 0), 640, 444, 300, 900, 2) == [(pw, ph) for pw in range(637, 641) for ph in range(441, 445)]
    assert free_sizes((33, 40, 0, 0, 0), 640, 444, 20, 900, 3) == [(pw, ph) for pw in range(32, 37) for ph in range(37, 44)]
    assert free_window((300, 199, 340, 244, 0), 640, 444, 300, 200) == (336, 340, 240, 244)
    assert free_window((300, 199, 340, 244, 0), 640, 444, 301, 201)[:2] == (336, 339)
    xa, xb, _, _ = free_window((300, 199, 340, 244, 0), 640, 444, 305, 199)
    assert xa > xb                                                              # an empty window
    assert free_window((600, 430, 3, 5, 0), 640, 444, 600, 430) == (0, 7, 1, 9)
    for bad in (0, 5, -1):
        with pytest.raises(ValueError):
            locate_free_ref(np.zeros((64, 64, 3), np.uint8), np.zeros((40, 40, 3), np.uint8), 32, 48, bad, start=(40, 40, 0, 0, 0))
    # ties: on a flat frame every candidate costs 0 -- the smallest pw, then ph, then y, then x
    flat = np.full((64, 80, 3), 9, np.uint8)
    assert locate_free_ref(flat, np.full((40, 40, 3), 9, np.uint8), 32, 48, 2, start=(40, 40, 10, 10, 0)) == (38, 38, 6, 6, 0)


# ---- header, ABI ---------------------------------------------------------------------------------------------------------------
def test_header_states_the_free_stage():
    text = open(os.path.join(ROOT, "include", "ssw.h")).read()
    assert text.index("ssw_locate_scaled_rgb8(ssw_ctx") < text.index("a free height") < text.index("ssw_locate_free_rgb8(ssw_ctx")
    doc = " ".join(text[text.index("a free height"):text.index("ssw_locate_free_rgb8(ssw_ctx")].split())
    for phrase in ("1 <= a <= 4", "exactly what ssw_locate_scaled_rgb8 answers", "status codes pass through", "|pw - pw0| <= a", "|ph - ph0| <= a",
                   "wmin <= pw <= wmax", "min(pw, ph) >= 32", "pw <= W, ph <= H", "free of the aspect rule", "[x0 - 4, x0 + 4]", "[0, W - pw]",
                   "[y0 - 4, y0 + 4]", "[0, H - ph]", "empty after clipping contributes nothing", "over all pw ph pixels", "resize_common.hpp",
                   "alpha channel is ignored", "No coarse pass and no top-8", "smallest SAD / (pw ph)", "cross-multiplication in 64 bits",
                   "ties: smaller pw, then smaller ph, then y, then x", "never above A0's", "at most 81 sizes x 81 positions",
                   "beyond +-4 pixels are not searched", "deliberately squeezed picture", "smooth regions stay ambiguous", "R is never stored",
                   "waits for the stream three times", "SSW_ERR_BAD_ARG", "SSW_ERR_UNSUPPORTED", "n == 0: SSW_OK", "SSW_STAGE_LOCATE", "SSW_STAGE_RESIZE",
                   "pw, ph, x, y of each placement are OUTPUTS"):
        assert phrase in doc, phrase
    sig = L.SIGNATURES["ssw_locate_free_rgb8"][1]
    assert len(sig) == 10 and sig[:7] == L.SIGNATURES["ssw_locate_scaled_rgb8"][1][:7] and sig[7] == C.POINTER(C.c_uint32)
    assert "SSW_STAGE_COUNT = 15" in text and len(L.STAGES) == 15 and L.LOCATE_FREE_MAX_SLACK == SLACK_MAX


# ---- Python: Locate(aspect=...) -----------------------------------------------------------------------------------------------
def test_aspect_entries_are_validated():
    import spread_spectrum_watermarking_amd as wm
    assert wm.Locate(widths=(300, 900), aspect=2).aspect_slack() == 2 and api.Locate(scale=(0.5, 2), aspect=4).aspect_slack() == 4
    assert api.Locate(widths=(300, 900)).aspect_slack() == 0 and api.Locate(widths=(300, 900), aspect=0).aspect_slack() == 0
    assert api.Locate().aspect_slack() == 0 and api.Locate(60, 50).aspect_slack() == 0 and api.Locate().aspect is None
    assert api.Locate(widths=(300, 900), aspect=2).width_range(200) == (300, 900)
    assert api.Locate(widths=(3, 4)) == api.Locate(None, None, (3, 4), None, None, None) != api.Locate(widths=(3, 4), aspect=1)
    for bad in (api.Locate(widths=(3, 9), aspect=5), api.Locate(widths=(3, 9), aspect=-1), api.Locate(widths=(3, 9), aspect=1.5),
                api.Locate(widths=(3, 9), aspect=True), api.Locate(60, 50, aspect=1), api.Locate(aspect=2), api.Locate(60, 50, aspect=0)):
        with pytest.raises(ValueError):
            bad.aspect_slack()
        with pytest.raises(ValueError):
            bad.width_range(100)
    for bad in (api.Locate(turned=True, aspect=1), api.Locate(turned=(-3, 3), aspect=0)):
        with pytest.raises(ValueError):
            bad.turned_range()
    f = api.Located(api.Placement(80, 55, 480, 333), 400000, 400000 / (480 * 333))
    assert f.size == (480, 333)


# ---- CLI ---------------------------------------------------------------------------------------------------------------------
def test_locate_option_takes_a_slack_after_a_range():
    p = cli.build_parser()
    common = ["trace", "cat.jpg", "--suspects", "cut.png", "b=c.png", "--marks", "x.json"]
    a = p.parse_args(common + ["--locate", "cut.png=300..900~2", "--locate", "b=c.png=64..64~4"])
    assert a.locates == {"cut.png": api.Locate(widths=(300, 900), aspect=2), "b=c.png": api.Locate(widths=(64, 64), aspect=4)}
    assert cli.parse_locate("cut.png=300..900~0", ["cut.png"]) == ("cut.png", api.Locate(widths=(300, 900), aspect=0))
    assert cli.parse_locate("cut.png=300..900", ["cut.png"]) == ("cut.png", api.Locate(widths=(300, 900)))          # as before
    for bad in ("cut.png=300..900~5", "cut.png=300..900~", "cut.png=300..900~-1", "cut.png=300..900~2~2", "cut.png=300..900~1.5", "cut.png=300..900~02",
                "cut.png=300~2..900", "cut.png=400x320~2", "cut.png~2", "cut.png=rotate:?~2", "cut.png=300..900 ~2", "cut.png=300..900~٢"):
        with pytest.raises(ValueError):
            cli.parse_locate(bad, ["cut.png"])
        with pytest.raises(SystemExit):
            p.parse_args(common + ["--locate", bad])
    f = api.Located(api.Placement(80, 55, 480, 333), 479520, 3.0)
    assert cli.located_text(f, True) == "80,55 as 480x333 (mean luma difference 3.00)"           # the record reads as before


# ---- the library calls `locate` makes -------------------------------------------------------------------------------------------
class AnsweringLib(fake_ssw.FakeLib):
    """fake_ssw's recording stand-in, whose locate calls also answer: pw = 400 + 10 i, ph = 320, x = i, y = 2 i, SAD = 1000"""
    def _call(self, name, args):
        rc = super()._call(name, args)
        if name in ("ssw_locate_rgb8", "ssw_locate_scaled_rgb8", "ssw_locate_free_rgb8"):
            pl, n, sad = args[5], int(args[-2]), args[-1]
            for i in range(n):
                if name != "ssw_locate_rgb8":
                    pl[i].pw, pl[i].ph = 400 + 10 * i, 320
                pl[i].x, pl[i].y, sad[i] = i, 2 * i, 1000
        return rc


def answering_context():
    ctx = api.Context.__new__(api.Context)
    ctx._lib, ctx.handle, ctx.device_id = AnsweringLib(), C.c_void_p(fake_ssw.HANDLE), 0
    return ctx


def locate_calls(entries):
    base = np.zeros((444, 640, 3), np.uint8)
    sus = [np.zeros((50 + i, 60 + i, 3 + i % 2), np.uint8) for i in range(len(entries))]
    ctx = answering_context()
    found = api.locate(base, sus, entries, ctx=ctx)
    assert not ctx._lib.live                                                   # every device block was freed
    return [c for c in ctx._lib.calls if c[0].startswith("ssw_locate")], found


def test_entries_without_aspect_make_exactly_the_calls_of_before():
    plain = [api.Locate(), api.Locate(widths=(300, 500)), api.Locate(60, 50), api.Locate(scale=(1, 4))]
    calls, _ = locate_calls(plain)
    assert [c[0] for c in calls] == ["ssw_locate_rgb8", "ssw_locate_scaled_rgb8"]
    zero, _ = locate_calls([api.Locate(), api.Locate(widths=(300, 500), aspect=0), api.Locate(60, 50), api.Locate(scale=(1, 4), aspect=None)])
    assert zero == calls                                                       # aspect 0 / None: the same calls with the same arguments
    only, _ = locate_calls([api.Locate(), api.Locate(60, 50)])
    assert [c[0] for c in only] == ["ssw_locate_rgb8"]
    # with aspect entries beside them: the same two calls, same arguments, same order, then the new one
    mixed, found = locate_calls([api.Locate(), api.Locate(widths=(300, 500)), api.Locate(widths=(200, 640), aspect=2), api.Locate(60, 50),
                                 api.Locate(scale=(1, 4)), api.Locate(scale=(2, 3), aspect=4)])
    assert [c[0] for c in mixed] == ["ssw_locate_rgb8", "ssw_locate_scaled_rgb8", "ssw_locate_free_rgb8"]
    assert [len(c[1]) for c in mixed] == [8, 9, 10]
    assert [c[1][-2] for c in mixed] == [2, 2, 2]                              # n of each call
    assert [f.size for f in found] == [(60, 50), (400, 320), (400, 320), (60, 50), (410, 320), (410, 320)]
    assert [(f.placement.x, f.placement.y) for f in found] == [(0, 0), (0, 0), (0, 0), (1, 2), (1, 2), (1, 2)]


def test_entries_with_aspect_make_one_call():
    calls, found = locate_calls([api.Locate(widths=(300, 500), aspect=1), api.Locate(scale=(2, 3), aspect=4), api.Locate(widths=(64, 64), aspect=2)])
    assert [c[0] for c in calls] == ["ssw_locate_free_rgb8"]
    args = calls[0][1]
    assert args[0] == "ctx" and args[1][0] == "dev" and args[2:4] == [640, 444] and args[8] == 3
    assert args[6] == bytes((L.ScaleRange * 3)(L.ScaleRange(300, 500), L.ScaleRange(122, 183), L.ScaleRange(64, 64))).hex()      # scale=(2, 3) of a 61-wide suspect
    assert args[7] == bytes((C.c_uint32 * 3)(1, 4, 2)).hex()
    assert [f.size for f in found] == [(400, 320), (410, 320), (420, 320)] and found[2].sad == 1000
    # through _resolve_locates, as trace_many and Reader.trace go: still one call, and the placements found
    base = np.zeros((444, 640, 3), np.uint8)
    sus = [np.zeros((50, 60, 3), np.uint8), np.zeros((44, 64, 3), np.uint8)]
    ctx = answering_context()
    out, got = api._resolve_locates(base, sus, [api.Locate(widths=(240, 640), aspect=2), api.Placement(1, 2)], ctx)
    assert [c[0] for c in ctx._lib.calls if c[0].startswith("ssw_locate")] == ["ssw_locate_free_rgb8"]
    assert out == [api.Placement(0, 0, 400, 320), api.Placement(1, 2)] and sorted(got) == [0]
