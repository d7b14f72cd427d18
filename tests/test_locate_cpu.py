"""Locating cut-outs (ssw_locate_rgb8): the parts that need no GPU -- the numpy restatement of the definition in include/ssw.h
(the yardstick of tests/test_locate_gpu.py, which imports it from here), what it finds on the reference's photograph, the
Python resolution of `Locate` entries and the CLI's --locate."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from oracle import oracle as O
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd import api, cli


# ---- the definition of include/ssw.h (ssw_locate_rgb8), restated ---------------------------------------------------------------
def luma(rgb):
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    return (77 * r + 150 * g + 29 * b + 128) >> 8


def box4(lum):
    """(sum of the 4 x 4 lumas at (x, y) + 8) >> 4 at every position where the box fits: [h - 3][w - 3]."""
    c = np.cumsum(np.cumsum(np.pad(lum, ((1, 0), (1, 0))), 0), 1)
    return (c[4:, 4:] - c[:-4, 4:] - c[4:, :-4] + c[:-4, :-4] + 8) >> 4


def restored(s, pw, ph):
    """Step 1: R = S at its own size, else the CatmullRom resize of its colour channels (the oracle's; alpha is ignored)."""
    rgb = np.ascontiguousarray(s[..., :3])
    return rgb if (s.shape[1], s.shape[0]) == (pw, ph) else O.resize_rgb8(rgb, pw, ph)


def locate_ref(base, r, window=None, details=False):
    """Steps 2-7 on the restored suspect r -> (x, y, sad).  window = (x0, x1, y0, y1), inclusive: only these candidate
    positions (a test's way to bound CPU time on large frames)."""
    (H, W), (ph, pw) = base.shape[:2], r.shape[:2]
    lo, lr = luma(base), luma(r)
    f = 4 if min(pw, ph) >= 64 else 1
    b, t = (box4(lo), box4(lr)[::4, ::4][:ph // 4, :pw // 4]) if f == 4 else (lo, lr)
    x0, x1, y0, y1 = window or (0, W - pw, 0, H - ph)
    nx, ny = x1 - x0 + 1, y1 - y0 + 1
    d = np.zeros((ny, nx), np.int64)
    for j in range(t.shape[0]):
        for i in range(t.shape[1]):
            d += np.abs(b[y0 + f * j:y0 + f * j + ny, x0 + f * i:x0 + f * i + nx] - t[j, i])
    ys, xs = np.mgrid[y0:y1 + 1, x0:x1 + 1]
    top = np.lexsort((xs.ravel(), ys.ravel(), d.ravel()))[:8]                  # smallest (D, y, x)
    fine = [(int(np.abs(lr - lo[y:y + ph, x:x + pw]).sum()), int(y), int(x)) for y, x in zip(ys.ravel()[top], xs.ravel()[top])]
    sad, y, x = min(fine)
    return (x, y, sad, np.sort(d.ravel())[:2]) if details else (x, y, sad)


# ---- what it finds ----------------------------------------------------------------------------------------------------------
CUTS = [(161, 61, 400, 320), (237, 93, 163, 127), (3, 5, 600, 430), (301, 150, 70, 66), (333, 177, 40, 33), (0, 0, 639, 443)]
AMBIGUOUS = (5, 5, 90, 70)          # background only: the documented ambiguous case; the restatement answers (5, 7)


def cat():
    g = np.load(os.path.join(GOLDEN, "cat_decoded_u8.npz"))
    return g["cat"], g["watermarked_with_1"]


def cut(img, x, y, w, h):
    return np.ascontiguousarray(img[y:y + h, x:x + w])


@pytest.mark.parametrize("rect", CUTS, ids=lambda r: "%d,%d,%dx%d" % r)
def test_cut_outs_of_the_marked_cat_are_found_exactly(rect):
    base, marked = cat()
    assert base.shape == (444, 640, 3)
    x, y, w, h = rect
    gx, gy, sad, d2 = locate_ref(base, cut(marked, *rect), details=True)
    print(rect, "->", (gx, gy), "sad", sad, "mean", round(sad / (w * h), 3), "coarse winner / runner-up", d2, round(d2[0] / max(d2[1], 1), 3))
    assert (gx, gy) == (x, y)
    assert sad == int(np.abs(luma(cut(marked, *rect)) - luma(cut(base, *rect))).sum())
    assert (min(w, h) >= 64) == (rect != (333, 177, 40, 33))            # the one case of the f = 1 path


@pytest.mark.parametrize("rect,div", [((161, 61, 400, 320), 2), ((237, 93, 164, 128), 4)], ids=["halved", "quartered"])
def test_scaled_cut_outs_given_back_their_size_are_found_exactly(rect, div):
    base, marked = cat()
    x, y, w, h = rect
    small = O.resize_rgb8(cut(marked, *rect), w // div, h // div)
    gx, gy, sad = locate_ref(base, restored(small, w, h))
    print(rect, "/", div, "->", (gx, gy), "mean", round(sad / (w * h), 3))
    assert (gx, gy) == (x, y)


def test_background_only_cut_out_is_the_documented_ambiguous_case():
    base, marked = cat()
    gx, gy, sad = locate_ref(base, cut(marked, *AMBIGUOUS))
    print("ambiguous", AMBIGUOUS, "->", (gx, gy), "sad", sad)
    assert (gx, gy) == (5, 7)            # recorded, not the truth (5, 5): the grey background has no features to hold on to


def test_alpha_is_ignored_and_tiny_suspects_work():
    base, marked = cat()
    c = cut(marked, 301, 150, 70, 66)
    rgba = np.concatenate([c, np.random.default_rng(1).integers(0, 256, c.shape[:2] + (1,), dtype=np.uint8)], 2)
    assert locate_ref(base, restored(rgba, 70, 66)) == locate_ref(base, c)
    x, y, sad = locate_ref(base, cut(base, 7, 9, 1, 1))
    assert sad == 0 and luma(base)[y, x] == luma(base)[9, 7]             # the first pixel of that luma in (y, x) order
    assert (luma(base)[:y].ravel() != luma(base)[9, 7]).all() and (luma(base)[y, :x] != luma(base)[9, 7]).all()
    assert locate_ref(base, base.copy()) == (0, 0, 0)


# ---- header, ABI ---------------------------------------------------------------------------------------------------------------
def test_header_restates_the_definition():
    text = open(os.path.join(ROOT, "include", "ssw.h")).read()
    doc = text[text.index("locating a cut-out"):text.index("ssw_locate_rgb8(ssw_ctx")]
    for phrase in ("(77 R + 150 G + 29 B + 128) >> 8", "min(pw, ph) >= 64", "+ 8) >> 4", "(D, y, x)", "(SAD, y, x)", "x, y of each placement are OUTPUTS",
                   "mostly transparent is not supported", "featureless region is ambiguous", "synchronises", "bounded for any n",
                   "SSW_ERR_BAD_ARG", "SSW_ERR_UNSUPPORTED", "n == 0: SSW_OK", "SSW_STAGE_LOCATE", "resize_common.hpp", "attack_crop.rs:56-70"):
        assert phrase in doc, phrase
    assert len(L.SIGNATURES["ssw_locate_rgb8"][1]) == 8
    assert L.STAGES[13:] == ["locate", "locate_coarse"] and L.STAGES[8] == "resize" and len(L.STAGES) == 15
    assert "SSW_STAGE_LOCATE = 13" in text and "SSW_STAGE_COUNT = 15" in text and "SSW_STAGE_DCT_COL_MAIN = 12" in text


# ---- Python: Locate entries are resolved with one locate call, without a device ---------------------------------------------------
def test_locate_entries_are_resolved_by_one_call():
    import spread_spectrum_watermarking_amd as wm
    assert wm.Locate is api.Locate and wm.Located is api.Located and callable(wm.locate)
    assert (api.Locate().w, api.Locate().h) == (None, None)
    base = np.zeros((444, 640, 3), np.uint8)
    sus = [np.zeros((50, 60, 3), np.uint8), np.zeros((444, 640, 3), np.uint8), np.zeros((25, 30, 4), np.uint8), np.zeros((8, 8, 3), np.uint8)]
    calls = []

    def fake(b, suspects, sizes, ctx):
        calls.append(([s.shape for s in suspects], list(sizes)))
        return [api.Located(api.Placement(10 + i, 20 + i, z.w or s.shape[1], z.h or s.shape[0]), 100, 0.5) for i, (s, z) in enumerate(zip(suspects, sizes))]
    pls = [api.Locate(), None, api.Locate(60, 50), api.Placement(1, 2)]
    out, found = api._resolve_locates(base, sus, pls, None, fake)
    assert len(calls) == 1 and calls[0][0] == [(50, 60, 3), (25, 30, 4)] and calls[0][1] == [api.Locate(), api.Locate(60, 50)]
    assert out == [api.Placement(10, 20, 60, 50), None, api.Placement(11, 21, 60, 50), api.Placement(1, 2)] and sorted(found) == [0, 2]
    assert pls[0] == api.Locate()                                      # the caller's list is not modified
    # the resolved list is what _placed_suspects takes today
    _, _, pl = api._placed_suspects(sus, out, 640, 444)
    assert [(p.x, p.y, p.pw, p.ph) for p in pl] == [(10, 20, 60, 50), (0, 0, 640, 444), (11, 21, 60, 50), (1, 2, 8, 8)]
    # no Locate entry: nothing is called
    assert api._resolve_locates(base, sus, [None] * 4, None, fake) == ([None] * 4, {}) and len(calls) == 1
    with pytest.raises(ValueError):
        api._resolve_locates(None, sus, pls, None, fake)               # a reader's trace without base=
    with pytest.raises(ValueError):
        api._resolve_locates(base, sus, pls[:2], None, fake)
    # the sizes handed to the C side
    pl = api._locate_sizes(sus[:3], [None, api.Locate(), (60, 50)], 640, 444)
    assert [(p.w, p.h, p.channels, p.x, p.y, p.pw, p.ph) for p in pl] == [(60, 50, 3, 0, 0, 60, 50), (640, 444, 3, 0, 0, 640, 444), (30, 25, 4, 0, 0, 60, 50)]
    for bad in ([api.Locate(5, None)], [(641, 10)], [(10, 445)], [(0, 0)], [None, None]):
        with pytest.raises(ValueError):
            api._locate_sizes(sus[:1], bad, 640, 444)
    import inspect
    for fn in (api.restore, api.trace_many, api.Reader.trace):
        assert "Locate" in inspect.getsource(fn) and "_resolve_locates" in inspect.getsource(fn), fn


# ---- CLI ---------------------------------------------------------------------------------------------------------------------
def test_locate_option_parser():
    p = cli.build_parser()
    common = ["trace", "cat.jpg", "--suspects", "a.png", "b=c.png", "--marks", "x.json"]
    a = p.parse_args(common + ["--locate", "a.png"])
    assert a.locates == {"a.png": api.Locate()} and a.placements == {}
    a = p.parse_args(common + ["--locate", "a.png=400x320", "--locate", "b=c.png"])
    assert a.locates == {"a.png": api.Locate(400, 320), "b=c.png": api.Locate()}
    assert p.parse_args(common + ["--locate", "b=c.png=10x20"]).locates == {"b=c.png": api.Locate(10, 20)}
    assert p.parse_args(common).locates == {}
    a = p.parse_args(common + ["--locate", "a.png", "--place", "b=c.png=1,2"])
    assert a.locates == {"a.png": api.Locate()} and a.placements == {"b=c.png": api.Placement(1, 2, None, None)}
    for bad in ("a.png=400", "a.png=400x", "a.png=x320", "a.png=0x5", "a.png=-4x5", "a.png=4x5x6", "a.png=", "a.png=4.5x3"):
        with pytest.raises(ValueError):
            cli.parse_locate(bad, ["a.png"])
        with pytest.raises(SystemExit):
            p.parse_args(common + ["--locate", bad])
    with pytest.raises(SystemExit):
        p.parse_args(common + ["--locate", "c.png"])                                     # not among --suspects
    with pytest.raises(SystemExit):
        p.parse_args(common + ["--locate", "a.png", "--locate", "a.png=4x4"])            # located twice
    with pytest.raises(SystemExit):
        p.parse_args(common + ["--locate", "a.png", "--place", "a.png=1,2"])             # both placed and located
    assert cli.parse_place("a.png=1,2,3x4") == ("a.png", api.Placement(1, 2, 3, 4))      # untouched
