"""The crop rows of the strength report, without a GPU.  `crop_ref` restates ssw_crop_attack_rgb8 and ssw_crop_search_attack_rgb8
as the compositions include/ssw.h defines them by -- `resample_ref` (Pillow's resize), `locate_ref`, `locate_scaled_ref` and the
restore restatement, all imported from the files that check them -- and tests/test_crop_gpu.py holds the device to it, with
equality.  Checked here: what the oracle answers on the cat for the placed and the scaled crops (recorded in
tests/golden/crop_answers.json by tests/golden/gen_crop_answers.py), the geometry of `Crop`, the command line's grammar and
rows, and the report's library calls on the recording stand-in of tests/fake_ssw.py."""
import argparse
import ctypes as C
import functools
import io
import json
import math
import os
import re

import numpy as np
import pytest

import fake_ssw
from conftest import GOLDEN, ROOT
from oracle import oracle as O
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd import api, cli
from spread_spectrum_watermarking_amd.api import Placement
from test_jpeg_cpu import cat_image
from test_locate_cpu import cut, locate_ref
from test_locate_scale_cpu import locate_scaled_ref
from test_resample_cpu import FILTERS, pil_resize, resample_ref

K, COPIES, ALPHAS = 1000, 3, (0.1, 0.02)
# the four placed rectangles of the report's table: the reference's own (tests/attack_crop.rs), then centred 0.75, 0.5, 0.25
PLACED = [(340, 160, 225, 225), (80, 55, 480, 333), (160, 111, 320, 222), (240, 166, 160, 111)]
# crop -> thumbnail, the widths searched
SCALED = [((80, 55, 480, 333), (240, 166), (240, 640)), ((160, 111, 320, 222), (160, 111), (160, 640)), ((340, 160, 225, 225), (150, 150), (150, 444))]
ANSWERS = os.path.join(GOLDEN, "crop_answers.json")


@functools.lru_cache(maxsize=1)
def marks():
    return np.random.default_rng(3).standard_normal((8, K)).astype(np.float32)


def recorded():
    with open(ANSWERS) as f:
        return json.load(f)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
class CropRef:
    def __init__(self, thumb, found, sad, out):
        self.thumb, self.found, self.sad, self.out = thumb, found, sad, out


def crop_ref(base, frame, rect, thumb=None, filt="bicubic", search=None):
    """One job of ssw_crop_attack_rgb8 (search None) or ssw_crop_search_attack_rgb8 (search (0, 0) or (wmin, wmax)): T as it
    would leak, the placement (x, y, pw, ph) -- given, or found -- its SAD (None when given) and the restored frame"""
    from test_restore_gpu import restore_ref
    x, y, cw, ch = rect
    T = cut(frame, x, y, cw, ch)
    if thumb is not None:
        T = resample_ref(T, thumb[0], thumb[1], FILTERS[filt])
    sad = None
    if search is None:
        found = (x, y, cw, ch)
    elif tuple(search) == (0, 0):
        gx, gy, sad = locate_ref(base, T)
        found = (gx, gy, T.shape[1], T.shape[0])
    else:
        pw, ph, gx, gy, sad = locate_scaled_ref(base, T, *search)
        found = (gx, gy, pw, ph)
    found = tuple(int(v) for v in found)
    return CropRef(T, found, None if sad is None else int(sad), restore_ref(base, T, Placement(*found)))


def test_the_restatement_is_a_composition_of_checked_parts():
    from PIL import Image
    rng = np.random.default_rng(5)
    base = rng.integers(0, 256, (67, 131, 3), dtype=np.uint8)
    frame = np.clip(base.astype(np.int64) + rng.integers(-2, 3, base.shape), 0, 255).astype(np.uint8)
    r = crop_ref(base, frame, (3, 5, 65, 33))
    assert np.array_equal(r.thumb, frame[5:38, 3:68]) and r.found == (3, 5, 65, 33) and r.sad is None
    assert np.array_equal(r.out[5:38, 3:68], frame[5:38, 3:68])                  # the reference's complement: the copy inside ...
    mask = np.ones(base.shape[:2], bool)
    mask[5:38, 3:68] = False
    assert np.array_equal(r.out[mask], base[mask])                               # ... the original outside
    for name, f in FILTERS.items():                                             # the thumbnail is Pillow's crop().resize()
        t = crop_ref(base, frame, (3, 5, 65, 33), (21, 11), name)
        pil = np.asarray(Image.fromarray(frame).crop((3, 5, 68, 38)).resize((21, 11), [Image.BOX, Image.BILINEAR, Image.BICUBIC, Image.LANCZOS][f]))
        assert np.array_equal(t.thumb, pil) and np.array_equal(t.thumb, pil_resize(frame[5:38, 3:68], 21, 11, f))
        assert np.array_equal(t.out[mask], base[mask]) and t.out.shape == base.shape
        assert np.array_equal(t.out[5:38, 3:68], O.resize_rgb8(t.thumb, 65, 33))    # brought back by the CatmullRom of restore
    s = crop_ref(base, frame, (40, 20, 48, 40), search=(0, 0))                   # noise: the search finds the very place
    assert s.found == (40, 20, 48, 40) and s.sad > 0 and np.array_equal(s.out, crop_ref(base, frame, (40, 20, 48, 40)).out)
    whole = crop_ref(base, frame, (0, 0, 131, 67))
    assert np.array_equal(whole.out, frame)


# ---- what the oracle answers on the cat ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def marked_copies(alpha):
    rgb = O.u8_to_f32(cat_image())
    return [O.f32_to_u8(O.embed_frame(rgb, marks()[c], alpha=alpha)) for c in range(COPIES)]


def similarity(frame, c, alpha, which):
    ext, _ = O.extract_frame(O.u8_to_f32(cat_image()), O.u8_to_f32(frame), marks()[c], alpha=alpha)
    return float(O.similarity(ext, marks()[which]))


# the figures of the report's first table: own-mark similarity of copies 0 .. 2, alpha 0.1 and 0.02
TABLE = {(340, 160, 225, 225): ([5.93, 8.19, 11.38], [6.31, 8.31, 10.42]), (80, 55, 480, 333): ([16.63, 21.38, 22.34], [16.34, 19.26, 20.19]),
         (160, 111, 320, 222): ([10.75, 12.05, 14.87], [10.94, 10.84, 13.69]), (240, 166, 160, 111): ([4.05, 5.15, 7.15], [4.43, 4.70, 6.50])}


@pytest.mark.parametrize("rect", PLACED, ids=lambda r: "%d,%d,%dx%d" % r)
def test_placed_crops_on_the_cat(rect):
    """Similarity falls roughly with the square root of the share kept, and alpha hardly matters: the reference's own crop
    (17.8 % kept) is under 6 sigma for one copy in three."""
    base, rec = cat_image(), recorded()["placed"]["%d,%d,%dx%d" % rect]
    assert base.shape == (444, 640, 3)
    for alpha, table in zip(ALPHAS, TABLE[rect]):
        outs = [crop_ref(base, marked_copies(alpha)[c], rect).out for c in range(COPIES)]
        own = [round(similarity(o, c, alpha, c), 2) for c, o in enumerate(outs)]
        innocent = round(max(abs(similarity(o, c, alpha, c + 3)) for c, o in enumerate(outs)), 2)
        print(rect, alpha, "own", own, "innocent", innocent, "kept %.1f %%" % (100 * rect[2] * rect[3] / (640 * 444)))
        assert own == rec[str(alpha)]["own"] == table and innocent == rec[str(alpha)]["innocent"] and innocent <= 1.8
        found = crop_ref(base, marked_copies(alpha)[0], rect, search=(0, 0)).found
        assert found == rect == tuple(rec[str(alpha)]["found"])                  # locate_ref finds copy 0's rectangle exactly


# the second table: found (x, y, pw, ph), then similarity found / placed at alpha 0.1 and at 0.02
SCALED_TABLE = {(80, 55, 480, 333): ((80, 56, 480, 332), (15.12, 16.59), (6.68, 16.02)), (160, 111, 320, 222): ((160, 111, 320, 222), (10.74, 10.74), (10.80, 10.80)),
                (340, 160, 225, 225): ((340, 160, 225, 225), (5.90, 5.90), (6.22, 6.22))}


@pytest.mark.parametrize("rect,thumb,rng", SCALED, ids=lambda v: "x".join(map(str, v)))
def test_crop_then_thumbnail_on_the_cat(rect, thumb, rng):
    """Height 333 halves to 166 and the ladder's kept-aspect height of width 480 is 332: the first case is answered one row off,
    and at alpha 0.02 that row costs most of the similarity.  The ladder runs once per case here (alpha 0.1); the answer at
    alpha 0.02 is the recorded one, laid back by the restore restatement."""
    base, rec = cat_image(), recorded()["scaled"]["%d,%d,%dx%d->%dx%d" % (rect + thumb)]
    want, at01, at002 = SCALED_TABLE[rect]
    r = crop_ref(base, marked_copies(0.1)[0], rect, thumb, "bicubic", rng)
    placed = crop_ref(base, marked_copies(0.1)[0], rect, thumb, "bicubic")
    sims = (round(similarity(r.out, 0, 0.1, 0), 2), round(similarity(placed.out, 0, 0.1, 0), 2))
    print(rect, thumb, rng, "->", r.found, "sad", r.sad, "sims found / placed", sims)
    assert r.found == want == tuple(rec["0.1"]["found"]) and r.sad == rec["0.1"]["sad"]
    assert sims == (rec["0.1"]["sim_found"], rec["0.1"]["sim_placed"]) == at01
    from test_restore_gpu import restore_ref
    assert tuple(rec["0.02"]["found"]) == want
    p = crop_ref(base, marked_copies(0.02)[0], rect, thumb, "bicubic")
    f = restore_ref(base, p.thumb, Placement(*rec["0.02"]["found"]))
    sims = (round(similarity(f, 0, 0.02, 0), 2), round(similarity(p.out, 0, 0.02, 0), 2))
    print(rect, thumb, "alpha 0.02: sims found / placed", sims)
    assert sims == (rec["0.02"]["sim_found"], rec["0.02"]["sim_placed"]) == at002


# ---- geometry and validation -----------------------------------------------------------------------------------------------------
def test_fraction_rounding_anchors_and_extremes():
    assert api.Crop(0.5).rect_in(640, 444) == (160, 111, 320, 222) and api.Crop(0.75).rect_in(640, 444) == (80, 55, 480, 333)
    assert api.Crop(0.25).rect_in(640, 444) == (240, 166, 160, 111)
    assert api.Crop(0.5).rect_in(131, 67) == (32, 16, 66, 34)                   # 65.5 and 33.5 round half up; (131 - 66) // 2, (67 - 34) // 2
    assert api.Crop(0.001).rect_in(131, 67) == (65, 33, 1, 1)                     # never less than a pixel
    assert api.Crop(1.0).rect_in(131, 67) == (0, 0, 131, 67) and api.Crop(1).rect_in(1, 1) == (0, 0, 1, 1)
    for anchor, (x, y) in {(0, 0): (0, 0), (1, 0): (65, 0), (0, 1): (0, 33), (1, 1): (65, 33), (0.5, 0.5): (32, 16)}.items():
        assert api.Crop(0.5, anchor=anchor).rect_in(131, 67)[:2] == (x, y)
    assert api.Crop.rect(340, 160, 225, 225).rect_in(640, 444) == (340, 160, 225, 225)
    assert api.Crop.rect(639, 443, 1, 1).rect_in(640, 444) == (639, 443, 1, 1) and api.Crop.rect(0, 0, 640, 444).rect_in(640, 444) == (0, 0, 640, 444)
    # thumbnails: Scale's rounding of the piece's sides
    assert api.Crop(0.75, scale=0.5).thumb(640, 444) == api.Scale(0.5).size(480, 333) == (240, 167)
    assert api.Crop(0.5, to=(160, 111)).thumb(640, 444) == (160, 111) and api.Crop(0.5).thumb(640, 444) is None
    assert api.Crop(0.5, scale=0.001).thumb(640, 444) == (1, 1)
    # searches
    assert api.Crop(0.5).search_range(640, 444) is None and api.Crop(0.5, search=True).search_range(640, 444) == (0, 0)
    assert api.Crop(0.5, search=False).search is None
    assert api.Crop(0.75, scale=0.5, search=True).search_range(640, 444) == (240, 640)
    assert api.Crop(0.5, scale=0.5, search=(200, 640)).search_range(640, 444) == (200, 640)
    assert api.Crop(0.5, search=(300, 340)).search_range(640, 444) == (300, 340)      # an unscaled piece whose size is searched as well
    # jobs and labels
    j = api.Crop(0.75, scale=0.5, filter="Lanczos").job(2, 640, 444)
    assert (j.frame, j.x, j.y, j.cw, j.ch, j.tw, j.th, j.filter) == (2, 80, 55, 480, 333, 240, 167, L.RESAMPLE_FILTERS["lanczos"])
    j = api.Crop.rect(1, 2, 3, 4, filter="box").job(0, 10, 10)
    assert (j.x, j.y, j.cw, j.ch, j.tw, j.th, j.filter) == (1, 2, 3, 4, 0, 0, 0)
    assert api.Crop(0.5).label == "crop 0.5" and api.Crop.rect(340, 160, 225, 225).label == "crop 340,160,225x225"
    assert api.Crop(0.75, scale=0.5, filter="lanczos").label == "crop 0.75 @ 0.5 lanczos" and api.Crop(0.5, to=(64, 53)).label == "crop 0.5 @ 64x53 bicubic"
    assert api.Crop(0.5, anchor=(0, 1)).label == "crop 0.5 anchor 0,1"
    assert C.sizeof(L.CropJob) == 32 and C.sizeof(L.CropSearch) == 8


def test_every_value_error_comes_before_a_context():
    z = np.zeros((40, 48, 3), np.uint8)
    before = api.default_context
    api.default_context = lambda: pytest.fail("a context was asked for")
    try:
        for bad in (lambda: api.Crop(0), lambda: api.Crop(1.5), lambda: api.Crop(-0.5), lambda: api.Crop("half"), lambda: api.Crop(float("nan")),
                    lambda: api.Crop(True), lambda: api.Crop(0.5, anchor=(0.5,)), lambda: api.Crop(0.5, anchor=(0, 1.5)), lambda: api.Crop(0.5, anchor=0.5),
                    lambda: api.Crop(0.5, scale=0.5, to=(10, 10)), lambda: api.Crop(0.5, scale=5), lambda: api.Crop(0.5, scale=-1),
                    lambda: api.Crop(0.5, to=(0, 10)), lambda: api.Crop(0.5, to=(10, 70000)), lambda: api.Crop(0.5, to=(10,)), lambda: api.Crop(0.5, to=10),
                    lambda: api.Crop(0.5, filter="nearest"), lambda: api.Crop(0.5, search=(0, 10)), lambda: api.Crop(0.5, search=(20, 10)),
                    lambda: api.Crop(0.5, search=(1.5, 10)), lambda: api.Crop(0.5, search=5), lambda: api.Crop(0.5, search=(10,)),
                    lambda: api.Crop.rect(-1, 0, 5, 5), lambda: api.Crop.rect(0, 0, 0, 5), lambda: api.Crop.rect(0, 0, 5, 2.5),
                    lambda: api.Crop(0.5, rectangle=(0, 0, 5, 5)), lambda: api.Crop(rectangle=(0, 0, 5)),
                    lambda: api.Crop.rect(44, 0, 5, 5).rect_in(48, 40), lambda: api.Crop.rect(0, 36, 5, 5).rect_in(48, 40),
                    lambda: api.crop_attack(z, [z], [api.Crop.rect(44, 0, 5, 5)]), lambda: api.crop_attack(z, [z], [0.5]),
                    lambda: api.crop_attack(z, [np.zeros((40, 49, 3), np.uint8)], [api.Crop(0.5)]), lambda: api.crop_attack(z[..., :2], [z], [api.Crop(0.5)]),
                    lambda: api.crop_search_attack(z, [z], [api.Crop(0.5, scale=0.5)]),            # a 12 x 10 thumbnail: the ladder refuses sides below 32
                    lambda: api.crop_search_attack(z, [z], [api.Crop(1.0, search=(20, 48))]),
                    lambda: api.crop_search_attack(z, [z], [api.Crop(1.0, search=(49, 60))]),      # no width fits the frame
                    lambda: api.crop_search_attack(z, [z], [api.Crop.rect(0, 0, 49, 5)]),
                    lambda: api.strength_report(z, [0.1], crops=[api.Crop.rect(0, 0, 49, 5)]), lambda: api.strength_report(z, [0.1], crops=[0.5]),
                    lambda: api.strength_report(z, [0.1], crops=[api.Crop(0.5, scale=0.5, search=True)])):
            with pytest.raises(ValueError):
                bad()
        assert api.crop_attack(z, [], [api.Crop(0.5)]) == [] and api.crop_attack(z, [z, z], []) == [[], []]
        assert api.crop_attack(z, [], [api.Crop(0.5)], thumbs=True) == ([], []) and api.crop_search_attack(z, [z], []) == ([[]], [[]])
    finally:
        api.default_context = before
    r = api.CropResult("crop 0.5", (320, 222), 8, 10.0, 1.0, 0, 30.0, 31.0)
    assert r.search is None and r.found == [] and math.isnan(r.kept) and r.thumb is None and math.isnan(r.ssim_min)
    from spread_spectrum_watermarking_amd import Crop, CropResult, crop_attack, crop_search_attack
    assert (Crop, CropResult, crop_attack, crop_search_attack) == (api.Crop, api.CropResult, api.crop_attack, api.crop_search_attack)
    assert api.StrengthRow(0.1, [], []).crops == []


# ---- the command line ----------------------------------------------------------------------------------------------------------
def test_cli_grammar():
    assert cli._crop_arg("0.5") == api.Crop(0.5) and cli._crop_arg("340,160,225x225") == api.Crop.rect(340, 160, 225, 225)
    assert cli._crop_arg("0.5:?") == api.Crop(0.5, search=True) and cli._crop_arg("0.75@0.5") == api.Crop(0.75, scale=0.5)
    assert cli._crop_arg("0.75@0.5:lanczos:?") == api.Crop(0.75, scale=0.5, filter="lanczos", search=True)
    assert cli._crop_arg("0.5@0.5:?200..640") == api.Crop(0.5, scale=0.5, search=(200, 640))
    assert cli._crop_arg("340,160,225x225@150x150:box") == api.Crop.rect(340, 160, 225, 225, to=(150, 150), filter="box")
    assert cli._crop_arg("10,20,30x40:?") == api.Crop.rect(10, 20, 30, 40, search=True)
    for bad in ("", "0.5:", "0.5:lanczos", "0.5@", "0.5@0", "0.5@x", "0.5:?9", "0.5:?9..1", "0.5:?1.5..9", "1.5", "0", "1,2,3", "1,2,3x", "1,2,3x4x5", "0.5@0.5:nearest",
                "0.5@0.5:?:bicubic", "0.5@0.5:bicubic:?:?", "a,b,cxd", "0.5@9"):
        with pytest.raises(argparse.ArgumentTypeError):
            cli._crop_arg(bad)
    words = "0.5 340,160,225x225 0.5:? 0.75@0.5 0.75@0.5:lanczos:? 0.5@0.5:?200..640".split()
    args = cli.build_parser().parse_args(["strength", "cat.png", "--alpha", "0.1", "--crop"] + words)
    assert args.crops == [api.Crop(0.5), api.Crop.rect(340, 160, 225, 225), api.Crop(0.5, search=True), api.Crop(0.75, scale=0.5),
                          api.Crop(0.75, scale=0.5, filter="lanczos", search=True), api.Crop(0.5, scale=0.5, search=(200, 640))]
    assert cli.build_parser().parse_args(["strength", "cat.png", "--alpha", "0.1"]).crops == []


def strength_output(rows, crops, as_json):
    """What cli.cmd_strength prints for `rows` (strength_report and the image file are stood in for)"""
    args = argparse.Namespace(file="cat.png", alpha=[0.1], length=50, copies=8, collude=[], method=[], similarity_exceed=6.0, jpeg=[], ssim=False,
                              filters=[], scales=[], rotations=[], crops=crops, json=as_json)
    before = cli.strength_report, cli._open_image
    seen = {}
    cli.strength_report, cli._open_image = (lambda *a, **k: seen.update(k) or rows), (lambda path: None)
    try:
        out = io.StringIO()
        assert cli.cmd_strength(args, out) == 0
        assert seen.get("crops", []) == crops
        return out.getvalue()
    finally:
        cli.strength_report, cli._open_image = before


def test_cli_prints_both_rows_and_json():
    q = [api.Quality((120, 90, 300), 170, 400, 3, 640 * 444)] * 8
    crops = [api.Crop(0.5), api.Crop(0.75, scale=0.5, search=True)]
    placed = api.CropResult("crop 0.5", (320, 222), 8, 10.75, 1.44, 0, 41.04, 42.96, rect=(160, 111, 320, 222), kept=0.25)
    found = [(80, 55, 480, 333)] * 7 + [(80, 56, 480, 332)]
    searched = api.CropResult(crops[1].label, (480, 333), 7, 5.46, 2.31, 0, 38.5, 39.25, rect=(80, 55, 480, 333), thumb=(240, 167), kept=0.5625,
                              search=(240, 640), found=found, found_exact=7, worst_offset=(0, 1), worst_size_error=(0, 1))
    rows = [api.StrengthRow(0.1, q, [], crops=[placed, searched])]
    lines = strength_output(rows, crops, False).splitlines()
    assert lines[-2] == "  crop 0.5 (320x222 at 160,111): own mark found 8/8, weakest 10.8, strongest innocent 1.4, 41.0 .. 43.0 dB, 25.0 % kept"
    assert lines[-1] == ("  crop 0.75 @ 0.5 bicubic (480x333 at 80,55 -> 240x167): place searched: exact in 7/8, worst offset 0,1, worst size 0x1, "
                         "own mark found 7/8, weakest 5.5, strongest innocent 2.3, 38.5 .. 39.2 dB, 56.2 % kept")
    doc = json.loads(strength_output(rows, crops, True))
    assert sorted(doc[0]["crops"][0]) == ["accused", "crop", "kept", "psnr_max", "psnr_min", "rect", "strongest_innocent", "survived", "thumb", "weakest_own"]
    assert doc[0]["crops"][0]["rect"] == [160, 111, 320, 222] and doc[0]["crops"][0]["thumb"] is None and doc[0]["crops"][0]["kept"] == 0.25
    assert {k: doc[0]["crops"][1][k] for k in ("search", "found_exact", "worst_offset", "worst_size_error", "thumb", "crop")} == {
        "search": [240, 640], "found_exact": 7, "worst_offset": [0, 1], "worst_size_error": [0, 1], "thumb": [240, 167], "crop": "crop 0.75 @ 0.5 bicubic"}
    assert doc[0]["crops"][1]["found"][-1] == [80, 56, 480, 332] and len(doc[0]["crops"][1]["found"]) == 8
    # without --crop the document has no such key and strength_report is not handed one
    rows = [api.StrengthRow(0.1, q, [])]
    assert "crops" not in json.loads(strength_output(rows, [], True))[0]


# ---- the report's calls on the recording stand-in --------------------------------------------------------------------------------
W, H, COPIES_FAKE = 96, 80, 3
AFTER_AN_ATTACK = ["ssw_fingerprint_trace_rgb8", "ssw_quality_rgb8", "ssw_copy_to_host", "ssw_copy_to_host"]
MIXED = [api.Crop(0.5), api.Crop(0.75, search=True), api.Crop.rect(1, 2, 30, 40, to=(15, 20), filter="box"), api.Crop(1.0, scale=0.5, search=True),
         api.Crop(0.75, scale=0.5, search=(40, 90))]


def report(ctx, crops=None, **more):
    kw = dict(k=50, copies=COPIES_FAKE, sizes=(2,), methods=("average",), seed=1)
    kw.update(more if crops is None else dict(more, crops=crops))
    frame = np.random.default_rng(11).integers(0, 256, (H, W, 3), dtype=np.uint8)
    return api.strength_report(frame, [0.02, 0.1], ctx=ctx, **kw)


def test_no_crops_make_the_calls_of_a_report_without_the_keyword():
    a, b = fake_ssw.fake_context(), fake_ssw.fake_context()
    report(a, scales=[api.Scale(0.5)], rotations=[api.Rotate(1.0)], ssim=True)
    report(b, (), scales=[api.Scale(0.5)], rotations=[api.Rotate(1.0)], ssim=True)
    assert a._lib.calls == b._lib.calls and a._lib.allocs == b._lib.allocs and b._lib.live == {}
    assert not any("crop" in c[0] for c in b._lib.calls)


def test_known_crops_make_one_call_and_searched_ones_one_more():
    ctx = fake_ssw.fake_context()
    rows = report(ctx, MIXED)
    calls = json.loads(json.dumps(ctx._lib.calls))
    names = [c[0] for c in calls]
    per_alpha = ["ssw_crop_attack_rgb8"] + AFTER_AN_ATTACK + ["ssw_crop_search_attack_rgb8"] + AFTER_AN_ATTACK
    assert names[-len(per_alpha):] == per_alpha and names.count("ssw_crop_attack_rgb8") == 2 and names.count("ssw_crop_search_attack_rgb8") == 2
    assert ctx._lib.live == {}
    # without the crop calls and what follows them the record is the plain report's
    plain = fake_ssw.fake_context()
    report(plain)
    rest, i = [], 0
    while i < len(calls):
        if "crop" in names[i]:
            i += 1 + len(AFTER_AN_ATTACK)
            continue
        rest.append(calls[i])
        i += 1
    assert rest == json.loads(json.dumps(plain._lib.calls))
    fb = W * H * 3
    placed, sought = [0, 2], [1, 3, 4]
    args = next(c[1] for c in calls if c[0] == "ssw_crop_attack_rgb8")
    jobs = (L.CropJob * (2 * COPIES_FAKE))(*[MIXED[i].job(c, W, H) for i in placed for c in range(COPIES_FAKE)])          # crop-major
    assert args == ["ctx", ["dev", fb, 0], ["dev", COPIES_FAKE * fb, 0], COPIES_FAKE, W, H, bytes(jobs).hex(), 2 * COPIES_FAKE, ["dev", 2 * COPIES_FAKE * fb, 0], None]
    args = next(c[1] for c in calls if c[0] == "ssw_crop_search_attack_rgb8")
    n = 3 * COPIES_FAKE
    jobs = (L.CropJob * n)(*[MIXED[i].job(c, W, H) for i in sought for c in range(COPIES_FAKE)])
    ranges = (L.CropSearch * n)(*[L.CropSearch(*r) for r in ((0, 0), (48, 96), (40, 90)) for _ in range(COPIES_FAKE)])
    assert args[:7] == ["ctx", ["dev", fb, 0], ["dev", COPIES_FAKE * fb, 0], COPIES_FAKE, W, H, bytes(jobs).hex()]
    assert args[7:] == [bytes(ranges).hex(), n, ["dev", n * fb, 0], None, bytes(C.sizeof(L.Placement) * n).hex(), "host"]
    # the rows: in the order given; the stand-in finds every piece at 0, 0 with size 0 x 0
    for row in rows:
        assert [r.crop for r in row.crops] == [m.label for m in MIXED]
        for r, m in zip(row.crops, MIXED):
            x, y, cw, ch = m.rect_in(W, H)
            assert r.rect == (x, y, cw, ch) and r.size == (cw, ch) and r.kept == cw * ch / (W * H) and r.thumb == m.thumb(W, H)
            assert r.search == m.search_range(W, H)
            if m.search is None:
                assert r.found == [] and r.found_exact == 0
            else:
                assert r.found == [(0, 0, 0, 0)] * COPIES_FAKE and r.worst_offset == (x, y) and r.worst_size_error == (cw, ch)
                assert r.found_exact == 0


def test_only_searched_crops_make_no_placed_call_and_an_error_leaves_nothing_live():
    ctx = fake_ssw.fake_context()
    rows = report(ctx, [api.Crop(0.75, search=True)], ssim=True)
    names = [c[0] for c in ctx._lib.calls]
    assert "ssw_crop_attack_rgb8" not in names and names.count("ssw_crop_search_attack_rgb8") == 2
    assert names[-7:] == ["ssw_crop_search_attack_rgb8"] + AFTER_AN_ATTACK + ["ssw_ssim_rgb8", "ssw_copy_to_host"]
    assert [len(r.crops) for r in rows] == [1, 1] and ctx._lib.live == {}
    for name in ("ssw_crop_attack_rgb8", "ssw_crop_search_attack_rgb8"):
        ctx = fake_ssw.fake_context({name: L.SSW_ERR_UNSUPPORTED})
        with pytest.raises(api.SswError) as e:
            report(ctx, MIXED)
        assert e.value.status == L.SSW_ERR_UNSUPPORTED and ctx._lib.calls[-1][0] == name and ctx._lib.live == {}


def test_crop_attack_and_search_on_the_stand_in():
    ctx = fake_ssw.fake_context()
    base = np.zeros((H, W, 3), np.uint8)
    images = list(np.random.default_rng(4).integers(0, 256, (2, H, W, 3), dtype=np.uint8))
    crops = [api.Crop(0.5, search=True), api.Crop.rect(3, 4, 20, 10, scale=0.5)]
    frames, thumbs = api.crop_attack(base, images, crops, thumbs=True, ctx=ctx)
    call = next(c for c in ctx._lib.calls if c[0] == "ssw_crop_attack_rgb8")
    jobs = (L.CropJob * 4)(*[c.job(i, W, H) for i in range(2) for c in crops])                # frame-major, as the other attacks'
    fb, tb = W * H * 3, 2 * (48 * 40 + 10 * 5) * 3
    assert call[1] == ["ctx", ["dev", fb, 0], ["dev", 2 * fb, 0], 2, W, H, bytes(jobs).hex(), 4, ["dev", 4 * fb, 0], ["dev", tb, 0]]
    assert [[t.shape for t in row] for row in thumbs] == [[(40, 48, 3), (5, 10, 3)]] * 2 and frames[1][1].shape == (H, W, 3)
    frames, found = api.crop_search_attack(base, images, [api.Crop(0.5), api.Crop(0.75, scale=0.5, search=(40, 90))], ctx=ctx)
    call = next(c for c in ctx._lib.calls if c[0] == "ssw_crop_search_attack_rgb8")
    ranges = (L.CropSearch * 4)(*[L.CropSearch(*r) for _ in range(2) for r in ((0, 0), (40, 90))])      # search=None is taken as True
    assert call[1][7] == bytes(ranges).hex() and call[1][8] == 4 and call[1][10] is None and call[1][12] == "host"
    assert [len(f) for f in found] == [2, 2] and ctx._lib.live == {}


# ---- the header ------------------------------------------------------------------------------------------------------------------
def test_header_declares_both_calls_and_states_the_composition():
    raw = open(os.path.join(ROOT, "include", "ssw.h")).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"typedef struct ssw_crop_job \{ uint32_t frame, x, y, cw, ch, tw, th, filter; \} ssw_crop_job;", text)
    assert re.search(r"typedef struct ssw_crop_search \{ uint32_t wmin, wmax; \} ssw_crop_search;", text)
    assert re.search(r"int ssw_crop_attack_rgb8\(ssw_ctx\* ctx, const uint8_t\* dev_base, const uint8_t\* dev_frames, size_t n_frames, size_t w, size_t h,\s*"
                     r"const ssw_crop_job\* jobs, size_t n_jobs, uint8_t\* dev_out, uint8_t\* dev_thumbs\);", text)
    assert re.search(r"int ssw_crop_search_attack_rgb8\(ssw_ctx\* ctx, const uint8_t\* dev_base, const uint8_t\* dev_frames, size_t n_frames, size_t w, size_t h,\s*"
                     r"const ssw_crop_job\* jobs, const ssw_crop_search\* searches, size_t n_jobs, uint8_t\* dev_out,\s*"
                     r"uint8_t\* dev_thumbs, ssw_placement\* host_found, uint64_t\* host_sad\);", text)
    comment = re.sub(r"\s+", " ", raw[raw.index("the crop attack: a part of the picture"):raw.index("typedef struct ssw_crop_job")])
    for part in ("ssw_resample_rgb8(C_j, cw, ch, tw, th, filter)", "ssw_restore_rgb8(dev_base, T_j, {w, h of T_j, 3, x, y, cw, ch})",
                 "ssw_locate_rgb8(dev_base, T_j)", "ssw_locate_scaled_rgb8(dev_base, T_j, {wmin, wmax})", "ssw_restore_rgb8(dev_base, T_j, host_found[j])",
                 "crop_cut_kernel", "crop_complement_kernel", "256 MiB", "PER GROUP", "n_jobs == 0 is checked first", "tests/attack_crop.rs:56-70"):
        assert part in comment, part
    assert re.search(r"SSW_STAGE_COUNT = 15\b", text) and len(L.STAGES) == 15                      # billed under the existing stages
    kinds = L.SIGNATURES["ssw_crop_attack_rgb8"][1]
    assert len(kinds) == 10 and kinds[6] == C.POINTER(L.CropJob)
    kinds = L.SIGNATURES["ssw_crop_search_attack_rgb8"][1]
    assert len(kinds) == 13 and kinds[7] == C.POINTER(L.CropSearch) and kinds[11] == C.POINTER(L.Placement)
    lib = L.load()
    assert hasattr(lib, "ssw_crop_attack_rgb8") and hasattr(lib, "ssw_crop_search_attack_rgb8")
    hpp = open(os.path.join(ROOT, "include", "ssw_crop.hpp")).read()
    assert "ssw_crop_attack_rgb8(" in hpp and "ssw_crop_search_attack_rgb8(" in hpp and '#include "ssw.hpp"' in hpp
