"""ssw_crop_attack_rgb8 and ssw_crop_search_attack_rgb8 on the GPU: dev_out, dev_thumbs, host_found and host_sad EQUAL -- no
tolerance -- the restatement `crop_ref` of tests/test_crop_cpu.py AND what the older public calls (resample, locate, restore)
make of numpy-sliced pieces.  Shapes: frames 96 x 80 and 131 x 67 (rows of 393 bytes: every byte phase), rectangles at x = 0, 1,
2, 3 and at each border, widths with 3 cw mod 16 in {0, 3, 13}, a 1 x 1 piece, the whole frame, 33 and more jobs (one past a
descriptor batch), several frames with jobs out of frame order, pointers one byte off, thumbnails in all four filters, searched
pieces at both coarse factors and over a range of widths, a call of two workspace groups, every error code, the billing, and
the report's rows on the cat against trace_many on frames made from the parts."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
from PIL import Image

from gpu_util import ctx, lib
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd import api, cli
from spread_spectrum_watermarking_amd._lib import check
from test_angle_gpu import Dev
from test_crop_cpu import crop_ref, recorded
from test_jpeg_cpu import cat_image, content

pytestmark = pytest.mark.gpu

PIL_FILTER = {"box": Image.BOX, "bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS}


def frames_of(w, h, n):
    """(base, n copies that differ from it by a little noise of their own)"""
    base = content("cat+noise", h, w)
    return base, [np.clip(base.astype(np.int64) + np.random.default_rng(70 + i).integers(-2, 3, base.shape), 0, 255).astype(np.uint8) for i in range(n)]


def job_of(j):
    """(frame, (x, y, cw, ch), thumb or None, filter) -> ssw_crop_job"""
    frame, rect, thumb, filt = j
    tw, th = thumb or (0, 0)
    return L.CropJob(frame, *rect, tw, th, L.RESAMPLE_FILTERS[filt] if thumb else 0)


def dev_crop(base, frames, jobs, searches=None, thumbs=True, off=0):
    """One call.  -> (out [n][h][w][3], the thumbnails or None, [(x, y, pw, ph)] or None, [sad] or None)"""
    frames = np.stack(frames)
    n, (_, h, w, _) = len(jobs), frames.shape
    arr = (L.CropJob * n)(*[job_of(j) for j in jobs])
    sizes = [j[2] or j[1][2:] for j in jobs]
    total = sum(3 * a * b for a, b in sizes)
    b, d = Dev(base, off), Dev(frames, off)
    out, th = Dev(np.full((n, h, w, 3), 0xA5, np.uint8), off), Dev(np.full(total + 8, 0x5A, np.uint8), off)
    found, sad = (L.Placement * n)(), np.full(n, 0xA5A5A5A5, np.uint64)
    try:
        if searches is None:
            check(lib().ssw_crop_attack_rgb8(ctx().handle, b.ptr, d.ptr, len(frames), w, h, arr, n, out.ptr, th.ptr if thumbs else None), "ssw_crop_attack_rgb8")
        else:
            rng = (L.CropSearch * n)(*[L.CropSearch(*s) for s in searches])
            check(lib().ssw_crop_search_attack_rgb8(ctx().handle, b.ptr, d.ptr, len(frames), w, h, arr, rng, n, out.ptr, th.ptr if thumbs else None, found,
                                                    sad.ctypes.data), "ssw_crop_search_attack_rgb8")
        host, flat = np.empty((n, h, w, 3), np.uint8), np.empty(total + 8, np.uint8)
        check(lib().ssw_copy_to_host(ctx().handle, host.ctypes.data, out.ptr, host.nbytes), "ssw_copy_to_host")
        check(lib().ssw_copy_to_host(ctx().handle, flat.ctypes.data, th.ptr, flat.nbytes), "ssw_copy_to_host")
    finally:
        for x in (b, d, out, th):
            x.free()
    pieces, at = [], 0
    for a, c in sizes:
        pieces.append(flat[at:at + 3 * a * c].reshape(c, a, 3))
        at += 3 * a * c
    assert (flat[at:] == 0x5A).all()                                     # nothing behind the last thumbnail was written
    if not thumbs:
        assert (flat == 0x5A).all()
    return (host, pieces if thumbs else None, None if searches is None else [(f.x, f.y, f.pw, f.ph) for f in found],
            None if searches is None else [int(s) for s in sad])


def parts(base, frames, jobs, searches=None):
    """The same results from the older public calls on numpy-sliced pieces: (out, thumbs, found, sad)"""
    c = ctx()
    pieces = [np.ascontiguousarray(frames[f][y:y + ch, x:x + cw]) for f, (x, y, cw, ch), _, _ in jobs]
    thumbs = [api.resample([p], t, filt, c)[0] if t else p for p, (_, _, t, filt) in zip(pieces, jobs)]
    if searches is None:
        placements, found, sad = [api.Placement(*j[1]) for j in jobs], None, None
    else:
        got = api.locate(base, thumbs, [api.Locate(widths=s) if s != (0, 0) else None for s in searches], c)
        placements = [g.placement for g in got]
        found, sad = [(p.x, p.y, p.w, p.h) for p in placements], [g.sad for g in got]
    return api.restore(base, thumbs, placements, c), thumbs, found, sad


def same(base, frames, jobs, what, searches=None, off=0, ref=True):
    out, thumbs, found, sad = dev_crop(base, frames, jobs, searches, True, off)
    p_out, p_thumbs, p_found, p_sad = parts(base, frames, jobs, searches)
    assert found == p_found and sad == p_sad, (what, found, p_found, sad, p_sad)
    for i, j in enumerate(jobs):
        assert np.array_equal(thumbs[i], p_thumbs[i]), (what, i, j, "thumbnail against resample")
        assert np.array_equal(out[i], p_out[i]), (what, i, j, "frame against restore")
        if ref:
            r = crop_ref(base, frames[j[0]], j[1], j[2], j[3], None if searches is None else searches[i])
            assert np.array_equal(thumbs[i], r.thumb), (what, i, j, "thumbnail against crop_ref")
            assert np.array_equal(out[i], r.out), (what, i, j, "frame against crop_ref")
            if searches is not None:
                assert found[i] == r.found and sad[i] == r.sad, (what, i, j, found[i], r.found, sad[i], r.sad)
    # and without the thumbnails: the same frames, nothing written where they would go
    again = dev_crop(base, frames, jobs, searches, False, off)
    assert np.array_equal(again[0], out) and again[2] == found and again[3] == sad, (what, "without dev_thumbs")
    return out, thumbs, found, sad


# ---- placed, unscaled: the complement kernel (and the cut, for the thumbnails) -------------------------------------------------------
def rectangles(w, h):
    """x = 0 .. 3 and each border; 3 cw mod 16 = 0 (16), 3 (1, 17), 13 (15); 1 x 1 in the corners; the whole frame; single rows and columns"""
    r = [(x, 1 + x, cw, 9) for x in (0, 1, 2, 3) for cw in (16, 17, 15, 1)]
    r += [(w - cw, h - 7, cw, 7) for cw in (16, 17, 15)] + [(0, 0, w, h), (0, 0, 1, 1), (w - 1, h - 1, 1, 1), (w - 1, 0, 1, 1), (0, h - 1, 1, 1)]
    r += [(0, 5, w, 1), (5, 0, 1, h), (1, 0, w - 1, h), (0, 1, w, h - 1), (w - 33, 3, 32, h - 3), (7, h - 1, 21, 1)]
    return r + [(x, h - 2, 29 + x, 2) for x in (0, 1, 2, 3)]


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("w,h", [(96, 80), (131, 67)])
def test_placed_rectangles_equal_the_restatement_and_the_parts(w, h, off):
    base, frames = frames_of(w, h, 3)
    rects = rectangles(w, h)
    jobs = [((2 * i + 1) % 3, r, None, "bicubic") for i, r in enumerate(rects)]          # several frames, not in frame order
    assert len(jobs) >= 33 and len({3 * r[2] % 16 for r in rects}) >= 3
    same(base, frames, jobs, f"{w}x{h} off {off}", off=off)


def test_thirty_three_jobs_of_one_rectangle_are_one_past_a_batch():
    base, frames = frames_of(131, 67, 2)
    jobs = [(i % 2, (3, 2, 125, 60), None, "bicubic") for i in range(33)]
    out, thumbs, _, _ = same(base, frames, jobs, "33 jobs", ref=False)
    r = [crop_ref(base, frames[f], (3, 2, 125, 60)) for f in range(2)]
    assert all(np.array_equal(out[i], r[i % 2].out) and np.array_equal(thumbs[i], r[i % 2].thumb) for i in range(33))


# ---- placed and scaled ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", [0, 3])
def test_scaled_pieces_equal_the_restatement_the_parts_and_pillow(off):
    base, frames = frames_of(96, 80, 2)
    jobs = [(1, (16, 20, 64, 48), (32, 24), "bicubic"), (1, (3, 7, 64, 48), (32, 24), "bicubic"), (0, (3, 7, 64, 48), (32, 24), "bicubic")]
    jobs += [(i % 2, (29, 41, 65, 33), (21, 11), f) for i, f in enumerate(PIL_FILTER)]
    jobs += [(0, (1, 1, 65, 33), None, "bicubic"), (1, (0, 0, 96, 80), (48, 40), "lanczos"), (0, (5, 5, 20, 10), (40, 20), "bilinear"), (1, (5, 5, 20, 10), (20, 10), "box")]
    _, thumbs, _, _ = same(base, frames, jobs, f"scaled off {off}", off=off)
    for (f, (x, y, cw, ch), t, filt), got in zip(jobs, thumbs):
        pil = Image.fromarray(frames[f]).crop((x, y, x + cw, y + ch))
        assert np.array_equal(got, np.asarray(pil.resize(t, PIL_FILTER[filt]) if t else pil))


# ---- searched ------------------------------------------------------------------------------------------------------------------------
def test_searched_pieces_equal_the_restatement_and_the_parts():
    """In a 200 x 160 frame: a 40 x 36 piece (coarse factor 1), a 72 x 64 piece (coarse factor 4), a 96 x 80 piece scaled to 64 x 53
    over the widths 64 .. 128; jobs of both kinds mixed in one call, two frames"""
    base, frames = frames_of(200, 160, 2)
    jobs = [(1, (97, 61, 40, 36), None, "bicubic"), (0, (50, 40, 96, 80), (64, 53), "bicubic"), (0, (31, 77, 72, 64), None, "bicubic"),
            (1, (3, 2, 40, 36), None, "bicubic")]
    searches = [(0, 0), (64, 128), (0, 0), (0, 0)]
    out, thumbs, found, sad = same(base, frames, jobs, "searched", searches)
    print("found", found, "sad", sad)
    assert found[0] == (97, 61, 40, 36) and found[2] == (31, 77, 72, 64) and found[3] == (3, 2, 40, 36)      # exact cut-outs of noisy copies
    assert abs(found[1][0] - 50) <= 1 and abs(found[1][1] - 40) <= 1 and abs(found[1][2] - 96) <= 1        # a resized copy: within a pixel


# ---- two workspace groups ----------------------------------------------------------------------------------------------------------
def test_a_call_of_two_workspace_groups_is_the_calls_it_is_made_of():
    """At 3840 x 2160 a scaled job keeps its piece (24.9 MB) and, without dev_thumbs, its thumbnail (6.2 MB) in the workspace: 10
    jobs are two groups (8 + 2).  The parts on numpy-sliced pieces are the reference; two rectangles alternate, so that no two
    neighbours share a resample call."""
    w, h, n = 3840, 2160, 10
    base = np.ascontiguousarray(np.tile(cat_image(), (5, 6, 1))[:h, :w])
    frame = np.clip(base.astype(np.int16) + np.random.default_rng(5).integers(-2, 3, base.shape, dtype=np.int16), 0, 255).astype(np.uint8)
    kinds = [((3, 1, 3836, 2158), (1918, 1079)), ((0, 0, 3840, 2160), (1920, 1080))]
    jobs = [(0, *kinds[i % 2], "bicubic") for i in range(n)]
    want, want_thumbs, _, _ = parts(base, [frame], jobs[:2])
    arr = (L.CropJob * n)(*[job_of(j) for j in jobs])
    c, fb = ctx(), w * h * 3
    b, d, out = Dev(base), Dev(frame[None]), c.alloc(n * fb)
    try:
        check(lib().ssw_crop_attack_rgb8(c.handle, b.ptr, d.ptr, 1, w, h, arr, n, out.ptr, None), "ssw_crop_attack_rgb8")
        got = out.to_host(np.uint8, (n, h, w, 3))
    finally:
        for x in (b, d, out):
            x.free()
    for i in range(n):
        assert np.array_equal(got[i], want[i % 2]), i
    assert not np.array_equal(want[0], want[1]) and not np.array_equal(want[0], base)


# ---- billing, errors -----------------------------------------------------------------------------------------------------------------
def test_placed_unscaled_jobs_bill_the_complement_alone():
    base, frames = frames_of(96, 80, 2)
    jobs = [(i % 2, (1 + i, 2, 40, 30), None, "bicubic") for i in range(5)]
    c = ctx()
    c.enable_timing(True)
    try:
        c.reset_timing()
        dev_crop(base, frames, jobs, thumbs=False)
        t = c.timing()
        assert t["resize"]["launches"] == 1 and t["resize"]["work"] == 5 * 6 * 96 * 80          # the complement: read once, written once
        assert all(v["launches"] == 0 for k, v in t.items() if k != "resize"), t                # no locate stage, no resample, no cut
        c.reset_timing()
        dev_crop(base, frames, jobs, thumbs=True)                                                # the thumbnails asked for: the cut beside it
        t = c.timing()
        assert t["resize"]["launches"] == 1 and t["convert"]["launches"] == 1 and t["convert"]["work"] == 5 * 6 * 40 * 30
        assert all(v["launches"] == 0 for k, v in t.items() if k not in ("resize", "convert")), t
        c.reset_timing()
        dev_crop(base, frames, [(0, (8, 8, 64, 48), None, "bicubic")], [(0, 0)], thumbs=False)      # searched: the locate stages as well
        t = c.timing()
        assert t["locate"]["launches"] >= 1 and t["locate_coarse"]["launches"] >= 1 and t["resize"]["launches"] == 1 and t["convert"]["launches"] == 1
    finally:
        c.enable_timing(False)


def test_errors():
    z = np.zeros((40, 48, 3), np.uint8)
    b, d, o, t = Dev(z), Dev(z[None]), Dev(z[None]), Dev(z[None])
    found, sad, h = (L.Placement * 1)(), np.zeros(1, np.uint64), ctx().handle
    s = sad.ctypes.data
    job = lambda *a: (L.CropJob * 1)(L.CropJob(*a))
    ok, own = job(0, 4, 4, 36, 32, 0, 0, 0), (L.CropSearch * 1)(L.CropSearch(0, 0))
    f, g = lib().ssw_crop_attack_rgb8, lib().ssw_crop_search_attack_rgb8
    try:
        for call in (lambda jobs, w=48, hh=40, base=b.ptr, fr=d.ptr, out=o.ptr, th=t.ptr, n=1: f(h, base, fr, n, w, hh, jobs, 1, out, th),
                     lambda jobs, w=48, hh=40, base=b.ptr, fr=d.ptr, out=o.ptr, th=t.ptr, n=1: g(h, base, fr, n, w, hh, jobs, own, 1, out, th, found, s)):
            assert call(ok) == L.SSW_OK
            assert call(ok, w=0) == L.SSW_ERR_BAD_DIMS and call(ok, hh=0) == L.SSW_ERR_BAD_DIMS and call(ok, w=65536) == L.SSW_ERR_BAD_DIMS
            assert call(job(0, 4, 4, 36, 32, 70000, 10, 2)) == L.SSW_ERR_BAD_DIMS and call(job(0, 4, 4, 36, 32, 10, 65536, 2)) == L.SSW_ERR_BAD_DIMS
            assert call(job(1, 4, 4, 36, 32, 0, 0, 0)) == L.SSW_ERR_BAD_ARG                       # no such frame
            assert call(ok, n=0) == L.SSW_ERR_BAD_ARG
            for bad in (job(0, 4, 4, 0, 32, 0, 0, 0), job(0, 4, 4, 36, 0, 0, 0, 0), job(0, 13, 4, 36, 32, 0, 0, 0), job(0, 4, 9, 36, 32, 0, 0, 0),
                        job(0, 48, 0, 1, 1, 0, 0, 0), job(0, 0xFFFFFFFF, 0, 2, 1, 0, 0, 0), job(0, 4, 4, 36, 32, 10, 0, 2), job(0, 4, 4, 36, 32, 0, 10, 2),
                        job(0, 4, 4, 36, 32, 18, 16, 4)):
                assert call(bad) == L.SSW_ERR_BAD_ARG, bytes(bad).hex()
            assert call(None) == L.SSW_ERR_BAD_ARG and call(ok, base=None) == L.SSW_ERR_BAD_ARG and call(ok, fr=None) == L.SSW_ERR_BAD_ARG
            assert call(ok, out=None) == L.SSW_ERR_BAD_ARG and call(ok, th=None) == L.SSW_OK
            for out, th in ((d.ptr, t.ptr), (b.ptr, t.ptr), (o.ptr, d.ptr), (o.ptr, b.ptr), (o.ptr, o.ptr)):      # an output over an input, or over the other
                assert call(ok, out=out, th=th) == L.SSW_ERR_BAD_ARG
        assert f(None, b.ptr, d.ptr, 1, 48, 40, ok, 1, o.ptr, None) == L.SSW_ERR_BAD_ARG
        assert g(None, b.ptr, d.ptr, 1, 48, 40, ok, own, 1, o.ptr, None, found, s) == L.SSW_ERR_BAD_ARG
        assert g(h, b.ptr, d.ptr, 1, 48, 40, ok, None, 1, o.ptr, None, found, s) == L.SSW_ERR_BAD_ARG
        assert g(h, b.ptr, d.ptr, 1, 48, 40, ok, own, 1, o.ptr, None, None, s) == L.SSW_ERR_BAD_ARG
        assert g(h, b.ptr, d.ptr, 1, 48, 40, ok, own, 1, o.ptr, None, found, None) == L.SSW_ERR_BAD_ARG
        assert f(h, None, None, 0, 0, 0, None, 0, None, None) == L.SSW_OK                          # n_jobs == 0 is checked first
        assert g(h, None, None, 0, 0, 0, None, None, 0, None, None, None, None) == L.SSW_OK
        # the parts' own refusals come through: a range whose smallest rung has a side below 32, a range that is reversed, none that fits
        for rng in ((20, 40), (40, 36), (49, 60)):
            assert g(h, b.ptr, d.ptr, 1, 48, 40, ok, (L.CropSearch * 1)(L.CropSearch(*rng)), 1, o.ptr, None, found, s) == L.SSW_ERR_BAD_ARG, rng
        assert g(h, b.ptr, d.ptr, 1, 48, 40, ok, (L.CropSearch * 1)(L.CropSearch(36, 40)), 1, o.ptr, None, found, s) == L.SSW_OK
        assert (found[0].x, found[0].y, found[0].pw, found[0].ph) == (0, 0, 36, 32) and sad[0] == 0      # an all-zero frame: the first position wins
    finally:
        for x in (b, d, o, t):
            x.free()


# ---- the report on the cat -------------------------------------------------------------------------------------------------------------
def test_the_report_says_what_trace_finds_in_pieces_pillow_made():
    """k = 1000, 3 copies, alpha 0.1, marks of default_rng(3).  A row is what trace_many makes of the frames the parts make of
    pieces that PIL.Image.crop(...).resize(...) made -- in float32 bits.  Crop(0.5, search=True) is placed exactly for every copy.
    Crop(0.75, scale=0.5) has a 240 x 167 thumbnail (Scale's rounding of 333 / 2), for which the ladder's kept-aspect heights are
    ph(480) = 334 and ph(479) = 333: no copy can be placed exactly and the row must say so; the restatement answers 81,55 479x333
    or 80,54 480x334 on the oracle's copies.  The 240 x 166 thumbnail of the issue's table is the fourth crop: copy 0 is answered
    80,56 480x332, the offset 0,1 (copy 1 of the oracle: 79,55 481x333)."""
    image, n, k, alpha = cat_image(), 3, 1000, 0.1
    c = ctx()
    h, w = image.shape[:2]
    marks = np.random.default_rng(3).standard_normal((n, k)).astype(np.float32)
    copies = api.Writer(image, api.WriteConfig(insertion=api.Insertion.Option2(alpha)), c).mark_copies_rgb8(list(marks))
    cfg = api.ReadConfig(extraction=api.Extraction.Option2(alpha))
    crops = [api.Crop.rect(340, 160, 225, 225), api.Crop(0.5, search=True), api.Crop(0.75, scale=0.5, search=True), api.Crop(0.75, to=(240, 166), search=True)]
    rows = api.strength_report(image, [alpha], copies=n, k=k, sizes=(2,), crops=crops, seed=3, ctx=c)[0].crops
    assert [r.crop for r in rows] == [m.label for m in crops]
    frames_placed, thumbs_placed = api.crop_attack(image, list(copies), crops, thumbs=True, ctx=c)
    frames_found, found = api.crop_search_attack(image, list(copies), crops[1:], c)
    for p, (row, crop) in enumerate(zip(rows, crops)):
        x, y, cw, ch = rect = crop.rect_in(w, h)
        t = crop.thumb(w, h)
        pieces = [Image.fromarray(copies[i]).crop((x, y, x + cw, y + ch)) for i in range(n)]
        pieces = [np.asarray(im.resize(t, Image.BICUBIC) if t else im) for im in pieces]
        assert all(np.array_equal(thumbs_placed[i][p], pieces[i]) for i in range(n))             # the thumbnails are Pillow's, byte for byte
        if crop.search is None:
            placements, got = [api.Placement(*rect)] * n, None
        else:
            rng = crop.search_range(w, h)
            located = api.locate(image, pieces, [api.Locate(widths=rng) if rng != (0, 0) else None] * n, c)
            placements = [g.placement for g in located]
            got = [(g.x, g.y, g.w, g.h) for g in placements]
        traced = api.trace_many(image, pieces, list(marks), threshold=6.0, config=cfg, ctx=c, placements=placements)
        sims = np.asarray(traced.sims, np.float32)
        own, others = np.diagonal(sims), sims[~np.eye(n, dtype=bool)]
        print(f"{row.crop}: found {got} own {own.tolist()} row {row}")
        assert np.float32(row.weakest_own).tobytes() == own.min().tobytes() and np.float32(row.strongest_innocent).tobytes() == others.max().tobytes()
        assert row.survived == int((own > np.float32(6.0)).sum()) and row.accused == int((others > np.float32(6.0)).sum())
        assert (row.rect, row.size, row.thumb, row.kept) == (rect, (cw, ch), t, cw * ch / (w * h))
        # and the frames of the Python calls are the frames the report traced
        made = [f[p] for f in frames_placed] if crop.search is None else [f[p - 1] for f in frames_found]
        again = np.asarray(api.trace_many(image, made, list(marks), threshold=6.0, config=cfg, ctx=c).sims, np.float32)
        assert again.tobytes() == sims.tobytes()
        if crop.search is None:
            assert row.search is None and row.found == []
            continue
        assert row.found == got == [(f[p - 1].placement.x, f[p - 1].placement.y, f[p - 1].placement.w, f[p - 1].placement.h) for f in found]
        assert row.search == crop.search_range(w, h) and row.found_exact == sum(g == rect for g in got)
        assert row.worst_offset == (max(abs(g[0] - x) for g in got), max(abs(g[1] - y) for g in got))
        assert row.worst_size_error == (max(abs(g[2] - cw) for g in got), max(abs(g[3] - ch) for g in got))
    assert rows[0].kept == 225 * 225 / (640 * 444) and rows[0].survived >= 2
    assert rows[1].found_exact == 3 and rows[1].worst_offset == (0, 0) and rows[1].search == (0, 0)
    assert rows[2].found_exact == 0 and max(rows[2].worst_offset + rows[2].worst_size_error) == 1      # 167 rows: no width has the true height
    assert rows[3].found[0] == tuple(recorded()["scaled"]["80,55,480x333->240x166"]["0.1"]["found"]) == (80, 56, 480, 332)
    assert rows[3].worst_offset[1] == 1 and rows[3].found_exact < 3 and max(rows[3].worst_offset + rows[3].worst_size_error) == 1


def test_cli_strength_prints_the_crop_rows(tmp_path, capsys):
    path = str(tmp_path / "cat.png")
    Image.fromarray(cat_image()).save(path)
    args = ["strength", path, "--alpha", "0.1", "--copies", "3", "--collude", "2", "--method", "average", "-n", "200", "--crop", "0.5", "340,160,225x225", "0.5:?",
            "0.5@0.5:?200..640"]
    assert cli.main(args) == 0
    lines = capsys.readouterr().out.splitlines()
    tail = r"own mark found \d/3, weakest -?\d+\.\d, strongest innocent -?\d+\.\d(, \d innocent accused)?, \d\d\.\d \.\. (\d\d\.\d|inf) dB, \d+\.\d % kept"
    import re
    assert re.fullmatch(r"  crop 0\.5 \(320x222 at 160,111\): " + tail, lines[-4]), lines[-4]
    assert re.fullmatch(r"  crop 340,160,225x225 \(225x225 at 340,160\): " + tail, lines[-3]) and lines[-3].endswith("17.8 % kept"), lines[-3]
    assert re.fullmatch(r"  crop 0\.5 \(320x222 at 160,111\): place searched: exact in 3/3, worst offset 0,0, worst size 0x0, " + tail, lines[-2]), lines[-2]
    assert re.fullmatch(r"  crop 0\.5 @ 0\.5 bicubic \(320x222 at 160,111 -> 160x111\): place searched: exact in \d/3, worst offset \d,\d, worst size \dx\d, " + tail,
                        lines[-1]), lines[-1]
    assert cli.main(args + ["--json"]) == 0
    doc = json.loads(capsys.readouterr().out)[0]["crops"]
    assert "search" not in doc[0] and doc[2]["search"] == [0, 0] and doc[3]["search"] == [200, 640] and doc[3]["thumb"] == [160, 111]
    assert doc[2]["found"] == [[160, 111, 320, 222]] * 3 and doc[1]["kept"] == 225 * 225 / (640 * 444)
