"""ssw_filter_rgb8 on the device against `filter_ref`, the numpy restatement of tests/test_filter_cpu.py (itself checked there
against Pillow byte for byte): every comparison is np.array_equal, there is no tolerance.  Shapes are the smallest at which the
kernels can go wrong: a single pixel, sides far below the halo of three passes (the clamping cases), odd sides, one axis inside
the halo and the other across several tiles, two tiles and a remainder on both axes, more jobs than two launches hold, byte
offsets 0 .. 3 of both pointers."""
import ctypes as C
import json
import re

import numpy as np
import pytest

import gpu_util as G
from gpu_util import ctx, lib
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd import api, cli
from spread_spectrum_watermarking_amd._lib import check
from test_collude_cpu import quality_ref
from test_filter_cpu import BLUR, MEDIAN3, UNSHARP, filter_ref, ref_of
from test_jpeg_cpu import CONTENTS, cat_image, content

pytestmark = pytest.mark.gpu

RADII = (0.3, 1.0, 1.5, 2.4, 2.5, 8.0)                   # r = 0 twice, r = 1 up to its upper end, r = 2, r = 7
# every job of the equality tests as (kind, radius, percent, threshold): the median, a blur and UNSHARP(., 150, 3) per radius, the
# clamp extremes and the threshold that never fires
FILTERS = ([(MEDIAN3, 0.0, 0, 0)] + [(BLUR, r, 0, 0) for r in RADII] + [(UNSHARP, r, 150, 3) for r in RADII]
           + [(UNSHARP, 2.0, 1000, 0), (UNSHARP, 2.0, 1, 255)])
# (h, w); the last: the row kernel's tile is 256 x 8 pixels, the column kernel's 64 pixels (192 bytes) x 96 rows, the median's
# 64 x 32 -- two of the largest tiles + 37 columns and + 11 rows, which is also several of the smaller ones and a remainder
SHAPES = [(1, 1), (1, 7), (2, 3), (5, 4), (9, 31), (33, 17), (3, 300), (300, 3), (67, 131), (203, 549)]
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def cat():
    return cat_image()


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


def jobs_c(jobs):
    """jobs: (frame, (kind, radius, percent, threshold))"""
    return (L.FilterJob * max(len(jobs), 1))(*[L.FilterJob(f, *args) for f, args in jobs])


def dev_filter(frames, jobs, off_in=0, off_out=0, extra=0):
    """frames [n, h, w, 3], jobs (frame, filter) pairs -> [len(jobs) + extra, h, w, 3]: `extra` frames behind the last job's
    that the call must leave as they were.  Also checks that the input is unchanged."""
    n, h, w, _ = frames.shape
    d, o = Dev(frames, off_in), Dev((len(jobs) + extra) * h * w * 3, off_out)
    check(lib().ssw_filter_rgb8(ctx().handle, d.ptr, n, w, h, jobs_c(jobs), len(jobs), o.ptr), "ssw_filter_rgb8")
    out = o.host(np.uint8, (len(jobs) + extra, h, w, 3))
    assert np.array_equal(d.host(np.uint8, frames.shape), frames), "the call changed its input"
    d.free(); o.free()
    return out


def every_kind(h, w, seed=0):
    return np.stack([content(kind, h, w, seed) for kind in CONTENTS])


def ref(frame, args):
    return filter_ref(frame, *args)


# ---- equality ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SHAPES)
def test_equals_the_restatement_for_every_content_and_filter(h, w):
    frames = every_kind(h, w)
    jobs = [(f, args) for f in range(3) for args in FILTERS]
    out = dev_filter(frames, jobs)
    for i, (f, args) in enumerate(jobs):
        assert np.array_equal(out[i], ref(frames[f], args)), (CONTENTS[f], args)


def test_equals_the_restatement_on_the_cat(cat):
    """640 x 444: 2.5 tiles of the row kernel, 10 of the column kernel and the median, 4.6 bands of 96 rows."""
    h, w = cat.shape[:2]
    frames = np.stack([cat, content("binary", h, w)])
    jobs = [(0, args) for args in FILTERS] + [(1, (MEDIAN3, 0.0, 0, 0)), (1, (BLUR, 8.0, 0, 0)), (1, (UNSHARP, 1.0, 1000, 0))]
    out = dev_filter(frames, jobs)
    for i, (f, args) in enumerate(jobs):
        assert np.array_equal(out[i], ref(frames[f], args)), (f, args)


# ---- jobs --------------------------------------------------------------------------------------------------------------------
def test_forty_jobs_out_of_order_with_repeats_and_nothing_beyond_the_last():
    h, w = 19, 17
    frames = np.stack([content(CONTENTS[i % 3], h, w, seed=i) for i in range(5)])
    rng = np.random.default_rng(11)
    jobs = [(int(rng.integers(0, 5)), FILTERS[int(rng.integers(0, len(FILTERS)))]) for _ in range(40)]     # three launch groups: 16, 16 and 8 jobs
    jobs[3], jobs[20], jobs[39] = (4, FILTERS[4]), (4, FILTERS[4]), (0, FILTERS[0])       # a frame twice under one filter, far apart
    jobs[5], jobs[25] = (1, FILTERS[0]), (2, FILTERS[0])                                   # a median among the blurs of two groups
    assert {args[0] for _, args in jobs[:16]} == {BLUR, UNSHARP, MEDIAN3}                 # a group mixes the kinds
    out = dev_filter(frames, jobs, extra=1)
    for i, (f, args) in enumerate(jobs):
        assert np.array_equal(out[i], ref(frames[f], args)), (i, f, args)
    assert np.all(out[40] == SENTINEL)
    for i in (0, 17, 39):                                                                   # alone = inside the batch
        assert np.array_equal(dev_filter(frames, [jobs[i]])[0], out[i]), i


@pytest.mark.parametrize("h,w", [(9, 31), (19, 70)])
def test_at_every_byte_offset(h, w):
    frames = every_kind(h, w, seed=2)
    jobs = [(2, (MEDIAN3, 0.0, 0, 0)), (0, (BLUR, 1.5, 0, 0)), (1, (UNSHARP, 2.5, 150, 3))]
    want = np.stack([ref(frames[f], args) for f, args in jobs])
    for off_in in range(4):
        for off_out in range(4):
            out = dev_filter(frames, jobs, off_in, off_out, extra=1)
            assert np.array_equal(out[:3], want) and np.all(out[3] == SENTINEL), (off_in, off_out)


# ---- workspace ---------------------------------------------------------------------------------------------------------------
def test_a_small_call_after_a_large_one_gives_what_a_fresh_context_gives():
    small = every_kind(9, 31, seed=5)
    jobs = [(0, (BLUR, 8.0, 0, 0)), (1, (UNSHARP, 1.0, 150, 3)), (2, (MEDIAN3, 0.0, 0, 0)), (2, (BLUR, 0.3, 0, 0))]
    with G.fresh_ctx():
        want = dev_filter(small, jobs)
    with G.fresh_ctx():
        large = every_kind(100, 300, seed=6)
        big = dev_filter(large, [(f, (BLUR, r, 0, 0)) for f in range(3) for r in (1.0, 6.0)])
        assert np.array_equal(big[1], ref(large[0], (BLUR, 6.0, 0, 0)))
        assert np.array_equal(dev_filter(small, jobs), want)                                # on planes the large call left full
    assert np.array_equal(want, np.stack([ref(small[f], args) for f, args in jobs]))


# ---- status codes ------------------------------------------------------------------------------------------------------------
def test_status_codes():
    f, hd = lib().ssw_filter_rgb8, ctx().handle
    frames = every_kind(8, 16, seed=7)
    d, o = Dev(frames), Dev(2 * 8 * 16 * 3)
    good_jobs = [(0, (UNSHARP, 2.0, 150, 3)), (2, (MEDIAN3, 0.0, 0, 0))]
    good = jobs_c(good_jobs)
    untouched = lambda: np.all(o.host(np.uint8, (2 * 8 * 16 * 3,)) == SENTINEL)
    assert f(None, d.ptr, 3, 16, 8, good, 2, o.ptr) == L.SSW_ERR_BAD_ARG
    assert f(hd, None, 3, 16, 8, good, 2, o.ptr) == L.SSW_ERR_BAD_ARG
    assert f(hd, d.ptr, 3, 16, 8, None, 2, o.ptr) == L.SSW_ERR_BAD_ARG
    assert f(hd, d.ptr, 3, 16, 8, good, 2, None) == L.SSW_ERR_BAD_ARG
    nan, inf = float("nan"), float("inf")
    bad_jobs = [(3, (MEDIAN3, 0.0, 0, 0)), (0xFFFFFFFF, (BLUR, 1.0, 0, 0)),                  # a frame the call does not have
                (0, (3, 0.0, 0, 0)), (0, (0xFFFFFFFF, 1.0, 0, 0)),                           # a kind there is not
                (0, (BLUR, 0.0, 0, 0)), (0, (BLUR, -1.0, 0, 0)), (0, (BLUR, 8.5, 0, 0)), (0, (BLUR, nan, 0, 0)), (0, (BLUR, inf, 0, 0)),
                (0, (UNSHARP, 0.0, 150, 3)), (0, (UNSHARP, 9.0, 150, 3)), (0, (UNSHARP, nan, 150, 3)), (0, (UNSHARP, -inf, 150, 3)),
                (0, (UNSHARP, 2.0, 0, 3)), (0, (UNSHARP, 2.0, 1001, 3)), (0, (UNSHARP, 2.0, 150, 256)), (0, (UNSHARP, 2.0, 0xFFFFFFFF, 3)),
                (0, (BLUR, 1.0, 1, 0)), (0, (BLUR, 1.0, 0, 1)),                               # fields the kind does not use
                (0, (MEDIAN3, 1.0, 0, 0)), (0, (MEDIAN3, nan, 0, 0)), (0, (MEDIAN3, 0.0, 1, 0)), (0, (MEDIAN3, 0.0, 0, 1))]
    for bad in bad_jobs:                                                                     # a bad job behind a good one: nothing is enqueued
        assert f(hd, d.ptr, 3, 16, 8, jobs_c([good_jobs[0], bad]), 2, o.ptr) == L.SSW_ERR_BAD_ARG, bad
    assert f(hd, d.ptr, 2, 16, 8, good, 2, o.ptr) == L.SSW_ERR_BAD_ARG                      # frame 2 of 2 frames
    for w, h in ((0, 8), (16, 0), (0, 0), (65536, 8), (8, 65536)):                          # a side of 0 or above 65535
        assert f(hd, d.ptr, 3, w, h, good, 2, o.ptr) == L.SSW_ERR_BAD_DIMS, (w, h)
    assert f(hd, d.ptr, 3, 16, 8, good, 0, o.ptr) == L.SSW_OK
    assert f(hd, None, 0, 0, 0, None, 0, None) == L.SSW_OK                                  # n_jobs == 0 comes first
    ctx().synchronize()
    assert untouched()
    assert f(hd, d.ptr, 3, 16, 8, good, 2, o.ptr) == L.SSW_OK
    assert np.array_equal(o.host(np.uint8, (2, 8, 16, 3)), np.stack([ref(frames[fr], args) for fr, args in good_jobs]))
    d.free(); o.free()


# ---- timing ------------------------------------------------------------------------------------------------------------------
def test_timed_as_convert_with_its_algorithmic_bytes():
    h, w = 41, 57
    frames = every_kind(h, w, seed=8)
    c = ctx()
    c.enable_timing(True)
    try:
        c.reset_timing()
        dev_filter(frames, [(0, FILTERS[0]), (1, FILTERS[3]), (1, FILTERS[9]), (2, FILTERS[0]), (0, FILTERS[6])])
        t = c.timing()
        assert t["convert"]["launches"] >= 1 and t["convert"]["work"] == 5 * 2 * 3 * w * h
        assert all(v["launches"] == 0 for k, v in t.items() if k != "convert") and len(t) == 15
    finally:
        c.enable_timing(False)


# ---- the Python wrapper ------------------------------------------------------------------------------------------------------
def test_python_filter_in_one_group_and_in_many(monkeypatch):
    h, w = 24, 40
    images = [content(CONTENTS[i % 3], h, w, seed=20 + i) for i in range(4)]
    fs = [api.Filter.blur(1.5), api.Filter.median(), api.Filter.unsharp(), api.Filter.unsharp(0.5, 300, 10)]
    want = [[ref_of(im, f) for f in fs] for im in images]
    for cap in (api.UPLOAD_GROUP_BYTES, 5 * h * w * 3, 1):                                   # one group | frames and jobs split | a job a group
        monkeypatch.setattr(api, "UPLOAD_GROUP_BYTES", cap)
        got = api.filter(images, fs, ctx())
        assert len(got) == 4 and all(len(g) == 4 for g in got)
        for i in range(4):
            for j in range(4):
                assert np.array_equal(got[i][j], want[i][j]), (cap, i, j)


# ---- the report --------------------------------------------------------------------------------------------------------------
def same(a, b):
    return a == b or (a != a and b != b)


def test_strength_report_equals_the_chain_through_the_host(cat):
    """Field for field against mark_copies_rgb8 -> filter_ref on the host -> trace_many -> quality_ref.  The last assertions rest on
    the oracle, not on the device (tests/test_filter_cpu.py::test_which_alpha_survives_which_filter computes them: the own marks of
    the 8 copies of default_rng(3) after filter_ref, weakest .. strongest, the strongest other mark in brackets):
      alpha 0.02   blur 1: 16.76 .. 18.14 (1.77)     blur 3: 2.04 .. 2.90 (0.64)       median 3: 18.33 .. 21.40 (2.32)
                   unsharp 2,150,3: 3.43 .. 5.86 (1.12)
      alpha 0.1    blur 1: 29.68 .. 31.31 (1.83)     blur 3: 11.49 .. 12.45 (1.09)     median 3: 30.06 .. 31.72 (2.12)
                   unsharp 2,150,3: 18.40 .. 20.52 (1.85)
    alpha 0.1 survives all four in every copy; alpha 0.02 survives blur 1 and the median in every copy and neither blur 3 nor the
    default unsharp mask in any."""
    alphas, n, k = [0.02, 0.1], 8, 1000
    fs = [api.Filter.blur(1), api.Filter.blur(3), api.Filter.median(), api.Filter.unsharp()]
    c = ctx()
    c.transfer_stats(reset=True)
    rows = api.strength_report(cat, alphas, filters=fs, seed=3, ctx=c)
    moved = c.transfer_stats(reset=True)
    # as before: the original and the marks went up, statistics and similarities came down -- no frame crossed PCIe
    assert cat.nbytes <= moved["h2d_bytes"] < 1.1 * cat.nbytes and 0 < moved["d2h_bytes"] < cat.nbytes // 100, moved
    plain = api.strength_report(cat, alphas, seed=3, ctx=c)
    marks = np.random.default_rng(3).standard_normal((n, k)).astype(np.float32)
    for r, p in zip(rows, plain):
        assert (r.alpha, r.quality, r.collusions, r.jpeg, r.ssim) == (p.alpha, p.quality, p.collusions, p.jpeg, p.ssim) and p.filters == []
        copies = api.Writer(cat, api.WriteConfig(insertion=api.Insertion.Option2(r.alpha)), c).mark_copies_rgb8(list(marks))
        filtered = [ref_of(copy, f) for f in fs for copy in copies]
        traced = api.trace_many(cat, filtered, list(marks), threshold=6.0, config=api.ReadConfig(extraction=api.Extraction.Option2(r.alpha)), ctx=c)
        assert [j.filter for j in r.filters] == ["blur 1", "blur 3", "median 3", "unsharp 2,150,3"]
        for i, j in enumerate(r.filters):
            sims = np.asarray(traced.sims[i * n:(i + 1) * n])
            own, others = np.diagonal(sims), sims[~np.eye(n, dtype=bool)]
            psnr = [api.Quality(tuple(s[:3]), s[3], s[4], s[5], cat.shape[0] * cat.shape[1]).psnr
                    for s in (quality_ref(cat, f) for f in filtered[i * n:(i + 1) * n])]
            print(f"alpha {r.alpha}: {j}")
            assert same(j.weakest_own, float(own.min())) and same(j.strongest_innocent, float(others.max())), (r.alpha, j)
            assert j.survived == int((own > np.float32(6.0)).sum()) and j.accused == int((others > np.float32(6.0)).sum()), (r.alpha, j)
            assert (j.psnr_min, j.psnr_max) == (min(psnr), max(psnr)), (r.alpha, j)
            assert j.ssim_min != j.ssim_min and j.ssim_max != j.ssim_max                    # not asked for
    faint, strong = rows
    assert [j.survived for j in strong.filters] == [n, n, n, n] and all(j.accused == 0 for j in strong.filters + faint.filters)
    assert [j.survived for j in faint.filters] == [n, 0, n, 0]                 # blur 3 and the unsharp mask erase a faint mark
    assert strong.filters[1].psnr_max < strong.filters[0].psnr_min                           # a wider blur, further from the original
    lone = api.strength_report(cat[:64, :64], [0.1], k=100, copies=1, sizes=(), filters=[api.Filter.median()], seed=1, ctx=c)
    assert lone[0].filters[0].strongest_innocent != lone[0].filters[0].strongest_innocent and lone[0].filters[0].accused == 0
    with_ssim = api.strength_report(cat[:64, :64], [0.1], k=100, copies=2, sizes=(), filters=[api.Filter.blur(1)], ssim=True, seed=1, ctx=c)
    assert 0.0 < with_ssim[0].filters[0].ssim_min <= with_ssim[0].filters[0].ssim_max < 1.0


def test_cli_strength_prints_the_filter_rows(cat, tmp_path, capsys):
    from PIL import Image
    path = str(tmp_path / "cat.png")
    Image.fromarray(cat).save(path)
    assert cli.main(["strength", path, "--alpha", "0.1", "--copies", "4", "--collude", "2", "--method", "average", "--jpeg", "75",
                     "--filter", "blur:1.5", "median", "unsharp:2,150,3"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[3].startswith("  average of 2: found 2/2") and lines[4].startswith("  jpeg 75: ") and len(lines) == 8
    row = r"  %s: own mark found %d/%d, weakest \d+\.\d, strongest innocent -?\d+\.\d, \d\d\.\d \.\. \d\d\.\d dB"
    for line, label in zip(lines[5:], ("blur 1.5", "median 3", "unsharp 2,150,3")):
        assert re.fullmatch(row % (re.escape(label), 4, 4), line), line
    assert cli.main(["strength", path, "--alpha", "0.1", "--copies", "2", "--collude", "2", "--method", "max", "-n", "100", "--ssim", "--filter", "median"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert re.fullmatch(row % ("median 3", 2, 2) + r", ssim 0\.\d\d \.\. [01]\.\d\d", lines[-1]), lines[-1]
    assert cli.main(["strength", path, "--alpha", "0.1", "--copies", "2", "--collude", "2", "--method", "max", "-n", "100", "--filter", "blur:2", "--json"]) == 0
    doc = json.loads(capsys.readouterr().out)
    assert [sorted(j) for j in doc[0]["filters"]] == [["accused", "filter", "psnr_max", "psnr_min", "strongest_innocent", "survived", "weakest_own"]]
    assert doc[0]["filters"][0]["filter"] == "blur 2" and 20.0 < doc[0]["filters"][0]["psnr_min"] <= doc[0]["filters"][0]["psnr_max"] < 60.0
    assert doc[0]["jpeg"] == []
    assert cli.main(["strength", path, "--alpha", "0.1", "--copies", "2", "--collude", "2", "--method", "max", "-n", "100", "--json"]) == 0
    assert json.loads(capsys.readouterr().out)[0]["filters"] == []
    for bad in ("blur:0", "blur:8.5", "unsharp:2,0,3", "sharpen"):
        with pytest.raises(SystemExit):
            cli.main(["strength", path, "--alpha", "0.1", "--filter", bad])
