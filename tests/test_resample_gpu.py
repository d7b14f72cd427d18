"""ssw_resample_rgb8 and ssw_scale_attack_rgb8 on the device against `resample_ref`, the numpy restatement of
tests/test_resample_cpu.py (itself checked there against Pillow byte for byte): every comparison is np.array_equal, there is no
tolerance.  Shapes are the smallest at which the kernels can go wrong: a single pixel, a single row and a single column, odd
sides, rows of 3 and 900 bytes, more columns than one run of the row kernel and more bytes than one block of the column kernel
hold, a ratio at which the row kernel's run shrinks and one at which it reads global memory, byte offsets 0 .. 3 of both
pointers."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import gpu_util as G
from conftest import ROOT
from gpu_util import ctx, lib
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd import api, cli
from spread_spectrum_watermarking_amd._lib import check
from test_jpeg_cpu import cat_image
from test_resample_cpu import BICUBIC, BILINEAR, BOX, CONTENTS, LANCZOS, NAMES, SHAPES, content, resample_ref, targets

pytestmark = pytest.mark.gpu

LIBDIR = os.path.join(ROOT, "spread_spectrum_watermarking_amd", "lib")
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


def dev_resample(frames, nw, nh, filt, off_in=0, off_out=0):
    """frames [n, h, w, 3] -> [n, nh, nw, 3] and the SENTINEL byte behind the last frame; also checks that the input is unchanged."""
    n, h, w, _ = frames.shape
    d, o = Dev(frames, off_in), Dev(n * nh * nw * 3 + 1, off_out)
    check(lib().ssw_resample_rgb8(ctx().handle, d.ptr, n, w, h, nw, nh, filt, o.ptr), "ssw_resample_rgb8")
    out = o.host(np.uint8, (n * nh * nw * 3 + 1,))
    assert np.array_equal(d.host(np.uint8, frames.shape), frames), "the call changed its input"
    d.free(); o.free()
    assert out[-1] == SENTINEL, "a byte behind the last frame was written"
    return out[:-1].reshape(n, nh, nw, 3)


def jobs_c(jobs):
    """jobs: (frame, nw, nh, filter)"""
    return (L.ScaleJob * max(len(jobs), 1))(*[L.ScaleJob(*j) for j in jobs])


def dev_scale_attack(frames, jobs, extra=0):
    n, h, w, _ = frames.shape
    d, o = Dev(frames), Dev((len(jobs) + extra) * h * w * 3)
    check(lib().ssw_scale_attack_rgb8(ctx().handle, d.ptr, n, w, h, jobs_c(jobs), len(jobs), o.ptr), "ssw_scale_attack_rgb8")
    out = o.host(np.uint8, (len(jobs) + extra, h, w, 3))
    assert np.array_equal(d.host(np.uint8, frames.shape), frames), "the call changed its input"
    d.free(); o.free()
    return out


def every_kind(h, w, seed=0):
    return np.stack([content(kind, h, w, seed) for kind in CONTENTS])


# ---- equality ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SHAPES)
def test_equals_the_restatement_for_every_content_target_and_filter(h, w):
    frames = every_kind(h, w)                                                    # six frames: a batch of five and a batch of one
    for nw, nh, filters in targets(h, w):
        for f in filters:
            out = np.concatenate([dev_resample(frames[:5], nw, nh, f), dev_resample(frames[5:], nw, nh, f)])
            for i, kind in enumerate(CONTENTS):
                assert np.array_equal(out[i], resample_ref(frames[i], nw, nh, f)), (kind, nw, nh, NAMES[f])


def test_equals_the_restatement_on_the_cat(cat):
    """640 x 444: three runs of the row kernel, two blocks of a row of the column kernel."""
    for nw, nh, f in ((320, 222, BICUBIC), (80, 56, LANCZOS), (211, 147, BILINEAR), (641, 444, BOX), (640, 111, LANCZOS)):
        assert np.array_equal(dev_resample(cat[None], nw, nh, f)[0], resample_ref(cat, nw, nh, f)), (nw, nh, NAMES[f])


@pytest.mark.parametrize("h,w,nw,nh", [(3, 300, 3, 3), (3, 300, 3, 2), (9, 1100, 40, 9), (2, 6000, 2, 1), (2, 6000, 1, 2)])
def test_the_reductions_with_the_most_taps(h, w, nw, nh):
    """300 -> 3 columns with LANCZOS: 600 taps a column, the most at these sizes.  1100 -> 40: a run of 256 columns no longer fits
    the LDS and the host halves it.  6000 -> 2 and -> 1: not even four columns fit, taps and samples come from global memory."""
    frames = np.stack([content("noise", h, w, 3), content("checker3", h, w)])
    for f in (LANCZOS, BICUBIC, BOX):
        out = dev_resample(frames, nw, nh, f)
        for i in range(2):
            assert np.array_equal(out[i], resample_ref(frames[i], nw, nh, f)), (i, NAMES[f])


@pytest.mark.parametrize("h,w", [(5, 4), (67, 131)])
def test_at_every_byte_offset(h, w):
    frames = every_kind(h, w, seed=2)[:3]
    cases = [(max(1, w // 2), max(1, h // 2), BICUBIC), (w, 2 * h, LANCZOS), (w + 1, h, BILINEAR)]     # both passes, columns only, rows only
    want = [np.stack([resample_ref(fr, nw, nh, f) for fr in frames]) for nw, nh, f in cases]
    for off_in in range(4):
        for off_out in range(4):
            for (nw, nh, f), ref in zip(cases, want):
                assert np.array_equal(dev_resample(frames, nw, nh, f, off_in, off_out), ref), (off_in, off_out, nw, nh)


# ---- workspace ---------------------------------------------------------------------------------------------------------------
def test_a_small_call_after_a_large_one_gives_what_a_fresh_context_gives():
    small = every_kind(9, 31, seed=5)[:3]
    jobs = [(0, 15, 4, BICUBIC), (1, 15, 4, BICUBIC), (2, 7, 9, LANCZOS)]
    with G.fresh_ctx():
        want = dev_resample(small, 15, 4, LANCZOS), dev_scale_attack(small, jobs)
    with G.fresh_ctx():
        large = every_kind(100, 300, seed=6)
        big = dev_resample(large, 150, 50, LANCZOS)
        assert np.array_equal(big[1], resample_ref(large[1], 150, 50, LANCZOS))
        assert np.array_equal(dev_resample(small, 15, 4, LANCZOS), want[0])       # on tables and planes the large call left full
        assert np.array_equal(dev_scale_attack(small, jobs), want[1])
    assert np.array_equal(want[0], np.stack([resample_ref(f, 15, 4, LANCZOS) for f in small]))


# ---- the attack --------------------------------------------------------------------------------------------------------------
def there_and_back(frame, nw, nh, f):
    """ssw_resize_rgb8(ssw_resample_rgb8(frame)): the two calls the attack must equal bit for bit"""
    h, w = frame.shape[:2]
    thumb = dev_resample(frame[None], nw, nh, f)
    return thumb[0] if (nw, nh) == (w, h) else G.resize_rgb8(thumb, w, h)[0]


def test_forty_jobs_out_of_order_with_repeats_and_nothing_beyond_the_last():
    h, w = 19, 17
    frames = np.stack([content(CONTENTS[i % 6], h, w, seed=i) for i in range(5)])
    sizes = [(8, 9, BICUBIC), (8, 9, LANCZOS), (17, 19, BOX), (34, 38, BILINEAR), (5, 19, LANCZOS), (17, 6, BICUBIC), (1, 1, BOX), (18, 18, BICUBIC)]
    rng = np.random.default_rng(11)
    jobs = [(int(rng.integers(0, 5)),) + sizes[int(rng.integers(0, len(sizes)))] for _ in range(40)]
    jobs[3], jobs[4], jobs[5] = (4,) + sizes[0], (4,) + sizes[0], (1,) + sizes[0]           # a batch of three, a frame twice in it
    jobs[20], jobs[21], jobs[39] = (2,) + sizes[2], (0,) + sizes[2], (4,) + sizes[0]        # same-size jobs: copies; a repeat far apart
    out = dev_scale_attack(frames, jobs, extra=1)
    memo = {}
    for i, j in enumerate(jobs):
        if j not in memo:
            memo[j] = there_and_back(frames[j[0]], *j[1:])
        assert np.array_equal(out[i], memo[j]), (i, j)
    assert np.array_equal(out[20], frames[2]) and np.array_equal(out[21], frames[0])        # nw == w && nh == h is a plain copy
    assert np.all(out[40] == SENTINEL)
    for i in (0, 4, 39):                                                                     # alone = inside the batch
        assert np.array_equal(dev_scale_attack(frames, [jobs[i]])[0], out[i]), i


def test_every_job_equals_resample_then_resize(cat):
    frames = np.stack([cat[:120, :200], content("noise", 120, 200), content("checker3", 120, 200)])
    jobs = [(f, nw, nh, filt) for f in range(3) for nw, nh, filt in ((100, 60, BICUBIC), (25, 15, LANCZOS), (400, 240, BILINEAR), (66, 120, BOX))]
    out = dev_scale_attack(frames, jobs)                                                      # frame-major: every job a batch of its own
    for i, j in enumerate(jobs):
        assert np.array_equal(out[i], there_and_back(frames[j[0]], *j[1:])), j


# ---- status codes ------------------------------------------------------------------------------------------------------------
def test_status_codes():
    rs, sa, hd = lib().ssw_resample_rgb8, lib().ssw_scale_attack_rgb8, ctx().handle
    frames = every_kind(8, 16, seed=7)[:3]
    fb = 8 * 16 * 3
    d, o = Dev(frames), Dev(2 * fb)
    untouched = lambda: np.all(o.host(np.uint8, (2 * fb,)) == SENTINEL)
    # n_frames == 0 / n_jobs == 0 come first
    assert rs(hd, None, 0, 0, 0, 0, 0, 99, None) == L.SSW_OK and sa(hd, None, 0, 0, 0, None, 0, None) == L.SSW_OK
    assert rs(hd, d.ptr, 0, 16, 8, 8, 4, BICUBIC, o.ptr) == L.SSW_OK and sa(hd, d.ptr, 3, 16, 8, jobs_c([(0, 8, 4, 2)]), 0, o.ptr) == L.SSW_OK
    # a null pointer
    assert rs(None, d.ptr, 2, 16, 8, 8, 4, BICUBIC, o.ptr) == L.SSW_ERR_BAD_ARG
    assert rs(hd, None, 2, 16, 8, 8, 4, BICUBIC, o.ptr) == L.SSW_ERR_BAD_ARG
    assert rs(hd, d.ptr, 2, 16, 8, 8, 4, BICUBIC, None) == L.SSW_ERR_BAD_ARG
    good = jobs_c([(0, 8, 4, BICUBIC), (2, 16, 8, BOX)])
    assert sa(None, d.ptr, 3, 16, 8, good, 2, o.ptr) == L.SSW_ERR_BAD_ARG
    assert sa(hd, None, 3, 16, 8, good, 2, o.ptr) == L.SSW_ERR_BAD_ARG
    assert sa(hd, d.ptr, 3, 16, 8, None, 2, o.ptr) == L.SSW_ERR_BAD_ARG
    assert sa(hd, d.ptr, 3, 16, 8, good, 2, None) == L.SSW_ERR_BAD_ARG
    # frame >= n_frames, behind a good job: nothing is enqueued
    for bad in ((3, 8, 4, BICUBIC), (0xFFFFFFFF, 8, 4, BICUBIC)):
        assert sa(hd, d.ptr, 3, 16, 8, jobs_c([(0, 8, 4, BICUBIC), bad]), 2, o.ptr) == L.SSW_ERR_BAD_ARG, bad
    assert sa(hd, d.ptr, 2, 16, 8, good, 2, o.ptr) == L.SSW_ERR_BAD_ARG                      # frame 2 of 2 frames
    # an unknown filter
    for bad in (4, 0xFFFFFFFF):
        assert sa(hd, d.ptr, 3, 16, 8, jobs_c([(0, 8, 4, BICUBIC), (1, 8, 4, bad)]), 2, o.ptr) == L.SSW_ERR_BAD_ARG, bad
    for bad in (4, -1):
        assert rs(hd, d.ptr, 2, 16, 8, 8, 4, bad, o.ptr) == L.SSW_ERR_BAD_ARG, bad
    # an overlapping dev_out
    inside = C.c_void_p(d.ptr.value + fb)
    assert rs(hd, d.ptr, 3, 16, 8, 8, 4, BICUBIC, inside) == L.SSW_ERR_BAD_ARG
    assert rs(hd, d.ptr, 3, 16, 8, 8, 4, BICUBIC, d.ptr) == L.SSW_ERR_BAD_ARG
    assert sa(hd, d.ptr, 3, 16, 8, good, 2, inside) == L.SSW_ERR_BAD_ARG
    ctx().synchronize()
    assert np.array_equal(d.host(np.uint8, frames.shape), frames)
    # a side of 0 or above 65535
    for w, h, nw, nh in ((0, 8, 8, 4), (16, 0, 8, 4), (16, 8, 0, 4), (16, 8, 8, 0), (65536, 8, 8, 4), (16, 65536, 8, 4), (16, 8, 65536, 4), (16, 8, 8, 65536)):
        assert rs(hd, d.ptr, 2, w, h, nw, nh, BICUBIC, o.ptr) == L.SSW_ERR_BAD_DIMS, (w, h, nw, nh)
        assert sa(hd, d.ptr, 3, w, h, jobs_c([(0, 8, 4, BICUBIC), (0, nw, nh, BICUBIC)]), 2, o.ptr) == L.SSW_ERR_BAD_DIMS, (w, h, nw, nh)
    ctx().synchronize()
    assert untouched()
    assert sa(hd, d.ptr, 3, 16, 8, good, 2, o.ptr) == L.SSW_OK
    got = o.host(np.uint8, (2, 8, 16, 3))
    assert np.array_equal(got[0], there_and_back(frames[0], 8, 4, BICUBIC)) and np.array_equal(got[1], frames[2])
    d.free(); o.free()


# ---- timing ------------------------------------------------------------------------------------------------------------------
def test_timed_as_convert_with_the_stated_bytes():
    h, w = 41, 57
    frames = every_kind(h, w, seed=8)[:3]
    c = ctx()
    dev_resample(frames, 20, 30, BICUBIC)                                      # the way back's tap tables: made before the timed calls
    dev_scale_attack(frames, [(0, 20, 30, BICUBIC), (0, 57, 10, BOX)])
    c.enable_timing(True)
    try:
        c.reset_timing()
        dev_resample(frames, 20, 30, BICUBIC)                                  # both passes
        dev_resample(frames, 20, 41, LANCZOS)                                  # rows only: no plane
        dev_resample(frames, 57, 10, BOX)                                      # columns only
        t = c.timing()
        want = 3 * ((3 * w * h + 6 * 20 * h + 3 * 20 * 30) + (3 * w * h + 3 * 20 * h) + (3 * w * h + 3 * w * 10))
        assert t["convert"]["launches"] >= 3 and t["convert"]["work"] == want
        assert all(v["launches"] == 0 for k, v in t.items() if k != "convert") and len(t) == 15
        c.reset_timing()
        dev_scale_attack(frames, [(0, 20, 30, BICUBIC), (2, 20, 30, BICUBIC), (1, 57, 10, BOX), (1, 57, 41, BOX)])
        t = c.timing()
        there = 2 * (3 * w * h + 6 * 20 * h + 3 * 20 * 30) + (3 * w * h + 3 * w * 10) + 2 * 3 * w * h
        back = 2 * (3 * 20 * 30 + 3 * w * h) + (3 * w * 10 + 3 * w * h)        # as ssw_restore_rgb8 bills a resized whole frame
        assert t["convert"]["work"] == there and t["resize"]["work"] == back
        assert all(v["launches"] == 0 for k, v in t.items() if k not in ("convert", "resize"))
    finally:
        c.enable_timing(False)


# ---- the Python wrappers -----------------------------------------------------------------------------------------------------
def test_python_resample_and_scale_attack_in_one_group_and_in_many(monkeypatch):
    h, w = 24, 40
    images = [content(CONTENTS[i % 6], h, w, seed=20 + i) for i in range(4)]
    scales = [api.Scale(0.5), api.Scale(0.25, "lanczos"), api.Scale.to(50, 24, "bilinear"), api.Scale(1)]
    want = [[there_and_back(im, *s.size(w, h), L.RESAMPLE_FILTERS[s.filter]) for s in scales] for im in images]
    thumbs = [resample_ref(im, 13, 7, LANCZOS) for im in images]
    for cap in (api.UPLOAD_GROUP_BYTES, 5 * h * w * 3, 1):                                   # one group | frames and jobs split | a job a group
        monkeypatch.setattr(api, "UPLOAD_GROUP_BYTES", cap)
        got = api.scale_attack(images, scales, ctx())
        assert len(got) == 4 and all(len(g) == 4 for g in got)
        for i in range(4):
            for j in range(4):
                assert np.array_equal(got[i][j], want[i][j]), (cap, i, j)
        small = api.resample(images, (13, 7), "lanczos", ctx())
        assert len(small) == 4 and all(np.array_equal(a, b) for a, b in zip(small, thumbs)), cap
    assert np.array_equal(want[0][3], images[0])


# ---- the report --------------------------------------------------------------------------------------------------------------
def same(a, b):
    return a == b or (a != a and b != b)


def test_strength_report_equals_the_chain_through_the_host(cat):
    """Field for field against mark_copies_rgb8 -> api.scale_attack -> trace_many -> api.quality -> api.ssim."""
    alphas, n, k = [0.02, 0.1], 3, 200
    scales = [api.Scale(0.5), api.Scale(0.25, "lanczos")]
    c = ctx()
    rows = api.strength_report(cat, alphas, copies=n, k=k, sizes=(2,), scales=scales, ssim=True, seed=3, ctx=c)
    plain = api.strength_report(cat, alphas, copies=n, k=k, sizes=(2,), ssim=True, seed=3, ctx=c)
    marks = np.random.default_rng(3).standard_normal((n, k)).astype(np.float32)
    for r, p in zip(rows, plain):
        assert (r.alpha, r.quality, r.collusions, r.jpeg, r.ssim, r.filters) == (p.alpha, p.quality, p.collusions, p.jpeg, p.ssim, p.filters) and p.scales == []
        copies = api.Writer(cat, api.WriteConfig(insertion=api.Insertion.Option2(r.alpha)), c).mark_copies_rgb8(list(marks))
        per_copy = api.scale_attack(list(copies), scales, c)
        attacked = [per_copy[i][j] for j in range(len(scales)) for i in range(n)]
        traced = api.trace_many(cat, attacked, list(marks), threshold=6.0, config=api.ReadConfig(extraction=api.Extraction.Option2(r.alpha)), ctx=c)
        quality, ssims = api.quality(cat, attacked, c), api.ssim(cat, attacked, c)
        assert [(j.scale, j.size) for j in r.scales] == [("scale 0.5 bicubic", (320, 222)), ("scale 0.25 lanczos", (160, 111))]
        for i, j in enumerate(r.scales):
            sims = np.asarray(traced.sims[i * n:(i + 1) * n])
            own, others = np.diagonal(sims), sims[~np.eye(n, dtype=bool)]
            psnr = [q.psnr for q in quality[i * n:(i + 1) * n]]
            mean = [s.mean for s in ssims[i * n:(i + 1) * n]]
            print(f"alpha {r.alpha}: {j}")
            assert same(j.weakest_own, float(own.min())) and same(j.strongest_innocent, float(others.max())), (r.alpha, j)
            assert j.survived == int((own > np.float32(6.0)).sum()) and j.accused == int((others > np.float32(6.0)).sum()), (r.alpha, j)
            assert (j.psnr_min, j.psnr_max) == (min(psnr), max(psnr)), (r.alpha, j)
            assert (j.ssim_min, j.ssim_max) == (min(mean), max(mean)), (r.alpha, j)


def test_the_report_says_what_trace_finds_in_a_thumbnail_pillow_made(cat):
    """The claim the feature makes: for alpha 0.1 and Scale(0.5), copy c shrunk by PIL.Image.resize((320, 222), BICUBIC) itself and
    handed to trace_many as it is has the similarities of row c of the report's matrix -- exactly, in float32 bits."""
    from PIL import Image
    n, k, alpha = 3, 200, 0.1
    c = ctx()
    marks = np.random.default_rng(3).standard_normal((n, k)).astype(np.float32)
    copies = api.Writer(cat, api.WriteConfig(insertion=api.Insertion.Option2(alpha)), c).mark_copies_rgb8(list(marks))
    # the report's matrix: the report keeps only its folds, so the same device chain is run here on the copies
    attacked = [a[0] for a in api.scale_attack(list(copies), [api.Scale(0.5)], c)]
    cfg = api.ReadConfig(extraction=api.Extraction.Option2(alpha))
    matrix = np.asarray(api.trace_many(cat, attacked, list(marks), threshold=6.0, config=cfg, ctx=c).sims, np.float32)
    row = api.strength_report(cat, [alpha], copies=n, k=k, sizes=(2,), scales=[api.Scale(0.5)], seed=3, ctx=c)[0].scales[0]
    own, others = np.diagonal(matrix), matrix[~np.eye(n, dtype=bool)]
    assert row.weakest_own == float(own.min()) and row.strongest_innocent == float(others.max()) and row.size == (320, 222)
    for i in range(n):
        thumb = np.asarray(Image.fromarray(copies[i]).resize((320, 222), Image.BICUBIC))
        sims = np.asarray(api.trace_many(cat, [thumb], list(marks), threshold=6.0, config=cfg, ctx=c, placements=[None]).sims, np.float32)[0]     # a suspect of another size: restored, then traced
        print(f"copy {i}: thumbnail {sims.tolist()} report {matrix[i].tolist()}")
        assert sims.tobytes() == matrix[i].tobytes(), i
    assert row.survived == n and row.accused == 0


def test_cli_strength_prints_the_scale_rows(cat, tmp_path, capsys):
    from PIL import Image
    path = str(tmp_path / "cat.png")
    Image.fromarray(cat).save(path)
    assert cli.main(["strength", path, "--alpha", "0.1", "--copies", "3", "--collude", "2", "--method", "average", "-n", "200",
                     "--scale", "0.5", "0.25:lanczos"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[3].startswith("  average of 2: found 2/2") and len(lines) == 6
    row = r"  %s: own mark found \d/3, weakest -?\d+\.\d, strongest innocent -?\d+\.\d(, \d innocent accused)?, \d\d\.\d \.\. \d\d\.\d dB"
    for line, label in zip(lines[4:], ("scale 0.5 bicubic (320x222)", "scale 0.25 lanczos (160x111)")):
        assert re.fullmatch(row % re.escape(label), line), line
    assert cli.main(["strength", path, "--alpha", "0.1", "--copies", "3", "--collude", "2", "--method", "average", "-n", "200",
                     "--scale", "0.5", "0.25:lanczos", "--json"]) == 0
    doc = json.loads(capsys.readouterr().out)
    assert [s["scale"] for s in doc[0]["scales"]] == ["scale 0.5 bicubic", "scale 0.25 lanczos"]
    assert [s["size"] for s in doc[0]["scales"]] == [[320, 222], [160, 111]]
    assert sorted(doc[0]["scales"][0]) == ["accused", "psnr_max", "psnr_min", "scale", "size", "strongest_innocent", "survived", "weakest_own"]
    assert doc[0]["scales"][0]["survived"] == 3 and 20.0 < doc[0]["scales"][0]["psnr_min"] <= doc[0]["scales"][0]["psnr_max"] < 60.0


# ---- the C++ wrappers --------------------------------------------------------------------------------------------------------
def test_cpp_wrappers_equal_the_c_calls(tmp_path):
    exe = str(tmp_path / "scale_wrappers_test")
    done = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "scale_wrappers_test.cpp"), "-o", exe,
                           "-L", LIBDIR, "-lssw_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True, text=True)
    assert done.stderr == "", done.stderr
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
