"""ssw_jpeg_rgb8 on the device against `jpeg_ref`, the numpy restatement of tests/test_jpeg_cpu.py (itself checked there against
PIL byte for byte): every comparison is np.array_equal, there is no tolerance.  Shapes are the smallest at which the kernels can
go wrong: one block, one MCU, odd sides, a last band of 8 rows (the chroma's bottom padding), thin strips, more than two strips
of 16 MCUs with a remainder and more than two bands, more jobs than two launches hold, byte offsets 0 .. 3 of both pointers."""
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
from test_jpeg_cpu import CONTENTS, cat_image, content, jpeg_ref

pytestmark = pytest.mark.gpu

QUALITIES = (1, 10, 50, 75, 95, 100)
# (h, w); the last: a strip of the codec kernel is 256 pixels wide, a band 16 rows high -- two strips + 37 columns, two bands + 11 rows
SHAPES = [(8, 8), (16, 16), (19, 17), (47, 33), (40, 56), (41, 57), (8, 100), (100, 8), (43, 549)]
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
    return (L.JpegJob * max(len(jobs), 1))(*[L.JpegJob(f, q) for f, q in jobs])


def dev_jpeg(frames, jobs, off_in=0, off_out=0, extra=0):
    """frames [n, h, w, 3], jobs (frame, quality) pairs -> [len(jobs) + extra, h, w, 3]: `extra` frames behind the last job's
    that the call must leave as they were.  Also checks that the input is unchanged."""
    n, h, w, _ = frames.shape
    d, o = Dev(frames, off_in), Dev((len(jobs) + extra) * h * w * 3, off_out)
    check(lib().ssw_jpeg_rgb8(ctx().handle, d.ptr, n, w, h, jobs_c(jobs), len(jobs), o.ptr), "ssw_jpeg_rgb8")
    out = o.host(np.uint8, (len(jobs) + extra, h, w, 3))
    assert np.array_equal(d.host(np.uint8, frames.shape), frames), "the call changed its input"
    d.free(); o.free()
    return out


def every_kind(h, w, seed=0):
    return np.stack([content(kind, h, w, seed) for kind in CONTENTS])


# ---- equality ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SHAPES)
def test_equals_the_restatement_for_every_content_and_quality(h, w):
    frames = every_kind(h, w)
    jobs = [(f, q) for f in range(3) for q in QUALITIES]
    out = dev_jpeg(frames, jobs)
    for i, (f, q) in enumerate(jobs):
        assert np.array_equal(out[i], jpeg_ref(frames[f], q)), (CONTENTS[f], q)


def test_equals_the_restatement_on_the_cat(cat):
    """640 x 444: 444 = 27 * 16 + 12 rows, 2.5 strips; the photograph at every quality, noise and 0 / 255 bytes at two."""
    h, w = cat.shape[:2]
    frames = np.stack([cat, content("noise", h, w), content("binary", h, w)])
    jobs = [(0, q) for q in QUALITIES] + [(f, q) for f in (1, 2) for q in (1, 75)]
    out = dev_jpeg(frames, jobs)
    for i, (f, q) in enumerate(jobs):
        assert np.array_equal(out[i], jpeg_ref(frames[f], q)), (f, q)


# ---- jobs --------------------------------------------------------------------------------------------------------------------
def test_forty_jobs_out_of_order_with_repeats_and_nothing_beyond_the_last():
    h, w = 19, 17
    frames = np.stack([content(CONTENTS[i % 3], h, w, seed=i) for i in range(5)])
    rng = np.random.default_rng(11)
    jobs = [(int(rng.integers(0, 5)), int(rng.integers(1, 101))) for _ in range(40)]       # three launches: 16, 16 and 8 jobs
    jobs[3], jobs[20], jobs[39] = (4, 50), (4, 50), (0, 50)                                # a frame twice at one quality, far apart
    out = dev_jpeg(frames, jobs, extra=1)
    ref = {}
    for i, job in enumerate(jobs):
        if job not in ref:
            ref[job] = jpeg_ref(frames[job[0]], job[1])
        assert np.array_equal(out[i], ref[job]), (i, job)
    assert np.all(out[40] == SENTINEL)
    for i in (0, 17, 39):                                                                   # alone = inside the batch
        assert np.array_equal(dev_jpeg(frames, [jobs[i]])[0], out[i]), i


@pytest.mark.parametrize("h,w", [(19, 17), (40, 56)])
def test_at_every_byte_offset(h, w):
    frames = every_kind(h, w, seed=2)
    jobs = [(2, 10), (0, 75), (1, 100)]
    ref = np.stack([jpeg_ref(frames[f], q) for f, q in jobs])
    for off_in in range(4):
        for off_out in range(4):
            out = dev_jpeg(frames, jobs, off_in, off_out, extra=1)
            assert np.array_equal(out[:3], ref) and np.all(out[3] == SENTINEL), (off_in, off_out)


# ---- workspace ---------------------------------------------------------------------------------------------------------------
def test_a_small_call_after_a_large_one_gives_what_a_fresh_context_gives():
    small = every_kind(19, 17, seed=5)
    jobs = [(0, 30), (1, 60), (2, 90)]
    with G.fresh_ctx():
        want = dev_jpeg(small, jobs)
    with G.fresh_ctx():
        large = every_kind(100, 300, seed=6)
        big = dev_jpeg(large, [(f, q) for f in range(3) for q in (5, 85)])
        assert np.array_equal(big[1], jpeg_ref(large[0], 85))
        assert np.array_equal(dev_jpeg(small, jobs), want)                                  # on planes the large call left full
    assert np.array_equal(want, np.stack([jpeg_ref(small[f], q) for f, q in jobs]))


# ---- status codes ------------------------------------------------------------------------------------------------------------
def test_status_codes():
    f, hd = lib().ssw_jpeg_rgb8, ctx().handle
    frames = every_kind(8, 16, seed=7)
    d, o = Dev(frames), Dev(2 * 8 * 16 * 3)
    good = jobs_c([(0, 75), (2, 1)])
    untouched = lambda: np.all(o.host(np.uint8, (2 * 8 * 16 * 3,)) == SENTINEL)
    assert f(None, d.ptr, 3, 16, 8, good, 2, o.ptr) == L.SSW_ERR_BAD_ARG
    assert f(hd, None, 3, 16, 8, good, 2, o.ptr) == L.SSW_ERR_BAD_ARG
    assert f(hd, d.ptr, 3, 16, 8, None, 2, o.ptr) == L.SSW_ERR_BAD_ARG
    assert f(hd, d.ptr, 3, 16, 8, good, 2, None) == L.SSW_ERR_BAD_ARG
    for bad in ((0, 0), (0, 101), (0, 0xFFFFFFFF), (3, 50), (0xFFFFFFFF, 50)):              # a bad job behind a good one: nothing is enqueued
        assert f(hd, d.ptr, 3, 16, 8, jobs_c([(0, 75), bad]), 2, o.ptr) == L.SSW_ERR_BAD_ARG, bad
    assert f(hd, d.ptr, 2, 16, 8, good, 2, o.ptr) == L.SSW_ERR_BAD_ARG                      # frame 2 of 2 frames
    for w, h in ((7, 8), (16, 7), (1, 1), (4, 64)):                                         # a side below 8
        assert f(hd, d.ptr, 3, w, h, good, 2, o.ptr) == L.SSW_ERR_BAD_ARG, (w, h)
    for w, h in ((0, 8), (16, 0), (0, 0), (65536, 8), (8, 65536)):                          # empty, or more than a JPEG holds
        assert f(hd, d.ptr, 3, w, h, good, 2, o.ptr) == L.SSW_ERR_BAD_DIMS, (w, h)
    assert f(hd, d.ptr, 3, 16, 8, good, 0, o.ptr) == L.SSW_OK
    assert f(hd, None, 0, 0, 0, None, 0, None) == L.SSW_OK                                  # n_jobs == 0 comes first
    ctx().synchronize()
    assert untouched()
    assert f(hd, d.ptr, 3, 16, 8, good, 2, o.ptr) == L.SSW_OK
    assert np.array_equal(o.host(np.uint8, (2, 8, 16, 3)), np.stack([jpeg_ref(frames[0], 75), jpeg_ref(frames[2], 1)]))
    d.free(); o.free()


# ---- timing ------------------------------------------------------------------------------------------------------------------
def test_timed_as_convert_with_its_algorithmic_bytes():
    h, w = 41, 57
    frames = every_kind(h, w, seed=8)
    c = ctx()
    c.enable_timing(True)
    try:
        c.reset_timing()
        dev_jpeg(frames, [(0, 50), (1, 50), (1, 90), (2, 10), (0, 1)])
        t = c.timing()
        assert t["convert"]["launches"] >= 1 and t["convert"]["work"] == 5 * (2 * 3 * w * h + 2 * (w * h + 2 * 29 * 21))
        assert all(v["launches"] == 0 for k, v in t.items() if k != "convert") and len(t) == 15
    finally:
        c.enable_timing(False)


# ---- the Python wrapper ------------------------------------------------------------------------------------------------------
def test_python_jpeg_in_one_group_and_in_many(monkeypatch):
    h, w = 24, 40
    images = [content(CONTENTS[i % 3], h, w, seed=20 + i) for i in range(4)]
    qs = [90, 10, 55]
    want = [[jpeg_ref(im, q) for q in qs] for im in images]
    for cap in (api.UPLOAD_GROUP_BYTES, 5 * h * w * 3, 1):                                   # one group | frames and jobs split | a job a group
        monkeypatch.setattr(api, "UPLOAD_GROUP_BYTES", cap)
        got = api.jpeg(images, qs, ctx())
        assert len(got) == 4 and all(len(g) == 3 for g in got)
        for i in range(4):
            for j in range(3):
                assert np.array_equal(got[i][j], want[i][j]), (cap, i, j)


# ---- the report --------------------------------------------------------------------------------------------------------------
def same(a, b):
    return a == b or (a != a and b != b)


def test_strength_report_equals_the_chain_through_the_host(cat):
    """Field for field against mark_copies_rgb8 -> jpeg_ref on the host -> trace_many -> quality_ref.  The last assertions rest on
    the oracle, not on the device (own marks of the 8 copies of default_rng(3) after jpeg_ref): alpha 0.1 30.71 .. 32.37 at quality
    75 and 18.20 .. 20.13 at quality 10; alpha 0.02 24.83 .. 26.93 at quality 75, and at quality 10 3.74 .. 5.75 for seven copies and
    6.46 for one; no other mark above 2.28 anywhere."""
    alphas, qs, n, k = [0.02, 0.1], (75, 10), 8, 1000
    c = ctx()
    c.transfer_stats(reset=True)
    rows = api.strength_report(cat, alphas, jpeg=qs, seed=3, ctx=c)
    moved = c.transfer_stats(reset=True)
    # as before: the original and the marks went up, statistics and similarities came down -- no frame crossed PCIe
    assert cat.nbytes <= moved["h2d_bytes"] < 1.1 * cat.nbytes and 0 < moved["d2h_bytes"] < cat.nbytes // 100, moved
    plain = api.strength_report(cat, alphas, seed=3, ctx=c)
    marks = np.random.default_rng(3).standard_normal((n, k)).astype(np.float32)
    for r, p in zip(rows, plain):
        assert (r.alpha, r.quality, r.collusions) == (p.alpha, p.quality, p.collusions) and p.jpeg == []
        copies = api.Writer(cat, api.WriteConfig(insertion=api.Insertion.Option2(r.alpha)), c).mark_copies_rgb8(list(marks))
        coded = [jpeg_ref(copy, q) for q in qs for copy in copies]
        traced = api.trace_many(cat, coded, list(marks), threshold=6.0, config=api.ReadConfig(extraction=api.Extraction.Option2(r.alpha)), ctx=c)
        assert [j.quality for j in r.jpeg] == list(qs)
        for i, j in enumerate(r.jpeg):
            sims = np.asarray(traced.sims[i * n:(i + 1) * n])
            own, others = np.diagonal(sims), sims[~np.eye(n, dtype=bool)]
            psnr = [api.Quality(tuple(s[:3]), s[3], s[4], s[5], cat.shape[0] * cat.shape[1]).psnr
                    for s in (quality_ref(cat, f) for f in coded[i * n:(i + 1) * n])]
            print(f"alpha {r.alpha}, quality {j.quality}: {j}")
            assert same(j.weakest_own, float(own.min())) and same(j.strongest_innocent, float(others.max())), (r.alpha, j)
            assert j.survived == int((own > np.float32(6.0)).sum()) and j.accused == int((others > np.float32(6.0)).sum()), (r.alpha, j)
            assert (j.psnr_min, j.psnr_max) == (min(psnr), max(psnr)), (r.alpha, j)
    strong, faint = rows[1], rows[0]
    assert strong.jpeg[0].survived == n and strong.jpeg[1].survived == n and strong.jpeg[0].accused == 0
    assert faint.jpeg[0].survived == n and faint.jpeg[1].survived < n             # a quality-10 copy of a faint mark is lost
    assert strong.jpeg[1].psnr_max < strong.jpeg[0].psnr_min < strong.quality[0].psnr + 1.0      # coarser tables, further from the original
    lone = api.strength_report(cat[:64, :64], [0.1], k=100, copies=1, sizes=(), jpeg=(50,), seed=1, ctx=c)
    assert lone[0].jpeg[0].strongest_innocent != lone[0].jpeg[0].strongest_innocent and lone[0].jpeg[0].accused == 0


def test_cli_strength_prints_the_jpeg_rows(cat, tmp_path, capsys):
    from PIL import Image
    path = str(tmp_path / "cat.png")
    Image.fromarray(cat).save(path)
    assert cli.main(["strength", path, "--alpha", "0.1", "--copies", "4", "--collude", "2", "--method", "average", "--jpeg", "75", "10"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[3].startswith("  average of 2: found 2/2") and len(lines) == 6
    row = r"  jpeg %d: own mark found 4/4, weakest \d+\.\d, strongest innocent -?\d+\.\d, \d\d\.\d \.\. \d\d\.\d dB"
    assert re.fullmatch(row % 75, lines[4]), lines[4]
    assert re.fullmatch(row % 10, lines[5]), lines[5]
    assert cli.main(["strength", path, "--alpha", "0.1", "--copies", "2", "--collude", "2", "--method", "max", "-n", "100", "--jpeg", "50", "--json"]) == 0
    doc = json.loads(capsys.readouterr().out)
    assert [sorted(j) for j in doc[0]["jpeg"]] == [["accused", "psnr_max", "psnr_min", "quality", "strongest_innocent", "survived", "weakest_own"]]
    assert doc[0]["jpeg"][0]["quality"] == 50 and 20.0 < doc[0]["jpeg"][0]["psnr_min"] <= doc[0]["jpeg"][0]["psnr_max"] < 60.0
    assert cli.main(["strength", path, "--alpha", "0.1", "--copies", "2", "--collude", "2", "--method", "max", "-n", "100", "--json"]) == 0
    assert json.loads(capsys.readouterr().out)[0]["jpeg"] == []
    with pytest.raises(SystemExit):
        cli.main(["strength", path, "--alpha", "0.1", "--jpeg", "0"])
