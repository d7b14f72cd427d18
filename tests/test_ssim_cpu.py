"""ssw_ssim_rgb8 (include/ssw.h) without a GPU: the numpy restatement of the definition -- what the device results must EQUAL
(tests/test_ssim_gpu.py imports it) -- its known answers and properties, and the surfaces (header, Python)."""
import math
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd import api
import spread_spectrum_watermarking_amd as wm

ONE = 1 << 30


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def luma_ref(img, dtype=np.int64):
    p = np.asarray(img).astype(dtype)
    return (77 * p[..., 0] + 150 * p[..., 1] + 29 * p[..., 2] + 128) >> 8


def ssim_ref(base, copy, dtype=np.int64):
    """base, copy [h, w, 3] u8 -> (stats[0], stats[1], the map int32 [ny, nx]); every integer up to the division in `dtype`."""
    a, b = luma_ref(base, dtype), luma_ref(copy, dtype)
    h, w = a.shape
    cells = lambda x: x[:h // 4 * 4, :w // 4 * 4].reshape(h // 4, 4, w // 4, 4).sum(axis=(1, 3), dtype=dtype)
    win = lambda c: c[:-1, :-1] + c[:-1, 1:] + c[1:, :-1] + c[1:, 1:]
    s1, s2, ss, s12 = win(cells(a)), win(cells(b)), win(cells(a * a + b * b)), win(cells(a * b))
    vars_, covar = 64 * ss - s1 * s1 - s2 * s2, 64 * s12 - s1 * s2
    n1, n2 = 2 * s1 * s2 + 416, 2 * covar + 235963
    d1, d2 = s1 * s1 + s2 * s2 + 416, vars_ + 235963
    assert all(x.dtype == dtype for x in (n1, n2, d1, d2))
    q = (n1.astype(np.float64) * n2.astype(np.float64)) / (d1.astype(np.float64) * d2.astype(np.float64))
    t = np.floor(q * float(ONE) + 0.5).astype(np.int64)
    key = ((t.reshape(-1) + ONE).astype(np.uint64) << np.uint64(32)) | np.arange(t.size, dtype=np.uint64)
    return int(t.sum()), int(key.min()), t.astype(np.int32)


# ---- the frames both test files use ------------------------------------------------------------------------------------------
def cat_pair():
    g = np.load(os.path.join(GOLDEN, "cat_decoded_u8.npz"))      # the decoded porcelain_cat_grey_background.jpg and watermarked_with_1.png
    return np.ascontiguousarray(g["cat"]), np.ascontiguousarray(g["watermarked_with_1"])


CONTENTS = ("noise", "binary", "checkerboard")


def pair(kind, w, h, seed=0):
    """(original, copy) u8 [h, w, 3]: uniform noise and the same +- 6; random 0 / 255 bytes twice (the largest sums, negative
    covariances); a checkerboard and its negative (the most negative value)."""
    rng = np.random.default_rng([seed, h, w, CONTENTS.index(kind)])
    if kind == "noise":
        a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        return a, np.clip(a.astype(np.int16) + rng.integers(-6, 7, a.shape), 0, 255).astype(np.uint8)
    if kind == "binary":
        return tuple((rng.integers(0, 2, (h, w, 3), dtype=np.uint8) * 255).astype(np.uint8) for _ in range(2))
    y, x = np.mgrid[0:h, 0:w]
    a = np.repeat((((x + y) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)
    return a, 255 - a


# ---- known answers -----------------------------------------------------------------------------------------------------------
def test_known_answers_on_the_cat():
    cat, marked = cat_pair()
    assert cat.shape == (444, 640, 3)
    s, key, t = ssim_ref(cat, marked)
    assert t.shape == (110, 159)
    assert s == 18_638_317_194_866 and round(s / (ONE * t.size), 8) == 0.99246916
    assert key == 8_083_853_789_443_929_881
    assert (key >> 32) - ONE == 808_427_057 == int(t.min()) and round(808_427_057 / ONE, 8) == 0.75290637
    assert key & 0xFFFFFFFF == 14105 == 88 * 159 + 113 == int(np.argmin(t))


def test_golden_files_decode_to_the_stored_frames():
    from PIL import Image
    cat, marked = cat_pair()
    assert np.array_equal(np.asarray(Image.open(os.path.join(GOLDEN, "watermarked_with_1.png")).convert("RGB")), marked)


def test_known_answers_on_the_37_by_21_pair():
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, (21, 37, 3), dtype=np.uint8)           # bytes, as frames are
    b = np.clip(a + rng.integers(-6, 7, a.shape), 0, 255)
    s, key, t = ssim_ref(a, b)
    assert t.shape == (4, 8) and s == 34_313_286_561 and int(t.min()) == 1_071_782_930


def test_extreme_pairs():
    a, b = pair("checkerboard", 16, 16)
    s, _, t = ssim_ref(a, b)
    assert round(s / (ONE * t.size), 5) == -0.99646 and np.all(t == t[0, 0])
    s, _, t = ssim_ref(np.zeros((16, 16, 3), np.uint8), np.full((16, 16, 3), 255, np.uint8))
    assert f"{s / (ONE * t.size):.4e}" == "1.5618e-06"


def test_equal_frames_give_one_everywhere_and_the_first_window():
    for kind in CONTENTS:
        a, _ = pair(kind, 37, 21)
        s, key, t = ssim_ref(a, a)
        assert np.all(t == ONE) and s == ONE * t.size and key == (2 * ONE) << 32, kind      # index 0


@pytest.mark.parametrize("kind", ["checkerboard", "binary", "extremes"])
def test_values_stay_within_one(kind):
    if kind == "extremes":
        a, b = np.zeros((24, 40, 3), np.uint8), np.full((24, 40, 3), 255, np.uint8)
    else:
        a, b = pair(kind, 40, 24)
    for x, y in ((a, b), (b, a)):
        _, key, t = ssim_ref(x, y)
        assert np.all(np.abs(t.astype(np.int64)) <= ONE) and t.min() > -ONE and 0 < key >> 32 <= 2 * ONE


@pytest.mark.parametrize("kind", CONTENTS + ("cat", "extremes"))
def test_32_bit_integers_suffice(kind):
    if kind == "cat":
        a, b = cat_pair()
    elif kind == "extremes":
        a, b = np.full((16, 16, 3), 255, np.uint8), np.full((16, 16, 3), 255, np.uint8)
        b[::2] = 0
    else:
        a, b = pair(kind, 37, 21)
    wide, narrow = ssim_ref(a, b), ssim_ref(a, b, np.int32)
    assert wide[:2] == narrow[:2] and np.array_equal(wide[2], narrow[2])


@pytest.mark.parametrize("w,h,nx,ny", [(8, 8, 1, 1), (11, 11, 1, 1), (12, 8, 2, 1), (15, 16, 2, 3)])
def test_window_geometry(w, h, nx, ny):
    a, b = pair("noise", w, h)
    s, key, t = ssim_ref(a, b)
    assert t.shape == (ny, nx) == api._ssim_windows(w, h)[::-1]
    # the trailing pixels take no part, and a window is the 8 x 8 pixels at four times its index
    b2 = b.copy()
    b2[h // 4 * 4:], b2[:, w // 4 * 4:] = 0, 0
    assert np.array_equal(ssim_ref(a, b2)[2], t)
    for wy in range(ny):
        for wx in range(nx):
            alone = ssim_ref(a[4 * wy:4 * wy + 8, 4 * wx:4 * wx + 8], b[4 * wy:4 * wy + 8, 4 * wx:4 * wx + 8])
            assert alone[2].shape == (1, 1) and alone[2][0, 0] == t[wy, wx] and alone[0] == t[wy, wx]


# ---- the surfaces ------------------------------------------------------------------------------------------------------------
def test_ssim_figures_from_hand_made_statistics():
    worst = ONE // 4
    stats = np.array([[3 * ONE + ONE // 2, ((worst + ONE) << 32) | 7], [np.uint64(-5 * ONE & (2 ** 64 - 1)), (1 << 32) | 11]], np.uint64)
    a, b = api._ssims(stats, 4, 3)
    assert (a.sum, a.worst, a.worst_index, a.windows_x, a.windows_y, a.map) == (3 * ONE + ONE // 2, worst, 7, 4, 3, None)
    assert a.mean == 3.5 / 12 and a.worst_value == 0.25 and a.worst_position == (12, 4)
    assert (b.sum, b.worst, b.worst_index) == (-5 * ONE, 1 - ONE, 11) and b.mean == -5 / 12 and b.worst_position == (12, 8)
    maps = np.arange(24, dtype=np.int32).reshape(2, 3, 4)
    assert np.array_equal(api._ssims(stats, 4, 3, maps)[1].map, maps[1])
    s = wm.Ssim(ONE, ONE, 0, 1, 1)
    assert s.mean == 1.0 and s.worst_value == 1.0 and s.worst_position == (0, 0)


def test_ssim_refuses_small_frames_before_any_context(monkeypatch):
    monkeypatch.setattr(api, "default_context", lambda: pytest.fail("a context was asked for"))
    small = np.zeros((9, 7, 3), np.uint8)                          # 7 wide
    with pytest.raises(ValueError, match="at least 8 x 8"):
        wm.ssim(small, [small])
    with pytest.raises(ValueError, match="at least 8 x 8"):
        wm.ssim(small.transpose(1, 0, 2), [small.transpose(1, 0, 2)])
    with pytest.raises(ValueError, match="at least 8 x 8"):
        wm.strength_report(small, [0.1], ssim=True)
    with pytest.raises(ValueError):
        wm.ssim(np.zeros((8, 8, 3), np.uint8), [np.zeros((8, 9, 3), np.uint8)])
    assert wm.ssim(small, []) == []


def test_report_rows_build_with_their_old_arguments():
    row = api.StrengthRow(0.1, [], [])
    assert row.ssim == [] and row.jpeg == []
    assert api.StrengthRow(0.1, [], [], [1]).jpeg == [1]
    j = api.JpegResult(75, 8, 20.0, 3.0, 0, 33.0, 35.0)
    assert math.isnan(j.ssim_min) and math.isnan(j.ssim_max) and j.psnr_max == 35.0
    plain = api._jpeg_result(50, np.eye(2, dtype=np.float32) * 9, [api.Quality((1, 1, 1), 1, 3, 1, 64)] * 2, 6.0)
    assert plain.survived == 2 and math.isnan(plain.ssim_min)
    both = api._jpeg_result(50, np.eye(2, dtype=np.float32) * 9, [api.Quality((1, 1, 1), 1, 3, 1, 64)] * 2, 6.0,
                            [api.Ssim(ONE // 2, 0, 0, 1, 1), api.Ssim(ONE, 0, 0, 1, 1)])
    assert (both.ssim_min, both.ssim_max) == (0.5, 1.0)


def test_header_declares_the_call_and_its_constants():
    text = open(os.path.join(ROOT, "include", "ssw.h")).read()
    decl = re.search(r"int ssw_ssim_rgb8\(ssw_ctx\* ctx, const uint8_t\* dev_base, size_t n_base, const uint8_t\* dev_copies, size_t n, size_t w,"
                     r"\s+size_t h,\s+uint64_t\* dev_stats, int32_t\* dev_map\);", text)
    assert decl and text.index("ssw_jpeg_rgb8(") < decl.start()
    for name, value in (("SSW_SSIM_MIN_SIDE", "8"), ("SSW_SSIM_ONE", "1 << 30"), ("SSW_SSIM_STATS", "2"),
                        ("SSW_SSIM_TILE_W", str(L.SSIM_TILE_W)), ("SSW_SSIM_TILE_H", str(L.SSIM_TILE_H))):
        assert re.search(rf"\b{name} = {re.escape(value)}\b", text), name
    assert (L.SSIM_MIN_SIDE, L.SSIM_ONE, L.SSIM_STATS) == (8, ONE, 2)
    comment = text[text.rfind("/*", 0, decl.start()):decl.start()]
    for phrase in ("x264 / FFmpeg", "no bit equality", "luma only", "not the Gaussian 11 x 11", "trailing pixels ignored", "no multi-scale variant",
                   "no host-streaming form", "235963", "tests/test_ssim_cpu.py"):
        assert phrase in comment, phrase
    assert "ssw_ssim_rgb8" in L.SIGNATURES and len(L.SIGNATURES["ssw_ssim_rgb8"][1]) == 9
