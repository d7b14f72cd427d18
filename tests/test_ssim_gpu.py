"""ssw_ssim_rgb8 on the device against the numpy restatement of tests/test_ssim_cpu.py: every comparison is an equality, there is
no tolerance.  Shapes are the smallest at which the kernel can go wrong: one window, trailing pixels, rows that are no multiple
of four bytes, one block and the first size that needs a second one in either axis, thin strips of many blocks, byte offsets
0 .. 3 of the frame pointers, more copies than blocks and more blocks than copies (the stagger)."""
import ctypes as C
import json
import re

import numpy as np
import pytest

from gpu_util import ctx, fresh_ctx, lib
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd import api, cli
from spread_spectrum_watermarking_amd._lib import check
from test_collude_gpu import SENTINEL, Dev, same
from test_ssim_cpu import CONTENTS, ONE, cat_pair, pair, ssim_ref

pytestmark = pytest.mark.gpu

T_W, T_H = L.SSIM_TILE_W, L.SSIM_TILE_H              # pixels of windows a block owns (SSW_SSIM_TILE_W x _H; csrc/ssim.hip: SS_WX, SS_WY)
GUARD = 64

SMALL = [(8, 8), (11, 11), (12, 8), (8, 12), (13, 9), (37, 21), (16, 16)]                    # (w, h)
WIDTHS = [(w, 24) for w in (T_W - 4, T_W, T_W + 3, T_W + 4, T_W + 8, 2 * T_W + 4)]           # T_W + 4: the last width of one block
HEIGHTS = [(40, h) for h in (T_H - 4, T_H, T_H + 4, T_H + 8, 2 * T_H + 4)]
STRIPS = [(4099, 8), (8, 4099)]


def windows(w, h):
    return w // 4 - 1, h // 4 - 1


def dev_ssim(base, copies, off_base=0, off_copies=0, off_map=0, want_map=True, c=None):
    """base [h, w, 3] or [n, h, w, 3]; copies [n, h, w, 3] -> ([n][2] python ints, the map int32 [n, ny, nx] or None).  The
    statistics and the map start as garbage, and the GUARD bytes behind both must stay as they were."""
    n, h, w, _ = copies.shape
    nx, ny = windows(w, h)
    b, cp, s = Dev(base, off_base), Dev(copies, off_copies), Dev(n * 16 + GUARD)
    m = Dev(n * nx * ny * 4 + GUARD, off_map) if want_map else None
    check(lib().ssw_ssim_rgb8((c or ctx()).handle, b.ptr, 1 if base.ndim == 3 else n, cp.ptr, n, w, h, s.ptr, m.ptr if m else None), "ssw_ssim_rgb8")
    raw = s.host(np.uint8, (n * 16 + GUARD,))
    assert np.all(raw[n * 16:] == SENTINEL), "written beyond stats [n][2]"
    stats = raw[:n * 16].copy().view(np.uint64).reshape(n, 2)
    tmap = None
    if m:
        raw = m.host(np.uint8, (n * nx * ny * 4 + GUARD,))
        assert np.all(raw[n * nx * ny * 4:] == SENTINEL), "written beyond the map [n][ny][nx]"
        tmap = raw[:n * nx * ny * 4].copy().view(np.int32).reshape(n, ny, nx)
    for x in (b, cp, s, m):
        if x:
            x.free()
    return [[int(stats.view(np.int64)[i, 0]), int(stats[i, 1])] for i in range(n)], tmap


def check_against_ref(bases, copies, stats, tmap):
    for i in range(len(copies)):
        s, key, t = ssim_ref(bases[i] if bases.ndim == 4 else bases, copies[i])
        assert stats[i] == [s, key], (i, stats[i], [s, key])
        if tmap is not None:
            assert np.array_equal(tmap[i], t), i


# ---- shapes and contents -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SMALL + WIDTHS + HEIGHTS + STRIPS)
def test_every_content_equals_the_restatement(w, h):
    pairs = [pair(kind, w, h) for kind in CONTENTS]                 # one call: three originals, a copy of each
    bases, copies = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    stats, tmap = dev_ssim(bases, copies)
    check_against_ref(bases, copies, stats, tmap)


def test_the_cat_pair_and_its_known_answers():
    cat, marked = cat_pair()
    stats, tmap = dev_ssim(cat, marked[None])
    assert stats[0] == [18_638_317_194_866, 8_083_853_789_443_929_881]
    assert tmap.shape == (1, 110, 159) and tmap[0, 88, 113] == 808_427_057 == tmap.min()
    check_against_ref(cat, marked[None], stats, tmap)


@pytest.mark.parametrize("n", [1, 2, 17])
def test_one_original_and_one_per_copy(n):
    w, h = T_W + 8, T_H + 8                                         # four blocks: they start at copies 0 .. 3 (mod n)
    base, _ = pair("noise", w, h, 7)
    rng = np.random.default_rng(n)
    copies = np.clip(base[None].astype(np.int16) + rng.integers(-9, 10, (n, h, w, 3)), 0, 255).astype(np.uint8)
    copies[n // 2, 8:40, 16:80] = 255 - copies[n // 2, 8:40, 16:80]                         # every copy has its own answer
    stats, tmap = dev_ssim(base, copies)
    check_against_ref(base, copies, stats, tmap)
    assert len({tuple(s) for s in stats}) == n
    per_copy = np.stack([base] * n)
    per_copy[n - 1] = pair("noise", w, h, 8)[0]                     # and with its own original
    stats2, tmap2 = dev_ssim(per_copy, copies)
    check_against_ref(per_copy, copies, stats2, tmap2)


@pytest.mark.parametrize("w,h", [(19, 17), (56, 40)])
def test_at_every_byte_offset(w, h):
    bases = np.stack([pair(kind, w, h, 3)[0] for kind in CONTENTS[:2]])
    copies = np.stack([pair(kind, w, h, 3)[1] for kind in CONTENTS[:2]])
    want = [list(ssim_ref(b, c)[:2]) for b, c in zip(bases, copies)]
    maps = np.stack([ssim_ref(b, c)[2] for b, c in zip(bases, copies)])
    for off_base in range(4):
        for off_copies in range(4):
            stats, tmap = dev_ssim(bases, copies, off_base, off_copies, off_map=4 * ((off_base + off_copies) % 4))
            assert stats == want and np.array_equal(tmap, maps), (off_base, off_copies)
    for off_map in (0, 4, 8, 12):
        stats, tmap = dev_ssim(bases[0], copies[:1], 1, 2, off_map)
        assert stats == want[:1] and np.array_equal(tmap, maps[:1]), off_map


def test_without_a_map_the_statistics_are_the_same():
    w, h = T_W + 8, T_H + 4
    base, copy = pair("noise", w, h, 11)
    copies = np.stack([copy, pair("binary", w, h, 11)[1]])
    with_map, tmap = dev_ssim(base, copies)                         # dev_ssim checks the guard bytes behind stats and the map
    without, none = dev_ssim(base, copies, want_map=False)
    assert none is None and without == with_map
    check_against_ref(base, copies, with_map, tmap)


def test_a_small_call_after_a_large_one():
    big = [pair("noise", 2 * T_W + 4, 2 * T_H + 4, 5)]
    small = pair("binary", 13, 9, 5)
    with fresh_ctx():
        alone = dev_ssim(small[0], small[1][None])
    with fresh_ctx():
        dev_ssim(big[0][0], np.stack([big[0][1]] * 3))
        after = dev_ssim(small[0], small[1][None])
    assert after[0] == alone[0] and np.array_equal(after[1], alone[1])
    check_against_ref(small[0], small[1][None], *after)


def test_of_two_equally_damaged_windows_the_first_wins():
    w, h = 2 * T_W + 16, 2 * T_H + 16
    rng = np.random.default_rng(13)
    base = np.tile(rng.integers(64, 192, (8, 8, 3), dtype=np.uint8), (h // 8, w // 8, 1))   # every window at an even index is the same
    copy = base.copy()
    hits = [(70, 17), (2, 1)]                                       # (wx, wy): in the last block and in the first, same phase
    for wx, wy in hits:
        copy[4 * wy:4 * wy + 8, 4 * wx:4 * wx + 8] = 255 - copy[4 * wy:4 * wy + 8, 4 * wx:4 * wx + 8]
    s, key, t = ssim_ref(base, copy)
    nx = windows(w, h)[0]
    worst = np.flatnonzero(t.reshape(-1) == t.min())
    assert [int(i) for i in worst] == [1 * nx + 2, 17 * nx + 70]    # the restatement agrees that there are two
    stats, tmap = dev_ssim(base, copy[None])
    assert stats[0] == [s, key] and stats[0][1] & 0xFFFFFFFF == 1 * nx + 2
    assert np.array_equal(tmap[0], t)


# ---- status codes -------------------------------------------------------------------------------------------------------------
def test_status_codes():
    f, h = lib().ssw_ssim_rgb8, ctx().handle
    base, copy = pair("noise", 12, 8)
    copies = np.stack([copy] * 3)
    b, c, s, m = Dev(base), Dev(copies), Dev(3 * 16), Dev(3 * 2 * 4)
    untouched = lambda: np.all(s.host(np.uint8, (3 * 16,)) == SENTINEL) and np.all(m.host(np.uint8, (3 * 2 * 4,)) == SENTINEL)
    assert f(None, b.ptr, 1, c.ptr, 3, 12, 8, s.ptr, m.ptr) == L.SSW_ERR_BAD_ARG
    assert f(h, None, 1, c.ptr, 3, 12, 8, s.ptr, m.ptr) == L.SSW_ERR_BAD_ARG
    assert f(h, b.ptr, 1, None, 3, 12, 8, s.ptr, m.ptr) == L.SSW_ERR_BAD_ARG
    assert f(h, b.ptr, 1, c.ptr, 3, 12, 8, None, m.ptr) == L.SSW_ERR_BAD_ARG
    for n_base in (0, 2, 4):
        assert f(h, b.ptr, n_base, c.ptr, 3, 12, 8, s.ptr, m.ptr) == L.SSW_ERR_BAD_ARG, n_base
    for w, hh in ((7, 8), (12, 7), (1, 1), (7, 2 ** 20), (2 ** 31, 4)):
        assert f(h, b.ptr, 1, c.ptr, 3, w, hh, s.ptr, m.ptr) == L.SSW_ERR_BAD_ARG, (w, hh)
    assert f(h, b.ptr, 1, c.ptr, 3, 0, 8, s.ptr, m.ptr) == L.SSW_ERR_BAD_DIMS
    assert f(h, b.ptr, 1, c.ptr, 3, 12, 0, s.ptr, m.ptr) == L.SSW_ERR_BAD_DIMS
    assert f(h, b.ptr, 1, c.ptr, 3, 2 ** 31 + 1, 8, s.ptr, m.ptr) == L.SSW_ERR_BAD_DIMS
    assert f(h, b.ptr, 1, c.ptr, 3, 8, 2 ** 31 + 1, s.ptr, m.ptr) == L.SSW_ERR_BAD_DIMS
    side = 4 * (2 ** 16 + 1)                                         # 2^16 x 2^16 windows: an index no longer fits 32 bits
    assert f(h, b.ptr, 1, c.ptr, 3, side, side, s.ptr, m.ptr) == L.SSW_ERR_BAD_DIMS
    assert f(h, b.ptr, 1, c.ptr, 0, 12, 8, s.ptr, m.ptr) == L.SSW_OK
    assert f(h, None, 7, None, 0, 0, 0, None, None) == L.SSW_OK      # n == 0 comes first
    ctx().synchronize()
    assert untouched()
    assert f(h, b.ptr, 1, c.ptr, 3, 12, 8, s.ptr, m.ptr) == L.SSW_OK
    want = ssim_ref(base, copy)
    assert [int(v) for v in s.host(np.uint64, (3, 2))[2]] == [want[0], want[1]]
    assert np.array_equal(m.host(np.int32, (3, 1, 2))[1], want[2])
    for x in (b, c, s, m):
        x.free()
    assert (L.SSIM_MIN_SIDE, L.SSIM_ONE, L.SSIM_STATS) == (8, ONE, 2)


# ---- timing -------------------------------------------------------------------------------------------------------------------
def test_the_call_is_timed_as_convert_with_its_algorithmic_bytes():
    w, h, n = 70, 40, 4
    fb, (nx, ny) = w * h * 3, windows(w, h)
    base, copy = pair("noise", w, h, 17)
    copies = np.stack([copy] * n)
    c = ctx()
    c.enable_timing(True)
    try:
        c.reset_timing()
        dev_ssim(base, copies, want_map=False)
        t = c.timing()
        assert t["convert"]["launches"] >= 1 and t["convert"]["work"] == (1 + n) * fb + 16 * n
        assert all(v["launches"] == 0 for k, v in t.items() if k != "convert") and len(t) == 15
        c.reset_timing()
        dev_ssim(np.stack([base] * n), copies)
        assert c.timing()["convert"]["work"] == (n + n) * fb + 16 * n + 4 * nx * ny * n
    finally:
        c.enable_timing(False)


# ---- the host wrappers --------------------------------------------------------------------------------------------------------
def test_ssim_in_one_group_and_in_many(monkeypatch):
    w, h, n = 56, 40, 5
    base, _ = pair("noise", w, h, 19)
    rng = np.random.default_rng(19)
    copies = list(np.clip(base[None].astype(np.int16) + rng.integers(-20, 21, (n, h, w, 3)), 0, 255).astype(np.uint8))
    bases = [pair("noise", w, h, 20 + i)[0] for i in range(n)]
    one = api.ssim(base, copies, ctx(), maps=True)
    one_each = api.ssim(bases, copies, ctx())
    monkeypatch.setattr(api, "UPLOAD_GROUP_BYTES", 2 * w * h * 3)   # two copies a group; one when every copy has its original
    many = api.ssim(base, copies, ctx(), maps=True)
    many_each = api.ssim(np.stack(bases), copies, ctx())
    for i in range(n):
        s, key, t = ssim_ref(base, copies[i])
        for got in (one[i], many[i]):
            assert (got.sum, got.worst, got.worst_index, got.windows_x, got.windows_y) == (s, int(t.min()), int(np.argmin(t)), 13, 9)
            assert np.array_equal(got.map, t) and got.mean == s / (ONE * 117)
            assert got.worst_position == (4 * (got.worst_index % 13), 4 * (got.worst_index // 13))
        s, key, t = ssim_ref(bases[i], copies[i])
        assert one_each[i] == many_each[i] == api.Ssim(s, (key >> 32) - ONE, key & 0xFFFFFFFF, 13, 9)


@pytest.fixture(scope="module")
def reports():
    cat = cat_pair()[0]
    return cat, api.strength_report(cat, [0.02, 0.1], jpeg=(75,), ssim=True, seed=3, ctx=ctx()), \
        api.strength_report(cat, [0.02, 0.1], jpeg=(75,), seed=3, ctx=ctx())


def test_strength_report_with_ssim_equals_the_host_wrappers(reports):
    cat, rows, _ = reports
    marks = np.random.default_rng(3).standard_normal((8, 1000)).astype(np.float32)
    for r in rows:
        copies = api.Writer(cat, api.WriteConfig(insertion=api.Insertion.Option2(r.alpha)), ctx()).mark_copies_rgb8(list(marks))
        assert r.ssim == api.ssim(cat, copies, ctx()) and len(r.ssim) == 8
        coded = [c[0] for c in api.jpeg(copies, [75], ctx())]
        mean = [s.mean for s in api.ssim(cat, coded, ctx())]
        assert (r.jpeg[0].ssim_min, r.jpeg[0].ssim_max) == (min(mean), max(mean))
        print(f"alpha {r.alpha}: SSIM {min(s.mean for s in r.ssim):.4f} .. {max(s.mean for s in r.ssim):.4f}, "
              f"worst window {min(s.worst_value for s in r.ssim):.4f}; after JPEG 75: {min(mean):.4f} .. {max(mean):.4f}")
    assert min(s.mean for s in rows[0].ssim) > max(s.mean for s in rows[1].ssim)           # a weaker mark is less visible
    assert all(-1.0 < s.worst_value <= s.mean < 1.0 for r in rows for s in r.ssim)


def test_strength_report_without_ssim_is_what_it_was(reports):
    _, with_ssim, without = reports
    for a, b in zip(with_ssim, without):
        assert b.ssim == [] and len(a.ssim) == 8
        assert (a.alpha, a.quality) == (b.alpha, b.quality)
        for x, y in zip(a.collusions + a.jpeg, b.collusions + b.jpeg):
            assert type(x) is type(y)
            for name in ("method", "size", "weakest_colluder", "strongest_innocent", "found", "accused", "quality", "survived", "weakest_own",
                         "psnr_min", "psnr_max"):
                assert same(getattr(x, name, None), getattr(y, name, None)), name
        assert all(j.ssim_min != j.ssim_min and j.ssim_max != j.ssim_max for j in b.jpeg) and len(b.jpeg) == 1


def test_cli_strength_prints_the_ssim_line_only_when_asked(tmp_path, capsys, monkeypatch):
    from PIL import Image
    path = str(tmp_path / "cat.png")
    Image.fromarray(cat_pair()[0]).save(path)
    monkeypatch.setattr(cli, "strength_report", lambda *a, **k: api.strength_report(*a, seed=3, **k))     # the same marks in every run
    args = ["strength", path, "--alpha", "0.1", "--copies", "4", "--collude", "2", "--method", "average", "--jpeg", "75"]
    assert cli.main(args) == 0
    plain = capsys.readouterr().out.splitlines()
    assert plain[0] == "-" and plain[1] == "  Alpha: 0.1" and len(plain) == 5 and not any("ssim" in x.lower() for x in plain)
    assert re.fullmatch(r"  PSNR: 3\d\.\d\d \.\. 3\d\.\d\d dB over 4 copies \(largest byte difference \d+\)", plain[2])
    assert plain[3].startswith("  average of 2: found 2/2, weakest colluder ")
    assert re.fullmatch(r"  jpeg 75: own mark found 4/4, weakest \d+\.\d, strongest innocent -?\d+\.\d, \d\d\.\d \.\. \d\d\.\d dB", plain[4])
    assert cli.main(args + ["--ssim"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert re.fullmatch(r"  SSIM: 0\.\d{4} \.\. 0\.\d{4} over 4 copies, worst window -?0\.\d{4} at \d+,\d+ \(copy [0-3]\)", lines[3]), lines[3]
    m = re.fullmatch(r"(.* dB), ssim 0\.\d\d \.\. 0\.\d\d", lines[5])
    assert m and lines[:3] + [lines[4], m.group(1)] == plain
    assert cli.main(args + ["--json"]) == 0
    doc = json.loads(capsys.readouterr().out)
    assert "ssim" not in json.dumps(doc)
    assert cli.main(args + ["--json", "--ssim"]) == 0
    with_ssim = json.loads(capsys.readouterr().out)
    for c, old in zip(with_ssim[0]["copies"], doc[0]["copies"]):
        assert -1.0 < c["ssim_worst"] <= c["ssim"] < 1.0 and len(c["ssim_worst_at"]) == 2
        assert {k: v for k, v in c.items() if not k.startswith("ssim")} == old
    assert with_ssim[0]["jpeg"] == doc[0]["jpeg"] and with_ssim[0]["collusions"] == doc[0]["collusions"]
