"""The scale attack's reference and its surfaces, without a GPU.  `resample_ref` is the numpy restatement of Pillow's 8-bit
resample (Image.resize with BOX, BILINEAR, BICUBIC or LANCZOS; Resample.c) -- the definition include/ssw.h states, which the
device results must EQUAL (tests/test_resample_gpu.py imports it).  It is checked here byte for byte against Pillow itself;
then the host's tap tables against its own, the surfaces (header, ctypes table, Python, CLI) and the report's call record."""
import argparse
import ctypes as C
import functools
import io
import json
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd import api, cli
import spread_spectrum_watermarking_amd as wm
import fake_ssw
from test_jpeg_cpu import cat_image

# ---- the restatement ---------------------------------------------------------------------------------------------------------
BOX, BILINEAR, BICUBIC, LANCZOS = range(4)
FILTERS = {"box": BOX, "bilinear": BILINEAR, "bicubic": BICUBIC, "lanczos": LANCZOS}
SUPPORT = {BOX: 0.5, BILINEAR: 1.0, BICUBIC: 2.0, LANCZOS: 3.0}
BITS = 22


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x                                   # libm's sin, as Pillow's C calls it


def weight(filt, x):
    if filt == BOX:
        return 1.0 if -0.5 < x <= 0.5 else 0.0
    if filt == BILINEAR:
        x = abs(x)
        return 1.0 - x if x < 1.0 else 0.0
    if filt == BICUBIC:
        a, x = -0.5, abs(x)
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        return (((x - 5) * x + 8) * x - 4) * a if x < 2.0 else 0.0
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


@functools.lru_cache(maxsize=4096)
def tables(n_in, n_out, filt):
    """One axis: a tuple of (left, integer taps) per output sample; Python floats are C doubles, every operation rounded once."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support, ss = SUPPORT[filt] * fs, 1.0 / fs
    out = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = max(min(int(center + support + 0.5), n_in) - xmin, 0)
        k = [weight(filt, (x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in k:
            ww += v
        if ww != 0.0:
            k = [v / ww for v in k]
        out.append((xmin, tuple(int(v * (1 << BITS) - 0.5) if v < 0 else int(v * (1 << BITS) + 0.5) for v in k)))
    return tuple(out)


def resample_pass(a, n_out, filt):
    """a [lines, n_in, 3] u8 -> [lines, n_out, 3] u8 along axis 1; the sums are exact integers and must fit an int32."""
    res = np.empty((a.shape[0], n_out, a.shape[2]), np.uint8)
    wide = a.astype(np.int64)
    for xx, (left, taps) in enumerate(tables(a.shape[1], n_out, filt)):
        s = np.tensordot(wide[:, left:left + len(taps)], np.asarray(taps, np.int64), axes=(1, 0)) + (1 << (BITS - 1))
        assert s.size == 0 or (-(1 << 31) <= s.min() and s.max() < (1 << 31))
        res[:, xx] = np.clip(s >> BITS, 0, 255)
    return res


def resample_ref(frame, nw, nh, filt):
    """frame [h, w, 3] u8 -> [nh, nw, 3] u8: the rows first, into bytes, then the columns; a pass that changes nothing is skipped."""
    a = np.ascontiguousarray(frame)
    h, w = a.shape[:2]
    if nw != w:
        a = resample_pass(a, nw, filt)
    if nh != h:
        a = resample_pass(a.transpose(1, 0, 2), nh, filt).transpose(1, 0, 2)
    return np.ascontiguousarray(a)


def scale_size(w, h, factor):
    return max(1, int(w * factor + 0.5)), max(1, int(h * factor + 0.5))


# ---- the grid both test files use --------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 7), (2, 3), (5, 4), (9, 31), (33, 17), (3, 300), (300, 3), (67, 131), (120, 200)]     # (h, w)
CONTENTS = ("noise", "checker1", "checker3", "white", "black", "ramp")
NAMES = {BOX: "box", BILINEAR: "bilinear", BICUBIC: "bicubic", LANCZOS: "lanczos"}


def targets(h, w):
    """(nw, nh, filters): half; a third of the width only; a quarter of the height only (one pass is skipped); double; 1 x 1;
    one column more and one row less; an eighth by LANCZOS"""
    every = (BOX, BILINEAR, BICUBIC, LANCZOS)
    return [(max(1, w // 2), max(1, h // 2), every), (max(1, w // 3), h, every), (w, max(1, h // 4), every), (2 * w, 2 * h, every),
            (1, 1, every), (w + 1, max(h - 1, 1), every), (max(1, w // 8), max(1, h // 8), (LANCZOS,))]


def content(kind, h, w, seed=0):
    """random bytes; a 0 / 255 checkerboard of period 1 and of period 3 (both clamps: the negative lobes overshoot); constant
    255 and 0; a ramp"""
    y, x = np.mgrid[0:h, 0:w]
    if kind == "noise":
        return np.random.default_rng([seed, h, w]).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind in ("checker1", "checker3"):
        p = 1 if kind == "checker1" else 3
        return np.repeat((((x // p + y // p) % 2) * 255).astype(np.uint8)[..., None], 3, 2)
    if kind in ("white", "black"):
        return np.full((h, w, 3), 255 if kind == "white" else 0, np.uint8)
    return np.stack([(x * 255 // max(w - 1, 1)), (y * 255 // max(h - 1, 1)), ((x + y) * 7 % 256)], -1).astype(np.uint8)


def pil_resize(img, nw, nh, filt):
    from PIL import Image
    f = {BOX: Image.BOX, BILINEAR: Image.BILINEAR, BICUBIC: Image.BICUBIC, LANCZOS: Image.LANCZOS}[filt]
    return np.asarray(Image.fromarray(img).resize((nw, nh), f))


# ---- the restatement against Pillow ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("h,w", SHAPES)
def test_restatement_equals_pillow(h, w, kind):
    img = content(kind, h, w)
    for nw, nh, filters in targets(h, w):
        for f in filters:
            assert np.array_equal(resample_ref(img, nw, nh, f), pil_resize(img, nw, nh, f)), (nw, nh, NAMES[f])


@pytest.mark.parametrize("factor", (0.5, 0.25, 0.125, 0.33))
def test_restatement_equals_pillow_on_the_cat_and_back(factor):
    cat = cat_image()
    assert cat.shape == (444, 640, 3)
    nw, nh = scale_size(640, 444, factor)
    for f in (BOX, BILINEAR, BICUBIC, LANCZOS):
        small = resample_ref(cat, nw, nh, f)
        assert np.array_equal(small, pil_resize(cat, nw, nh, f)), NAMES[f]
        assert np.array_equal(resample_ref(small, 640, 444, f), pil_resize(small, 640, 444, f)), NAMES[f]


def test_properties_of_the_tables():
    for f in (BOX, BILINEAR, BICUBIC, LANCZOS):
        for n_in, n_out in ((640, 320), (444, 222), (300, 3), (7, 14), (1, 5), (5, 1)):
            for left, taps in tables(n_in, n_out, f):
                assert 0 <= left and left + len(taps) <= n_in and len(taps) >= 1
                assert abs(sum(taps) - (1 << BITS)) <= len(taps)                  # normalised, each tap rounded once
                assert all(-(1 << 23) < t < (1 << 23) for t in taps)              # the device's 24-bit multiply applies
    assert tables(4, 2, BOX) == ((0, (1 << 21, 1 << 21)), (2, (1 << 21, 1 << 21)))
    assert tables(2, 2, BICUBIC)[0] == (0, (1 << 22, 0)) or tables(2, 2, BICUBIC)[0][1][0] == 1 << 22
    flat = np.full((3, 9, 3), 200, np.uint8)
    assert np.all(resample_ref(flat, 4, 2, LANCZOS) == 200)


def test_the_host_tables_follow_the_rule(tmp_path):
    """csrc/resample_tables.hpp, the header the library's host code includes: left, count and every integer tap of every
    in, out in 1 .. 48, the 4K pairs and 640 -> 1280 with the four filters, against `tables` -- a sin that differs from
    Python's would show here."""
    exe = str(tmp_path / "resample_tables_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "spread_spectrum_watermarking_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "resample_tables_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    big = [(3840, o) for o in (1920, 1280, 960, 480, 7)] + [(2160, o) for o in (1080, 720, 270, 1)] + [(640, 1280)]
    want = [(i, o, f) for f in range(4) for i, o in [(i, o) for i in range(1, 49) for o in range(1, 49)] + big]
    lines = r.stdout.splitlines()
    assert len(lines) == len(want) == 4 * (48 * 48 + 10)
    for (n_in, n_out, f), line in zip(want, lines):
        parts = line.split(" | ")
        assert [int(v) for v in parts[0].split()][:3] == [n_in, n_out, f] and len(parts) == n_out + 1
        got = []
        for p in parts[1:]:
            v = [int(x) for x in p.split()]
            assert v[1] == len(v) - 2
            got.append((v[0], tuple(v[2:])))
        ref = tables(n_in, n_out, f)
        assert tuple(got) == ref, (n_in, n_out, NAMES[f])
        assert int(parts[0].split()[3]) == max(1, max(len(t) for _, t in ref))


# ---- surfaces ----------------------------------------------------------------------------------------------------------------
def test_symbols_declared_exported_bound_and_described():
    text = open(os.path.join(ROOT, "include", "ssw.h")).read()
    lib = C.CDLL(L.LIB_PATH)
    for name, n_args in (("ssw_resample_rgb8", 9), ("ssw_scale_attack_rgb8", 8)):
        assert hasattr(lib, name) and len(L.SIGNATURES[name][1]) == n_args
    assert C.sizeof(L.ScaleJob) == 16 and [f[0] for f in L.ScaleJob._fields_] == ["frame", "nw", "nh", "filter"]
    assert L.RESAMPLE_FILTERS == {"box": 0, "bilinear": 1, "bicubic": 2, "lanczos": 3} == FILTERS
    assert text.index("ssw_filter_rgb8(") < text.index("ssw_resample_rgb8(") < text.index("ssw_scale_attack_rgb8(") < text.index("---- 16-bit frames")
    comment = " ".join(text[text.index("int ssw_filter_rgb8("):text.index("int ssw_scale_attack_rgb8(")].split())
    for phrase in ("typedef struct ssw_scale_job { uint32_t frame; uint32_t nw; uint32_t nh; uint32_t filter; } ssw_scale_job;",
                   "SSW_RESAMPLE_BOX = 0, SSW_RESAMPLE_BILINEAR = 1, SSW_RESAMPLE_BICUBIC = 2, SSW_RESAMPLE_LANCZOS = 3",
                   "tests/test_resample_cpu.py", "PIL.Image.resize", "center = (xx + 0.5) * scale", "(int) (center - support + 0.5)",
                   "k[x] * 2^22 - 0.5", "(2^21 + sum_x in[xmin + x] * tap[x]) >> 22", "rows first", "is skipped", "libm's sin",
                   "ssw_restore_rgb8", "No alignment is assumed", "SSW_STAGE_CONVERT", "SSW_STAGE_RESIZE", "3 w h + 2 * 3 nw h + 3 nw nh",
                   "SSW_ERR_BAD_DIMS", "65535", "must not overlap", "HAMMING"):
        assert phrase in comment, phrase
    assert "resample.hip" in open(os.path.join(ROOT, "spread_spectrum_watermarking_amd", "csrc", "Makefile")).read()
    assert "SSW_STAGE_COUNT = 15" in text and len(L.STAGES) == 15
    tables_hpp = open(os.path.join(ROOT, "spread_spectrum_watermarking_amd", "csrc", "resample_tables.hpp")).read()
    assert "fp contract(off)" in tables_hpp


def test_the_docs_describe_the_scale_attack():
    for path in ("README.md", "DESIGN.md"):
        text = " ".join(open(os.path.join(ROOT, path)).read().split())
        assert "ssw_scale_attack_rgb8" in text and "ssw_resample_rgb8" in text, path
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 4.16" in design and design.count("§4.16") >= 2


def test_scale_validation_labels_and_sizes():
    for name in ("resample", "scale_attack", "Scale", "ScaleResult", "strength_report"):
        assert hasattr(wm, name), name
    S = api.Scale
    assert (S(0.5).label, S(0.25, "lanczos").label, S.to(640, 360, "LANCZOS").label, S(2).label, S(0.125, "box").label) == (
        "scale 0.5 bicubic", "scale 0.25 lanczos", "scale 640x360 lanczos", "scale 2 bicubic", "scale 0.125 box")
    assert S(0.5).size(640, 444) == (320, 222) and S(0.33).size(640, 444) == (211, 147) and S(0.125).size(640, 444) == (80, 56)
    assert S(0.5).size(5, 1) == (3, 1) and S(0.01).size(7, 3) == (1, 1) and S.to(640, 360).size(9, 9) == (640, 360) and S(4).size(3, 2) == (12, 8)
    for w, h, f in ((640, 444, 0.33), (31, 9, 0.5), (1, 1, 0.125)):
        assert S(f).size(w, h) == scale_size(w, h, f)
    j = S(0.25, "lanczos").job(5, 640, 444)
    assert (j.frame, j.nw, j.nh, j.filter) == (5, 160, 111, L.RESAMPLE_LANCZOS)
    j = S.to(7, 9, "box").job(1, 640, 444)
    assert (j.frame, j.nw, j.nh, j.filter) == (1, 7, 9, L.RESAMPLE_BOX)
    assert S(0.5) == S(0.5, "BICUBIC") and hash(S(0.5)) == hash(S(0.5, "bicubic"))
    with pytest.raises(Exception):
        S(0.5).factor = 1.0                                                   # frozen
    for bad in (0, -1, 4.5, float("nan"), float("inf"), "2", True, None):
        with pytest.raises(ValueError):
            S(bad)
    for bad in ("hamming", "nearest", 2, None):
        with pytest.raises(ValueError):
            S(0.5, bad)
    for nw, nh in ((0, 5), (5, 0), (65536, 5), (5.0, 5), (True, 5)):
        with pytest.raises(ValueError):
            S.to(nw, nh)
    img = np.zeros((1, 1, 3), np.uint8)
    assert api.scale_attack([], [S(0.5)]) == [] and api.scale_attack([img], []) == [[]] and api.resample([], (3, 3)) == []
    for bad in (np.zeros((8, 8), np.uint8), np.zeros((8, 8, 4), np.uint8), np.zeros((8, 8, 3), np.float32)):
        with pytest.raises(ValueError):                                      # grey, RGBA, f32: no GPU needed
            api.scale_attack([bad], [S(0.5)])
        with pytest.raises(ValueError):
            api.resample([bad], (4, 4))
    for bad in (0.5, "0.5", ("scale", 0.5), None):
        with pytest.raises(ValueError):
            api.scale_attack([img], [S(0.5), bad])
        with pytest.raises(ValueError):
            api.strength_report(np.zeros((16, 16, 3), np.uint8), [0.1], scales=[bad])
    for size, filt in (((0, 4), "bicubic"), ((4, 65536), "bicubic"), ((4, 4), "hamming"), ((4.0, 4), "box")):
        with pytest.raises(ValueError):
            api.resample([img], size, filt)
    row = api.StrengthRow(0.1, [], [])
    assert row.scales == [] and api.StrengthRow(0.1, [], []).scales is not row.scales
    r = api.ScaleResult("scale 0.5 bicubic", (320, 222), 8, 30.2, 1.4, 0, 33.0, 35.1)
    assert (r.scale, r.size, r.survived, r.weakest_own, r.accused, r.psnr_max) == ("scale 0.5 bicubic", (320, 222), 8, 30.2, 0, 35.1)
    assert r.ssim_min != r.ssim_min
    assert [f.name for f in api.ScaleResult.__dataclass_fields__.values()][2:] == [f.name for f in api.FilterResult.__dataclass_fields__.values()][1:]


def test_cli_scale_parser():
    p = cli.build_parser()
    a = p.parse_args(["strength", "photo.jpg", "--alpha", "0.02", "0.1"])
    assert a.scales == []
    a = p.parse_args(["strength", "photo.jpg", "--alpha", "0.1", "--scale", "0.5", "0.25:lanczos", "640x360:bilinear", "2:box", "--json"])
    assert [s.label for s in a.scales] == ["scale 0.5 bicubic", "scale 0.25 lanczos", "scale 640x360 bilinear", "scale 2 box"] and a.json
    for bad in ("0", "5", "x", "0.5:hamming", "640x", "x360", "0x5", "640x360x2", "nan", "-1", "0.5:"):
        with pytest.raises(SystemExit):
            p.parse_args(["strength", "photo.jpg", "--alpha", "0.1", "--scale", bad])


def _cli(rows, as_json, scales):
    args = argparse.Namespace(file="cat.png", alpha=[0.02], length=50, copies=3, collude=[2], method=["average"], similarity_exceed=6.0,
                              jpeg=[], ssim=True, filters=[], scales=scales, json=as_json)
    before = cli.strength_report, cli._open_image
    cli.strength_report, cli._open_image = (lambda *a, **k: rows), (lambda path: None)
    try:
        out = io.StringIO()
        assert cli.cmd_strength(args, out) == 0
        return out.getvalue()
    finally:
        cli.strength_report, cli._open_image = before


def test_cli_rows_and_json_of_the_scales():
    rows = fake_ssw.cli_rows()[:2]
    nan = float("nan")
    rows[0].scales = [api.ScaleResult("scale 0.5 bicubic", (320, 222), 3, 18.26, 2.04, 0, 33.04, 35.96, 0.9512, 0.9749),
                      api.ScaleResult("scale 640x360 lanczos", (640, 360), 1, 3.949, 6.51, 2, 24.0, float("inf"), 0.5, 1.0)]
    rows[1].scales = [api.ScaleResult("scale 0.125 box", (80, 56), 0, 1.5, nan, 0, 27.0, 28.0)]
    scales = [api.Scale(0.5), api.Scale.to(640, 360, "lanczos")]
    text = _cli(rows, False, scales).splitlines()
    assert "  scale 0.5 bicubic (320x222): own mark found 3/3, weakest 18.3, strongest innocent 2.0, 33.0 .. 36.0 dB, ssim 0.95 .. 0.97" in text
    assert ("  scale 640x360 lanczos (640x360): own mark found 1/3, weakest 3.9, strongest innocent 6.5, 2 innocent accused, "
            "24.0 .. inf dB, ssim 0.50 .. 1.00") in text
    assert "  scale 0.125 box (80x56): own mark found 0/1, weakest 1.5, strongest innocent none, 27.0 .. 28.0 dB" in text
    first = [i for i, l in enumerate(text) if l.startswith("  scale ")][0]
    assert text[first - 1].startswith("  unsharp 2,150,3:")                    # after the filter rows
    doc = json.loads(_cli(rows, True, scales))
    assert doc[0]["scales"] == [
        {"scale": "scale 0.5 bicubic", "size": [320, 222], "survived": 3, "accused": 0, "weakest_own": 18.26, "strongest_innocent": 2.04,
         "psnr_min": 33.04, "psnr_max": 35.96},
        {"scale": "scale 640x360 lanczos", "size": [640, 360], "survived": 1, "accused": 2, "weakest_own": 3.949, "strongest_innocent": 6.51,
         "psnr_min": 24.0, "psnr_max": "inf"}]
    assert doc[1]["scales"][0]["strongest_innocent"] is None
    # without --scale the document is the one it was: no key
    assert all("scales" not in d for d in json.loads(_cli(fake_ssw.cli_rows(), True, [])))


# ---- the call record ---------------------------------------------------------------------------------------------------------
def test_report_with_scales_calls_attack_trace_quality_ssim():
    ctx = fake_ssw.fake_context()
    scales = [api.Scale(0.5), api.Scale.to(5, 7, "lanczos")]
    img = fake_ssw.frames(1)[0]
    plain = fake_ssw.fake_context()
    api.strength_report(img, [0.02, 0.1], ctx=plain, k=50, copies=3, sizes=(2,), methods=("average",), seed=1, ssim=True)
    rows = api.strength_report(img, [0.02, 0.1], ctx=ctx, k=50, copies=3, sizes=(2,), methods=("average",), seed=1, ssim=True, scales=scales)
    assert [[s.scale for s in r.scales] for r in rows] == [["scale 0.5 bicubic", "scale 5x7 lanczos"]] * 2
    assert [s.size for s in rows[0].scales] == [(12, 8), (5, 7)]
    W, H, FB = fake_ssw.W, fake_ssw.H, fake_ssw.FB
    calls = [c for c in ctx._lib.calls if c[0] not in ("ssw_copy_to_dev", "ssw_copy_to_host")]
    base = [c for c in plain._lib.calls if c[0] not in ("ssw_copy_to_dev", "ssw_copy_to_host")]
    per = len(base) // 2
    assert len(calls) == len(base) + 2 * 4
    for a in range(2):
        mine = calls[a * (per + 4):(a + 1) * (per + 4)]
        assert [c[0] for c in mine[:per]] == [c[0] for c in base[a * per:(a + 1) * per]]
        attack, trace, quality, ssim = mine[per:]
        assert (attack[0], trace[0], quality[0], ssim[0]) == ("ssw_scale_attack_rgb8", "ssw_fingerprint_trace_rgb8", "ssw_quality_rgb8", "ssw_ssim_rgb8")
        jobs = np.frombuffer(bytes.fromhex(attack[1][5]), np.uint32).reshape(-1, 4).tolist()
        assert jobs == [[c, 12, 8, L.RESAMPLE_BICUBIC] for c in range(3)] + [[c, 5, 7, L.RESAMPLE_LANCZOS] for c in range(3)]    # parameter-major
        assert attack[1][:5] == ["ctx", ["dev", 3 * FB, 0], 3, W, H] and attack[1][6:] == [6, ["dev", 6 * FB, 0]]
        assert trace[1][3] == ["dev", 6 * FB, 0] and trace[1][4:8] == [6, W, H, 50]
        assert quality[1][3:7] == [["dev", 6 * FB, 0], 6, W, H]
        assert ssim[1][3:7] == [["dev", 6 * FB, 0], 6, W, H] and ssim[1][7] == ["dev", 6 * 8 * L.SSIM_STATS, 0]
    assert not ctx._lib.live
    # the wrapper: one call per group, jobs in frame order
    ctx = fake_ssw.fake_context()
    out = api.scale_attack(fake_ssw.frames(2), scales, ctx)
    assert len(out) == 2 and len(out[0]) == 2 and out[0][0].shape == (H, W, 3)
    (call,) = [c for c in ctx._lib.calls if c[0] == "ssw_scale_attack_rgb8"]
    assert np.frombuffer(bytes.fromhex(call[1][5]), np.uint32).reshape(-1, 4).tolist() == [
        [0, 12, 8, 2], [0, 5, 7, 3], [1, 12, 8, 2], [1, 5, 7, 3]]
    ctx = fake_ssw.fake_context()
    out = api.resample(fake_ssw.frames(3), (5, 7), "box", ctx)
    assert len(out) == 3 and out[0].shape == (7, 5, 3)
    (call,) = [c for c in ctx._lib.calls if c[0] == "ssw_resample_rgb8"]
    assert call[1] == ["ctx", ["dev", 3 * FB, 0], 3, W, H, 5, 7, 0, ["dev", 3 * 5 * 7 * 3, 0]] and not ctx._lib.live
