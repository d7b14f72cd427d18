"""ssw_quality_rgb8 / ssw_collude_rgb8 (include/ssw.h) without a GPU: the numpy restatement of the two definitions -- what the
device results must EQUAL (tests/test_collude_gpu.py imports it) -- its own properties, the surfaces (header, ctypes table,
Python, CLI, C++), and the premise of the strength report restated through the oracle: an averaged forgery of marked copies
still carries every colluder's mark."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd import api, cli
import spread_spectrum_watermarking_amd as wm

NAMES = ("ssw_quality_rgb8", "ssw_collude_rgb8")
METHODS = ("average", "median", "min", "max", "minmax", "mosaic")
LIBDIR = os.path.join(ROOT, "spread_spectrum_watermarking_amd", "lib")


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def collude_ref(copies, method, members):
    """copies [n, h, w, 3] u8, method a name of METHODS or its number, members indices into copies -> the forgery [h, w, 3] u8."""
    method = METHODS[method] if isinstance(method, (int, np.integer)) else method
    v = np.asarray(copies)[list(members)].astype(np.int64)           # [c, h, w, 3] in member order
    c, s = v.shape[0], np.sort(v, axis=0)
    if method == "average":
        r = (v.sum(axis=0) + c // 2) // c
    elif method == "median":
        r = (s[(c - 1) // 2] + s[c // 2] + 1) >> 1
    elif method == "min":
        r = s[0]
    elif method == "max":
        r = s[c - 1]
    elif method == "minmax":
        r = (s[0] + s[c - 1] + 1) >> 1
    elif method == "mosaic":
        y, x = np.mgrid[0:v.shape[1], 0:v.shape[2]]
        r = np.take_along_axis(v, (((x >> 5) + (y >> 5)) % c)[None, :, :, None], axis=0)[0]
    else:
        raise ValueError(method)
    return r.astype(np.uint8)


def luma_ref(img):
    p = np.asarray(img).astype(np.int64)
    return (77 * p[..., 0] + 150 * p[..., 1] + 29 * p[..., 2] + 128) >> 8


def quality_ref(base, copy):
    """-> the six values of one copy: SSE of R, G, B, SSE of the luma, changed bytes, max |d| (python ints)."""
    d = np.asarray(copy).astype(np.int64) - np.asarray(base).astype(np.int64)
    dl = luma_ref(copy) - luma_ref(base)
    return [int((d[..., ch] ** 2).sum()) for ch in range(3)] + [int((dl ** 2).sum()), int((d != 0).sum()), int(np.abs(d).max(initial=0))]


# ---- properties of the restatement -------------------------------------------------------------------------------------------
def pool(n, h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def test_a_single_member_is_copied_by_every_method():
    p = pool(3, 40, 70)
    for m in METHODS:
        assert np.array_equal(collude_ref(p, m, [2]), p[2]), m
        assert np.array_equal(collude_ref(p, METHODS.index(m), [2]), p[2]), m


def test_identical_members_give_that_frame():
    p = pool(2, 33, 35, 1)
    for m in METHODS:
        for c in (2, 5, 16):
            assert np.array_equal(collude_ref(p, m, [1] * c), p[1]), (m, c)


def test_median_of_an_odd_count_is_an_element_and_average_cannot_overflow():
    p = pool(5, 9, 11, 2)
    med = collude_ref(p, "median", range(5))
    assert np.all((med[None] == p).any(axis=0))
    assert np.array_equal(med, np.median(p, axis=0).astype(np.uint8))
    white = np.full((1, 4, 4, 3), 255, np.uint8)
    assert np.all(collude_ref(white, "average", [0] * 16) == 255)
    two = np.stack([np.zeros((2, 2, 3), np.uint8), np.full((2, 2, 3), 1, np.uint8)])
    assert np.all(collude_ref(two, "average", [0, 1]) == 1) and np.all(collude_ref(two, "median", [0, 1]) == 1)      # halves round up
    assert np.all(collude_ref(two, "minmax", [0, 1, 1]) == 1) and np.all(collude_ref(two, "average", [0, 0, 1]) == 0)


def test_mosaic_takes_whole_tiles_in_member_order():
    p = pool(5, 40, 70, 3)
    for c in (2, 3, 5):
        out = collude_ref(p, "mosaic", range(c))
        assert np.array_equal(out[32:40, 64:70], p[3 % c][32:40, 64:70])          # tile (2, 1)
        assert np.array_equal(out[0:32, 0:32], p[0][0:32, 0:32]) and np.array_equal(out[0:32, 32:64], p[1][0:32, 32:64])
    out = collude_ref(p, "mosaic", [4, 4, 2])                                        # members repeat and are out of order
    assert np.array_equal(out[0:32, 32:64], p[4][0:32, 32:64]) and np.array_equal(out[32:40, 32:64], p[2][32:40, 32:64])


def test_quality_of_equal_frames_is_zero_and_counts_what_differs():
    p = pool(2, 5, 33, 4)
    assert quality_ref(p[0], p[0]) == [0] * 6
    b, c = np.zeros((2, 3, 3), np.uint8), np.zeros((2, 3, 3), np.uint8)
    c[0, 1] = (3, 0, 4)
    c[1, 2] = (0, 200, 0)
    assert quality_ref(b, c) == [9, 200 * 200, 16, ((77 * 3 + 29 * 4 + 128) >> 8) ** 2 + ((150 * 200 + 128) >> 8) ** 2, 3, 200]
    assert quality_ref(c, b) == quality_ref(b, c)


# ---- surfaces ----------------------------------------------------------------------------------------------------------------
def header_comment(text, name):
    decl = text.index(name + "(")
    return text[text.rfind("/*", 0, decl):decl]


def test_symbols_declared_exported_bound_and_cited():
    text = open(os.path.join(ROOT, "include", "ssw.h")).read()
    lib = C.CDLL(L.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in L.SIGNATURES, n
    section = text[text.index("strength of a mark"):text.index("ssw_collude_rgb8(")]
    assert "algorithm.rs:604-606" in section and ":389-393" in section and "tests/test_collude_cpu.py" in section
    assert "SSW_STAGE_CONVERT" in section and section.count("No alignment is assumed") == 2
    q = " ".join(header_comment(text, "ssw_quality_rgb8").split())
    for phrase in ("(77 R + 150 G + 29 B + 128) >> 8", "n_base == 1", "n_base == n", "max |d|", "d != 0", "zeroes dev_stats"):
        assert phrase in q, phrase
    c = " ".join(section[section.index("A forged copy"):].split())
    for phrase in ("(sum of v + c / 2) / c", "(s[(c-1)/2] + s[c/2] + 1) >> 1", "s[0]", "s[c-1]", "(s[0] + s[c-1] + 1) >> 1",
                   "v[((x >> 5) + (y >> 5)) % c]", "1 <= count <= 16", "32 per launch", "must not overlap"):
        assert phrase in c, phrase
    assert len(L.SIGNATURES["ssw_quality_rgb8"][1]) == 8 and len(L.SIGNATURES["ssw_collude_rgb8"][1]) == 8
    assert C.sizeof(L.Coalition) == 72
    for i, m in enumerate(METHODS):
        assert L.COLLUDE_METHODS[m] == i and re.search(rf"SSW_COLLUDE_{m.upper()} = {i}\b", text), m
    assert "collude.hip" in open(os.path.join(ROOT, "spread_spectrum_watermarking_amd", "csrc", "Makefile")).read()


def test_the_number_of_stages_has_not_changed():
    text = open(os.path.join(ROOT, "include", "ssw.h")).read()
    assert re.search(r"SSW_STAGE_COUNT = 15\b", text) and len(L.STAGES) == 15 and L.STAGES[9] == "convert"


def test_the_two_colluders_sentences_are_qualified():
    for path in ("README.md", os.path.join("include", "ssw.h"), os.path.join("include", "ssw.hpp")):
        text = " ".join(open(os.path.join(ROOT, path)).read().replace("//", " ").split())
        assert "for an averaged forgery; see the strength report" in text, path


def test_python_surface():
    for name in ("Quality", "quality", "collude", "strength_report", "StrengthRow", "Collusion"):
        assert hasattr(wm, name), name
    q = api.Quality((0, 0, 0), 0, 0, 0, 100)
    assert q.psnr == math.inf and q.psnr_luma == math.inf and q.changed_fraction == 0.0
    q = api.Quality((100, 100, 100), 50, 30, 2, 100)
    assert abs(q.psnr - 10 * math.log10(255 ** 2)) < 1e-12 and abs(q.psnr_luma - 10 * math.log10(255 ** 2 * 2)) < 1e-12
    assert q.changed_fraction == 0.1
    img = np.zeros((8, 8, 3), np.uint8)
    with pytest.raises(ValueError):
        api.strength_report(img, [0.1], copies=3, sizes=(2, 4))              # before any device work: no GPU needed
    with pytest.raises(ValueError):
        api.strength_report(img, [0.1], methods=("mean",))
    with pytest.raises(ValueError):
        api._coalition("median", [0, 3], 3)
    with pytest.raises(ValueError):
        api._coalition("median", [0] * 17, 3)
    c = api._coalition("MinMax", [2, 0, 2], 3)
    assert (c.method, c.count, list(c.member[:3])) == (L.COLLUDE_MINMAX, 3, [2, 0, 2])
    assert api.quality(img, []) == [] and api.collude([img], []) == []
    for bad in (np.zeros((8, 8), np.uint8), np.zeros((8, 8, 4), np.uint8), np.zeros((8, 8, 3), np.float32), np.zeros((0, 8, 3), np.uint8)):
        with pytest.raises(ValueError):                                      # grey, RGBA (no channel is dropped silently), f32, empty
            api.quality(img, [bad])
        with pytest.raises(ValueError):
            api.collude([bad], [("min", [0])])
        with pytest.raises(ValueError):
            api.strength_report(bad, [0.1])


def test_cli_parser_surface():
    p = cli.build_parser()
    a = p.parse_args(["strength", "photo.jpg", "--alpha", "0.02", "0.05", "0.1"])
    assert (a.command, a.file, a.alpha) == ("strength", "photo.jpg", [0.02, 0.05, 0.1])
    assert (a.length, a.copies, a.collude, a.method, a.similarity_exceed, a.json) == (1000, 8, [2, 4], list(METHODS), 6.0, False)
    a = p.parse_args(["strength", "x.png", "--alpha", "0.1", "-n", "64", "--copies", "4", "--collude", "3", "--method", "min", "mosaic",
                      "--similarity-exceed", "5", "--json"])
    assert (a.length, a.copies, a.collude, a.method, a.similarity_exceed, a.json) == (64, 4, [3], ["min", "mosaic"], 5.0, True)
    with pytest.raises(SystemExit):
        p.parse_args(["strength", "x.png"])                                  # --alpha is required
    with pytest.raises(SystemExit):
        p.parse_args(["strength", "x.png", "--alpha", "0.1", "--method", "mean"])
    with pytest.raises(SystemExit):
        p.parse_args(["strength", "x.png", "--alpha", "0.1", "--ordering", "legacy"])      # the report has the issue's options only
    # the old subcommands parse as before
    a = p.parse_args(["fingerprint", "cat.jpg", "--copies", "5"])
    assert (a.command, a.copies, a.length, a.alpha, a.method) == ("fingerprint", 5, 1000, 0.1, "option2")
    a = p.parse_args(["watermark", "cat.jpg"])
    assert (a.command, a.length, a.ordering, a.alpha, a.method) == ("watermark", 1000, "energy", 0.1, "option2")
    a = p.parse_args(["test", "a.png", "b.png", "c.json"])
    assert (a.command, a.similarity_exceed, a.watermark_files) == ("test", 6.0, ["c.json"])
    a = p.parse_args(["trace", "a.png", "--suspects", "b.png", "--marks", "c.json"])
    assert (a.command, a.base, a.suspects, a.marks, a.similarity_exceed) == ("trace", "a.png", ["b.png"], ["c.json"], 6.0)
    a = p.parse_args(["identify", "s.png", "--catalogue", "c.npz"])
    assert (a.command, a.top) == ("identify", 1)


CPP = r"""
#include "ssw.hpp"
int main() {
    wm::Context ctx(0);
    wm::ImageRgb8 img(8, 8), a(8, 8), b(8, 8);
    std::vector<wm::Quality> q = wm::quality(ctx, img, {&a, &b});
    std::vector<wm::ImageRgb8> f = wm::collude(ctx, {&a, &b}, {wm::Coalition{SSW_COLLUDE_MEDIAN, {0, 1}}, wm::Coalition{SSW_COLLUDE_MOSAIC, {1}}});
    if (!(q[0].psnr() > 0.0) || q[1].changed_fraction() != 0.0 || q[0].psnr_luma() < 0.0) return 2;
    return (int)(q.size() + f.size()) - 4;
}
"""


def test_cpp_quality_and_collude_compile_and_link(tmp_path):
    src = tmp_path / "collude.cpp"
    src.write_text(CPP)
    exe = str(tmp_path / "collude")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                    "-L", LIBDIR, "-lssw_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert os.path.exists(exe)


# ---- the premise, through the oracle ---------------------------------------------------------------------------------------
def test_an_averaged_forgery_still_names_every_colluder():
    """The cat, default_rng(3), 8 marks of 1000, alpha 0.1, copies quantised like into_rgb8().  Measured with this oracle: the
    average of the first 2 copies scores 21.86 for its weakest colluder and 1.30 for the strongest innocent, of the first 4
    copies 14.15 and 1.45; copy 0 lies at 31.40 dB.  Nothing is asserted about the other methods: they are what the report is
    for (three colluders taking the median or the minimum already fall below 6)."""
    from oracle import oracle as O
    cat = np.load(os.path.join(GOLDEN, "cat_decoded_u8.npz"))["cat"]
    marks = np.random.default_rng(3).standard_normal((8, 1000)).astype(np.float32)
    rgb = O.u8_to_f32(cat)
    copies = np.stack([O.f32_to_u8(O.embed_frame(rgb, m, alpha=0.1)) for m in marks])
    q = quality_ref(cat, copies[0])
    psnr = 10 * math.log10(255 ** 2 * cat.size / sum(q[:3]))
    print(f"PSNR of copy 0: {psnr:.2f} dB")
    assert 31.0 < psnr < 32.0
    for c in (2, 4):
        forged = collude_ref(copies, "average", range(c))
        ext, _ = O.extract_frame(rgb, O.u8_to_f32(forged), marks[0], alpha=0.1)
        sims = np.array([O.similarity(ext, m) for m in marks])
        print(f"average of {c}: colluders {sims[:c].min():.2f} .. {sims[:c].max():.2f}, innocents up to {sims[c:].max():.2f}")
        assert np.all(sims[:c] > 6.0) and np.all(sims[c:] < 6.0), (c, sims)
