"""ssw_filter_rgb8 (include/ssw.h) without a GPU: `filter_ref`, the numpy restatement of Pillow's GaussianBlur, UnsharpMask and
MedianFilter(3) -- integer arithmetic on the bytes, the blur's three constants made in `float` as Pillow's C makes them -- which
the device results must EQUAL (tests/test_filter_gpu.py imports it).  It is checked here byte for byte against Pillow itself;
then its properties, known answers, the surfaces (header, ctypes table, Python, CLI, C++), the host's constants against the
rule, and the premise of the report rows restated through the oracle: which alpha survives which filter."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd import api, cli
import spread_spectrum_watermarking_amd as wm
from test_jpeg_cpu import CONTENTS, cat_image, content

LIBDIR = os.path.join(ROOT, "spread_spectrum_watermarking_amd", "lib")
BLUR, UNSHARP, MEDIAN3 = 0, 1, 2
RADII = (0.3, 0.5, 1, 1.5, 2, 3.3, 4, 6, 8)
UNSHARPS = ((150, 3), (50, 0), (300, 10))                                    # (percent, threshold)
SHAPES = [(1, 1), (1, 7), (2, 3), (5, 4), (8, 8), (9, 31), (33, 17), (64, 70), (3, 100)]   # (h, w)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def blur_constants(radius):
    """(r, ww, fw) of a Gaussian blur of sigma `radius`: Pillow's _gaussian_blur_radius and ImagingBoxBlur, every operation
    rounded to float as its C does (the square root and the floor are taken in double and rounded)."""
    f = np.float32
    rad = f(radius)
    s2 = f(f(rad * rad) / f(3))
    big_l = f(np.sqrt(12.0 * float(s2) + 1.0))
    l = f(np.floor((float(big_l) - 1.0) / 2.0))
    a = f(f(f(2) * l + f(1)) * f(f(l * f(l + f(1))) - f(f(3) * s2)))
    a = f(a / f(f(6) * f(s2 - f(f(l + f(1)) * f(l + f(1))))))
    rho = f(l + a)
    r = int(rho)
    ww = int(f(f(1 << 24) / f(f(rho * f(2)) + f(1))))
    return r, ww, ((1 << 24) - (2 * r + 1) * ww) // 2


def box_pass(a, r, ww, fw):
    """One box pass along the last axis; indices are clamped against the array, which is the whole frame's line."""
    n = a.shape[-1]
    i = np.arange(n)
    acc = sum(a[..., np.clip(i + d, 0, n - 1)] for d in range(-r, r + 1))
    far = a[..., np.clip(i - r - 1, 0, n - 1)] + a[..., np.clip(i + r + 1, 0, n - 1)]
    return (ww * acc + fw * far + a.dtype.type(1 << 23)) >> a.dtype.type(24)


_BLURRED = {}                                                                # the last blurs: UNSHARP of a frame reuses BLUR's


def blur_ref(img, radius, dtype=np.int64):
    img = np.ascontiguousarray(img)
    key = (img.shape, hashlib.sha256(img.tobytes()).digest(), float(np.float32(radius)), dtype)
    if key not in _BLURRED:
        if len(_BLURRED) >= 32:
            _BLURRED.clear()
        r, ww, fw = blur_constants(radius)
        a = img.astype(dtype).transpose(0, 2, 1)                             # [h, 3, w]: three passes along the rows
        for _ in range(3):
            a = box_pass(a, r, dtype(ww), dtype(fw))
        a = a.transpose(2, 1, 0)                                             # [w, 3, h]: three along the columns
        for _ in range(3):
            a = box_pass(a, r, dtype(ww), dtype(fw))
        _BLURRED[key] = a.transpose(2, 0, 1).astype(np.uint8)
    return _BLURRED[key].copy()


def filter_ref(img, kind, radius=0.0, percent=0, threshold=0):
    """img [h, w, 3] u8 -> what Pillow's GaussianBlur(radius) / UnsharpMask(radius, percent, threshold) / MedianFilter(3) gives."""
    img = np.asarray(img)
    if kind == BLUR:
        return blur_ref(img, radius)
    if kind == UNSHARP:
        p = img.astype(np.int64)
        d = p - blur_ref(img, radius).astype(np.int64)
        step = np.sign(d) * (np.abs(d) * percent // 100)                     # the division truncates toward zero
        return np.where(np.abs(d) > threshold, np.clip(p + step, 0, 255), p).astype(np.uint8)
    assert kind == MEDIAN3
    h, w, _ = img.shape
    p = np.pad(img, ((1, 1), (1, 1), (0, 0)), mode="edge")
    return np.sort(np.stack([p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)]), 0)[4]


def ref_of(img, f):
    """`filter_ref` of an api.Filter"""
    return filter_ref(img, f.kind, f.radius, f.percent, f.threshold)


# ---- the restatement against Pillow ------------------------------------------------------------------------------------------
def pil_filter(img, kind, radius=0.0, percent=0, threshold=0):
    from PIL import Image, ImageFilter
    f = {BLUR: lambda: ImageFilter.GaussianBlur(radius), UNSHARP: lambda: ImageFilter.UnsharpMask(radius, percent, threshold),
         MEDIAN3: lambda: ImageFilter.MedianFilter(3)}[kind]()
    return np.asarray(Image.fromarray(img).filter(f))


def every_filter():
    yield (MEDIAN3,)
    for radius in RADII:
        yield (BLUR, radius)
        for percent, threshold in UNSHARPS:
            yield (UNSHARP, radius, percent, threshold)


@pytest.mark.parametrize("kind", ("noise", "binary"))
@pytest.mark.parametrize("h,w", SHAPES)
def test_restatement_equals_pillow_on_small_shapes(h, w, kind):
    img = content(kind, h, w)
    for args in every_filter():
        assert np.array_equal(filter_ref(img, *args), pil_filter(img, *args)), args


def test_restatement_equals_pillow_at_every_radius():
    img = content("noise", 23, 37, seed=1)
    for i in range(1, 81):
        assert np.array_equal(filter_ref(img, BLUR, i / 10), pil_filter(img, BLUR, i / 10)), i / 10


@pytest.mark.parametrize("name", ["cat", "watermarked_with_1"])
def test_restatement_equals_pillow_on_the_photographs(name):
    from PIL import Image
    img = cat_image() if name == "cat" else np.asarray(Image.open(os.path.join(GOLDEN, "watermarked_with_1.png")).convert("RGB"))
    assert img.shape == (444, 640, 3)
    for args in ((MEDIAN3,), (BLUR, 0.5), (BLUR, 2), (BLUR, 8), (UNSHARP, 2, 150, 3), (UNSHARP, 1, 1000, 0)):
        assert np.array_equal(filter_ref(img, *args), pil_filter(img, *args)), args


# ---- properties and known answers --------------------------------------------------------------------------------------------
def test_the_constants():
    assert blur_constants(8.0) == (7, 1052688, 493448) and blur_constants(1.0) == (0, 11184811, 2796202)
    assert blur_constants(2.4)[0] == 1 and blur_constants(2.5)[0] == 2                   # either side of the step
    assert blur_constants(1e-5) == (0, 1 << 24, 0)                                       # 2 rho + 1 rounds to 1: the identity
    for i in range(1, 81):
        r, ww, fw = blur_constants(i / 10)
        assert 0 <= r <= 7 and 0 < ww <= 1 << 24 and 0 <= fw < 1 << 24
        assert (2 * r + 1) * ww + 2 * fw in ((1 << 24) - 1, 1 << 24)                     # the weights sum to 2^24, or one less


def test_32_bit_integers_suffice():
    """The device keeps every value in 32 bits unsigned: the blur run on uint32 arrays (numpy wraps silently) gives what it
    gives on int64 arrays, also on frames of 0 / 255 bytes and on an all-255 frame, which reach 255 * 2^24 + 2^23."""
    frames = [content(kind, 21, 34, seed=3) for kind in CONTENTS] + [np.full((9, 11, 3), 255, np.uint8)]
    for img in frames:
        for radius in (1e-5, 0.3, 1, 2.5, 8):
            narrow = blur_ref(img, radius, np.uint32)
            assert np.array_equal(narrow, blur_ref(img, radius)), radius
    assert np.array_equal(blur_ref(frames[-1], 8), frames[-1]) and np.array_equal(blur_ref(frames[0], 1e-5), frames[0])
    assert 255 * (1 << 24) + (1 << 23) < 1 << 32


def test_a_flat_frame_stays_flat_and_the_edge_is_clamped_in_every_pass():
    for colour in ((0, 0, 0), (255, 255, 255), (200, 30, 90)):
        img = np.empty((13, 21, 3), np.uint8)
        img[:] = colour
        for args in ((MEDIAN3,), (BLUR, 3.3), (UNSHARP, 2, 150, 3)):
            assert np.array_equal(filter_ref(img, *args), img), (colour, args)
    # a blur of the frame padded with its edge beforehand is NOT the blur of the frame: the second pass repeats the first
    # pass's edge OUTPUT.  Tiled implementations that pad the input go wrong exactly here.
    img = content("noise", 12, 40, seed=4)
    r = blur_constants(2.5)[0]
    pad = 3 * (r + 1)
    padded = np.pad(img, ((pad, pad), (pad, pad), (0, 0)), mode="edge")
    assert not np.array_equal(filter_ref(padded, BLUR, 2.5)[pad:-pad, pad:-pad], filter_ref(img, BLUR, 2.5))


def test_unsharp_threshold_and_clamp():
    img = content("noise", 10, 14, seed=5)
    assert np.array_equal(filter_ref(img, UNSHARP, 2, 1, 255), img)                      # |d| never exceeds 255
    b = blur_ref(img, 2).astype(int)
    out = filter_ref(img, UNSHARP, 2, 1000, 0).astype(int)
    d = img.astype(int) - b
    assert np.array_equal(out[d == 0], img[d == 0]) and np.all(out[d > 25] == 255) and np.all(out[d < -25] == 0)
    assert filter_ref(np.array([[[7, 7, 7]]], np.uint8), UNSHARP, 1, 150, 3).tolist() == [[[7, 7, 7]]]
    # trunc(-3 * 150 / 100) = -4 in C, not the floor -5
    one = np.zeros((1, 9, 3), np.uint8) + 100
    one[0, 4] = 90
    got, blurred = filter_ref(one, UNSHARP, 1, 150, 0)[0, :, 0].astype(int), blur_ref(one, 1)[0, :, 0].astype(int)
    for x in range(9):
        dd = int(one[0, x, 0]) - blurred[x]
        assert got[x] == int(one[0, x, 0]) + (abs(dd) * 150 // 100) * (1 if dd > 0 else -1), x


KNOWN = {   # sha256 of the cat's filtered bytes, and the pixel (y 195, x 394), which lies on an edge; a later change to filter_ref is noticed here
    "median 3": ("12158c07e38f0b9aa538173c07fdb6d40da4320f165cfc709b60ee3138bfda46",
                 (178, 155, 139)),
    "blur 1": ("a88f844a2f4308c4f6b7391eb845d336908a3c9e6faf1f29d90401bd6fad6a8d",
                 (171, 140, 123)),
    "blur 8": ("fdc474f2f5b1540ad84bc4b59cd5ca147112e13c78cda4d4b798ed6dece48ab7",
                 (160, 141, 130)),
    "unsharp 2,150,3": ("c16e480e2fe4a6bc2557a2fe268f6af5bd640d7a788ce6c915d162b8f96d603d",
                        (255, 255, 246)),
}


def test_known_answers_on_the_cat():
    cat = cat_image()
    for f in (api.Filter.median(), api.Filter.blur(1), api.Filter.blur(8), api.Filter.unsharp()):
        out = ref_of(cat, f)
        digest, pixel = KNOWN[f.label]
        assert hashlib.sha256(out.tobytes()).hexdigest() == digest, f.label
        assert tuple(int(v) for v in out[195, 394]) == pixel, f.label


# ---- surfaces ----------------------------------------------------------------------------------------------------------------
def test_symbol_declared_exported_bound_and_described():
    text = open(os.path.join(ROOT, "include", "ssw.h")).read()
    assert hasattr(C.CDLL(L.LIB_PATH), "ssw_filter_rgb8") and "ssw_filter_rgb8" in L.SIGNATURES
    assert len(L.SIGNATURES["ssw_filter_rgb8"][1]) == 8 and C.sizeof(L.FilterJob) == 20
    assert [f[0] for f in L.FilterJob._fields_] == ["frame", "kind", "radius", "percent", "threshold"]
    assert (L.FILTER_BLUR, L.FILTER_UNSHARP, L.FILTER_MEDIAN3) == (0, 1, 2)
    assert text.index("ssw_ssim_rgb8(") < text.index("ssw_filter_rgb8(") < text.index("16-bit frames")
    decl = text.index("int ssw_filter_rgb8(")
    comment = " ".join(text[text.index("int ssw_ssim_rgb8("):decl].split())
    for phrase in ("typedef struct ssw_filter_job { uint32_t frame; uint32_t kind; float radius; uint32_t percent; uint32_t threshold; } ssw_filter_job;",
                   "SSW_FILTER_BLUR = 0, SSW_FILTER_UNSHARP = 1, SSW_FILTER_MEDIAN3 = 2", "tests/test_filter_cpu.py", "GaussianBlur", "UnsharpMask",
                   "MedianFilter(3)", "s2 = radius * radius / 3", "fw = (2^24 - (2 r + 1) ww) / 2", "+ 2^23) >> 24", "applied anew in every pass",
                   "ww = 1052688, fw = 493448", "truncating toward zero", "fifth smallest", "must be 0", "must not overlap",
                   "No alignment is assumed", "SSW_STAGE_CONVERT", "2 * 3 w h", "1 .. 1000", "SSW_ERR_BAD_DIMS", "65535"):
        assert phrase in comment, phrase
    assert "filter.hip" in open(os.path.join(ROOT, "spread_spectrum_watermarking_amd", "csrc", "Makefile")).read()
    assert "SSW_STAGE_COUNT = 15" in text and len(L.STAGES) == 15


def test_the_docs_describe_the_filters():
    for path in ("README.md", "DESIGN.md"):
        text = " ".join(open(os.path.join(ROOT, path)).read().split())
        assert "ssw_filter_rgb8" in text, path
    assert "### 4.15" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_python_surface_refuses_before_any_device_work():
    for name in ("filter", "Filter", "FilterResult", "strength_report", "StrengthRow"):
        assert hasattr(wm, name), name
    F = api.Filter
    assert (F.blur(1.5).label, F.unsharp().label, F.median().label, F.blur(2).label) == ("blur 1.5", "unsharp 2,150,3", "median 3", "blur 2")
    assert F.unsharp(1.5, 300, 10).label == "unsharp 1.5,300,10" and F.blur(8.0).radius == 8.0
    j = F.unsharp(2, 150, 3).job(5)
    assert (j.frame, j.kind, j.radius, j.percent, j.threshold) == (5, L.FILTER_UNSHARP, 2.0, 150, 3)
    j = F.median().job(1)
    assert (j.frame, j.kind, j.radius, j.percent, j.threshold) == (1, L.FILTER_MEDIAN3, 0.0, 0, 0)
    for bad in (0, -1, 8.1, float("nan"), float("inf"), 1e-50, "2", True, None):
        with pytest.raises(ValueError):
            F.blur(bad)
        with pytest.raises(ValueError):
            F.unsharp(bad)
    for percent, threshold in ((0, 3), (1001, 3), (150, -1), (150, 256), (150.5, 3), (150, 3.0)):
        with pytest.raises(ValueError):
            F.unsharp(2, percent, threshold)
    img = np.zeros((1, 1, 3), np.uint8)
    assert api.filter([], [F.median()]) == [] and api.filter([img], []) == [[]]
    for bad in (np.zeros((8, 8), np.uint8), np.zeros((8, 8, 4), np.uint8), np.zeros((8, 8, 3), np.float32), np.zeros((0, 8, 3), np.uint8)):
        with pytest.raises(ValueError):                                      # grey, RGBA, f32, empty: no GPU needed
            api.filter([bad], [F.median()])
    with pytest.raises(ValueError):
        api.filter([img, np.zeros((1, 2, 3), np.uint8)], [F.median()])        # one size
    for bad in ("median", 3, ("blur", 1.0), None):
        with pytest.raises(ValueError):
            api.filter([img], [F.median(), bad])
        with pytest.raises(ValueError):
            api.strength_report(np.zeros((16, 16, 3), np.uint8), [0.1], filters=[bad])
    # the new field comes last and defaults to nothing: positional construction as before
    row = api.StrengthRow(0.1, [], [])
    assert row.filters == [] and api.StrengthRow(0.1, [], []).filters is not row.filters
    r = api.FilterResult("blur 1.5", 8, 30.2, 1.4, 0, 33.0, 35.1)
    assert (r.filter, r.survived, r.weakest_own, r.strongest_innocent, r.accused, r.psnr_min, r.psnr_max) == ("blur 1.5", 8, 30.2, 1.4, 0, 33.0, 35.1)
    assert r.ssim_min != r.ssim_min and r.ssim_max != r.ssim_max
    assert [f.name for f in api.FilterResult.__dataclass_fields__.values()][1:] == [f.name for f in api.JpegResult.__dataclass_fields__.values()][1:]


def test_cli_parser_surface():
    p = cli.build_parser()
    a = p.parse_args(["strength", "photo.jpg", "--alpha", "0.02", "0.1"])
    assert a.filters == [] and a.jpeg == []
    assert (a.length, a.copies, a.collude, a.similarity_exceed, a.json, a.ssim) == (1000, 8, [2, 4], 6.0, False, False)
    a = p.parse_args(["strength", "photo.jpg", "--alpha", "0.1", "--filter", "blur:1.5", "median", "unsharp:2,150,3", "unsharp", "unsharp:1", "--json"])
    assert [f.label for f in a.filters] == ["blur 1.5", "median 3", "unsharp 2,150,3", "unsharp 2,150,3", "unsharp 1,150,3"] and a.json
    for bad in ("blur", "blur:0", "blur:9", "blur:x", "blur:1,2", "median:5", "unsharp:2,0", "unsharp:2,150,256", "unsharp:2,150,3,4", "sharpen", "blur:nan"):
        with pytest.raises(SystemExit):
            p.parse_args(["strength", "photo.jpg", "--alpha", "0.1", "--filter", bad])


CPP = r"""
#include "ssw.hpp"
int main() {
    wm::Context ctx(0);
    wm::ImageRgb8 a(5, 3), b(5, 3);
    std::vector<wm::ImageRgb8> out = wm::filter(ctx, {&a, &b}, {wm::FilterJob::blur(0, 1.5f), wm::FilterJob::median(1), wm::FilterJob::unsharp(0)});
    return (int)out.size() - 3 + (int)out[0].width - 5;
}
"""


def test_cpp_filter_compiles_and_links(tmp_path):
    src = tmp_path / "filter.cpp"
    src.write_text(CPP)
    exe = str(tmp_path / "filter")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                    "-L", LIBDIR, "-lssw_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert os.path.exists(exe)


# ---- the host's constants ----------------------------------------------------------------------------------------------------
def test_the_host_constants_follow_the_rule(tmp_path):
    """csrc/filter_tables.hpp, the header the library's host code includes: (r, ww, fw) of the 80 radii 0.1 .. 8.0 and of 2.4, 2.5
    and 8.0 as the library makes them, against `blur_constants`."""
    exe = str(tmp_path / "filter_tables_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "spread_spectrum_watermarking_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "filter_tables_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    radii = [i / 10 for i in range(1, 81)] + [2.4, 2.5, 8.0]
    assert len(lines) == 83
    for radius, line in zip(radii, lines):
        v = line.split()
        assert v[0] == "radius" and np.float32(float(v[1])) == np.float32(radius), line
        assert tuple(int(x) for x in v[2:]) == blur_constants(radius), line
    assert lines[-1] == "radius 8 7 1052688 493448" and lines[9] == "radius 1 0 11184811 2796202"
    assert lines[-3].split()[2] == "1" and lines[-2].split()[2] == "2"


# ---- the premise, through the oracle -----------------------------------------------------------------------------------------
REPORT_FILTERS = (("blur 1", (BLUR, 1.0)), ("blur 3", (BLUR, 3.0)), ("median 3", (MEDIAN3,)), ("unsharp 2,150,3", (UNSHARP, 2.0, 150, 3)))


def oracle_similarities(alpha, filters=REPORT_FILTERS, copies=8):
    """The cat, default_rng(3), marks of 1000: copy c embedded by the oracle, quantised like into_rgb8(), filtered by the
    restatement, extracted by the oracle -> {label: sims [copies][copies]}, row c against every mark."""
    from oracle import oracle as O
    cat = cat_image()
    marks = np.random.default_rng(3).standard_normal((8, 1000)).astype(np.float32)
    rgb = O.u8_to_f32(cat)
    out = {label: np.zeros((copies, 8)) for label, _ in filters}
    for c in range(copies):
        copy = O.f32_to_u8(O.embed_frame(rgb, marks[c], alpha=alpha))
        for label, args in filters:
            ext, _ = O.extract_frame(rgb, O.u8_to_f32(filter_ref(copy, *args)), marks[c], alpha=alpha)
            out[label][c] = [O.similarity(ext, m) for m in marks]
    return out


def test_which_alpha_survives_which_filter():
    """What tests/test_filter_gpu.py asserts of the report's rows, measured here with the oracle and `filter_ref` on all 8 copies
    (own mark: weakest .. strongest; the strongest other mark):
      alpha 0.02   blur 1: 16.76 .. 18.14 (1.77), 8/8 found     blur 3: 2.04 .. 2.90 (0.64), 0/8
                   median 3: 18.33 .. 21.40 (2.32), 8/8         unsharp 2,150,3: 3.43 .. 5.86 (1.12), 0/8
      alpha 0.1    blur 1: 29.68 .. 31.31 (1.83), 8/8           blur 3: 11.49 .. 12.45 (1.09), 8/8
                   median 3: 30.06 .. 31.72 (2.12), 8/8         unsharp 2,150,3: 18.40 .. 20.52 (1.85), 8/8
    A mark of alpha 0.1 survives all four; one of alpha 0.02 survives a blur of sigma 1 and the median in every copy and is lost
    in every copy to a blur of sigma 3 and to the default unsharp mask."""
    for alpha in (0.02, 0.1):
        sims = oracle_similarities(alpha)
        for label, s in sims.items():
            own, others = np.diagonal(s), s[~np.eye(8, dtype=bool)]
            print(f"alpha {alpha}, {label}: own {own.min():.2f} .. {own.max():.2f}, strongest other {others.max():.2f}, found {(own > 6.0).sum()}/8")
            assert others.max() < 6.0, (alpha, label)
            lost = alpha == 0.02 and label in ("blur 3", "unsharp 2,150,3")
            assert np.all(own < 6.0) if lost else np.all(own > 6.0), (alpha, label, own)
