"""ssw_jpeg_rgb8 (include/ssw.h) without a GPU: `jpeg_ref`, the numpy restatement of the lossy part of baseline JPEG as
PIL / libjpeg-turbo do it (4:2:0, the Annex K tables scaled by libjpeg's rule, the `islow` DCT, fancy upsampling) -- what the
device results must EQUAL (tests/test_jpeg_gpu.py imports it).  It is checked here byte for byte against PIL's own save / open
round trip; then its properties, the surfaces (header, ctypes table, Python, CLI, C++), the exhaustive proof of the quantiser's
reciprocal division, and the premise of the report restated through the oracle: what a JPEG leaves of a mark depends on alpha."""
import ctypes as C
import io
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd import api, cli
import spread_spectrum_watermarking_amd as wm

LIBDIR = os.path.join(ROOT, "spread_spectrum_watermarking_amd", "lib")
QUALITIES = (1, 10, 25, 50, 75, 90, 95, 100)
SHAPES = [(8, 8), (9, 8), (15, 16), (16, 16), (17, 17), (31, 33), (40, 56), (41, 57), (39, 23), (64, 64), (65, 48), (8, 100), (100, 8)]   # (h, w)
CONTENTS = ("noise", "binary", "cat+noise")


# ---- the restatement ---------------------------------------------------------------------------------------------------------
K = dict(a=2446, b=3196, c=4433, d=6270, e=7373, f=9633, g=12299, h=15137, i=16069, j=16819, k=20995, l=25172)  # FIX(x), 13 bits
LUM = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
       18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
CHR = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32


def D(x, n):
    return (x + (1 << (n - 1))) >> n                              # arithmetic shift


def qtable(base, q):
    """The 8 x 8 table of quality q (1 .. 100): libjpeg's jpeg_quality_scaling + jpeg_add_quant_table, baseline."""
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((np.array(base).reshape(8, 8) * s + 50) // 100, 1, 255).astype(np.int64)


def fpass(d, first):
    """One pass of the `islow` forward DCT over the 8 values along the last axis."""
    d0, d1, d2, d3, d4, d5, d6, d7 = [d[..., i] for i in range(8)]
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n, o = (11 if first else 15), [None] * 8
    o[0], o[4] = ((t10 + t11) << 2, (t10 - t11) << 2) if first else (D(t10 + t11, 2), D(t10 - t11, 2))
    z1 = (t12 + t13) * K['c']
    o[2], o[6] = D(z1 + t13 * K['d'], n), D(z1 - t12 * K['h'], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * K['f']
    t4, t5, t6, t7 = t4 * K['a'], t5 * K['j'], t6 * K['l'], t7 * K['g']
    z1, z2, z3, z4 = -z1 * K['e'], -z2 * K['k'], -z3 * K['i'] + z5, -z4 * K['b'] + z5
    o[7], o[5], o[3], o[1] = D(t4 + z1 + z3, n), D(t5 + z2 + z4, n), D(t6 + z2 + z3, n), D(t7 + z1 + z4, n)
    return np.stack(o, -1)


def ipass(d, first):
    """One pass of the `islow` inverse DCT over the 8 values along the last axis."""
    i0, i1, i2, i3, i4, i5, i6, i7 = [d[..., i] for i in range(8)]
    z1 = (i2 + i6) * K['c']
    t2, t3 = z1 - i6 * K['h'], z1 + i2 * K['d']
    t0, t1 = (i0 + i4) << 13, (i0 - i4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = i7, i5, i3, i1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * K['f']
    t0, t1, t2, t3 = t0 * K['a'], t1 * K['j'], t2 * K['l'], t3 * K['g']
    z1, z2, z3, z4 = -z1 * K['e'], -z2 * K['k'], -z3 * K['i'] + z5, -z4 * K['b'] + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    n = 11 if first else 18
    return np.stack([D(t10 + t3, n), D(t11 + t2, n), D(t12 + t1, n), D(t13 + t0, n),
                     D(t13 - t0, n), D(t12 - t1, n), D(t11 - t2, n), D(t10 - t3, n)], -1)


def codec(p, q):
    """p [8m, 8n] 0 .. 255, q an 8 x 8 table -> the decoded plane: forward DCT, quantise, dequantise, inverse DCT per 8 x 8 block."""
    H, W = p.shape
    b = p.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3) - 128
    c = fpass(b, True)
    c = fpass(c.swapaxes(-1, -2), False).swapaxes(-1, -2)                          # rows, then columns
    k = np.sign(c) * ((np.abs(c) + ((q * 8) >> 1)) // (q * 8))                     # round half away from zero
    r = ipass((k * q).swapaxes(-1, -2), True).swapaxes(-1, -2)                     # columns, then rows
    r = ipass(r, False)
    return np.clip(r + 128, 0, 255).transpose(0, 2, 1, 3).reshape(H, W)


def jpeg_ref(img, quality):
    """img [h, w, 3] u8 -> what PIL's save(quality=quality) / open round trip gives, [h, w, 3] u8."""
    p = np.asarray(img).astype(np.int64)
    h, w, _ = p.shape
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    pw = (-w) % 16
    Y = np.pad(Y, ((0, (-h) % 16), (0, pw)), mode='edge')

    def down(a):                                                                   # full resolution: right edge to 16, bottom to an even height
        a = np.pad(a, ((0, h & 1), (0, pw)), mode='edge')
        s = a[0::2, 0::2] + a[0::2, 1::2] + a[1::2, 0::2] + a[1::2, 1::2]
        s = (s + (1 + (np.arange(s.shape[1]) & 1))[None, :]) >> 2                  # bias 1, 2, 1, 2 ... along a row
        return np.pad(s, ((0, (-s.shape[0]) % 8), (0, 0)), mode='edge')            # the DOWNSAMPLED last row is repeated, not the input's

    ch, cw = (h + 1) // 2, (w + 1) // 2

    def up(a):                                                                     # triangle filter on the ch x cw real samples, edges repeated
        a = a[:ch, :cw]
        ab = np.pad(a, ((1, 1), (0, 0)), mode='edge')
        out = np.zeros((2 * ch, 2 * cw), np.int64)
        for v in (0, 1):
            cs = 3 * a + (ab[:-2] if v == 0 else ab[2:])
            last = np.concatenate([cs[:, :1], cs[:, :-1]], 1)
            nxt = np.concatenate([cs[:, 1:], cs[:, -1:]], 1)
            out[v::2, 0::2] = (3 * cs + last + 8) >> 4
            out[v::2, 1::2] = (3 * cs + nxt + 7) >> 4
        return out[:h, :w]

    ql, qc = qtable(LUM, quality), qtable(CHR, quality)
    y = codec(Y, ql)[:h, :w]
    cb = up(codec(down(Cb), qc)) - 128
    cr = up(codec(down(Cr), qc)) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def cat_image():
    return np.ascontiguousarray(np.load(os.path.join(GOLDEN, "cat_decoded_u8.npz"))["cat"])


def content(kind, h, w, seed=0):
    """The three kinds of frames both test files use: uniform noise, random 0 / 255 bytes (the largest coefficients), and
    a piece of the cat with a little noise (a photograph's statistics)."""
    rng = np.random.default_rng([seed, h, w, CONTENTS.index(kind)])
    if kind == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "binary":
        return (rng.integers(0, 2, (h, w, 3), dtype=np.uint8) * 255).astype(np.uint8)
    cat = cat_image()
    reps = (-(-h // cat.shape[0]), -(-w // cat.shape[1]), 1)
    piece = np.tile(cat, reps)[:h, :w].astype(np.int16)
    return np.clip(piece + rng.integers(-8, 9, (h, w, 3)), 0, 255).astype(np.uint8)


# ---- the restatement against PIL ---------------------------------------------------------------------------------------------
def pil_round_trip(img, quality):
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(img).save(f, "JPEG", quality=quality)
    f.seek(0)
    return np.asarray(Image.open(f).convert("RGB"))


def needs_pil_jpeg():
    try:
        from PIL import features
        ok = features.check("jpg")
    except ImportError:
        ok = False
    if not ok:
        pytest.skip("PIL has no JPEG codec")


@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("h,w", SHAPES)
def test_restatement_equals_pil_on_small_shapes(h, w, kind):
    needs_pil_jpeg()
    img = content(kind, h, w)
    for q in QUALITIES:
        assert np.array_equal(jpeg_ref(img, q), pil_round_trip(img, q)), q


@pytest.mark.parametrize("name", ["cat", "watermarked_with_1"])
def test_restatement_equals_pil_on_the_photographs(name):
    needs_pil_jpeg()
    from PIL import Image
    img = cat_image() if name == "cat" else np.asarray(Image.open(os.path.join(GOLDEN, "watermarked_with_1.png")).convert("RGB"))
    assert img.shape == (444, 640, 3)
    for q in QUALITIES:
        assert np.array_equal(jpeg_ref(img, q), pil_round_trip(img, q)), q


# ---- properties of the restatement -------------------------------------------------------------------------------------------
def test_a_flat_frame_comes_back_flat():
    for colour in ((0, 0, 0), (255, 255, 255), (128, 128, 128), (200, 30, 90)):
        img = np.empty((23, 41, 3), np.uint8)
        img[:] = colour
        for q in (1, 50, 100):
            out = jpeg_ref(img, q)
            assert np.all(out == out[0, 0]), (colour, q)
    grey = np.full((16, 16, 3), 128, np.uint8)
    assert np.array_equal(jpeg_ref(grey, 100), grey)                       # (128, 128, 128) is a fixed point of both colour tables


def test_the_tables_follow_libjpegs_scaling_rule():
    assert np.all(qtable(LUM, 100) == 1) and np.all(qtable(CHR, 100) == 1)
    assert np.array_equal(qtable(LUM, 50), np.array(LUM).reshape(8, 8)) and np.array_equal(qtable(CHR, 50), np.array(CHR).reshape(8, 8))
    assert np.all(qtable(LUM, 1) == 255) and np.all(qtable(CHR, 1) == 255)              # scale 5000 %, clipped for baseline
    q49 = qtable(LUM, 49)                                                               # scale 5000 // 49 = 102
    assert q49[0, 0] == (16 * 102 + 50) // 100 == 16 and q49[7, 7] == (99 * 102 + 50) // 100 == 101 and q49[0, 7] == 62
    assert qtable(LUM, 75)[0, 0] == 8 and qtable(CHR, 75)[7, 7] == 50                   # scale 50 %
    for q in range(1, 101):
        for base in (LUM, CHR):
            t = qtable(base, q)
            assert t.min() >= 1 and t.max() <= 255 and (q == 100 or np.all(t >= qtable(base, q + 1)))


def test_the_chroma_bottom_rows_repeat_the_downsampled_row():
    """A 40-row frame ends 8 rows into its last band of 16: the four padding rows of its chroma blocks repeat the last
    DOWNSAMPLED row, while the luma repeats the last input row.  Padding the input instead changes the decoded frame."""
    img = content("noise", 40, 56, seed=7)
    padded = np.pad(img, ((0, 8), (0, 8), (0, 0)), mode="edge")
    assert not np.array_equal(jpeg_ref(padded, 50)[:40, :56], jpeg_ref(img, 50))
    odd = content("noise", 41, 57, seed=7)                                  # an odd height repeats one input row first; then both agree
    assert np.array_equal(jpeg_ref(np.pad(odd, ((0, 7), (0, 7), (0, 0)), mode="edge"), 50)[:41, :57], jpeg_ref(odd, 50))


def test_32_bit_integers_suffice():
    """The device keeps every value in 32 bits: the block codec run on int32 planes (numpy wraps silently) gives what it gives
    on int64 planes, also on planes of 0 / 255 samples, which have the largest coefficients."""
    for kind in CONTENTS:
        img = content(kind, 48, 32, seed=3)
        for q in (1, 50, 100):
            for base in (LUM, CHR):
                for ch in range(3):
                    narrow = codec(img[..., ch].astype(np.int32), qtable(base, q).astype(np.int32))
                    assert narrow.dtype == np.int32
                    assert np.array_equal(narrow, codec(img[..., ch].astype(np.int64), qtable(base, q))), (kind, q, ch)


# ---- surfaces ----------------------------------------------------------------------------------------------------------------
def test_symbol_declared_exported_bound_and_described():
    text = open(os.path.join(ROOT, "include", "ssw.h")).read()
    assert hasattr(C.CDLL(L.LIB_PATH), "ssw_jpeg_rgb8") and "ssw_jpeg_rgb8" in L.SIGNATURES
    assert len(L.SIGNATURES["ssw_jpeg_rgb8"][1]) == 8 and C.sizeof(L.JpegJob) == 8
    assert [f[0] for f in L.JpegJob._fields_] == ["frame", "quality"]
    assert text.index("ssw_collude_rgb8(") < text.index("ssw_jpeg_rgb8(") < text.index("16-bit frames")
    decl = text.index("int ssw_jpeg_rgb8(")
    comment = " ".join(text[text.index("ssw_collude_rgb8("):decl].split())
    for phrase in ("typedef struct ssw_jpeg_job { uint32_t frame; uint32_t quality; } ssw_jpeg_job;", "4:2:0", "islow", "tests/test_jpeg_cpu.py",
                   "(19595 R + 38470 G + 7471 B + 32768) >> 16", "5000 / q", "200 - 2 q", "round half away from zero", "must not overlap",
                   "No alignment is assumed", "SSW_STAGE_CONVERT", "1 .. 100", "a side below 8", "SSW_ERR_BAD_DIMS", "the last DOWNSAMPLED row"):
        assert phrase in comment, phrase
    assert "jpeg.hip" in open(os.path.join(ROOT, "spread_spectrum_watermarking_amd", "csrc", "Makefile")).read()
    assert "SSW_STAGE_COUNT = 15" in text and len(L.STAGES) == 15


def test_the_docs_no_longer_call_the_jpeg_attack_out_of_scope():
    for path in ("README.md", "DESIGN.md"):
        text = " ".join(open(os.path.join(ROOT, path)).read().split())
        assert "PIL on the host does the real one" not in text, path
        assert "ssw_jpeg_rgb8" in text, path
    assert "4.13" in open(os.path.join(ROOT, "DESIGN.md")).read()


def test_python_surface_refuses_before_any_device_work():
    for name in ("jpeg", "JpegResult", "strength_report", "StrengthRow"):
        assert hasattr(wm, name), name
    img = np.zeros((8, 8, 3), np.uint8)
    assert api.jpeg([], [50]) == [] and api.jpeg([img], []) == [[]]
    for bad in (np.zeros((8, 8), np.uint8), np.zeros((8, 8, 4), np.uint8), np.zeros((8, 8, 3), np.float32), np.zeros((0, 8, 3), np.uint8),
                np.zeros((7, 8, 3), np.uint8), np.zeros((8, 7, 3), np.uint8)):
        with pytest.raises(ValueError):                                      # grey, RGBA, f32, empty, a side below 8: no GPU needed
            api.jpeg([bad], [50])
    with pytest.raises(ValueError):
        api.jpeg([img, np.zeros((8, 16, 3), np.uint8)], [50])                # one size
    for q in (0, 101, -1, 50.5, "high"):
        with pytest.raises(ValueError):
            api.jpeg([img], [75, q])
    for q in (0, 101):
        with pytest.raises(ValueError):
            api.strength_report(np.zeros((16, 16, 3), np.uint8), [0.1], jpeg=(q,))
    with pytest.raises(ValueError):
        api.strength_report(np.zeros((7, 16, 3), np.uint8), [0.1], jpeg=(50,))
    # the new field comes last and defaults to nothing: positional construction as before
    row = api.StrengthRow(0.1, [], [])
    assert row.jpeg == [] and api.StrengthRow(0.1, [], []).jpeg is not row.jpeg
    r = api.JpegResult(75, 8, 31.5, 1.7, 0, 36.1, 38.0)
    assert (r.quality, r.survived, r.weakest_own, r.strongest_innocent, r.accused, r.psnr_min, r.psnr_max) == (75, 8, 31.5, 1.7, 0, 36.1, 38.0)


def test_cli_parser_surface():
    p = cli.build_parser()
    a = p.parse_args(["strength", "photo.jpg", "--alpha", "0.02", "0.1"])
    assert a.jpeg == []
    assert (a.length, a.copies, a.collude, a.similarity_exceed, a.json) == (1000, 8, [2, 4], 6.0, False)
    a = p.parse_args(["strength", "photo.jpg", "--alpha", "0.1", "--jpeg", "90", "75", "50", "--json"])
    assert a.jpeg == [90, 75, 50] and a.json
    with pytest.raises(SystemExit):
        p.parse_args(["strength", "photo.jpg", "--alpha", "0.1", "--jpeg", "high"])


CPP = r"""
#include "ssw.hpp"
int main() {
    wm::Context ctx(0);
    wm::ImageRgb8 a(16, 8), b(16, 8);
    std::vector<wm::ImageRgb8> out = wm::jpeg(ctx, {&a, &b}, {wm::JpegJob{0, 75}, wm::JpegJob{1, 10}, wm::JpegJob{0, 100}});
    return (int)out.size() - 3 + (int)out[0].width - 16;
}
"""


def test_cpp_jpeg_compiles_and_links(tmp_path):
    src = tmp_path / "jpeg.cpp"
    src.write_text(CPP)
    exe = str(tmp_path / "jpeg")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                    "-L", LIBDIR, "-lssw_hip", f"-Wl,-rpath,{LIBDIR}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert os.path.exists(exe)


# ---- the quantiser's division ------------------------------------------------------------------------------------------------
def test_the_reciprocal_division_is_exact_and_the_host_tables_follow_the_rule(tmp_path):
    """csrc/jpeg_tables.hpp, the header the kernel and the host code include: n / d as the high half of n * (0xFFFFFFFF / d + 1)
    for every d = 8 .. 2040 (every 8 q among them) and every n <= 2^17 + 1020; and the tables the host makes for every quality."""
    exe = str(tmp_path / "jpeg_tables_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "spread_spectrum_watermarking_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "jpeg_tables_test.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == f"checked 2033 divisors, numerators 0 .. {2 ** 17 + 1020}"
    assert len(lines) == 101
    for q, line in enumerate(lines[1:], start=1):
        v = line.split()
        assert v[:2] == ["q", str(q)] and len(v) == 130
        assert [int(x) for x in v[2:66]] == qtable(LUM, q).ravel().tolist(), q
        assert [int(x) for x in v[66:]] == qtable(CHR, q).ravel().tolist(), q


# ---- the premise, through the oracle -----------------------------------------------------------------------------------------
def test_what_a_jpeg_leaves_of_a_mark_depends_on_alpha():
    """The cat, default_rng(3), marks of 1000, copy 0 quantised like into_rgb8() and compressed by the restatement.  Measured
    with this oracle: at alpha 0.1 and quality 50 the own mark scores 30.94 and the strongest of the seven other marks 1.67; at
    alpha 0.02 and quality 10 the own mark scores 3.74 -- the quality-10 thumbnail of a faintly marked copy cannot be traced."""
    from oracle import oracle as O
    cat = cat_image()
    marks = np.random.default_rng(3).standard_normal((8, 1000)).astype(np.float32)
    rgb = O.u8_to_f32(cat)

    def sims(alpha, quality):
        copy = O.f32_to_u8(O.embed_frame(rgb, marks[0], alpha=alpha))
        ext, _ = O.extract_frame(rgb, O.u8_to_f32(jpeg_ref(copy, quality)), marks[0], alpha=alpha)
        return np.array([O.similarity(ext, m) for m in marks])

    s = sims(0.1, 50)
    print(f"alpha 0.1, quality 50: own {s[0]:.2f}, strongest innocent {s[1:].max():.2f}")
    assert s[0] > 6.0 and np.all(s[1:] < 6.0), s
    s = sims(0.02, 10)
    print(f"alpha 0.02, quality 10: own {s[0]:.2f}")
    assert s[0] < 6.0, s
