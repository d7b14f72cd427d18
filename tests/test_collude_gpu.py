"""ssw_quality_rgb8 / ssw_collude_rgb8 on the device against the numpy restatement of tests/test_collude_cpu.py: every comparison
is np.array_equal, there is no tolerance.  Shapes are the smallest at which the kernels can go wrong: one pixel (no whole group of
four), widths whose rows are no multiple of four bytes, a MOSAIC tile boundary in both axes with partial last tiles, more than
one block, more than two launches of 32 descriptors, byte offsets 0 .. 3 of every frame pointer, sums beyond 32 bits."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN
from gpu_util import ctx, lib
from spread_spectrum_watermarking_amd import _lib as L
from spread_spectrum_watermarking_amd import api, cli
from spread_spectrum_watermarking_amd._lib import check
from test_collude_cpu import METHODS, collude_ref, quality_ref

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (33, 5), (70, 40), (257, 3)]                 # (w, h)
COUNTS = (1, 2, 3, 4, 5, 8, 15, 16)
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def cat():
    return np.ascontiguousarray(np.load(os.path.join(GOLDEN, "cat_decoded_u8.npz"))["cat"])


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


def coalitions_c(coalitions):
    return (L.Coalition * max(len(coalitions), 1))(*[L.Coalition(METHODS.index(m) if isinstance(m, str) else m, len(mem),
                                                                 (C.c_uint32 * 16)(*mem)) for m, mem in coalitions])


def dev_collude(copies, coalitions, off_in=0, off_out=0):
    n, h, w, _ = copies.shape
    d, o = Dev(copies, off_in), Dev(len(coalitions) * h * w * 3, off_out)
    check(lib().ssw_collude_rgb8(ctx().handle, d.ptr, n, w, h, coalitions_c(coalitions), len(coalitions), o.ptr), "ssw_collude_rgb8")
    out = o.host(np.uint8, (len(coalitions), h, w, 3))
    d.free(); o.free()
    return out


def dev_quality(base, copies, off_base=0, off_copies=0):
    """base [h, w, 3] or [n, h, w, 3]; copies [n, h, w, 3] -> [n][6] python ints.  The statistics start as garbage."""
    n, h, w, _ = copies.shape
    b, c, s = Dev(base, off_base), Dev(copies, off_copies), Dev(n * 48)
    check(lib().ssw_quality_rgb8(ctx().handle, b.ptr, 1 if base.ndim == 3 else n, c.ptr, n, w, h, s.ptr), "ssw_quality_rgb8")
    out = s.host(np.uint64, (n, 6))
    for x in (b, c, s):
        x.free()
    return [[int(v) for v in row] for row in out]


def pool(n, w, h, seed=0, extremes=False):
    p = np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    if extremes:
        p[1], p[n - 2] = 0, 255
    return p


def every_method_and_count(n, seed):
    """One coalition per (method, count): members drawn with repeats and in no order, so that they repeat and are out of order."""
    rng = np.random.default_rng(seed)
    return [(m, [int(i) for i in rng.integers(0, n, c)]) for m in METHODS for c in COUNTS]


# ---- collude -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extremes", [False, True], ids=["random", "with-black-and-white"])
@pytest.mark.parametrize("w,h", SHAPES)
def test_collude_every_method_and_count(w, h, extremes):
    p = pool(16, w, h, w * 7 + h, extremes)
    co = every_method_and_count(16, w + h)
    co += [(m, list(range(c))) for m in ("median", "mosaic") for c in (3, 16)]          # and in order
    out = dev_collude(p, co)
    for i, (m, mem) in enumerate(co):
        assert np.array_equal(out[i], collude_ref(p, m, mem)), (m, mem)


@pytest.fixture(scope="module")
def cat_pool(cat):
    """Copies that differ from the cat by a little, as marked copies do: ties and near-ties among the members are the rule."""
    rng = np.random.default_rng(5)
    return np.clip(cat[None].astype(np.int16) + rng.integers(-3, 4, (16,) + cat.shape), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("method", METHODS)
def test_collude_the_cat(cat_pool, method):
    """A real frame (640 x 444): more than one block per coalition, MOSAIC tiles of every kind."""
    co = [c for c in every_method_and_count(16, 11) if c[0] == method]
    out = dev_collude(cat_pool, co)
    for i, (m, mem) in enumerate(co):
        assert np.array_equal(out[i], collude_ref(cat_pool, m, mem)), (m, mem)


def test_collude_seventy_coalitions_in_order_and_each_alone():
    w, h = 70, 40
    p = pool(9, w, h, 21, True)
    rng = np.random.default_rng(22)
    co = [(METHODS[int(rng.integers(0, 6))], [int(i) for i in rng.integers(0, 9, int(rng.integers(1, 17)))]) for _ in range(70)]
    out = dev_collude(p, co)                                      # three launches of 32, 32 and 6 descriptors
    for i, (m, mem) in enumerate(co):
        assert np.array_equal(out[i], collude_ref(p, m, mem)), (i, m, mem)
    for i in range(70):                                           # alone = inside the batch, whatever its slot and launch
        assert np.array_equal(dev_collude(p, [co[i]])[0], out[i]), (i, co[i])


@pytest.mark.parametrize("w,h", [(33, 5), (70, 40)])
def test_collude_at_every_byte_offset(w, h):
    p = pool(5, w, h, 31)
    co = [(m, [4, 0, 2, 2, 1][:c]) for m in METHODS for c in (2, 5)]
    ref = np.stack([collude_ref(p, m, mem) for m, mem in co])
    for off_in in range(4):
        for off_out in range(4):
            assert np.array_equal(dev_collude(p, co, off_in, off_out), ref), (off_in, off_out)


# ---- quality -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SHAPES)
def test_quality_one_original_and_one_per_copy(w, h):
    base = pool(33, w, h, 41)
    copies = pool(33, w, h, 42, True)
    copies[5] = base[0]                                            # equal to the one original: all zero
    copies[7] = base[7]                                            # equal to its own original
    alone = [dev_quality(base[0], copies[i:i + 1])[0] for i in range(33)]
    for n in (1, 3, 33):
        got = dev_quality(base[0], copies[:n])
        assert got == [quality_ref(base[0], c) for c in copies[:n]], n
        assert got == alone[:n], n                                 # each copy alone gives its row of the batch
    assert alone[5] == [0] * 6
    alone = [dev_quality(base[i:i + 1], copies[i:i + 1])[0] for i in range(33)]      # one original per copy (n_base == n == 1)
    for n in (3, 33):
        got = dev_quality(base[:n], copies[:n])
        assert got == [quality_ref(b, c) for b, c in zip(base[:n], copies[:n])], n
        assert got == alone[:n], n
    assert alone[7] == [0] * 6


def test_quality_the_cat(cat):
    rng = np.random.default_rng(43)
    copies = np.clip(cat[None].astype(np.int16) + rng.integers(-9, 10, (3,) + cat.shape), 0, 255).astype(np.uint8)
    copies[1] = cat
    copies = np.concatenate([copies, copies[:2] ^ 1, copies[2:] ^ 128])            # 6 copies: every residue of 278 blocks mod n occurs
    got = dev_quality(cat, copies)
    assert got == [quality_ref(cat, c) for c in copies] and got[1] == [0] * 6
    assert got == [dev_quality(cat, copies[i:i + 1])[0] for i in range(6)]          # each copy alone, more than one block
    bases = copies[::-1].copy()
    got = dev_quality(bases, copies)
    assert got == [quality_ref(b, c) for b, c in zip(bases, copies)]
    assert got == [dev_quality(bases[i:i + 1], copies[i:i + 1])[0] for i in range(6)]


@pytest.mark.parametrize("w,h", [(33, 5), (70, 40)])
def test_quality_at_every_byte_offset(w, h):
    base, copies = pool(3, w, h, 51), pool(3, w, h, 52)
    one = [quality_ref(base[0], c) for c in copies]
    each = [quality_ref(b, c) for b, c in zip(base, copies)]
    for off_base in range(4):
        for off_copies in range(4):
            assert dev_quality(base[0], copies, off_base, off_copies) == one, (off_base, off_copies)
            assert dev_quality(base, copies, off_base, off_copies) == each, (off_base, off_copies)


def test_quality_sums_beyond_32_bits():
    w, h = 2048, 1100
    black, white = np.zeros((h, w, 3), np.uint8), np.full((1, h, w, 3), 255, np.uint8)
    sse = 255 * 255 * w * h
    assert sse > 2 ** 32
    assert dev_quality(black, white) == [[sse, sse, sse, sse, 3 * w * h, 255]]        # the luma of white is 255
    assert dev_quality(white[0], white) == [[0] * 6]


# ---- status codes -------------------------------------------------------------------------------------------------------------
def test_quality_status_codes():
    q, h = lib().ssw_quality_rgb8, ctx().handle
    p = pool(3, 8, 4, 61)
    b, c, s = Dev(p[0]), Dev(p), Dev(3 * 48)
    untouched = lambda: np.all(s.host(np.uint8, (3 * 48,)) == SENTINEL)
    assert q(None, b.ptr, 1, c.ptr, 3, 8, 4, s.ptr) == L.SSW_ERR_BAD_ARG
    assert q(h, None, 1, c.ptr, 3, 8, 4, s.ptr) == L.SSW_ERR_BAD_ARG
    assert q(h, b.ptr, 1, None, 3, 8, 4, s.ptr) == L.SSW_ERR_BAD_ARG
    assert q(h, b.ptr, 1, c.ptr, 3, 8, 4, None) == L.SSW_ERR_BAD_ARG
    for n_base in (0, 2, 4):
        assert q(h, b.ptr, n_base, c.ptr, 3, 8, 4, s.ptr) == L.SSW_ERR_BAD_ARG, n_base
    assert q(h, b.ptr, 1, c.ptr, 3, 0, 4, s.ptr) == L.SSW_ERR_BAD_DIMS
    assert q(h, b.ptr, 1, c.ptr, 3, 8, 0, s.ptr) == L.SSW_ERR_BAD_DIMS
    assert q(h, b.ptr, 1, c.ptr, 3, 2 ** 31 + 1, 1, s.ptr) == L.SSW_ERR_BAD_DIMS       # beyond the kernels' 32-bit coordinates
    assert q(h, b.ptr, 1, c.ptr, 3, 1, 2 ** 31 + 1, s.ptr) == L.SSW_ERR_BAD_DIMS
    assert q(h, b.ptr, 1, c.ptr, 0, 8, 4, s.ptr) == L.SSW_OK
    assert q(h, None, 7, None, 0, 0, 0, None) == L.SSW_OK             # n == 0 comes first
    ctx().synchronize()
    assert untouched()
    for x in (b, c, s):
        x.free()


def test_collude_status_codes():
    f, h = lib().ssw_collude_rgb8, ctx().handle
    p = pool(3, 8, 4, 62)
    d, o = Dev(p), Dev(2 * 96)
    good = coalitions_c([("median", [0, 1, 2]), ("mosaic", [2, 2])])
    untouched = lambda: np.all(o.host(np.uint8, (2 * 96,)) == SENTINEL)
    assert f(None, d.ptr, 3, 8, 4, good, 2, o.ptr) == L.SSW_ERR_BAD_ARG
    assert f(h, None, 3, 8, 4, good, 2, o.ptr) == L.SSW_ERR_BAD_ARG
    assert f(h, d.ptr, 3, 8, 4, None, 2, o.ptr) == L.SSW_ERR_BAD_ARG
    assert f(h, d.ptr, 3, 8, 4, good, 2, None) == L.SSW_ERR_BAD_ARG
    bad = [L.Coalition(1, 0, (C.c_uint32 * 16)()), L.Coalition(1, 17, (C.c_uint32 * 16)()), L.Coalition(1, 2, (C.c_uint32 * 16)(0, 3)),
           L.Coalition(6, 1, (C.c_uint32 * 16)(0)), L.Coalition(0xFFFFFFFF, 1, (C.c_uint32 * 16)(0))]
    for x in bad:                                                      # a bad descriptor behind a good one: nothing is enqueued
        assert f(h, d.ptr, 3, 8, 4, (L.Coalition * 2)(good[0], x), 2, o.ptr) == L.SSW_ERR_BAD_ARG, (x.method, x.count)
    assert f(h, d.ptr, 2, 8, 4, good, 2, o.ptr) == L.SSW_ERR_BAD_ARG       # member 2 of 2 copies
    assert f(h, d.ptr, 3, 0, 4, good, 2, o.ptr) == L.SSW_ERR_BAD_DIMS
    assert f(h, d.ptr, 3, 8, 0, good, 2, o.ptr) == L.SSW_ERR_BAD_DIMS
    assert f(h, d.ptr, 3, 2 ** 31 + 1, 1, good, 2, o.ptr) == L.SSW_ERR_BAD_DIMS      # beyond the kernels' 32-bit coordinates
    assert f(h, d.ptr, 3, 1, 2 ** 31 + 1, good, 2, o.ptr) == L.SSW_ERR_BAD_DIMS
    assert f(h, d.ptr, 3, 8, 4, good, 0, o.ptr) == L.SSW_OK
    assert f(h, None, 0, 0, 0, None, 0, None) == L.SSW_OK
    ctx().synchronize()
    assert untouched()
    assert f(h, d.ptr, 3, 8, 4, good, 2, o.ptr) == L.SSW_OK
    assert np.array_equal(o.host(np.uint8, (2, 4, 8, 3)), np.stack([collude_ref(p, "median", [0, 1, 2]), collude_ref(p, "mosaic", [2, 2])]))
    d.free(); o.free()


# ---- timing -------------------------------------------------------------------------------------------------------------------
def test_both_calls_are_timed_as_convert_with_their_algorithmic_bytes():
    w, h = 70, 40
    fb = w * h * 3
    p = pool(5, w, h, 71)
    co = [("median", [0, 1, 2]), ("mosaic", [4, 3]), ("average", [0] * 16)]
    c = ctx()
    c.enable_timing(True)
    try:
        c.reset_timing()
        dev_quality(p[0], p[1:])
        t = c.timing()
        assert t["convert"]["launches"] >= 1 and t["convert"]["work"] == (1 + 4) * fb + 48 * 4
        c.reset_timing()
        dev_quality(p[:4], p[1:])
        assert c.timing()["convert"]["work"] == (4 + 4) * fb + 48 * 4
        c.reset_timing()
        dev_collude(p, co)
        t = c.timing()
        assert t["convert"]["launches"] >= 1 and t["convert"]["work"] == (4 + 3 + 17) * fb
        assert all(v["launches"] == 0 for k, v in t.items() if k != "convert")
        assert len(t) == 15
    finally:
        c.enable_timing(False)


# ---- the chain on the cat -----------------------------------------------------------------------------------------------------
def test_chain_embed_quality_collude_trace_on_the_device(cat):
    h, w = cat.shape[:2]
    fb, k, n = w * h * 3, 1000, 8
    marks = np.random.default_rng(3).standard_normal((n, k)).astype(np.float32)
    co = [("average", [0, 1]), ("average", [0, 1, 2, 3]), ("median", [0, 1, 2]), ("min", [0, 1, 2, 3]), ("mosaic", [0, 1, 2, 3])]
    cfg = L.Config(L.ORDER_ENERGY, L.OPTION2, 0.1, L.PRECISION_F64)
    img, dm = Dev(cat), Dev(marks)
    copies, stats, forged = Dev(n * fb), Dev(n * 48), Dev(len(co) * fb)
    ext, sims, nex = Dev(len(co) * k * 4), Dev(len(co) * n * 4), Dev(len(co) * 4)
    hd = ctx().handle
    check(lib().ssw_fingerprint_embed_rgb8(hd, C.byref(cfg), img.ptr, w, h, dm.ptr, n, k, copies.ptr, None), "embed")
    check(lib().ssw_quality_rgb8(hd, img.ptr, 1, copies.ptr, n, w, h, stats.ptr), "quality")
    check(lib().ssw_collude_rgb8(hd, copies.ptr, n, w, h, coalitions_c(co), len(co), forged.ptr), "collude")
    check(lib().ssw_fingerprint_trace_rgb8(hd, C.byref(cfg), img.ptr, forged.ptr, len(co), w, h, k, dm.ptr, n, C.c_float(6.0), ext.ptr,
                                           sims.ptr, None, None, nex.ptr), "trace")
    host_copies = copies.host(np.uint8, (n, h, w, 3))
    got_forged = forged.host(np.uint8, (len(co), h, w, 3))
    for i, (m, mem) in enumerate(co):
        assert np.array_equal(got_forged[i], collude_ref(host_copies, m, mem)), m
    q = [[int(v) for v in row] for row in stats.host(np.uint64, (n, 6))]
    assert q == [quality_ref(cat, c) for c in host_copies]
    psnr = 10 * math.log10(255 ** 2 * cat.size / sum(q[0][:3]))
    s, e = sims.host(np.float32, (len(co), n)), nex.host(np.uint32, (len(co),))
    print(f"PSNR of copy 0: {psnr:.2f} dB; weakest colluder / strongest innocent: "
          + ", ".join(f"{m} of {len(mem)}: {s[i, :len(mem)].min():.2f} / {s[i, len(mem):].max():.2f}" for i, (m, mem) in enumerate(co)))
    assert 31.0 < psnr < 32.0
    assert [int(j) for j in np.nonzero(s[0] > 6.0)[0]] == [0, 1] and e[0] == 2
    assert [int(j) for j in np.nonzero(s[1] > 6.0)[0]] == [0, 1, 2, 3] and e[1] == 4
    for x in (img, dm, copies, stats, forged, ext, sims, nex):
        x.free()


def same(a, b):
    return a == b or (a != a and b != b)


def test_strength_report_equals_its_public_pieces(cat):
    alphas, n, k, sizes = [0.05, 0.1], 8, 1000, (2, 4)
    c = ctx()
    c.transfer_stats(reset=True)
    rows = api.strength_report(cat, alphas, seed=3, ctx=c)
    moved = c.transfer_stats(reset=True)
    # the original and the marks went up, statistics and similarities came down: no marked frame crossed PCIe
    assert cat.nbytes <= moved["h2d_bytes"] < 1.1 * cat.nbytes and 0 < moved["d2h_bytes"] < cat.nbytes // 100, moved
    marks = np.random.default_rng(3).standard_normal((n, k)).astype(np.float32)
    plan = [(m, s) for m in METHODS for s in sizes]
    assert [r.alpha for r in rows] == alphas
    for r in rows:
        copies = api.Writer(cat, api.WriteConfig(insertion=api.Insertion.Option2(r.alpha)), c).mark_copies_rgb8(list(marks))
        forged = api.collude(copies, [(m, range(s)) for m, s in plan], c)
        quality = api.quality(cat, copies, c)
        traced = api.trace_many(cat, forged, list(marks), threshold=6.0, config=api.ReadConfig(extraction=api.Extraction.Option2(r.alpha)), ctx=c)
        assert r.quality == quality and len(quality) == n
        assert [(x.method, x.size) for x in r.collusions] == plan
        for i, x in enumerate(r.collusions):
            sims = traced.sims[i]
            assert same(x.weakest_colluder, float(sims[:x.size].min())) and same(x.strongest_innocent, float(sims[x.size:].max())), (r.alpha, x)
            assert x.found == int((sims[:x.size] > np.float32(6.0)).sum()) and x.accused == int((sims[x.size:] > np.float32(6.0)).sum())
            assert r.collusion(x.method, x.size) is x
        for f, (m, s) in zip(forged, plan):
            assert np.array_equal(f, collude_ref(copies, m, range(s))), (m, s)
    strong = rows[1]
    assert strong.collusion("average", 2).found == 2 and strong.collusion("average", 4).found == 4
    assert all(x.accused == 0 for x in strong.collusions if x.method == "average")
    assert rows[0].quality[0].psnr > rows[1].quality[0].psnr              # a weaker mark is less visible
    # no coalitions: the quality alone; one copy: nobody is innocent
    only = api.strength_report(cat[:64, :64], [0.1], k=100, copies=2, sizes=(), seed=1, ctx=c)
    assert only[0].collusions == [] and len(only[0].quality) == 2
    lone = api.strength_report(cat[:64, :64], [0.1], k=100, copies=1, sizes=(1,), methods=("min",), seed=1, ctx=c)
    assert math.isnan(lone[0].collusions[0].strongest_innocent) and lone[0].collusions[0].accused == 0


def test_cli_strength_prints_the_report(cat, tmp_path, capsys):
    from PIL import Image
    path = str(tmp_path / "cat.png")
    Image.fromarray(cat).save(path)
    assert cli.main(["strength", path, "--alpha", "0.1", "--copies", "4", "--collude", "2", "--method", "average", "min"]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == "-" and lines[1] == "  Alpha: 0.1" and re.fullmatch(r"  PSNR: 3\d\.\d\d \.\. 3\d\.\d\d dB over 4 copies \(largest byte difference \d+\)", lines[2])
    assert lines[3].startswith("  average of 2: found 2/2, weakest colluder ") and ", strongest innocent " in lines[3]
    assert lines[4].startswith("  min of 2: found ") and len(lines) == 5
    assert cli.main(["strength", path, "--alpha", "0.1", "--copies", "2", "--collude", "2", "--method", "max", "-n", "100", "--json"]) == 0
    import json
    doc = json.loads(capsys.readouterr().out)
    assert doc[0]["alpha"] == 0.1 and len(doc[0]["copies"]) == 2 and doc[0]["collusions"][0]["strongest_innocent"] is None
