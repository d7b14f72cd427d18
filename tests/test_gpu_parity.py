"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on identical inputs.

Bars (BASELINE.json north star):
  * integer / index work and un-fused f32 arithmetic (yiq, ordering, embed, extract Option1/2,
    similarity): bit-exact.
  * DCT, f64 ("canonical") precision: >= 99.9 % of coefficients bit-identical to the oracle's
    correctly rounded transform, the rest within 1 ulp-scale (2e-7 of the plane's AC max).
  * DCT, f32 MFMA precision: <= 1e-6 of the plane's largest coefficient (the DC term; measured
    <= 3.3e-7.  The reference's own tests use 1e-4 abs on inputs whose DC is 12..47, i.e. ~2e-6).
  * extracted marks: per element |d_i| <= 1e-5 * max(1, |ref_i|) (canonical; _ext_within_1e5); f32 precision: median <= 1e-5, max <= 2e-3
    (an f32 FFT such as rustdct's sits at median 1e-6 / max 1.6e-4 from the exact transform, see
    DESIGN.md "Numerics"); similarity delta < 1e-4 in both.
"""
import json
import os

import numpy as np
import pytest

import gpu_util as G
from conftest import f32_to_u8, u8_to_f32
from oracle import oracle as O
from spread_spectrum_watermarking_amd import _lib as L
import spread_spectrum_watermarking_amd as wm

pytestmark = pytest.mark.gpu

F32, F64 = L.PRECISION_F32, L.PRECISION_F64
# precisions of the folded paths: f64 only (SSW_PRECISION_F32 runs the dense kernels: covered by the known-answer and
# single_simple tests below)
PRECISIONS = [F64]


_ext_within_1e5 = G.ext_within_1e5


def ac_max(plane):
    return np.abs(np.asarray(plane, np.float64).reshape(-1)[1:]).max()


# ---- yiq ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (5, 5), (3, 7), (33, 17), (444, 640), (270, 480)])
def test_rgb_to_yiq_bit_exact(shape):
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    rgb = rng.random(shape + (3,)).astype(np.float32)
    y, i, q = G.rgb_to_yiq(rgb)
    ry, ri, rq = O.rgb_to_yiq(rgb)
    assert np.array_equal(y[0], ry) and np.array_equal(i[0], ri) and np.array_equal(q[0], rq)
    y_only = G.rgb_to_yiq(rgb, with_iq=False)[0]
    assert np.array_equal(y_only[0], ry)


@pytest.mark.parametrize("shape", [(1, 1), (5, 5), (3, 7), (33, 17), (444, 640)])
def test_yiq_to_rgb_bit_exact_and_clamped(shape):
    rng = np.random.default_rng(11)
    y = rng.random(shape).astype(np.float32)
    i = (rng.random(shape).astype(np.float32) - 0.5) * 1.4      # drives some pixels out of gamut
    q = (rng.random(shape).astype(np.float32) - 0.5) * 1.2
    got = G.yiq_to_rgb(y, i, q)[0]
    ref = O.yiq_to_rgb(y, i, q)
    assert np.array_equal(got, ref)
    assert got.min() >= 0.0 and got.max() <= 1.0
    if y.size >= 100:
        assert (got == 0.0).any() and (got == 1.0).any()


def test_yiq_known_answers(known_answers):
    ka = known_answers["yiq_triples"]
    for p in ka["pairs"]:
        rgb = np.array(p["rgb"], np.float32).reshape(1, 1, 3)
        y, i, q = G.rgb_to_yiq(rgb)
        assert np.abs(np.array([y[0, 0, 0], i[0, 0, 0], q[0, 0, 0]]) - p["yiq"]).max() <= ka["tol"]
        back = G.yiq_to_rgb(y[0], i[0], q[0])
        assert np.abs(back.reshape(3) - p["rgb"]).max() <= ka["tol"]


# ---- dct ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [F32, F64])
@pytest.mark.parametrize("case", ["dct2d_almost_identity", "dct2d_no_ones", "dct2d_larger", "dct2d_ortho_4x3"])
def test_dct_reference_known_answers(known_answers, precision, case):
    """The reference's own scipy-derived goldens (src/dct2d.rs:268-524), tolerance 1e-4 abs."""
    ka = known_answers[case]
    x = np.array(ka["input"], np.float32).reshape(ka["h"], ka["w"])
    if "dct2" in ka:
        c = G.dct2d(x, L.DCT2, precision)
        assert np.abs(c.ravel() - ka["dct2"]).max() <= ka["tol"]
        back = G.dct2d(c, L.DCT3, precision)
        assert np.abs(back - x).max() <= ka["tol"]
    if "dct2_orthogonal" in ka:
        c = G.dct2d(x, L.DCT2_ORTHOGONAL, precision)
        assert np.abs(c.ravel() - ka["dct2_orthogonal"]).max() <= ka["tol"]


SHAPES = [(1, 1), (1, 7), (7, 1), (3, 3), (5, 4), (4, 5), (16, 24), (37, 74), (135, 240), (130, 129),
          (444, 640), (256, 256), (300, 128)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dct_type", [L.DCT2, L.DCT2_ORTHOGONAL, L.DCT3])
def test_dct_canonical_matches_oracle_bits(shape, dct_type):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    x = rng.random(shape).astype(np.float32)
    if dct_type == L.DCT3:
        x = O.dct2d(x, O.DCT2)                      # realistic coefficient plane as input
    ref = O.dct2d(x, dct_type, O.BACKEND_F64)
    got = G.dct2d(x, dct_type, F64)
    scale = max(ac_max(ref) if ref.size > 1 else abs(float(ref.ravel()[0])), 1e-30)
    assert np.abs(got.astype(np.float64) - ref).max() <= 2e-7 * scale
    if ref.size >= 64:
        assert np.mean(got == ref) >= 0.999


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dct_type", [L.DCT2, L.DCT2_ORTHOGONAL, L.DCT3])
def test_dct_f32_mfma_within_tolerance(shape, dct_type):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    x = rng.random(shape).astype(np.float32)
    if dct_type == L.DCT3:
        x = O.dct2d(x, O.DCT2)
    ref = O.dct2d(x, dct_type, O.BACKEND_F64)
    got = G.dct2d(x, dct_type, F32)
    scale = max(float(np.abs(ref).max()), 1e-30)     # the DC term for DCT2; ~1 for DCT3 (pixel domain)
    # forward: measured <= 3.3e-7 of the DC term; inverse: <= 1.3e-6 of the pixel range (an 8-bit step is 3.9e-3)
    assert np.abs(got.astype(np.float64) - ref).max() <= (4e-6 if dct_type == L.DCT3 else 1e-6) * scale


@pytest.mark.parametrize("shape", [(16, 16), (64, 128), (72, 136), (200, 328), (1080, 1920)])
@pytest.mark.parametrize("dct_type", [L.DCT2, L.DCT2_ORTHOGONAL, L.DCT3])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_dct_folded_equals_dense(shape, dct_type, precision):
    """The even/odd-folded GEMMs (default where W%8 == 0 / H%8 == 0) against the dense ones."""
    rng = np.random.default_rng(shape[0] + shape[1])
    x = rng.random((2,) + shape).astype(np.float32)
    if dct_type == L.DCT3:
        x = np.stack([O.dct2d(p, O.DCT2) for p in x])
    folded = G.dct2d(x, dct_type, precision)
    G.ctx().set_dct_folding(False)
    try:
        dense = G.dct2d(x, dct_type, precision)
    finally:
        G.ctx().set_dct_folding(True)
    ref = np.stack([O.dct2d(p, dct_type) for p in x])
    # both are the correctly rounded transform
    assert np.mean(folded == ref) >= 0.999 and np.mean(dense == ref) >= 0.999
    assert np.mean(folded == dense) >= 0.999
    assert np.abs(folded.astype(np.float64) - ref).max() <= 2e-7 * max(ac_max(ref), 1.0)


@pytest.mark.parametrize("shape", [(16, 16), (24, 40), (40, 128), (72, 136), (136, 72), (200, 328), (264, 8),
                                   (64, 64), (80, 208), (208, 80), (144, 1040), (72, 128), (40, 160), (1080, 1920),
                                   (128, 256), (160, 192), (288, 136), (256, 128)])
@pytest.mark.parametrize("dct_type", [L.DCT2, L.DCT2_ORTHOGONAL, L.DCT3])
@pytest.mark.parametrize("level", [3, 4, 6])
def test_dct_operand_ready_path_matches(shape, dct_type, level):
    """Pre-folded f64 operand planes + VALU-free GEMM loop (folding level 3; level 4 folds the even
    half once more wherever the axis length is a multiple of 16; level 6 a third time on forward row
    passes whose length is a multiple of 32 -- the default, 5, does that from 3072 columns): same exact operands and f64
    products as the default path, only the summation order differs, so the rounded result
    must agree with it and with the oracle."""
    rng = np.random.default_rng(shape[0] * 5 + shape[1])
    x = rng.random((3,) + shape).astype(np.float32)
    if dct_type == L.DCT3:
        x = np.stack([O.dct2d(p, O.DCT2) for p in x])
    one = G.dct2d(x, dct_type, F64)
    G.ctx().set_dct_folding(level)
    try:
        three = G.dct2d(x, dct_type, F64)
    finally:
        G.ctx().set_dct_folding(True)
    ref = np.stack([O.dct2d(p, dct_type) for p in x])
    assert np.mean(three == one) >= 0.9999 and np.mean(three == ref) >= 0.998
    assert np.abs(three.astype(np.float64) - ref).max() <= 2e-7 * max(ac_max(ref), 1.0)


# (H, W): rows deep forward and inverse (W % 128), forward only (W % 64), first level only (W % 8); columns deep (H % 16,
# >= 256) or first level only (H % 8, or short); plus shapes the split does not take at all
ODD_SPLIT_SHAPES = [(256, 512), (272, 384), (264, 320), (136, 200), (512, 256), (304, 1024), (1080, 1920), (72, 136)]
# deep columns behind deep rows whose length 128 does not divide: the forward column pre-pass reads a class-major plane of ONE
# tile (csrc/dct_pair_prep.hip: pair_prep16_cols_onetile_kernel).  16 whole units of rows; 17 units (a partial store quad and
# the planes' padding up to their k-blocks); a row pass at level 2 (the sixteen-class order of the plane)
ONE_TILE_SHAPES = [(256, 320), (272, 320), (256, 1344)]


def test_one_tile_shapes_take_the_one_tile_column_prepass():
    """What makes ONE_TILE_SHAPES cover that kernel: a class-major plane (deep rows) whose width 128 does not divide, read by
    deep columns that are not at level 2 (those are the staged kernels' and need 128-column tiles)."""
    for h, w in ONE_TILE_SHAPES:
        p = G.ctx().transform_plan(3, w, h)
        assert w % 128 != 0 and p["class_major"] and p["rows_deep"] and p["cols_deep"] and not p["cols_level2"], (h, w, p)
    assert G.ctx().transform_plan(3, 1344, 256)["rows_level2"] and not G.ctx().transform_plan(3, 320, 256)["rows_level2"]


@pytest.mark.parametrize("shape", ODD_SPLIT_SHAPES + ONE_TILE_SHAPES)
@pytest.mark.parametrize("dct_type", [L.DCT2, L.DCT2_ORTHOGONAL, L.DCT3])
def test_odd_split_matches_exact_operands(shape, dct_type):
    """ssw_ctx_set_odd_split: the odd halves as rotated quarter-length cosine + sine pairs (default; "deep" pre-passes
    where the lengths allow) against the same transform with every operand an exact folded sum.  Both are the f64-
    accurate transform rounded once to f32: they agree except where that rounding sat on a tie, and both match the
    oracle like test_dct_operand_ready_path_matches."""
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    x = rng.random((3,) + shape).astype(np.float32)
    if dct_type == L.DCT3:
        x = np.stack([O.dct2d(p, O.DCT2) for p in x])
    split = G.dct2d(x, dct_type, F64)
    G.ctx().set_odd_split(False)
    try:
        exact = G.dct2d(x, dct_type, F64)
    finally:
        G.ctx().set_odd_split(True)
    ref = np.stack([O.dct2d(p, dct_type) for p in x])
    assert np.mean(split == exact) >= 0.9995
    assert np.mean(split == ref) >= 0.998 and np.mean(exact == ref) >= 0.998
    assert np.abs(split.astype(np.float64) - ref).max() <= 2e-7 * max(ac_max(ref), 1.0)
    # and back: the round trip through both directions of the split transform returns the input (dct2d.rs:213-217)
    if dct_type == L.DCT2:
        back = G.dct2d(split, L.DCT3, F64)
        assert np.abs(back - x).max() <= 4e-7


@pytest.mark.parametrize("precision", PRECISIONS)
def test_dct_batched_equals_single(precision):
    rng = np.random.default_rng(2)
    x = rng.random((5, 72, 136)).astype(np.float32)
    G.ctx().set_chunk_frames(2)                      # exercise the chunk loop incl. a ragged last chunk
    try:
        batched = G.dct2d(x, L.DCT2, precision)
    finally:
        G.ctx().set_chunk_frames(0)                      # back to automatic
    for f in range(5):
        assert np.array_equal(batched[f], G.dct2d(x[f], L.DCT2, precision))


@pytest.mark.parametrize("precision", PRECISIONS)
def test_dct_linearity_and_roundtrip_1080p(precision):
    """Size-independent properties at a BASELINE.json frame size (1920x1080)."""
    rgb = G.synth(3, 0, 2, 1920, 1080)
    a = O.rgb_to_yiq(rgb[0])[0]
    b = O.rgb_to_yiq(rgb[1])[0]
    ca, cb = G.dct2d(a, L.DCT2, precision), G.dct2d(b, L.DCT2, precision)
    s = (a.astype(np.float64) * 0.5 + b.astype(np.float64) * 0.25).astype(np.float32)
    cs = G.dct2d(s, L.DCT2, precision)
    lin = ca.astype(np.float64) * 0.5 + cb.astype(np.float64) * 0.25
    assert np.abs(cs - lin).max() <= 1e-6 * np.abs(lin).max()      # `s` itself is rounded to f32
    assert abs(float(ca[0, 0]) - 4.0 * float(a.astype(np.float64).sum())) <= 1e-6 * abs(float(ca[0, 0]))   # DC = 4 sum
    back = G.dct2d(ca, L.DCT3, precision)
    assert np.abs(back - a).max() <= 2e-7


# ---- ordering ----------------------------------------------------------------------------------
ORDERINGS = [L.ORDER_ENERGY, L.ORDER_ENERGY_ORTHOGONAL, L.ORDER_LEGACY]


def test_indices_known_answer(known_answers):
    ka = known_answers["indices"]
    c = np.array(ka["coefficients"], np.float32).reshape(1, 6)
    for k in range(1, 6):
        assert G.topk(c, k).tolist() == ka["expected"][:k]


@pytest.mark.parametrize("ordering", ORDERINGS)
def test_topk_matches_oracle_with_ties(ordering):
    rng = np.random.default_rng(5)
    c = rng.integers(-9, 10, size=(3, 40, 56)).astype(np.float32)      # many exact ties, +/- pairs, zeros
    for k in (1, 2, 17, 100, 1000, 40 * 56 - 1):
        got = G.topk(c, k, ordering)
        for f in range(3):
            assert np.array_equal(got[f], O.indices(c[f], ordering, k=k)), (ordering, k, f)


@pytest.mark.parametrize("ordering", ORDERINGS)
def test_topk_matches_oracle_on_real_coefficients(ordering, cat_images):
    y = O.rgb_to_yiq(u8_to_f32(cat_images["cat"]))[0]
    c = O.dct2d(y)
    ctx = G.ctx()
    ctx.reset_timing()
    for k in (1000, 4096, 10000):          # 4096 / 10000: the coarser sample strides and the counting-sort finish
        assert np.array_equal(G.topk(c, k, ordering), O.indices(c, ordering, k=k))
    st = ctx.select_stats()
    assert st["frames"] == 3 and st["exact_fallback_frames"] == 0, st     # an image never takes the whole-plane fallback


def test_exact_fallback_of_the_selection_is_counted():
    """A constant plane larger than the candidate buffer (every key equal: the sampled threshold keeps everything) takes
    the exact whole-plane select in the finish kernel -- same result as the oracle's stable sort -- and
    ssw_ctx_get_select_stats counts it.  Own context: the candidate buffer of a fresh one holds 65 536 keys."""
    import ctypes as C
    import spread_spectrum_watermarking_amd as wm
    from spread_spectrum_watermarking_amd.api import check
    ctx = wm.Context(0)
    c = np.full((2, 256, 320), 0.25, np.float32)       # 81 919 equal keys
    c[1] = np.random.default_rng(3).standard_normal((256, 320)).astype(np.float32)
    d, idx = ctx.to_device(c), ctx.alloc(2 * 300 * 4)
    check(ctx._lib.ssw_topk_indices(ctx.handle, d.ptr, 2, 320, 256, L.ORDER_ENERGY, 300, idx.ptr), "ssw_topk_indices")
    got = idx.to_host(np.uint32, (2, 300))
    for f in range(2):
        assert np.array_equal(got[f], O.indices(c[f], k=300))
    st = ctx.select_stats()
    assert st == {"frames": 2, "exact_fallback_frames": 1}, st
    ctx.reset_timing()
    assert ctx.select_stats() == {"frames": 0, "exact_fallback_frames": 0}
    d.free(); idx.free(); ctx.close()


@pytest.mark.parametrize("ordering", ORDERINGS)
def test_full_index_list_matches_oracle(ordering, cat_images):
    """Reader::indices() (algorithm.rs:506-508): the whole W*H-1 list, beyond the in-LDS top-k limit."""
    y = O.rgb_to_yiq(u8_to_f32(cat_images["cat"]))[0]
    c = O.dct2d(y)[:200, :320].copy()                                  # 64 000 coefficients
    c[5, 7] = c[9, 11]; c[100, 3] = -c[9, 11]                          # exact energy ties
    full = O.indices(c, ordering)
    for k in (20000, c.size - 1):
        assert np.array_equal(G.topk(c, k, ordering), full[:k])


def test_reader_indices_full_list_and_long_mark(cat_images):
    rgb = O.synth_frame(11, 0, 256, 144)
    reader = wm.Reader.base(rgb)
    coef = reader.coefficients().reshape(144, 256)
    full = reader.indices()                                            # k = None -> all n-1
    assert full.shape == (256 * 144 - 1,)
    assert np.array_equal(full, O.indices(coef))
    assert np.array_equal(reader.indices(1000), full[:1000])           # cached prefix
    mark = np.random.default_rng(3).standard_normal(20000).astype(np.float32)   # > 16384 coefficients
    w = wm.Writer(rgb)
    c0 = w.coefficient_image()
    w.embed([mark])
    assert np.array_equal(w.coefficient_image(), O.embed(c0, O.indices(c0, k=20000), [mark]))


def test_long_index_lists_at_full_hd():
    """Beyond the in-LDS top-k limit (16384 entries) at a BASELINE frame size: Reader::indices(k) and a 20000-long mark
    on a 1920x1080 frame take the full device sort (sort_full.hip) -- same list as the oracle's stable sort."""
    rgb = O.synth_frame(21, 2, 1920, 1080)
    reader = wm.Reader.base(rgb)
    coef = reader.coefficients().reshape(1080, 1920)
    ref = O.indices(coef, k=40000)
    assert np.array_equal(reader.indices(40000), ref)
    assert np.array_equal(reader.indices(16385), ref[:16385])
    mark = np.random.default_rng(8).standard_normal(20000).astype(np.float32)
    marks = np.stack([mark, mark[::-1].copy()])
    frames = np.stack([rgb, O.synth_frame(21, 3, 1920, 1080)])
    res = G.batch_embed(frames, marks, want_idx=True)                  # batch path, two frames, k > 16384
    assert np.array_equal(res["idx"][0], ref[:20000].astype(np.uint32))
    ext, sims = G.batch_extract(frames, res["rgb"], 20000, marks)
    assert np.all(sims > 0.97 * np.linalg.norm(marks, axis=1)) and np.abs(ext - marks).max() < 0.1


def test_full_index_list_at_4k_and_batched_equals_the_stable_sort():
    """Reader::indices() with no limit on a 3840x2160 frame (8.3 M entries, src/algorithm.rs:200-210, :506-508): the
    library's own batched radix sort (sort_full.hip) against the oracle's stable sort, and three frames of different
    content sorted in one call (ssw_topk_indices with k beyond the top-k limit) against one-at-a-time results."""
    rgb = G.synth(9, 4, 1, 3840, 2160)[0]
    reader = wm.Reader.base(rgb)
    coef = reader.coefficients().reshape(2160, 3840)
    full = reader.indices()
    assert full.shape == (3840 * 2160 - 1,)
    assert np.array_equal(full, O.indices(coef))
    planes = np.stack([O.dct2d(O.rgb_to_yiq(O.synth_frame(5, f, 320, 200))[0]) for f in range(3)])
    planes[1, 7, 9] = planes[1, 100, 50] = -planes[1, 3, 3]            # exact energy ties
    k = 320 * 200 - 1
    got = G.topk(planes, k)
    for f in range(3):
        assert np.array_equal(got[f], O.indices(planes[f]))
        assert np.array_equal(got[f], G.topk(planes[f], k))


def test_topk_degenerate_planes():
    z = np.zeros((2, 9, 13), np.float32)                               # every key ties: index order
    assert np.array_equal(G.topk(z, 50)[0], np.arange(1, 51))
    z[1, 0, 0] = 1e9                                                   # a huge DC must be ignored
    z[1, 3, 4] = -2.0
    assert G.topk(z, 3)[1].tolist() == [3 * 13 + 4, 1, 2]
    one = np.array([[5.0, 3.0]], np.float32)                           # n-1 == 1
    assert G.topk(one, 1).tolist() == [1]


def test_topk_rejects_bad_k():
    c = np.zeros((4, 4), np.float32)
    with pytest.raises(wm.SswError) as e:
        G.topk(c, 16)
    assert e.value.status == L.SSW_ERR_K_TOO_LARGE


# ---- embed / extract / similarity -----------------------------------------------------------------
def test_embedder_known_answers(known_answers):
    f, a = np.float32, np.float32(0.1)
    ka = known_answers["embedder_single"]
    c = np.array(ka["coefficients"], np.float32).reshape(1, 6)
    idx = G.topk(c, 3).reshape(1, 3)
    emb = G.embed(c, idx, np.array(ka["mark"], np.float32).reshape(1, 1, 3))
    expected = np.array([f(-3), f(5) * (f(1) + f(1) * a), f(-8) * (f(1) + f(1) * a), f(7) * (f(1) - f(0.5) * a), f(1), f(2)], np.float32)
    assert np.array_equal(emb[0], expected)                           # assert_eq! in the reference
    ext = G.extract(c, emb, idx)
    assert np.abs(ext[0] - np.array(ka["mark"], np.float32)).max() < ka["extract_tol"]
    ka = known_answers["embedder_single_and_zero"]
    emb2 = G.embed(c, idx, np.array(ka["marks"], np.float32).reshape(1, 2, 3))
    assert np.array_equal(emb2[0], expected)
    ka = known_answers["embedder_multiple"]
    marks = np.array(ka["marks"], np.float32).reshape(1, 2, 3)
    emb3 = G.embed(c, idx, marks)
    assert np.array_equal(emb3[0], O.embed(c[0], idx[0], list(marks[0])))


@pytest.mark.parametrize("method", [L.OPTION1, L.OPTION2, L.OPTION3])
@pytest.mark.parametrize("n_marks", [1, 3])
def test_embed_extract_match_oracle(method, n_marks):
    rng = np.random.default_rng(method * 10 + n_marks)
    n, plane, k = 3, 5000, 700
    coef = (rng.standard_normal((n, plane)) * 100).astype(np.float32)
    idx = np.stack([rng.permutation(np.arange(1, plane))[:k] for _ in range(n)]).astype(np.uint32)
    marks = rng.standard_normal((n, n_marks, k)).astype(np.float32)
    emb = G.embed(coef, idx, marks, method, 0.1)
    ext = G.extract(coef, emb, idx, method, 0.1)
    for f in range(n):
        ref = O.embed(coef[f], idx[f], list(marks[f]), method, 0.1)
        ref_ext = O.extract(coef[f], ref, idx[f], k, method, 0.1)
        if method == L.OPTION3:      # expf / logf: libm vs ocml, <= 2 ulp
            assert np.abs(emb[f] - ref).max() <= 3e-7 * np.abs(ref).max()
            assert np.abs(ext[f] - ref_ext).max() <= 1e-4
        else:
            assert np.array_equal(emb[f], ref)
            assert np.array_equal(G.extract(coef, ref[None].repeat(n, 0), idx, method, 0.1)[f], ref_ext)


@pytest.mark.parametrize("k", [1, 3, 1000, 1024, 1025, 10000])
def test_similarity_bit_exact(k):
    rng = np.random.default_rng(k)
    e = rng.standard_normal((4, k)).astype(np.float32)
    m = rng.standard_normal((4, k)).astype(np.float32)
    got = G.similarity_batch(e, m)
    for f in range(4):
        assert got[f] == np.float32(O.similarity(e[f], m[f]))


@pytest.mark.parametrize("shape", [(3, 5, 1000), (130, 257, 1000), (16, 200, 10000), (7, 9, 33)])
def test_similarity_matrix_matches_pairwise_tester(shape):
    """One extraction against many stored marks (README.md:62 of the reference) as an MFMA GEMM:
    every entry equals Tester::similarity of that pair to 1e-4 relative (fma-chain vs sequential sums)."""
    b, m, k = shape
    rng = np.random.default_rng(b * m)
    marks_db = rng.standard_normal((m, k)).astype(np.float32)
    ext = rng.standard_normal((b, k)).astype(np.float32)
    ext[0] = marks_db[m // 2] * 0.97 + 0.05 * ext[0]                  # one genuine match
    got = G.similarity_matrix(ext, marks_db)
    ref = np.array([[O.similarity(e, mk) for mk in marks_db] for e in ext], np.float32)
    assert np.abs(got - ref).max() <= 1e-4 * max(1.0, np.abs(ref).max())
    assert got[0].argmax() == m // 2 and got[0, m // 2] > 0.9 * np.sqrt(k)


def test_extract_error_behaviour():
    c = np.zeros((1, 6), np.float32)
    with pytest.raises(wm.SswError) as e:
        G.extract(c, c, np.zeros((1, 6), np.uint32))                   # k >= n (algorithm.rs:553-555)
    assert e.value.status == L.SSW_ERR_K_TOO_LARGE


# ---- crate surface: Writer / Reader / Tester ------------------------------------------------------
@pytest.mark.parametrize("precision", [F32, F64])
def test_single_simple_flow(known_answers, marks, cat_images, precision):
    """tests/single_simple.rs through the GPU path (self-consistent decode)."""
    th = known_answers["single_simple_thresholds"]
    cat = cat_images["cat"]
    mark = marks["seed_1"]
    res = wm.Writer(cat, wm.WriteConfig(precision=precision)).mark([mark])
    img8 = f32_to_u8(res)
    reader = wm.Reader.base(cat, wm.ReadConfig(precision=precision))
    derived = wm.Reader.derived(img8, precision=precision)
    ext = reader.extract(derived, np.zeros(1000, np.float32))
    assert np.abs(ext - mark).max() < 0.16
    assert np.abs(ext - mark).mean() < th["mean_err"]
    tester = wm.Tester(ext)
    assert tester.similarity(mark).exceeds_sigma(th["sim_gt"])
    assert not tester.similarity(marks["seed_baaaaaad"]).exceeds_sigma(th["random_sim_lt"])
    # oracle on the same inputs
    o_img8 = f32_to_u8(O.embed_frame(u8_to_f32(cat), mark))
    o_ext, o_sim = O.extract_frame(u8_to_f32(cat), u8_to_f32(o_img8), mark)
    assert np.mean(img8 == o_img8) > (0.9999 if precision == F64 else 0.999)
    assert abs(tester.similarity(mark).similarity - o_sim) < 2e-2      # 8-bit quantisation noise dominates


def test_reference_png_carries_seed1_mark(marks, cat_images):
    reader = wm.Reader.base(cat_images["cat"])
    ext = reader.extract(wm.Reader.derived(cat_images["watermarked_with_1"]), 1000)
    assert wm.Tester(ext).similarity(marks["seed_1"]).similarity > 15.0
    assert abs(wm.Tester(ext).similarity(marks["seed_2"]).similarity) < 3.0


def test_canonical_pipeline_matches_oracle(marks, cat_images):
    """No 8-bit step: Writer::mark -> Reader::extract -> similarity, canonical precision, vs the oracle."""
    cat = u8_to_f32(cat_images["cat"])
    mark = marks["seed_1"]
    cfgw, cfgr = wm.WriteConfig(precision=F64), wm.ReadConfig(precision=F64)
    writer = wm.Writer(cat, cfgw)
    coef = writer.coefficient_image()
    ref_coef = O.dct2d(O.rgb_to_yiq(cat)[0])
    assert np.mean(coef == ref_coef) > 0.999
    res = writer.mark([mark])
    ref_res = O.embed_frame(cat, mark)
    assert np.abs(res - ref_res).max() <= 2e-7
    assert np.mean(res == ref_res) > 0.99
    reader = wm.Reader.base(cat, cfgr)
    assert np.array_equal(reader.indices(1000), O.indices(ref_coef, k=1000))
    ext = reader.extract(wm.Reader.derived(res, precision=F64), 1000)
    ref_ext, ref_sim = O.extract_frame(cat, ref_res, mark)
    assert _ext_within_1e5(ext, ref_ext)
    assert abs(wm.Tester(ext).similarity(mark).similarity - ref_sim) < 1e-4


def test_f32_pipeline_matches_oracle_tie_aware(marks, cat_images):
    """f32 MFMA precision: ordering checked tie-aware against oracle keys, values keyed by index."""
    cat = u8_to_f32(cat_images["cat"])
    mark = marks["seed_1"]
    writer = wm.Writer(cat, wm.WriteConfig(precision=F32))
    coef = writer.coefficient_image()
    ref_coef = O.dct2d(O.rgb_to_yiq(cat)[0])
    assert np.abs(coef - ref_coef).max() <= 1e-6 * np.abs(ref_coef).max()
    reader = wm.Reader.base(cat, wm.ReadConfig(precision=F32))
    idx = reader.indices(1000).astype(np.int64)
    assert len(set(idx.tolist())) == 1000 and idx.min() >= 1
    # (i) the GPU's own coefficients give exactly this order
    assert np.array_equal(idx, O.indices(coef, k=1000))
    # (ii) against the oracle's energies the order is monotone up to the DCT tolerance
    e = ref_coef.reshape(-1).astype(np.float64)[idx] ** 2
    assert np.all(e[1:] <= e[:-1] * (1 + 1e-3))
    # (iii) same index list fed to both sides -> extracted values agree, sims agree
    res = writer.mark([mark])
    ext = reader.extract(wm.Reader.derived(res, precision=F32), 1000)
    ref_res = O.embed(ref_coef, idx.astype(np.uint64), [mark])
    ref_y = O.dct2d(ref_res, O.DCT3)
    yiq = O.rgb_to_yiq(cat)
    ref_rgb = O.yiq_to_rgb(ref_y, yiq[1], yiq[2])
    assert np.abs(res - ref_rgb).max() <= 5e-6
    ref_derived = O.dct2d(O.rgb_to_yiq(ref_rgb)[0])
    ref_ext = O.extract(ref_coef, ref_derived, idx.astype(np.uint64), 1000)
    err = np.abs(ext - ref_ext)
    assert np.median(err) <= 1e-5 and err.max() <= 2e-3
    sim = wm.Tester(ext).similarity(mark).similarity
    assert abs(sim - O.similarity(ref_ext, mark)) < 1e-4 * abs(sim)


def test_writer_reader_error_behaviour(cat_images):
    small = np.random.default_rng(0).random((6, 8, 3)).astype(np.float32)
    w = wm.Writer(small)
    w.result()
    with pytest.raises(wm.SswError) as e:
        w.result()                                                     # `result(self)` consumed it
    assert e.value.status == L.SSW_ERR_CONSUMED
    base = wm.Reader.base(small)
    derived = wm.Reader.derived(small)
    with pytest.raises(wm.SswError) as e:
        derived._reader.extract(derived, 3)                            # unwrap() on a derived reader
    assert e.value.status == L.SSW_ERR_NOT_BASE
    with pytest.raises(wm.SswError) as e:
        derived._reader.indices(3)
    assert e.value.status == L.SSW_ERR_NOT_BASE
    with pytest.raises(wm.SswError) as e:
        base.extract(derived, 48)                                      # k >= coefficients
    assert e.value.status == L.SSW_ERR_K_TOO_LARGE
    other = wm.Reader.derived(np.zeros((6, 9, 3), np.float32))
    with pytest.raises(wm.SswError) as e:
        base.extract(other, 3)                                         # length mismatch
    assert e.value.status == L.SSW_ERR_LENGTH_MISMATCH
    with pytest.raises(wm.SswError) as e:
        wm.Tester(np.zeros(3, np.float32)).similarity(np.zeros(4, np.float32))
    assert e.value.status == L.SSW_ERR_LENGTH_MISMATCH
    with pytest.raises(wm.SswError) as e:
        wm.Writer(small, wm.WriteConfig(insertion=wm.Insertion.Custom(lambda i, o, m: o)))
    assert e.value.status == L.SSW_ERR_UNSUPPORTED
    with pytest.raises(wm.SswError) as e:
        wm.Reader.base(small, wm.ReadConfig(ordering=wm.OrderingMethod.Custom(lambda *a: 0)))
    assert e.value.status == L.SSW_ERR_UNSUPPORTED


def test_mark_longer_than_coefficients_is_truncated():
    small = np.random.default_rng(1).random((3, 4, 3)).astype(np.float32)     # 12 coefficients, 11 usable
    w = wm.Writer(small, wm.WriteConfig(insertion=wm.Insertion.Option1(0.5)))
    before = w.coefficient_image().reshape(-1)
    w.embed([np.ones(40, np.float32)])
    after = w.coefficient_image().reshape(-1)
    assert after[0] == before[0]
    assert np.array_equal(after[1:], before[1:] + np.float32(0.5))


def test_multiple_marks_ragged_lengths():
    rgb = O.synth_frame(9, 0, 96, 64)
    rng = np.random.default_rng(4)
    m1, m2 = rng.standard_normal(200).astype(np.float32), rng.standard_normal(120).astype(np.float32)
    w = wm.Writer(rgb, wm.WriteConfig(precision=F64))
    c0 = w.coefficient_image()
    w.embed([m1, m2])
    got = w.coefficient_image()
    idx = O.indices(c0, k=200)
    assert np.array_equal(got, O.embed(c0, idx, [m1, m2]))


# ---- batch path + synthetic frames ------------------------------------------------------------------
def test_synth_frames_bit_identical_to_oracle():
    got = G.synth(7, 3, 2, 160, 90)
    for f in range(2):
        assert np.array_equal(got[f], O.synth_frame(7, 3 + f, 160, 90))
    assert got.min() >= 0.0 and got.max() < 1.0


@pytest.mark.parametrize("precision", PRECISIONS)
def test_batch_path_equals_handles_and_oracle(precision):
    n, w, h, k = 5, 192, 108, 300
    rgb = G.synth(2, 0, n, w, h)
    marks = np.random.default_rng(8).standard_normal((n, k)).astype(np.float32)
    cfg = G.default_config(precision)
    G.ctx().set_chunk_frames(2)
    try:
        res = G.batch_embed(rgb, marks, cfg, want_coef=True, want_idx=True)
        ext, sims = G.batch_extract(rgb, res["rgb"], k, marks, cfg)
    finally:
        G.ctx().set_chunk_frames(0)                      # back to automatic
    for f in range(n):
        wr = wm.Writer(rgb[f], wm.WriteConfig(precision=precision))
        assert np.array_equal(res["coef"][f], wr.coefficient_image())
        assert np.array_equal(res["rgb"][f], wr.mark([marks[f]]))
        rd = wm.Reader.base(rgb[f], wm.ReadConfig(precision=precision))
        assert np.array_equal(res["idx"][f], rd.indices(k).astype(np.uint32))
        e1 = rd.extract(wm.Reader.derived(res["rgb"][f], precision=precision), k)
        assert np.array_equal(ext[f], e1)
        assert sims[f] == np.float32(wm.Tester(e1).similarity(marks[f]).similarity)
        assert sims[f] > 0.9 * np.linalg.norm(marks[f])
        o_res = O.embed_frame(rgb[f], marks[f])
        assert np.abs(res["rgb"][f] - o_res).max() <= 2e-7
        o_ext, o_sim = O.extract_frame(rgb[f], o_res, marks[f])
        assert abs(sims[f] - o_sim) < 1e-4 * abs(o_sim) + 1e-4


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("shape", [(80, 208), (144, 1040), (72, 128), (160, 1056), (128, 256)])
@pytest.mark.parametrize("level", [5, 6])
def test_batch_path_fused_colour_prepass_equals_handles(precision, shape, level):
    """Shapes that take the default GEMM strategy (W >= H, W % 16 == 0, H % 8 == 0): the batch entry
    points read the RGB frames in the first operand pre-pass (no f32 Y plane); the handle API converts
    first.  Same arithmetic, so coefficients, indices, marked frames and extraction are bit-identical --
    also from 8-bit frames."""
    h, w = shape
    n, k = 3, 200
    rgb = G.synth(5, 1, n, w, h)
    marks = np.random.default_rng(3).standard_normal((n, k)).astype(np.float32)
    cfg = G.default_config(precision)
    # level 6 = the default strategy without its 3072-column threshold for the third folding level, so that
    # the three-level colour pre-pass is exercised at test sizes (W % 32 == 0 shapes); handles and batch
    # calls use different contexts: set both
    G.ctx().set_dct_folding(level)
    wm.default_context().set_dct_folding(level)
    try:
        _fused_vs_handles(rgb, marks, cfg, precision, n, k)
    finally:
        G.ctx().set_dct_folding(True)
        wm.default_context().set_dct_folding(True)


def _fused_vs_handles(rgb, marks, cfg, precision, n, k):
    res = G.batch_embed(rgb, marks, cfg, want_coef=True, want_idx=True)
    ext, sims = G.batch_extract(rgb, res["rgb"], k, marks, cfg)
    for f in range(n):
        wr = wm.Writer(rgb[f], wm.WriteConfig(precision=precision))
        assert np.array_equal(res["coef"][f], wr.coefficient_image())
        assert np.array_equal(res["rgb"][f], wr.mark([marks[f]]))
        rd = wm.Reader.base(rgb[f], wm.ReadConfig(precision=precision))
        assert np.array_equal(res["idx"][f], rd.indices(k).astype(np.uint32))
        assert np.array_equal(ext[f], rd.extract(wm.Reader.derived(res["rgb"][f], precision=precision), k))
    frames8 = O.f32_to_u8(rgb)
    wm8 = G.batch_embed_rgb8(frames8, marks, cfg)
    assert np.array_equal(wm8, O.f32_to_u8(G.batch_embed(O.u8_to_f32(frames8), marks, cfg)["rgb"]))
    e8, s8 = G.batch_extract_rgb8(frames8, wm8, k, marks, cfg)
    e32, s32 = G.batch_extract(O.u8_to_f32(frames8), O.u8_to_f32(wm8), k, marks, cfg)
    assert np.array_equal(e8, e32) and np.array_equal(s8, s32)


# ---- BASELINE.json sizes and degenerate inputs ---------------------------------------------------
def test_full_hd_pipeline_parity_with_oracle():
    """configs[2] frame size (1920x1080), canonical precision: the whole embed -> extract -> similarity
    path of one frame against the oracle's exact pipeline."""
    w, h, k = 1920, 1080, 1000
    rgb = G.synth(4, 17, 1, w, h)
    assert np.array_equal(rgb[0], O.synth_frame(4, 17, w, h))
    mark = np.random.default_rng(17).standard_normal((1, k)).astype(np.float32)
    res = G.batch_embed(rgb, mark, want_coef=True, want_idx=True)
    ref_coef = O.dct2d(O.rgb_to_yiq(rgb[0])[0])
    assert np.mean(res["coef"][0] == ref_coef) > 0.9995
    assert np.array_equal(res["idx"][0], O.indices(ref_coef, k=k).astype(np.uint32))
    ref_marked = O.embed_frame(rgb[0], mark[0])
    assert np.abs(res["rgb"][0] - ref_marked).max() <= 2e-7 and np.mean(res["rgb"][0] == ref_marked) > 0.999
    ext, sims = G.batch_extract(rgb, res["rgb"], k, mark)
    ref_ext, ref_sim = O.extract_frame(rgb[0], ref_marked, mark[0])
    assert _ext_within_1e5(ext[0], ref_ext)
    assert abs(float(sims[0]) - ref_sim) < 1e-4


def test_4k_size_independent_properties():
    """BASELINE configs[1]/[3] frame size (3840x2160), default strategy: properties that need no CPU
    reference -- inverse(forward(x)) == x to f32 round-off, the operand-ready GEMMs agree with the dense
    ones (folding level 1), embed -> extract recovers the mark, linearity of the transform."""
    w, h, k = 3840, 2160, 1000
    rgb = G.synth(9, 5, 2, w, h)
    y = np.ascontiguousarray(rgb[..., 0] * np.float32(0.3) + rgb[..., 1] * np.float32(0.59))
    c = G.dct2d(y, L.DCT2, F64)
    back = G.dct2d(c, L.DCT3, F64)
    assert np.abs(back - y).max() <= 4e-7
    G.ctx().set_dct_folding(1)
    try:
        c1 = G.dct2d(y, L.DCT2, F64)
    finally:
        G.ctx().set_dct_folding(True)
    assert np.mean(c == c1) >= 0.9999 and np.abs(c - c1).max() <= 2e-7 * np.abs(c1).max()
    lin = G.dct2d(np.float32(0.5) * y[0] + np.float32(0.25) * y[1], L.DCT2, F64)
    assert np.abs(lin - (0.5 * c[0].astype(np.float64) + 0.25 * c[1])).max() <= 4e-7 * np.abs(c).max()
    marks = np.random.default_rng(11).standard_normal((2, k)).astype(np.float32)
    res = G.batch_embed(rgb, marks)
    ext, sims = G.batch_extract(rgb, res["rgb"], k, marks)
    assert np.all(sims > 0.97 * np.linalg.norm(marks, axis=1))
    assert np.abs(ext - marks).max() < 0.05                      # Option2, alpha 0.1: clamp / round-off of the round trip


def _whole_pipeline_vs_oracle(w, h, k, seed, frame):
    """One frame through ssw_batch_embed + ssw_batch_extract (canonical precision, default strategy incl.
    the pruned derived transform) against the oracle's exact pipeline: coefficients, the index list,
    the marked frame, the extracted mark and the similarity."""
    rgb = G.synth(seed, frame, 1, w, h)
    assert np.array_equal(rgb[0], O.synth_frame(seed, frame, w, h))
    mark = np.random.default_rng(seed * 100 + frame).standard_normal((1, k)).astype(np.float32)
    res = G.batch_embed(rgb, mark, want_coef=True, want_idx=True)
    ref_coef = O.dct2d(O.rgb_to_yiq(rgb[0])[0])
    assert np.mean(res["coef"][0] == ref_coef) > 0.9995
    assert np.abs(res["coef"][0].astype(np.float64) - ref_coef).max() <= 2e-7 * ac_max(ref_coef)
    assert np.array_equal(res["idx"][0], O.indices(ref_coef, k=k).astype(np.uint32))
    ref_marked = O.embed_frame(rgb[0], mark[0])
    assert np.abs(res["rgb"][0] - ref_marked).max() <= 2e-7 and np.mean(res["rgb"][0] == ref_marked) > 0.999
    ext, sims = G.batch_extract(rgb, res["rgb"], k, mark)
    ref_ext, ref_sim = O.extract_frame(rgb[0], ref_marked, mark[0])
    assert _ext_within_1e5(ext[0], ref_ext)
    assert abs(float(sims[0]) - ref_sim) < 1e-4
    # the oracle's own marked frame as the derived input: identical inputs on both sides, so extraction is
    # bit-exact wherever the 2 k coefficients it reads are (a canonical-precision coefficient differs from the
    # oracle's by one ulp with probability ~1e-6: allow a handful, each worth <= ulp / alpha in the mark)
    ext_o, sims_o = G.batch_extract(rgb, ref_marked[None], k, mark)
    assert np.mean(ext_o[0] == ref_ext) >= 0.999 and _ext_within_1e5(ext_o[0], ref_ext)
    assert abs(float(sims_o[0]) - ref_sim) < 1e-5 * abs(ref_sim)
    return rgb, mark, res


def test_4k_pipeline_parity_with_oracle():
    """BASELINE configs[1] / configs[3] frame size (3840x2160), k = 1000: the whole embed -> extract ->
    similarity path of one frame against the oracle (the reference flow of algorithm.rs:295-379, :462-562)."""
    _whole_pipeline_vs_oracle(3840, 2160, 1000, 21, 3)


def _frame_vs_oracle(rgb, mark, coef, idx, marked, ext, sim):
    """The bars of _whole_pipeline_vs_oracle on one frame of a batch call's outputs."""
    k = mark.size
    ref_coef = O.dct2d(O.rgb_to_yiq(rgb)[0])
    if coef is not None:
        assert np.mean(coef == ref_coef) > 0.9995
        assert np.abs(coef.astype(np.float64) - ref_coef).max() <= 2e-7 * ac_max(ref_coef)
    assert np.array_equal(idx, O.indices(ref_coef, k=k).astype(np.uint32))
    ref_marked = O.embed_frame(rgb, mark)
    assert np.abs(marked - ref_marked).max() <= 2e-7 and np.mean(marked == ref_marked) > 0.999
    ref_ext, ref_sim = O.extract_frame(rgb, ref_marked, mark)
    assert _ext_within_1e5(ext, ref_ext)
    assert abs(float(sim) - ref_sim) < 1e-4


def test_4k_bench_configuration_equals_handles_and_oracle():
    """The configuration bench.py times (BASELINE configs[3], per-GPU shard) in the shape GPUTEST owns: twenty
    3840x2160 frames in passes of eight, eight and four (set_chunk_frames(8): 17280 lines per pass > merge_max_lines, i.e.
    the unmerged eight-launch passes on 128-line tiles with the fused forward transform, two lanes, the pruned derived
    transform; the ragged last pass of four frames takes the unfused path on 64-line tiles through the same lanes) -- every
    frame's index list, marked frame, extracted mark and similarity bit for bit against the single-image handles (full
    transforms, merged single-frame launches), the first and the last frame against the oracle with the bars of
    _whole_pipeline_vs_oracle.  Reference flow: src/algorithm.rs:295-379, :462-562, :696-714."""
    w, h, k, n = 3840, 2160, 1000, 20
    ctx = G.ctx()
    rgb = G.synth(1, 0, n, w, h)                                 # bench.py's frames: seed 1, frames 0 .. n - 1
    marks = np.random.default_rng(41).standard_normal((n, k)).astype(np.float32)
    ctx.set_chunk_frames(8)
    ctx.reset_timing()
    try:
        res = G.batch_embed(rgb, marks, want_idx=True)
        ext, sims = G.batch_extract(rgb, res["rgb"], k, marks)
    finally:
        ctx.set_chunk_frames(0)
    ps, ss = ctx.prune_stats(), ctx.select_stats()
    assert ps["pruned_chunks"] == 3 and ps["redone_chunks"] == 0, ps
    assert ctx.transform_plan(8, w, h)["fused_cols"] and not ctx.transform_plan(4, w, h)["fused_cols"]
    assert ss["exact_fallback_frames"] == 0, ss
    for f in range(n):
        rd = wm.Reader.base(rgb[f])
        assert np.array_equal(res["idx"][f], rd.indices(k).astype(np.uint32)), f
        e = rd.extract(wm.Reader.derived(res["rgb"][f]), k)
        assert np.array_equal(ext[f], e), f
        assert sims[f] == np.float32(wm.Tester(e).similarity(marks[f]).similarity), f
        assert np.array_equal(res["rgb"][f], wm.Writer(rgb[f]).mark([marks[f]])), f
    for f in (0, n - 1):
        _frame_vs_oracle(rgb[f], marks[f], None, res["idx"][f], res["rgb"][f], ext[f], sims[f])


@pytest.mark.parametrize("case", [(3840, 2160, True), (1920, 1080, False)])
def test_handle_latency_options_do_not_change_results(case):
    """What the single-image handles do for latency only (r5): the host frame crosses PCIe in two to four bands of rows with
    the row pass of a band beside the upload of the next (`upload_bands`; every copy enqueued ahead of the kernels), a base
    reader queues its selection for the mark length the context's last extraction used (`speculate_k`), a single frame's
    pruned derived transform runs its classes in one launch per kind.  Same marked frame, index lists and extracted marks
    whatever the options, for extraction lengths shorter and longer than the speculated one; against the batch entry points
    (no bands, no speculation, unmerged for eight frames) bit for bit.  Reference flow: src/algorithm.rs:295-379, :462-562."""
    from spread_spectrum_watermarking_amd.api import tuning
    w, h, as_u8 = case
    rgb = G.synth(7, 0, 1, w, h)[0]
    img = f32_to_u8(rgb) if as_u8 else rgb
    mark = np.random.default_rng(43).standard_normal(2000).astype(np.float32)
    ks = (1000, 500, 2000, 1000)

    def run():
        c = G.ctx()
        marked = wm.Writer(img, ctx=c).mark_rgb8([mark[:1000]]) if as_u8 else wm.Writer(img, ctx=c).mark([mark[:1000]])
        out = [marked]
        for k in ks:                                              # the second base reader on speculates k = 1000, then 500, 2000
            rd = wm.Reader.base(img, ctx=c)
            out.append(rd.extract(wm.Reader.derived(marked, c), k))
            out.append(rd.indices(k))
        return out
    with tuning(upload_bands=2, speculate_k=0):
        ref = run()
    for bands, spec in ((2, 1), (3, 1), (4, 0), (4, 1)):
        with tuning(upload_bands=bands, speculate_k=spec):
            got = run()
        for a, b in zip(ref, got):
            assert np.array_equal(a, b), (bands, spec)
    # the batch entry points on the same frame
    if as_u8:
        marked = G.batch_embed_rgb8(img[None], mark[None, :1000])
        assert np.array_equal(marked[0], ref[0])
        ext, _ = G.batch_extract_rgb8(img[None], marked, 1000, mark[None, :1000])
        assert np.array_equal(ext[0], ref[1])
    else:
        res = G.batch_embed(rgb[None], mark[None, :1000], want_idx=True)
        assert np.array_equal(res["rgb"][0], ref[0])
        assert np.array_equal(res["idx"][0], ref[2].astype(np.uint32))
        ext, _ = G.batch_extract(rgb[None], res["rgb"], 1000, mark[None, :1000])
        assert np.array_equal(ext[0], ref[1])


def _mirror_tile(img_u8, w, h):
    """A natural image mirror-tiled (no seams: every tile is the reflection of its neighbour) and cropped to w x h."""
    ih, iw = img_u8.shape[:2]
    row = np.concatenate([img_u8, img_u8[:, ::-1]], axis=1)
    row = np.concatenate([row] * (w // (2 * iw) + 1), axis=1)[:, :w]
    col = np.concatenate([row, row[::-1]], axis=0)
    return np.ascontiguousarray(np.concatenate([col] * (h // (2 * ih) + 1), axis=0)[:h])


@pytest.mark.parametrize("shape", [(1920, 1080), (3840, 2160)])
def test_natural_image_at_level2_shapes_matches_the_oracle(shape, cat_images, marks):
    """The reference's own photograph (tests/single_simple.rs:13, 640x444: dense column kernels) mirror-tiled to the
    shapes whose default path is level 2 / pruned / sampled-threshold selection -- the 8-bit batch entry points against the
    oracle on identical inputs (u8 -> f32 by v / 255 on both sides), with the reference's seed-1 mark.  A natural
    spectrum must not push the selection to its exact fallback nor the pruned transform to a redo."""
    w, h = shape
    k = 1000
    img = _mirror_tile(cat_images["cat"], w, h)
    mark = marks["seed_1"][None, :k].astype(np.float32)
    ctx = G.ctx()
    ctx.reset_timing()
    wm8 = G.batch_embed_rgb8(img[None], mark)
    frame = u8_to_f32(img)
    o_marked = O.embed_frame(frame, mark[0])
    o_wm8 = f32_to_u8(o_marked)
    assert np.mean(wm8[0] == o_wm8) > 0.9999 and np.abs(wm8[0].astype(np.int16) - o_wm8).max() <= 1
    # identical 8-bit inputs on both sides: the oracle's own marked frame as the derived image
    ext, sims = G.batch_extract_rgb8(img[None], o_wm8[None], k, mark)
    o_ext, o_sim = O.extract_frame(frame, u8_to_f32(o_wm8), mark[0])
    assert np.mean(ext[0] == o_ext) >= 0.999 and _ext_within_1e5(ext[0], o_ext)
    assert abs(float(sims[0]) - o_sim) < 1e-5 * abs(o_sim) + 1e-5
    # the f32 entry points on the same frame: coefficients and the index list
    res = G.batch_embed(frame[None], mark, want_coef=True, want_idx=True)
    ref_coef = O.dct2d(O.rgb_to_yiq(frame)[0])
    # (a mirror-tiled image is the even extension of its 640-pixel tile: only every third / sixth frequency column is
    # non-zero mathematically, the others hold round-off on both sides -- bit-identity is asked of the real coefficients)
    real = np.abs(ref_coef) > 1e-6 * ac_max(ref_coef)
    assert real.mean() > 0.1 and np.mean(res["coef"][0][real] == ref_coef[real]) > 0.9995
    assert np.abs(res["coef"][0].astype(np.float64) - ref_coef).max() <= 2e-7 * ac_max(ref_coef)
    assert np.array_equal(res["idx"][0], O.indices(ref_coef, k=k).astype(np.uint32))
    ps, ss = ctx.prune_stats(), ctx.select_stats()
    assert ss["exact_fallback_frames"] == 0, ss
    assert ps["pruned_chunks"] >= 1 and ps["redone_chunks"] == 0, ps


def test_8k_pipeline_and_resize_attack_parity_with_oracle():
    """BASELINE configs[4]: a 7680x4320 frame with a 10000-coefficient mark -- coefficient, index, extracted
    mark and similarity parity; then the flow of tests/attack_resize.rs:17-66 at that size (embed ->
    into_rgb8 -> CatmullRom resize to 12.5 % and back -> extract) against the oracle's run of the same flow."""
    w, h, k = 7680, 4320, 10000
    rgb, mark, res = _whole_pipeline_vs_oracle(w, h, k, 31, 1)
    frame8 = O.f32_to_u8(rgb[0])
    del rgb, res
    wm8 = G.batch_embed_rgb8(frame8[None], mark)
    o_wm8 = O.f32_to_u8(O.embed_frame(O.u8_to_f32(frame8), mark[0]))
    assert np.mean(wm8[0] == o_wm8) > 0.9999                           # 1-ulp differences of the f32 frame flip few roundings
    small = G.resize_rgb8(o_wm8, w // 8, h // 8)
    o_small = O.resize_rgb8(o_wm8, w // 8, h // 8)
    assert np.array_equal(small, o_small)                               # resize kernels bit-exact at 8K
    back = G.resize_rgb8(o_small, w, h)
    o_back = O.resize_rgb8(o_small, w, h)
    assert np.array_equal(back, o_back)
    ext, sims = G.batch_extract_rgb8(frame8[None], o_back[None], k, mark)
    o_ext, o_sim = O.extract_frame(O.u8_to_f32(frame8), O.u8_to_f32(o_back), mark[0])
    # same 8-bit inputs on both sides: bit-exact extraction (up to the rare 1-ulp coefficient, see above)
    assert np.mean(ext[0] == o_ext) >= 0.999 and _ext_within_1e5(ext[0], o_ext)
    assert abs(float(sims[0]) - o_sim) < 1e-5 * abs(o_sim) + 1e-5
    # and the all-device flow from the device's own marked frame
    back_d = G.resize_rgb8(G.resize_rgb8(wm8[0], w // 8, h // 8), w, h)
    ext_d, sims_d = G.batch_extract_rgb8(frame8[None], back_d[None], k, mark)
    assert abs(float(sims_d[0]) - o_sim) < 0.05 and sims_d[0] > 6.0


# The fused resize tile at the edges of its shared front end (csrc/resize_common.hpp): what pick_resize_tile chooses for each
# shape, printed from a scratch build, is in the comment -- together a last tile partial in both axes, the 4-word and the 2-word
# vertical pieces, dynamic LDS above 64 KB and each of the three horizontal passes.
RESIZE_TILE_CASES = [
    (508, 500, 60, 68),      # down-scaling: tile 8 x 16, 4 x 9 tiles, last 4 x 12; full rows of tiles 4-word, the last row 2-word
    (300, 300, 100, 100),    # tile 16 x 64, 79616 B of LDS (> 64 KB), last 4 x 36: 2-word
    (100, 60, 200, 120),     # integer up-scaling (quads share their taps): tile 32 x 128, last 24 x 72
    (128, 64, 380, 252),     # up-scaling: tile 64 x 128, 72448 B of LDS (> 64 KB), 3 x 4 tiles, last 60 x 124
]


@pytest.mark.parametrize("w,h,nw,nh", RESIZE_TILE_CASES)
def test_resize_tile_edges_equal_the_oracle(w, h, nw, nh):
    frames = np.random.default_rng(w + nw).integers(0, 256, (2, h, w, 3), dtype=np.uint8)
    got = G.resize_rgb8(frames, nw, nh)
    for f in range(2):
        assert np.array_equal(got[f], O.resize_rgb8(frames[f], nw, nh)), f


def test_automatic_pass_size():
    """~2^30 pixels per internal pass, capped where the f64 operand planes of a pass would pass 4 GB, in whole groups of 8."""
    ctx = G.ctx()
    # 4K: 2^30 px = 129 frames, 4 GB / (3840 columns x 1080 padded sums x 8 B) = 129 -> 128; full HD: 517 -> 512
    assert ctx.pass_frames(10 ** 6, 3840, 2160) == 128 and ctx.pass_frames(10 ** 6, 1920, 1080) == 512
    assert ctx.pass_frames(10 ** 6, 7680, 4320) == 32 and ctx.pass_frames(5, 3840, 2160) == 5
    ctx.set_chunk_frames(7)
    try:
        assert ctx.pass_frames(100, 1920, 1080) == 7
    finally:
        ctx.set_chunk_frames(0)


def test_full_hd_batch_in_several_passes_equals_handles():
    """BASELINE configs[2] frame size through the chunk loop with two lanes: 132 frames of 1920x1080 in passes of
    43 (three full ones and a ragged one of 3): every frame's index list and extracted mark against per-frame
    Reader handles (full transforms), marked frames of every pass against Writer handles."""
    w, h, k = 1920, 1080, 1000
    n = 132
    rgb = G.synth(12, 0, n, w, h)
    marks = np.random.default_rng(13).standard_normal((n, k)).astype(np.float32)
    G.ctx().set_chunk_frames(43)
    try:
        res = G.batch_embed(rgb, marks, want_idx=True)
        ext, sims = G.batch_extract(rgb, res["rgb"], k, marks)
    finally:
        G.ctx().set_chunk_frames(0)
    stats = G.ctx().prune_stats()
    assert stats["redone_chunks"] == 0
    for f in range(n):
        rd = wm.Reader.base(rgb[f])
        assert np.array_equal(res["idx"][f], rd.indices(k).astype(np.uint32)), f
        e = rd.extract(wm.Reader.derived(res["rgb"][f]), k)
        assert np.array_equal(ext[f], e), f
        assert sims[f] == np.float32(wm.Tester(e).similarity(marks[f]).similarity)
    for f in (0, 64, 128, 129, n - 1):
        assert np.array_equal(res["rgb"][f], wm.Writer(rgb[f]).mark([marks[f]])), f
    o_marked = O.embed_frame(rgb[n - 1], marks[n - 1])                  # last frame of the ragged chunk vs the oracle
    o_ext, o_sim = O.extract_frame(rgb[n - 1], o_marked, marks[n - 1])
    assert np.abs(res["rgb"][n - 1] - o_marked).max() <= 2e-7 and abs(float(sims[n - 1]) - o_sim) < 1e-4


def test_operand_planes_beyond_4gb_are_sliced():
    """ssw_dct2d on 520 full-HD planes in ONE pass (set_chunk_frames(520)): the f64 operand planes would be
    4.3 GB, past the 32-bit scalar offsets of the GEMM's k-walk, so the call transforms the frames in
    groups; the result must equal transforming hand-made slices, bit for bit, forward and inverse."""
    w, h, n = 1920, 1080, 520
    ctx, lib = G.ctx(), G.lib()
    plane = w * h
    rng = np.random.default_rng(5)
    base = rng.random((8, h, w)).astype(np.float32)
    planes = np.concatenate([base * np.float32(1.0 - 0.001 * r) for r in range(n // 8)])      # 520 distinct planes
    assert planes.shape == (n, h, w)
    for dct_type in (L.DCT2, L.DCT3):
        d = ctx.to_device(planes)
        ctx.set_chunk_frames(n)
        try:
            rc = lib.ssw_dct2d(ctx.handle, dct_type, F64, n, w, h, d.ptr)
            assert rc == L.SSW_OK
            whole = d.to_host(np.float32, planes.shape)
        finally:
            ctx.set_chunk_frames(0)
            d.free()
        for lo, hi in ((0, 100), (100, 357), (357, n)):
            assert np.array_equal(whole[lo:hi], G.dct2d(planes[lo:hi], dct_type, F64)), (dct_type, lo)
        del whole


def test_empty_and_degenerate_calls():
    lib, ctx = G.lib(), G.ctx()
    cfg = G.default_config()
    buf = ctx.alloc(64)
    import ctypes as C
    # zero frames / zero-length marks are no-ops, not errors
    assert lib.ssw_dct2d(ctx.handle, L.DCT2, F64, 0, 16, 16, buf.ptr) == L.SSW_OK
    assert lib.ssw_rgb_to_yiq(ctx.handle, buf.ptr, 0, 4, 4, buf.ptr, None, None) == L.SSW_OK
    assert lib.ssw_batch_embed(ctx.handle, C.byref(cfg), buf.ptr, 0, 16, 16, buf.ptr, 10, buf.ptr, None, None) == L.SSW_OK
    assert lib.ssw_batch_extract(ctx.handle, C.byref(cfg), buf.ptr, buf.ptr, 0, 16, 16, 10, buf.ptr, None, None) == L.SSW_OK
    assert lib.ssw_topk_indices(ctx.handle, buf.ptr, 1, 4, 4, L.ORDER_ENERGY, 0, buf.ptr) == L.SSW_OK
    # bad arguments are reported, never crash
    assert lib.ssw_dct2d(ctx.handle, L.DCT2, F64, 1, 0, 16, buf.ptr) == L.SSW_ERR_BAD_DIMS
    assert lib.ssw_dct2d(ctx.handle, 7, F64, 1, 4, 4, buf.ptr) == L.SSW_ERR_BAD_ARG
    assert lib.ssw_dct2d(ctx.handle, L.DCT2, F64, 1, 4, 4, None) == L.SSW_ERR_BAD_ARG
    bad = L.Config(L.ORDER_ENERGY, 9, 0.1, F64)
    assert lib.ssw_batch_embed(ctx.handle, C.byref(bad), buf.ptr, 1, 4, 4, buf.ptr, 1, buf.ptr, None, None) == L.SSW_ERR_BAD_ARG
    buf.free()
    # a mark of length 0 leaves the image untouched up to the transform round trip
    small = O.synth_frame(1, 1, 32, 24)
    out = wm.Writer(small).mark([np.zeros(0, np.float32)])
    assert np.abs(out - small).max() < 1e-6
    ext = wm.Reader.base(small).extract(wm.Reader.derived(small), 0)
    assert ext.shape == (0,)
