"""Fingerprinting (csrc/fingerprint.hip, writer_mark_copies_impl) at every boundary of its own machinery: the line plan at
chosen R (tests/fingerprint_cases.py: R = 1, either side of the FP_KSTEP padding, one past FP_SLOT_BLOCKS, every line), frames
inside and one pixel either side of the 32- and 64-pixel tiles of fp_update_kernel, k = 0 and marks cut at w*h - 1 with several
copies, both clamps of the fused epilogue, the two memory-bound copy groupings and a workspace with a history.

References, in order of authority: the oracle's embed_frame per mark (f32_to_u8 of it for 8-bit), ssw_batch_embed(_rgb8) on the
same frame and marks, and the exact properties of the design (a copy alone = the copy in any company, handle form = device
form, a repeat = the first run, a fresh context = a used one).

Bars are the project's (tests/gpu_util.py): f32 max |d| <= 2e-7, 8-bit <= 1 LSB, per copy, always; at least 0.9999 of the
values identical over the pooled copies of a case.  A pool under 1e5 values would let 0.9999 pass fewer than ten differences,
so against the oracle it becomes a count there: no more differing values than ssw_batch_embed's output for the same frame and
marks has against the oracle, plus one per 1e4 pooled values (rounded up).  Every case prints its counts (`-s`)."""
import ctypes as C
import math

import numpy as np
import pytest

import fingerprint_cases as FC
import gpu_util as G
import spread_spectrum_watermarking_amd as wm
from gpu_util import batch_embed, batch_embed_rgb8, fingerprint, fresh_ctx
from oracle import oracle as O
from spread_spectrum_watermarking_amd import _lib as L
from test_limits_gpu import report

pytestmark = pytest.mark.gpu

O1, O2, O3 = L.OPTION1, L.OPTION2, L.OPTION3
OPTION3_MARKED_IDENTICAL = 0.82          # tests/test_fingerprint_gpu.py: device expf vs libm, against the oracle only
SMALL_POOL = 10 ** 5
CASES = FC.line_plan_cases()


def marks_for(n, k, seed):
    return np.random.default_rng(seed).standard_normal((n, k)).astype(np.float32)


def is_u8(a):
    return a.dtype == np.uint8


def oracle_copies(rgb, marks, method=O2, alpha=0.1):
    """O.embed_frame per mark (f32_to_u8 of it for an 8-bit frame)."""
    f = O.u8_to_f32(rgb) if is_u8(rgb) else rgb
    out = np.stack([O.embed_frame(f, m, method=method, alpha=alpha) for m in marks])
    return O.f32_to_u8(out) if is_u8(rgb) else out


def batch_copies(rgb, marks, cfg=None):
    rep = np.repeat(rgb[None], len(marks), 0)
    return batch_embed_rgb8(rep, marks, cfg) if is_u8(rgb) else batch_embed(rep, marks, cfg)["rgb"]


def unmarked(rgb):
    w = wm.Writer(rgb, ctx=G.ctx())
    return w.result_rgb8() if is_u8(rgb) else w.result()


def n_diff(a, b):
    return int(np.count_nonzero(a != b))


def assert_abs_bar(got, ref, what):
    """The absolute bars, per copy: f32 max |d| <= 2e-7 (assert_f32_bars), 8-bit <= 1 LSB (assert_u8_bars)."""
    for i in range(len(got)):
        if is_u8(got):
            d = np.abs(got[i].astype(np.int32) - ref[i].astype(np.int32)).max()
            assert d <= 1, (what, i, d)
        else:
            G.assert_f32_bars(got[i], ref[i], identical=0.0, what=f"{what} copy {i}")


def assert_bars(copies, oracle, batch, what, oracle_identical=0.9999):
    """The bars of the module docstring on the pooled copies of one case: `copies` against `oracle` and against `batch`."""
    pool = copies.size
    fp_o, batch_o, fp_b = n_diff(copies, oracle), n_diff(batch, oracle), n_diff(copies, batch)
    report(f"fingerprint {what}", pool=pool, fp_vs_oracle=fp_o, batch_vs_oracle=batch_o, fp_vs_batch=fp_b)
    assert_abs_bar(copies, oracle, f"{what} vs oracle")
    assert_abs_bar(copies, batch, f"{what} vs batch")
    if pool < SMALL_POOL and oracle_identical == 0.9999:
        assert fp_o <= batch_o + math.ceil(pool / 1e4), (what, fp_o, batch_o, pool)
    else:
        assert 1.0 - fp_o / pool >= oracle_identical, (what, fp_o, pool)
    assert 1.0 - fp_b / pool >= 0.9999, (what, fp_b, pool)


def assert_not_vacuous(copies, plain, what):
    """An equality test says something only if the marks are visible: every copy differs from the unmarked result by more than
    1e-3 somewhere (f32; 2 LSB for 8-bit) and the copies differ from each other."""
    for i in range(len(copies)):
        if is_u8(copies):
            assert np.abs(copies[i].astype(np.int32) - plain.astype(np.int32)).max() >= 2, (what, i)
        else:
            assert np.abs(copies[i] - plain).max() > 1e-3, (what, i)
        for j in range(i):
            assert not np.array_equal(copies[i], copies[j]), (what, i, j)


def as_dtype(rgb_f32, dtype):
    return O.f32_to_u8(rgb_f32) if dtype == "u8" else rgb_f32


# A. line plans -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["f32", "u8"])
@pytest.mark.parametrize("name", list(CASES))
def test_line_plan(name, dtype):
    """Every planted case, 3 copies: the device list is the planted one (8-bit: the oracle's list of the quantised frame, on
    the same R lines -- quantisation may swap neighbours 4 % apart), the bars, and each copy alone equals the copy in company."""
    w, h, coords = CASES[name]
    rgb = as_dtype(FC.case_frame(name), dtype)
    k = len(coords)
    marks = marks_for(3, k, FC.case_seed(name))
    copies, idx = fingerprint(rgb, marks, want_idx=True)
    if dtype == "f32":
        assert np.array_equal(idx, FC.flat(coords, w))
    else:
        assert np.array_equal(idx, O.indices(O.dct2d(O.rgb_to_yiq(O.u8_to_f32(rgb))[0]), k=k))
    lines = {FC.line_pos(w, h, int(i) // w, int(i) % w)[0] for i in idx}
    assert len(lines) == FC.named_R(name, w, h)
    assert_bars(copies, oracle_copies(rgb, marks), batch_copies(rgb, marks), f"{name} {dtype}")
    assert_not_vacuous(copies, unmarked(rgb), name)
    for i in range(3):
        assert np.array_equal(fingerprint(rgb, marks[i:i + 1])[0], copies[i]), i
    assert np.array_equal(fingerprint(rgb, marks[::-1])[::-1], copies)


@pytest.mark.parametrize("dtype", ["f32", "u8"])
@pytest.mark.parametrize("name", [n for n in CASES if n.endswith("-R1") or n.endswith("-Rlb")])
def test_line_plan_repeats_bit_equal(name, dtype):
    """R = 1 (40 entries in one slot) and R = lb: the atomics fill the slot lists in an order that differs between runs; the
    per-slot sort makes the summation order, and so every bit of the result, the same."""
    rgb = as_dtype(FC.case_frame(name), dtype)
    marks = marks_for(3, len(CASES[name][2]), FC.case_seed(name) + 5)
    first = fingerprint(rgb, marks)
    assert_not_vacuous(first, unmarked(rgb), name)
    for run in (1, 2):
        assert np.array_equal(fingerprint(rgb, marks), first), run


@pytest.mark.parametrize("method", [O1, O3], ids=["option1", "option3"])
@pytest.mark.parametrize("name", ["96x40-R17", "40x96-R33", "64x64-Rlb"])
def test_line_plan_other_methods(name, method):
    rgb = FC.case_frame(name)
    marks = marks_for(3, len(CASES[name][2]), FC.case_seed(name) + 2)
    cfg = G.default_config(L.PRECISION_F64, L.ORDER_ENERGY, method, 0.1)
    assert_bars(fingerprint(rgb, marks, cfg), oracle_copies(rgb, marks, method, 0.1), batch_copies(rgb, marks, cfg),
                f"{name} method {method}", OPTION3_MARKED_IDENTICAL if method == O3 else 0.9999)


# B. tiles and tiny frames ------------------------------------------------------------------------------------------------
# (w, h): one pixel, the shortest strips, strips of one tile side, inside one wave tile, one pixel either side of the 32-pixel
# wave tile and of the 64-pixel block tile, and a 16-wide frame of three tile rows
TINY = [(1, 1), (2, 1), (1, 2), (1, 64), (64, 1), (7, 5), (31, 33), (33, 31), (63, 65), (65, 63), (16, 130)]
SENTINEL = 0xA5


def raw_call(which, rgb, marks, n):
    """(status, output) of ssw_fingerprint_embed(_rgb8) (`which` = "fp") on rgb [h, w, 3] or of ssw_batch_embed(_rgb8) on the
    frame repeated n times; marks [n, k], k may be 0.  The output buffer is filled with SENTINEL bytes before the call."""
    lib, ctx = G.lib(), G.ctx()
    u8 = is_u8(rgb)
    h, w = rgb.shape[:2]
    k = marks.shape[1]
    cfg = G.default_config()
    sent = np.full((n, h, w, 3), SENTINEL, np.uint8) if u8 else np.frombuffer(bytes([SENTINEL]) * (n * h * w * 12), np.float32).reshape(n, h, w, 3)
    d = ctx.to_device(rgb if which == "fp" else np.repeat(rgb[None], n, 0))
    dm = ctx.to_device(marks) if marks.size else ctx.alloc(16)
    out = ctx.to_device(sent)
    if which == "fp":
        fn = lib.ssw_fingerprint_embed_rgb8 if u8 else lib.ssw_fingerprint_embed
        status = fn(ctx.handle, C.byref(cfg), d.ptr, w, h, dm.ptr, n, k, out.ptr, None)
    elif u8:
        status = lib.ssw_batch_embed_rgb8(ctx.handle, C.byref(cfg), d.ptr, n, w, h, dm.ptr, k, out.ptr)
    else:
        status = lib.ssw_batch_embed(ctx.handle, C.byref(cfg), d.ptr, n, w, h, dm.ptr, k, out.ptr, None, None)
    ctx.synchronize()
    res = out.to_host(sent.dtype, sent.shape)
    for b in (d, dm, out):
        b.free()
    return status, res, sent


def tiny_frames(w, h, dtype):
    noise = np.random.default_rng(100 * w + h).random((h, w, 3)).astype(np.float32)
    return {"noise": as_dtype(noise, dtype), "synth": as_dtype(O.synth_frame(21, w + h, w, h), dtype)}


@pytest.mark.parametrize("dtype", ["f32", "u8"])
@pytest.mark.parametrize("w, h", TINY, ids=[f"{w}x{h}" for w, h in TINY])
def test_tiny_frames(w, h, dtype):
    """k = 0, 1, w*h - 1 and w*h + 10 (cut at w*h - 1: the marks keep their stride of k, so copy i must carry its own mark) with
    3 copies.  The status is ssw_batch_embed's; where that is SSW_OK the bars hold; with nothing to mark (k = 0, one pixel)
    every copy is the unmarked result; a refused call leaves the output alone."""
    for content, rgb in tiny_frames(w, h, dtype).items():
        plain = unmarked(rgb)
        for k in (0, 1, w * h - 1, w * h + 10):
            what = f"{w}x{h} {dtype} {content} k={k}"
            marks = marks_for(3, k, 7 * w + h + k)
            st_b, batch, sent = raw_call("batch", rgb, marks, 3)
            st_f, copies, _ = raw_call("fp", rgb, marks, 3)
            assert st_f == st_b, (what, st_f, st_b)
            if st_b != L.SSW_OK:
                assert np.array_equal(copies.view(np.uint8), sent.view(np.uint8)), what
                continue
            if min(k, w * h - 1) == 0:
                for i in range(3):
                    assert np.array_equal(copies[i], plain), (what, i)
            assert_bars(copies, oracle_copies(rgb, marks), batch, what)


@pytest.mark.parametrize("dtype", ["f32", "u8"])
@pytest.mark.parametrize("w, h", [(7, 5), (33, 31), (16, 130)], ids=["7x5", "33x31", "16x130"])
def test_cut_marks_through_the_handle_form(w, h, dtype):
    """Writer.mark_copies(_rgb8) with marks of w*h + 10 values, 3 copies: the device form bit for bit, each copy its own mark."""
    rgb = tiny_frames(w, h, dtype)["noise"]
    marks = marks_for(3, w * h + 10, w + h)
    wr = wm.Writer(rgb, ctx=G.ctx())
    got = wr.mark_copies_rgb8(marks) if dtype == "u8" else wr.mark_copies(marks)
    assert_not_vacuous(got, unmarked(rgb), f"{w}x{h}")
    assert np.array_equal(got, fingerprint(rgb, marks))
    assert_bars(got, oracle_copies(rgb, marks), batch_copies(rgb, marks), f"handle form, cut marks, {w}x{h} {dtype}")


def test_cut_marks_past_one_group():
    """66 copies of a 7 x 5 frame with marks of 45 values (34 used): the second group of copies starts at mark 64 of a list
    whose stride is 45, not 34."""
    w, h, n = 7, 5, 66
    rgb = tiny_frames(w, h, "f32")["noise"]
    marks = marks_for(n, w * h + 10, 66)
    copies = fingerprint(rgb, marks)
    assert_not_vacuous(copies[[0, 63, 64, 65]], unmarked(rgb), "7x5 x 66")
    for i in (0, 63, 64, 65):
        assert np.array_equal(fingerprint(rgb, marks[i:i + 1])[0], copies[i]), i
    assert_bars(copies, oracle_copies(rgb, marks), batch_copies(rgb, marks), "7x5, 66 copies, cut marks")
    assert np.array_equal(wm.Writer(rgb, ctx=G.ctx()).mark_copies(marks), copies)


# C. clamps ---------------------------------------------------------------------------------------------------------------
CLAMP_K = 1000
CLAMP_CONFIGS = {"option2-alpha1": (O2, 1.0, 1.0), "option1-alpha0.5-marks-x4": (O1, 0.5, 4.0)}      # method, alpha, mark scale


# Cases in which ssw_batch_embed itself misses the oracle's bars, so the miss is not the fingerprint path's to answer for
# (measured on an MI355X; fingerprint and batch bit-identical in every one of them):
#   "selection": every AC coefficient of an all-255 frame, and most of the 8 x 8 checkerboard's on 40 x 96 (8 divides both
#       sides), is rounding residue of the forward transform, below 2^-20 of the largest.  k = 1000 reaches into them, their
#       order is decided by the last bits of two different transforms, and Option1 adds the mark to whichever are picked:
#       20553 / 12852 of 34560 values differ (checker f32 / u8, max 1.7e-2 / 4 LSB), 25782 / 20334 (ones 40 x 96, 3.0e-2 / 8 LSB),
#       27750 / 20997 of 36855 (ones 65 x 63, 2.8e-2 / 7 LSB).  Option2 multiplies the residue and moves nothing.
#   "transform": noise at Option2, alpha 1, 40 x 96 f32: the same index list as the oracle's, 517 of 34560 values differ and
#       one pixel (luma 0.56, far from either clamp) by 2.38e-7, for both paths alike.  Not the epilogue: there the luma itself
#       is four ulps of the second pass's f32 store away from the oracle's.  Supposed, not shown: entries of the f32 plane
#       between the two passes reach thousands at this strength (ulp 2^-12), and two of them one ulp off in the pixel's line
#       make 2 * 2^-12 / 2 * 4 / (W H) = 2.5e-7.
SHARED_WITH_BATCH = {(40, 96, "checker", "option1-alpha0.5-marks-x4", "f32"): "selection",
                     (40, 96, "checker", "option1-alpha0.5-marks-x4", "u8"): "selection",
                     (40, 96, "ones", "option1-alpha0.5-marks-x4", "f32"): "selection",
                     (40, 96, "ones", "option1-alpha0.5-marks-x4", "u8"): "selection",
                     (65, 63, "ones", "option1-alpha0.5-marks-x4", "f32"): "selection",
                     (65, 63, "ones", "option1-alpha0.5-marks-x4", "u8"): "selection",
                     (40, 96, "noise", "option2-alpha1", "f32"): "transform"}


def clamp_frame(content, w, h):
    """8-bit frames that sit on the clamps: 8 x 8 blocks of 0 and 255, all 0, all 255, and noise of standard deviation 110
    around 127.5 (an eighth of it clipped at either end)."""
    yy, xx = np.mgrid[0:h, 0:w]
    if content == "checker":
        grey = (((yy // 8 + xx // 8) & 1) * 255).astype(np.uint8)
        return np.repeat(grey[:, :, None], 3, 2)
    if content == "noise":
        v = 127.5 + 110.0 * np.random.default_rng(1000 * w + h).standard_normal((h, w, 3))
        return np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return np.full((h, w, 3), 0 if content == "zeros" else 255, np.uint8)


@pytest.mark.parametrize("dtype", ["f32", "u8"])
@pytest.mark.parametrize("conf", list(CLAMP_CONFIGS))
@pytest.mark.parametrize("content", ["checker", "zeros", "ones", "noise"])
@pytest.mark.parametrize("w, h", [(40, 96), (65, 63)], ids=["40x96", "65x63"])
def test_clamps(w, h, content, conf, dtype):
    """Strong marks on frames at the ends of the range: pair_clamp01_med3 and pair_round255 of the fused epilogue against the
    oracle and the batch path.  Precondition (on the oracle's own output): at least 1 % of the values at 0 and at least 1 % at
    255 (1.0).  A uniform frame can only reach its own end: an all-0 frame has an all-zero spectrum, which Option2 leaves as it
    is and Option1 moves by about 2 / sqrt(w h) = 0.03 per pixel, and the same holds below 255 -- there the 1 % is asked of
    that end alone.  Seven cases in which ssw_batch_embed misses the oracle in the same way are held to ssw_batch_embed bit for
    bit instead (SHARED_WITH_BATCH)."""
    method, alpha, scale = CLAMP_CONFIGS[conf]
    img = clamp_frame(content, w, h)
    rgb = img if dtype == "u8" else O.u8_to_f32(img)
    marks = marks_for(3, CLAMP_K, w + 3 * h) * np.float32(scale)
    ref = oracle_copies(rgb, marks, method, alpha)
    lo, hi = float(np.mean(ref == 0)), float(np.mean(ref == (255 if dtype == "u8" else 1.0)))
    assert content == "ones" or lo >= 0.01, lo
    assert content == "zeros" or hi >= 0.01, hi
    cfg = G.default_config(L.PRECISION_F64, L.ORDER_ENERGY, method, alpha)
    what = f"clamps {w}x{h} {content} {conf} {dtype} at0={lo:.3f} at1={hi:.3f}"
    copies, idx = fingerprint(rgb, marks, cfg, want_idx=True)
    batch = batch_copies(rgb, marks, cfg)
    shared = SHARED_WITH_BATCH.get((w, h, content, conf, dtype))
    if shared is None:
        return assert_bars(copies, ref, batch, what)
    # the batch path misses the oracle here for a reason that is not the fingerprint path's (below): both figures are printed,
    # the miss (and for "selection" its cause) is asserted so that the table cannot go stale, and the copies must be ssw_batch_embed's bit for bit
    fp_o, batch_o = n_diff(copies, ref), n_diff(batch, ref)
    err = float(np.abs(batch.astype(np.float64) - ref.astype(np.float64)).max())
    report(f"fingerprint {what}: {shared}", pool=copies.size, fp_vs_oracle=fp_o, batch_vs_oracle=batch_o, batch_max_err=err)
    assert err > (1 if dtype == "u8" else 2e-7), "ssw_batch_embed meets the oracle's bar here now: take the case out of SHARED_WITH_BATCH"
    assert np.array_equal(copies, batch), what
    f32 = O.u8_to_f32(rgb) if dtype == "u8" else rgb
    coef, _, _ = G.oracle_forward(f32)
    o_idx = O.indices(coef, k=CLAMP_K)
    if shared == "selection":
        disputed = np.setxor1d(idx.astype(np.int64), o_idx.astype(np.int64))
        mag = np.abs(coef.reshape(-1).astype(np.float64))
        assert disputed.size and mag[disputed].max() <= 2.0 ** -20 * mag.max(), (disputed.size, mag[disputed].max(), mag.max())
    else:
        assert np.array_equal(idx, o_idx)


# D. memory-bound groups --------------------------------------------------------------------------------------------------
def test_memory_bound_groups():
    """2048 x 2064 (w x h: columns first, la = 2064, lb = 2048), k = 2048, 85 copies, 8-bit.  A group's workspace per copy is
    s_pad * la * 8 + k * 8 = 2048 * 2064 * 8 + 2048 * 8 = 33 832 960 B, so the device form's groups are 2 GiB / per_copy = 63,
    then 22.  A copy's output is 2048 * 2064 * 3 = 12 681 216 B, so the handle form's outer groups are 1 GiB / out_bytes = 84,
    then 1, with inner groups 63 + 21 and 1.  per_copy <= 8 * pixels + 8 k, so no smaller frame makes the memory term bind below
    64 copies.  About 1.1 GB of host output per form and 3.5 GB of device memory."""
    w, h, k, n = 2048, 2064, 2048, 85
    with fresh_ctx():
        img = O.f32_to_u8(G.synth(31, 0, 1, w, h)[0])
        marks = marks_for(n, k, 31)
        copies = fingerprint(img, marks)
        plain = unmarked(img)
        assert_not_vacuous(copies[[0, 62, 63, 84]], plain, "device form")
        for i in (0, 62, 63, 84):
            assert np.array_equal(fingerprint(img, marks[i:i + 1])[0], copies[i]), i
        wr = wm.Writer(img, ctx=G.ctx())
        handle = wr.mark_copies_rgb8(marks)
        for i in (0, 62, 63, 83, 84):
            assert np.array_equal(handle[i], copies[i]), i
        del handle
        ref = O.f32_to_u8(O.embed_frame(O.u8_to_f32(img), marks[84]))
        report("fingerprint 2048x2064, copy 84 of 85 vs oracle", differing=n_diff(copies[84], ref), pool=ref.size)
        G.assert_u8_bars(copies[84], ref, "copy 84 vs oracle")
        for i in (63, 84):
            G.assert_u8_bars(copies[i], batch_embed_rgb8(img[None], marks[i:i + 1])[0], f"copy {i} vs batch")
        m = marks_for(1, k, 32)[0]
        assert np.array_equal(wr.mark_rgb8([m]), wm.Writer(img, ctx=G.ctx()).mark_rgb8([m]))


# E. workspace history ----------------------------------------------------------------------------------------------------
def history_cases():
    name = "96x40-R1"
    small = np.random.default_rng(75).random((5, 7, 3)).astype(np.float32)
    return [(FC.case_frame(name), marks_for(3, len(CASES[name][2]), 41)), (small, marks_for(3, 20, 42))]


def test_small_calls_after_a_large_one():
    """ctx->fingerprint[0..5] only grow and are reused: after 333 x 197, k = 500, 8 copies (R about 40, s_pad 208), the R = 1
    case and a 7 x 5 frame give what a fresh context gives, bit for bit."""
    with fresh_ctx():
        expect = [fingerprint(rgb, marks) for rgb, marks in history_cases()]
        for (rgb, _), e in zip(history_cases(), expect):
            assert_not_vacuous(e, unmarked(rgb), "fresh context")
    with fresh_ctx():
        fingerprint(O.synth_frame(40, 0, 333, 197), marks_for(8, 500, 40))
        for (rgb, marks), e in zip(history_cases(), expect):
            assert np.array_equal(fingerprint(rgb, marks), e)


def test_padding_rows_after_non_finite_planes():
    """R = 33 with infinite marks leaves non-finite dT rows in the workspace; the R = 17 case after it pads its plan to 32 rows
    at the same addresses (s_pad = 48 for both: the frame has 40 lines), which must be written as zeros, not trusted to be:
    0 * NaN is NaN."""
    big, small = "96x40-R33", "96x40-R17"
    rgb, marks = FC.case_frame(small), marks_for(3, len(CASES[small][2]), 43)
    with fresh_ctx():
        expect = fingerprint(rgb, marks)
        assert_not_vacuous(expect, unmarked(rgb), "fresh context")
    with fresh_ctx():
        poison = np.full((3, len(CASES[big][2])), np.inf, np.float32)
        fingerprint(FC.case_frame(big), poison)
        got = fingerprint(rgb, marks)
        assert np.isfinite(got).all()
        assert np.array_equal(got, expect)
